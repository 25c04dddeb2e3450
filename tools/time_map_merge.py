"""What a map change costs am355_apply_changes on a kept state, with the plain map rows merged into the stored map records
(am355_set_resident_map_merge) and without (host to host: each call ends with the incremental patch assembled on the host).

  (a) one change per call onto loggen.config("c3_map_lww", 1.0) without its last round: 32 actors, 10 000 keys, 313 ops per change,
      ~70 k op rows kept, no list in the document (without the switch such a call runs all of merge_run);
  (b) 40 changes per call onto the same document;
  (c) one map change per call onto the 1 M-op text + map document of tools/profile_apply_mixed.py (without the switch: merge_run_maps).
The changes that follow the kept rounds come from the same generator run with more rounds: the kept rounds are the same bytes. Before
the timed calls of a part: warm-up calls of the same shape.

    python tools/time_map_merge.py [--lib libam355.so] [--off] [--parts abc] [--label text]

--lib: another build of the engine (the parent commit's, for the A/B): a library without am355_set_resident_map_merge serves the calls
as before. --off: this library with the switch left off. Prints the per-call times, their median and max, and the path counters."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from automerge_classic_amd import engine, loggen  # noqa: E402
from automerge_classic_amd.loggen import ChangeLog  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None)
ap.add_argument("--off", action="store_true")
ap.add_argument("--parts", default="abc")
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--label", default="")
args = ap.parse_args()


def changes_of(log):
    arena, offs = bytes(log.arena), [int(x) for x in log.offsets]
    return [arena[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]


def line(what, ms):
    s = sorted(ms)
    return "%-34s median %.3f ms  max %.3f ms  min %.3f ms   [%s]" % (what, (s[(len(s) - 1) // 2] + s[len(s) // 2]) / 2, s[-1], s[0], " ".join("%.3f" % t for t in ms))


def session(what, head, batches, warm):
    eng = engine.Engine(0, args.lib) if args.lib else engine.Engine(0)
    has = hasattr(eng._L, "am355_set_resident_map_merge")
    if has and not args.off:
        eng.set_resident_map_merge(True)

    def call(batch):
        log = ChangeLog.from_changes(batch)
        t0 = time.perf_counter()
        eng.apply_changes(log)
        return (time.perf_counter() - t0) * 1e3
    call(head)
    rows = int(eng.stats().n_ops)
    ms = [call(b) for b in batches]
    print(line("%s, %d rows kept" % (what, rows), ms[warm:]))
    print("    resident counters (served, fell back, in place):", eng.resident_counters(), " maps-only calls:", eng.resident_maps_only_calls(),
          " map rows merged in place (calls, declined):", eng.resident_map_merge_calls() if has else "n/a", flush=True)
    eng.close()


print("time_map_merge%s: switch %s" % (" (" + args.label + ")" if args.label else "",
                                        "left off" if args.off else "on where the library has it"), flush=True)
NA, ROUNDS = 32, max(2, int(8 * args.scale))
if "a" in args.parts or "b" in args.parts:
    base = changes_of(loggen.config("c3_map_lww", args.scale))
    more = changes_of(loggen.generate(loggen.KIND_MAP_LWW, n_actors=NA, n_rounds=ROUNDS + 7, n_keys=10_000, seed=0x5EED0003))
    kept = NA * (ROUNDS - 1)
    assert more[:len(base)] == base, "the longer log does not begin with the configuration's"
    if "a" in args.parts:
        session("(a) 1 change of 313 ops per call", more[:kept], [[c] for c in more[kept:kept + 32]], 8)
    if "b" in args.parts:
        session("(b) 40 changes per call", more[:kept], [more[kept + 40 * j:kept + 40 * (j + 1)] for j in range(6)], 2)
if "c" in args.parts:
    text = changes_of(loggen.config("c4_text_single", args.scale))
    maps = changes_of(loggen.generate(loggen.KIND_MAP_LWW, n_actors=8, n_rounds=7, n_keys=64, seed=4242))
    session("(c) 1 map change beside a large Text", text + maps[:8], [[c] for c in maps[8:8 + 40]], 8)
