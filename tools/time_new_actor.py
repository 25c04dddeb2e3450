"""What the first change of a NEW actor costs am355_apply_changes on a large kept state, beside a known actor's call (host to host).

The state: loggen.config("c4_text_single", scale) but its last round -- 64 actors, ~1 M op rows at scale 1.0. The log itself cannot be
split so that some of its actors appear late: every change of a round depends on every change of the round before. The 16 newcomers are
therefore the first-round changes (200 characters each) of actors 1..16 of a second, independent concurrent-text log, delivered one per
call behind that log's setup change; beside each, one change of the held round by an actor the document knows. Before the timed calls:
eight known-actor calls and the second log's setup change (itself a newcomer's: the path is warm).

    python tools/time_new_actor.py [--lib libam355.so] [--scale 1.0] [--label text]

--lib: another build of the engine (the parent commit's, for the A/B): a library without am355_set_resident_new_actors serves the
newcomers by the full replay. Prints the per-call times, their median and max, and the path counters."""
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
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--label", default="")
args = ap.parse_args()


def changes_of(log):
    arena, offs = bytes(log.arena), [int(x) for x in log.offsets]
    return [arena[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]


N_NEW, WARM = 16, 8
base = changes_of(loggen.config("c4_text_single", args.scale))
assert len(base) > 1 + 64, "the scale leaves no round to hold back"
head, held = base[:-64], base[-64:]
late = changes_of(loggen.generate(loggen.KIND_TEXT_CONCURRENT, n_actors=N_NEW + 1, n_rounds=1, ins_per_change=200, del_per_change=50, n_objects=1,
                                  seed=0x5EED0A11))
late_setup, late_first = late[0], late[2:2 + N_NEW]   # (late[1]: the setup author's own first-round change, not a newcomer's)
assert len(late_first) == N_NEW

eng = engine.Engine(0, args.lib) if args.lib else engine.Engine(0)
switch = hasattr(eng._L, "am355_set_resident_new_actors")
if switch:
    eng.set_resident_new_actors(True)


def call(batch):
    log = ChangeLog.from_changes(batch)
    t0 = time.perf_counter()
    eng.apply_changes(log)   # (returns with the incremental patch assembled on the host: behind every device wait of the call)
    return (time.perf_counter() - t0) * 1e3


call(head)
rows = int(eng.stats().n_ops)
for j in range(WARM):
    call([held[j]])
call([late_setup])
new_ms, known_ms = [], []
for j in range(N_NEW):
    new_ms.append(call([late_first[j]]))
    known_ms.append(call([held[WARM + j]]))


def line(what, ms):
    s = sorted(ms)
    return "%-22s median %.3f ms  max %.3f ms  min %.3f ms   [%s]" % (what, (s[len(s) // 2 - 1] + s[len(s) // 2]) / 2, s[-1], s[0], " ".join("%.3f" % t for t in ms))


print("time_new_actor%s: c4_text_single scale %g, %d rows kept; switch %s" % (" (" + args.label + ")" if args.label else "", args.scale, rows,
                                                                              "on" if switch else "absent (full replay for newcomers)"))
print(line("newcomer's first change", new_ms))
print(line("known actor's change", known_ms))
print("resident counters (served, fell back, in place):", eng.resident_counters(),
      " new-actor calls (served, rank rewrites):", eng.resident_new_actor_calls() if switch else "n/a")
eng.close()
