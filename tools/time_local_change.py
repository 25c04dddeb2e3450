"""What Backend.applyLocalChange costs on the engine, host to host through the C ABI, onto a large resident state -- and what of it is
BUILDING the change: the same changes applied as remote ones (am355_apply_changes of the bytes encodeChange gives) are the comparison
row, which a library of the parent commit serves as well.

The state: loggen.config("c4_text_single", scale) -- ~1 M op rows at scale 1.0 -- applied in one call. A new author then types into the
Text behind its first element:
    (a) one character per change                      (17 calls; the first is the author's first change and is reported apart)
    (b) 200 characters per change                     (8 calls)
    (c) a paste of 100,000 characters, one op         (3 calls)

    python tools/time_local_change.py [--lib libam355.so] [--scale 1.0] [--remote] [--small] [--label text] [--trace]

--small: am355_set_local_small on (a library that has the switch): the changes of (a) and (b) are built by one workgroup (kl_small), the
paste of (c) lies beyond its limits and takes the bulk path; local_small_calls is printed. profiles/local_small_timings.txt is three
runs alternating in one session, two rounds: the parent commit's library, this one with the switch off, this one with --small.

--remote: the changes are encoded first (am355_encode_change of the shipped library, deps chained by hand) and applied with
am355_apply_changes of --lib. --trace: AM355_TRACE=1 for the timed calls, whose laps (request staged / expand + encodes / columns on the
host / container + hash / the apply path's own) go to stderr. The request is flattened before the clock starts: the time is the C call's.
Prints the per-call times, their median and max, and the path counters."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from automerge_classic_amd import engine, loggen  # noqa: E402
from automerge_classic_amd.loggen import ChangeLog  # noqa: E402

Z = "e7" * 16
SHAPES = (("one character", 1, 17), ("200 characters", 200, 8), ("100,000-character paste", 100_000, 3))


def requests_for(text_id, first_elem):
    reqs, seq, op, after = [], 0, None, first_elem
    for name, n, calls in SHAPES:
        for _ in range(calls):
            seq += 1
            reqs.append((name, {"actor": Z, "seq": seq, "startOp": op, "time": 0, "message": "", "deps": [],
                                "ops": [{"action": "set", "obj": text_id, "elemId": after, "insert": True, "values": ["x"] * n, "pred": []} if n > 1 else
                                        {"action": "set", "obj": text_id, "elemId": after, "insert": True, "value": "x", "pred": []}]}, n))
    return reqs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=engine.DEFAULT_LIB)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--remote", action="store_true")
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--label", default="")
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    log = loggen.config("c4_text_single", a.scale)
    eng = engine.Engine(0, a.lib)
    for sw in ("set_resident_new_actors", "set_resident_new_objects", "set_resident_counters"):
        if hasattr(eng._L, "am355_" + sw):
            getattr(eng, sw)(True)
    if a.small:
        eng.set_local_small(True)
    eng.apply_changes(log)
    st = eng.stats()
    whole = json.loads(eng.patch_json())
    text = next(v for prop in whole["diffs"]["props"].values() for v in prop.values() if v.get("type") == "text")
    text_id, first_elem, max_op, heads = text["objectId"], text["edits"][0]["elemId"], whole["maxOp"], whole["deps"]
    reqs = requests_for(text_id, first_elem)
    op = max_op + 1
    for _, r, n in reqs:   # op ids; every change types behind the last character of the one before
        r["startOp"] = op
        if r["seq"] > 1:
            r["ops"][0]["elemId"] = f"{op - 1}@{Z}"
        else:
            r["deps"] = list(heads)
        op += n
    encoded = []
    if a.remote:
        enc = engine.Engine(0)   # (the shipped library: the one with am355_encode_change)
        last = None
        for _, r, _n in reqs:
            rr = dict(r, deps=sorted(set(r["deps"]) | ({last} if last else set())))
            b, h = enc.encode_change(rr)
            encoded.append(b)
            last = h.hex()
        enc.close()
    if a.trace:
        os.environ["AM355_TRACE"] = "1"
    times = {}
    before = eng.resident_counters()
    for i, (name, r, n) in enumerate(reqs):
        if a.remote:
            cl = ChangeLog.from_changes([encoded[i]])
            import numpy as np
            arena = np.ascontiguousarray(cl.arena, dtype=np.uint8)
            offs = np.ascontiguousarray(cl.offsets, dtype=np.uint64)
            t0 = time.perf_counter()
            rc = eng._L.am355_apply_changes(eng._h, arena.ctypes.data, offs.ctypes.data, 1)
            dt = time.perf_counter() - t0
        else:
            lc, keep = engine.flatten_change_request(r)
            p, ln = ctypes.c_void_p(), ctypes.c_size_t()
            t0 = time.perf_counter()
            rc = eng._L.am355_apply_local_change(eng._h, ctypes.byref(lc), ctypes.byref(p), ctypes.byref(ln))
            dt = time.perf_counter() - t0
            del keep
        eng._check(rc)
        times.setdefault("first change of the author" if i == 0 else name, []).append(1e3 * dt)
    after = eng.resident_counters()
    mode = "remote (am355_apply_changes of the encoded bytes)" if a.remote else "local (am355_apply_local_change)"
    print(f"# {a.label or os.path.basename(a.lib)} | {mode} | state {st.n_ops} op rows, {st.n_changes} changes")
    for name, ts in times.items():
        print(f"{name:32s} calls {len(ts):2d}  median {statistics.median(ts):8.3f} ms  max {max(ts):8.3f} ms   [{' '.join(f'{t:.3f}' for t in ts)}]")
    print("resident counters (served, fell back, in place) added:", tuple(x - y for x, y in zip(after, before)),
          "" if a.remote else f"local_change_calls {eng.local_change_calls()}",
          f"local_small_calls {eng.local_small_calls()}" if hasattr(eng._L, "am355_local_small_calls") else "")
    eng.close()


if __name__ == "__main__":
    main()
