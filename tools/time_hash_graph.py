"""What the membership tests of the hash-graph queries cost on the device and on the engine's host index, host to host through the
C ABI (include/am355.h am355_find_changes / am355_changes_added, am355_set_graph_probe_min), and where the two cross.

Per size n, a context that holds n one-op changes of one actor (loggen KIND_TEXT_TYPING) is asked, alternating device / host:
    find_changes   of all n hashes of the context                   (n probes into the table over the context's hashes)
    changes_added  against an `other` that lacks the last change    (n probes into a table over the n - 1 hashes of `other`)
    changes_since  of the last change but one, after one apply_changes of one change   (the sync message after a keystroke: one probe,
                                                                     the indexes extended by one change)
The first call of each kind on a path is reported apart: it builds the path's table (device: k_graph_insert over all n; host: the
index and the dependents CSR). `--synthetic` times am355_test_hash_probe alone on random hashes -- a table of n and n probes, its own
allocations and uploads included: an upper bound of the device side at sizes no log is generated for.

    python tools/time_hash_graph.py [--lib libam355.so] [--sizes 1000,4000,32000,100000] [--synthetic 1000,...,1000000] [--reps 7]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from automerge_classic_amd import engine, loggen  # noqa: E402
from automerge_classic_amd.loggen import ChangeLog  # noqa: E402

DEVICE, HOST = 1, 0xFFFFFFFF


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def med(ts):
    return f"median {statistics.median(ts):9.3f} ms  min {min(ts):9.3f}  max {max(ts):9.3f}"


def one_size(lib, n, reps):
    changes = loggen.generate(loggen.KIND_TEXT_TYPING, n_ops=n, ops_per_change=1, seed=0x5EED0001).changes()   # n + 1 changes
    eng = engine.Engine(0, lib)
    for sw in ("set_resident_new_actors", "set_resident_new_objects", "set_resident_counters"):
        getattr(eng, sw)(True)
    t_apply = timed(lambda: eng.apply_changes(ChangeLog.from_changes(changes[:-1])))
    hs = np.ascontiguousarray(eng.hashes())
    m = hs.shape[0]
    other = np.ascontiguousarray(hs[: m - 1])
    out = np.zeros(m, dtype=np.uint32)
    p, cnt = ctypes.c_void_p(), ctypes.c_uint32()
    L, h = eng._L, eng._h

    def find():
        eng._check(L.am355_find_changes(h, hs.ctypes.data, m, out.ctypes.data))

    def added():
        eng._check(L.am355_changes_added(h, other.ctypes.data, m - 1, ctypes.byref(p), ctypes.byref(cnt)))
        assert cnt.value == 1

    print(f"## {m} changes (apply_changes of all: {t_apply:.1f} ms)")
    rows = {}
    for kind, fn in (("find_changes", find), ("changes_added", added)):
        first = {}
        for path, name in ((HOST, "host"), (DEVICE, "device")):
            eng.set_graph_probe_min(path)
            first[name] = timed(fn)
        ts = {"host": [], "device": []}
        for _ in range(reps):   # alternating
            for path, name in ((HOST, "host"), (DEVICE, "device")):
                eng.set_graph_probe_min(path)
                ts[name].append(timed(fn))
        for name in ("host", "device"):
            print(f"{kind:14s} {name:6s} first call {first[name]:9.3f} ms   then {med(ts[name])}")
        rows[kind] = (statistics.median(ts["host"]), statistics.median(ts["device"]))
    # the sync message after a keystroke: one more change applied, then getChanges(previous head)
    prev = bytes(hs[m - 1])
    one = ctypes.create_string_buffer(prev, 32)
    for path, name in ((HOST, "host"), (DEVICE, "device")):
        eng.set_graph_probe_min(path)
        if path == HOST:
            eng.apply_changes(ChangeLog.from_changes(changes[-1:]))
            print("   resident counters after the one-change call:", eng.resident_counters())
        ts = []
        for _ in range(reps):
            ts.append(timed(lambda: eng._check(L.am355_changes_since(h, one, 1, ctypes.byref(p), ctypes.byref(cnt)))))
        assert cnt.value == 1
        print(f"changes_since  {name:6s} first call {ts[0]:9.3f} ms   then {med(ts[1:])}   (one probe; first call: indexes extended by the new change"
              f"{', device table extended' if path == DEVICE else ''})")
    print("   graph_query_calls (device, host):", eng.graph_query_calls())
    eng.close()
    return m, rows


def synthetic(lib, n, reps):
    eng = engine.Engine(0, lib)
    rng = np.random.default_rng(n)
    table = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    queries = np.ascontiguousarray(table[rng.permutation(n)])
    out = np.zeros(n, dtype=np.uint32)
    ts = [timed(lambda: eng._check(eng._L.am355_test_hash_probe(eng._h, table.ctypes.data, n, queries.ctypes.data, n, out.ctypes.data))) for _ in range(reps + 1)]
    assert (out != 0xFFFFFFFF).all()
    # the same membership test by a Python dict is no yardstick; the host index is timed on real contexts above
    print(f"test_hash_probe  n = {n:8d}: table built and {n} probes, allocations and uploads included: first {ts[0]:9.3f} ms   then {med(ts[1:])}")
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=engine.DEFAULT_LIB)
    ap.add_argument("--sizes", default="1000,4000,32000,100000")
    ap.add_argument("--synthetic", default="1000,4000,32000,100000,1000000")
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    print(f"# {os.path.basename(a.lib)}: membership tests of the hash-graph queries, device (probe_min 1) against the host index (never), alternating")
    table = []
    for n in [int(x) for x in a.sizes.split(",") if x]:
        table.append(one_size(a.lib, n, a.reps))
    if table:
        print("## medians, host / device, ms")
        for m, rows in table:
            print(f"{m:9d} changes   " + "   ".join(f"{k} {v[0]:.3f} / {v[1]:.3f}" for k, v in rows.items()))
    for n in [int(x) for x in a.synthetic.split(",") if x]:
        synthetic(a.lib, n, a.reps)


if __name__ == "__main__":
    main()
