"""What an edit of a MAP by key costs: on the engine (am355_map_update / am355_map_locate: keys resolved to the records of their visible
values on the device, the change built and applied) against what a caller could do before with the same library -- am355_fetch_ir (the
record tables to the host), a host bisect over the map table in its own order, the request built in Python, am355_apply_local_change.
Host to host through the C ABI, one process, one GPU, two contexts that hold the same document and take the same edits, one by each
route, alternating; the two routes must return the same binary change every time. Every shape is run twice (`--runs`) so that the
spread between two runs of the same code stands beside the difference between the routes.

Documents:
  (T) the headline Text (c4_text_single) with 1,000 keys and a counter on _root: one key set, one increment, both in one change -- fresh
      (an untimed read of the Text in front: no stale edit table for either route), and directly behind a keystroke of another actor
      merged in place (the edit tables are stale: the map call does not rebuild them, fetch_ir does);
  (M) c3_map_lww (10,000 keys) with 10,000 more keys on _root: 1 key and 64 keys set per call (no Text to read in front: fetch_ir pays
      for the edit tables the call before left stale, as a caller's would);
  (G) a generated map of ~1,000,000 keys: map_locate of 1, 64 and 100,000 keys, one wavefront per key against one thread per key
      (am355_set_map_locate_thread), and fetch_ir + the host bisect for the same keys.

    python tools/time_map_update.py [--lib libam355.so] [--reps 7] [--runs 2] [--scale 1.0] [--docs T,M,G]
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from automerge_classic_amd import engine, loggen  # noqa: E402
from automerge_classic_amd.loggen import ChangeLog  # noqa: E402
from time_text_read import OBJ, PatchIR, fetch, med, text_id, timed, view  # noqa: E402

AUTHOR, TYPIST, MAKER = "e5" * 16, "d4" * 16, "1a" * 16
_ORDER = bytes(x - 2 if 0xF0 <= x <= 0xF4 else x + 5 if x in (0xEE, 0xEF) else x for x in range(256))   # utf16_order_byte (csrc/am355_rows.h)


def host_locate(ir, keys):
    """fetch_ir's tables: per key the records of _root that hold it, by a bisect over the map table in its own order"""
    obj = view(ir.objects, ir.n_objects, OBJ)
    recs = view(ir.map, ir.n_map, engine.IR_MAP_DTYPE)
    arena = view(ir.arena, ir.arena_len, np.dtype("u1"))
    begin, end = int(obj["map_begin"][0]), int(obj["map_end"][0])
    koff, klen = recs["key_off"], recs["key_len"]
    key_at = lambda r: arena[int(koff[r]):int(koff[r]) + int(klen[r])].tobytes().translate(_ORDER)   # noqa: E731
    out = []
    for key in keys:
        q = key.encode("utf-8").translate(_ORDER)
        lo, hi = begin, end
        while lo < hi:
            mid = (lo + hi) // 2
            if key_at(mid) < q:
                lo = mid + 1
            else:
                hi = mid
        ub = lo
        while ub < end and key_at(ub) == q:
            ub += 1
        out.append(recs[lo:ub])
    return out


def request_by_fold(eng, ir, ops, time):
    """fetch_ir + the bisect + context.js's rules (setMapKey :325-346, increment :546-573): the request the engine builds on the device"""
    fetch(eng, ir)
    off = view(ir.actor_off, ir.n_actors + 1, np.dtype("<u4"))
    raw = view(ir.actor_bytes, int(off[-1]), np.dtype("u1")).tobytes()
    actors = [raw[off[k]:off[k + 1]] for k in range(ir.n_actors)]
    out = []
    for op, held in zip(ops, host_locate(ir, [op[1] for op in ops])):
        preds = [f"{int(r['id_ctr'])}@{actors[int(r['id_actor'])].hex()}" for r in held[::-1]]
        if op[0] == "set":
            out.append({"action": "set", "obj": "_root", "key": op[1], "insert": False, "value": op[2], "datatype": "int", "pred": preds})
        else:
            out.append({"action": "inc", "obj": "_root", "key": op[1], "insert": False, "value": op[2], "pred": preds})
    clock = dict(zip(view(ir.clock_actor, ir.n_clock, np.dtype("<u4")).tolist(), view(ir.clock_seq, ir.n_clock, np.dtype("<u8")).tolist()))
    me = actors.index(bytes.fromhex(AUTHOR)) if bytes.fromhex(AUTHOR) in actors else None
    heads = view(ir.heads, 32 * ir.n_heads, np.dtype("u1")).tobytes()
    return {"actor": AUTHOR, "seq": int(clock.get(me, 0)) + 1, "startOp": int(ir.max_op) + 1, "time": time, "message": "",
            "deps": [heads[32 * k:32 * k + 32].hex() for k in range(ir.n_heads)], "ops": out}


def twins(lib):
    a, b = engine.Engine(0, lib), engine.Engine(0, lib)
    for eng in (a, b):
        for sw in ("set_resident_new_actors", "set_resident_new_objects", "set_resident_counters", "set_resident_map_merge", "set_local_small"):
            getattr(eng, sw)(True)
    return a, b


def root_keys_change(eng, n_keys, max_op, deps):
    ops = [{"action": "set", "obj": "_root", "key": "votes", "insert": False, "value": 0, "datatype": "counter", "pred": []}]
    ops += [{"action": "set", "obj": "_root", "key": f"key{j:07d}", "insert": False, "value": j, "datatype": "int", "pred": []} for j in range(n_keys)]
    return eng.encode_change({"actor": MAKER, "seq": 1, "startOp": max_op + 1, "time": 0, "message": "", "deps": deps, "ops": ops})[0]


def heads_of(eng):
    import json
    p = json.loads(eng.patch_json())
    return p["maxOp"], p["deps"]


def update_session(lib, base, n_keys, shapes, reps, with_text):
    """shapes: [(label, ops(k) -> [("set", key, int) | ("inc", key, delta)])]; every shape fresh and, with_text, behind a keystroke"""
    a, b = twins(lib)
    for eng in (a, b):
        eng.apply_changes(base)
    if n_keys:
        max_op, deps = heads_of(a)
        extra = root_keys_change(a, n_keys, max_op, deps)
        for eng in (a, b):
            eng.apply_changes(ChangeLog.from_changes([extra]))
    text = text_id(a) if with_text else None
    ir, row, clock = PatchIR(), [], [0]
    st = a.stats()
    print(f"## {st.n_ops} ops, {st.n_changes} changes, {st.n_map_values} map values")

    def one(label, make_ops, behind):
        ts = {"engine": [], "fold": []}
        for _ in range(reps):
            clock[0] += 1
            ops = make_ops(clock[0])
            if behind:
                for eng in (a, b):
                    typed = eng.text_splice(text, 10 + clock[0], 1, ["x"], TYPIST, time=clock[0])
                assert typed
            elif text:
                for eng in (a, b):
                    eng.text_locate(text, 0, 0)   # (untimed: edit tables the last call left stale are rebuilt for both routes before the clocks start)
            before = a.map_calls()[2]
            ta, got = timed(lambda: a.map_update("_root", ops, AUTHOR, time=clock[0]))
            launches = a.map_calls()[2] - before
            tb, want = timed(lambda: b.apply_local_change(request_by_fold(b, ir, ops, clock[0])))
            assert got == want, f"{label}: the two routes made different changes"
            ts["engine"].append(ta)
            ts["fold"].append(tb)
        tag = " behind an in-place Text merge" if behind else ""
        print(f"{label}{tag}: change of {len(got)} bytes, {launches} launches of the locate half")
        print(f"    map_update                             {med(ts['engine'])}")
        print(f"    fetch_ir + bisect + apply_local_change {med(ts['fold'])}")
        row.extend([statistics.median(ts["engine"]), statistics.median(ts["fold"])])

    for label, make_ops in shapes:
        one(label, make_ops, False)
    if with_text:
        for label, make_ops in shapes:
            one(label, make_ops, True)
    print(f"resident_counters (served, fell back, in place): {a.resident_counters()}; map merged in place {a.resident_map_merge_calls()}; counters in place "
          f"{a.resident_counter_calls()}; local_small_calls {a.local_small_calls()}; map_calls {a.map_calls()}")
    assert a.patch_json() == b.patch_json()
    a.close()
    b.close()
    return row


def locate_session(lib, n_keys, reps):
    """(G): map_locate on a generated map, wavefront per key against thread per key on one context, fetch_ir + bisect on its twin"""
    a, b = twins(lib)
    per, changes, max_op, deps = 125_000, [], 0, []
    for c in range(max(1, n_keys // per)):
        ops = [{"action": "set", "obj": "_root", "key": f"key{j:07d}", "insert": False, "value": j, "datatype": "int", "pred": []}
               for j in range(c * per, min(n_keys, (c + 1) * per))]
        change, digest = a.encode_change({"actor": MAKER, "seq": c + 1, "startOp": max_op + 1, "time": 0, "message": "", "deps": deps, "ops": ops})
        changes.append(change)
        max_op, deps = max_op + len(ops), [digest.hex()]
    for eng in (a, b):
        eng.load_changes(ChangeLog.from_changes(changes))
        eng.replay()
    total = min(n_keys, max(1, n_keys // per) * per)
    print(f"## a map of {a.stats().n_map_values} values")
    rng = np.random.default_rng(7)
    ir, row = PatchIR(), []
    fetch(b, ir)
    for n in (1, 64, 100_000):
        n = min(n, total)
        ts = {"wave": [], "thread": [], "host": []}
        for _ in range(reps):
            keys = [f"key{j:07d}" for j in rng.integers(0, total, n)]
            for mode in ("wave", "thread"):
                a.set_map_locate_thread(mode == "thread")
                t, (hits, recs) = timed(lambda: a.map_locate("_root", keys))
                assert int(hits["num"].sum()) == n == len(recs)
                ts[mode].append(t)
            if n <= 64:
                t, held = timed(lambda: (fetch(b, ir), host_locate(ir, keys))[1])
                assert sum(len(h) for h in held) == n
                ts["host"].append(t)
        a.set_map_locate_thread(False)
        print(f"map_locate of {n} keys (the binding's copies of keys and records included)")
        print(f"    one wavefront per key                  {med(ts['wave'])}")
        print(f"    one thread per key                     {med(ts['thread'])}")
        if ts["host"]:
            print(f"    fetch_ir (tables on the host) + bisect {med(ts['host'])}")
        row.extend([statistics.median(ts["wave"]), statistics.median(ts["thread"])])
    a.close()
    b.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=engine.DEFAULT_LIB)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--docs", default="T,M,G")
    arg = ap.parse_args()
    print(f"# {os.path.basename(arg.lib)}: a map edited by key, am355_map_update against am355_fetch_ir + a host bisect + am355_apply_local_change, "
          f"alternating; scale {arg.scale}")
    key = lambda k, n: f"key{(k * 7919) % n:07d}"   # noqa: E731
    for doc in arg.docs.split(","):
        rows = []
        for run in range(arg.runs):
            print(f"# document {doc}, run {run + 1}")
            if doc == "T":
                n = max(16, int(1000 * arg.scale))
                shapes = [("(a) one key set", lambda k: [("set", key(k, n), k)]), ("(b) one increment", lambda k: [("inc", "votes", 1)]),
                          ("(c) a key set and an increment", lambda k: [("set", key(k, n), k), ("inc", "votes", 2)])]
                rows.append(update_session(arg.lib, loggen.config("c4_text_single", arg.scale, False), n, shapes, arg.reps, True))
            elif doc == "M":
                n = max(80, int(10_000 * arg.scale))
                shapes = [("(a) one key set", lambda k: [("set", key(k, n), k)]), ("(b) 64 keys set", lambda k: [("set", key(64 * k + j, n), k) for j in range(64)])]
                rows.append(update_session(arg.lib, loggen.config("c3_map_lww", arg.scale, False), n, shapes, arg.reps, False))
            else:
                rows.append(locate_session(arg.lib, max(1000, int(1_000_000 * arg.scale)), arg.reps))
        what = {"T": "map_update | host route: (a) (b) (c) fresh, then (a) (b) (c) behind an in-place Text merge", "M": "map_update | host route: (a) (b)",
                "G": "wavefront per key | thread per key: 1, 64, 100,000 keys"}[doc]
        print(f"## medians per run, ms, {what}")
        for run, row in enumerate(rows):
            print(f"run {run + 1}  " + "  ".join(f"{x:8.3f}" for x in row))


if __name__ == "__main__":
    main()
