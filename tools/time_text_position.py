"""What resolving elemIds of a Text to positions costs: on the engine (am355_text_position: a search in the stored list order, deleted
elements included) against what a caller of the library could do before -- am355_fetch_ir (the record tables to the host) and a numpy
fold of the edit records into (elemId -> index) for the VISIBLE elements. The fold cannot answer for a deleted element at all: the
records do not hold it. Host to host through the C ABI, one process, one GPU, two contexts that hold the same document, one per route,
alternating; for the queried (visible) elements the two routes must agree every time. Every shape is run twice (`--runs`) so that the
spread between two runs of the same code stands beside the difference between the routes.

On the headline document (c4_text_single), elements spread over the whole Text:
  n = 0 (the heads pass and the length alone), 1, 16 and 100,000 queries
  -- each with the whole-document edit tables fresh (an untimed read in front), and
  -- directly behind a one-change apply_changes merged in place: the rebuild of the stale edit tables (ensure_ir_fresh) is inside both
     routes; the row -> position table is current there (the in-place merge keeps it), behind a full replay the first call builds it.
The engine's time is that of the C call with the (counter, rank) pairs prepared; the wrapper Engine.text_positions (id strings parsed,
ranks asked per call) is timed beside it for 1 and 16 queries.

    python tools/time_text_position.py [--lib libam355.so] [--reps 7] [--runs 2] [--scale 1.0]
"""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from automerge_classic_amd import engine, loggen  # noqa: E402
from automerge_classic_amd.loggen import ChangeLog  # noqa: E402
from time_text_read import EDIT, OBJ, PatchIR, fetch, med, text_id, timed, view  # noqa: E402

SIZES = (0, 1, 16, 100000)


def positions_by_fold(eng, ir, ctr, actor, q_ctr, q_actor):
    """fetch_ir + the fold: every visible element's (actor, counter) key with its index, sorted, the queries looked up. -1: not visible."""
    fetch(eng, ir)
    off = view(ir.actor_off, ir.n_actors + 1, np.dtype("<u4"))
    raw = view(ir.actor_bytes, int(off[-1]), np.dtype("u1")).tobytes()
    actors = [raw[off[k]:off[k + 1]] for k in range(ir.n_actors)]
    obj = view(ir.objects, ir.n_objects, OBJ)
    oi = int(np.nonzero((obj["id_ctr"] == ctr) & (obj["id_actor"] == actors.index(actor)))[0][-1])
    eb, ee = int(obj["edit_begin"][oi]), int(obj["edit_end"][oi])
    e = view(ir.edits, ir.n_edits + 1, EDIT)[eb:ee + 1]
    rec = e[:-1]
    counts = np.diff(e["first"]).astype(np.int64)
    length = int(rec["index"][-1] + counts[-1]) if len(rec) else 0
    starts = np.cumsum(counts) - counts
    within = np.arange(int(counts.sum()), dtype=np.int64) - np.repeat(starts, counts)
    keys = np.repeat((rec["elem_actor"].astype(np.int64) << 32) | rec["elem_ctr"].astype(np.int64), counts) + within
    index = np.repeat(rec["index"].astype(np.int64), counts) + within   # (an update record repeats the key and the index of the value it replaces)
    order = np.argsort(keys, kind="stable")
    keys, index = keys[order], index[order]
    want = (q_actor.astype(np.int64) << 32) | q_ctr.astype(np.int64)
    at = np.searchsorted(keys, want)
    at[at >= len(keys)] = 0
    return np.where(keys[at] == want, index[at], -1) if len(keys) else np.full(len(want), -1), length


def session(lib, log, reps, tail):
    changes = log.changes()
    head, rest = changes[:len(changes) - tail], changes[len(changes) - tail:]
    engines = []
    for _ in range(2):
        eng = engine.Engine(0, lib)
        for sw in ("set_resident_new_actors", "set_resident_new_objects", "set_resident_counters", "set_local_small"):
            getattr(eng, sw)(True)
        eng.apply_changes(ChangeLog.from_changes(head))
        engines.append(eng)
    a, b = engines
    ir = PatchIR()
    oid = text_id(a)
    ctr, actor = int(oid.split("@")[0]), bytes.fromhex(oid.split("@")[1])
    buf = (ctypes.c_uint8 * len(actor)).from_buffer_copy(actor)
    st = a.stats()
    runs, length = a.text_locate(oid, 0, a.text_locate(oid, 0, 0)[1])
    # the elements of the Text at the time of the first query (later changes add a few; the queried ones stay where an editor's would)
    elem_ctr = np.concatenate([np.arange(int(r["elem_ctr"]), int(r["elem_ctr"]) + int(r["count"]), dtype=np.uint32) for r in runs]) if len(runs) else np.zeros(0, np.uint32)
    elem_actor = np.repeat(runs["elem_actor"], runs["count"]).astype(np.uint32)
    print(f"## {st.n_ops} ops, {st.n_changes} changes, Text {oid[:10]}... of {length} elements in {len(runs)} runs")
    t = {}
    rows = []

    def call(eng, q):
        p, ln = ctypes.c_void_p(), ctypes.c_uint64()
        eng._check(eng._L.am355_text_position(eng._h, ctr, ctypes.cast(buf, ctypes.c_void_p), len(actor), q.ctypes.data if len(q) else None, len(q), ctypes.byref(p), ctypes.byref(ln)))
        out = np.zeros(len(q), dtype=engine.ELEM_POS_DTYPE)
        if len(q):
            ctypes.memmove(out.ctypes.data, p, len(q) * engine.ELEM_POS_DTYPE.itemsize)
        return out, int(ln.value)

    def one(n, behind_apply, n_reps):
        n = min(n, len(elem_ctr))
        pick = (np.arange(n, dtype=np.int64) * max(1, len(elem_ctr) // max(n, 1)) + (len(elem_ctr) // (2 * max(n, 1)))) % max(len(elem_ctr), 1) if n else np.zeros(0, np.int64)
        q = np.zeros(n, dtype=engine.ELEM_ID_DTYPE)
        q["ctr"], q["actor"] = elem_ctr[pick], elem_actor[pick]
        ids = [f"{int(c)}@{a.actor_of_rank(int(r))}" for c, r in zip(q["ctr"], q["actor"])] if 0 < n <= 16 else None
        key_a, key_b, key_w = (n, behind_apply, "engine"), (n, behind_apply, "fold"), (n, behind_apply, "wrapper")
        for k in (key_a, key_b, key_w):
            t.setdefault(k, [])
        launches = 0
        for _ in range(n_reps):
            if behind_apply:
                c = rest.pop(0)
                for eng in (a, b):
                    eng.apply_changes(ChangeLog.from_changes([c]))
            else:
                for eng in (a, b):
                    eng.object_text(oid)   # (untimed: the edit tables are fresh for both routes)
            before = a.text_position_calls()[1]
            ta, (got, length_a) = timed(lambda: call(a, q))
            launches = a.text_position_calls()[1] - before
            tb, (want, length_b) = timed(lambda: positions_by_fold(b, ir, ctr, actor, q["ctr"], q["actor"]))
            assert length_a == length_b, (length_a, length_b)
            vis = (got["status"] & 3) == engine.POS_VISIBLE
            assert np.array_equal(np.where(vis, got["position"].astype(np.int64), -1), want), f"{n} queries: the two routes disagree"
            t[key_a].append(ta)
            t[key_b].append(tb)
            if ids and not behind_apply:
                t[key_w].append(timed(lambda: a.text_positions(oid, ids))[0])
        tag = "behind an in-place apply_changes" if behind_apply else "tables fresh"
        print(f"{n:7d} queries, {tag}: {launches} launches")
        print(f"    am355_text_position                  {med(t[key_a])}")
        if t[key_w]:
            print(f"      Engine.text_positions (wrapper)    {med(t[key_w])}")
        print(f"    fetch_ir + fold (visible only)       {med(t[key_b])}")
        rows.extend([statistics.median(t[key_a]), statistics.median(t[key_b])])

    first = timed(lambda: call(a, np.zeros(0, dtype=engine.ELEM_ID_DTYPE)))[0]
    print(f"the first call of the context (builds the row -> position table, allocates): {first:8.3f} ms")
    for n in SIZES:
        one(n, False, reps if n < 1000 else 3)
    for n in SIZES:
        one(n, True, reps if n < 1000 else 2)
    print(f"resident_counters of the asked context (served, fell back, in place): {a.resident_counters()}; text_position_calls {a.text_position_calls()}")
    return a, b, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=engine.DEFAULT_LIB)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0)
    arg = ap.parse_args()
    print(f"# {os.path.basename(arg.lib)}: elemIds of a Text to positions, am355_text_position against am355_fetch_ir + a numpy fold, alternating; scale {arg.scale}")
    log = loggen.config("c4_text_single", arg.scale, False)
    all_rows = []
    for run in range(arg.runs):
        print(f"# run {run + 1}")
        a, b, rows = session(arg.lib, log, arg.reps, 4 * arg.reps + 8)
        all_rows.append(rows)
        a.close()
        b.close()
    print(f"## medians per run, ms, am355_text_position | fetch_ir + fold, for {SIZES} queries with fresh tables, then behind an in-place apply_changes")
    for run, row in enumerate(all_rows):
        print(f"run {run + 1}  " + "  ".join(f"{x:8.3f}" for x in row))


if __name__ == "__main__":
    main()
