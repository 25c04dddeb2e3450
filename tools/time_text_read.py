"""What reading the string of a Text costs: on the device (am355_object_text: the edit records gathered in HBM, the string copied down)
against what a caller could do before -- am355_fetch_ir (the three record tables to the host) and a fold of the edit records in numpy,
the same rule vectorised. Host to host through the C ABI, one process, one GPU, the two alternating; every shape is run twice
(`--runs`) so that the spread between two runs of the same code stands beside the difference between the two paths.

  (a) object_text   on the headline document (c4_text_single, 1,020,801 ops): behind a replay (the object looked up on the device, the
                    scratch grown) and again (steady)
  (b) fetch_ir + numpy fold of the same state: behind a replay (the tables copied down), and the fold alone
  (c) the same two directly behind a one-change apply_changes merged in place: the rebuild of the stale edit tables is inside both
  (d) (a) and (b) on a document typed character by character (c2_text_typing)
  (e) the gather written straight into pinned memory (am355_set_text_pinned_max) against device memory + one copy, per size

    python tools/time_text_read.py [--lib libam355.so] [--reps 7] [--runs 2] [--scale 1.0]
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


class PatchIR(ctypes.Structure):   # am355_patch_ir (include/am355.h)
    _fields_ = [("n_objects", ctypes.c_uint32), ("n_map", ctypes.c_uint32), ("n_edits", ctypes.c_uint32), ("n_values", ctypes.c_uint32),
                ("objects", ctypes.c_void_p), ("map", ctypes.c_void_p), ("edits", ctypes.c_void_p), ("max_op", ctypes.c_uint64),
                ("n_actors", ctypes.c_uint32), ("actor_off", ctypes.c_void_p), ("actor_bytes", ctypes.c_void_p), ("n_clock", ctypes.c_uint32),
                ("clock_actor", ctypes.c_void_p), ("clock_seq", ctypes.c_void_p), ("n_heads", ctypes.c_uint32), ("heads", ctypes.c_void_p),
                ("pending", ctypes.c_uint32), ("arena", ctypes.c_void_p), ("arena_len", ctypes.c_uint64)]


OBJ = np.dtype([(n, "<u4") for n in ("id_ctr", "id_actor", "type", "map_begin", "map_end", "edit_begin", "edit_end", "make_row")])
EDIT = np.dtype([(n, "<u4") for n in ("flags", "index", "id_ctr", "id_actor", "elem_ctr", "elem_actor", "first", "val_tl", "val_off", "pad")])


def view(ptr, count, dtype):
    return np.frombuffer((ctypes.c_uint8 * (count * dtype.itemsize)).from_address(ptr), dtype=dtype, count=count) if count else np.zeros(0, dtype)


def fold(ir, ctr, rank):
    """The rule of csrc/am355_text.hip over the host's copy of the record tables (values that begin with U+FEFF are not looked for:
    the documents timed here hold none)."""
    obj = view(ir.objects, ir.n_objects, OBJ)
    oi = int(np.nonzero((obj["id_ctr"] == ctr) & (obj["id_actor"] == rank))[0][-1])
    eb, ee = int(obj["edit_begin"][oi]), int(obj["edit_end"][oi])
    e = view(ir.edits, ir.n_edits + 1, EDIT)[eb:ee + 1]
    rec, nxt = e[:-1], e[1:]
    count = nxt["first"] - rec["first"]
    over = ((nxt["flags"] & 1) != 0) & (nxt["index"] == rec["index"] + count - 1)
    over[-1] = False
    live = np.where(rec["flags"] & 8, 0, count - over)
    is_str = ((rec["flags"] & (4 | 8 | 32)) == 0) & ((rec["val_tl"] & 15) == 6)
    nb = np.where(is_str, live.astype(np.int64) * (rec["val_tl"] >> 4), 0)
    end = np.cumsum(nb)
    total = int(end[-1]) if end.size else 0
    arena = view(ir.arena, ir.arena_len, np.dtype("u1"))
    src = np.repeat(rec["val_off"].astype(np.int64) - (end - nb), nb) + np.arange(total, dtype=np.int64)
    return arena[src].tobytes(), int(live.sum())


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return 1e3 * (time.perf_counter() - t0), r


def med(ts):
    return f"median {statistics.median(ts):8.3f} ms  min {min(ts):8.3f}  max {max(ts):8.3f}"


def text_id(eng):
    """the first Text of the document, from the patch"""
    import json
    stack = [json.loads(eng.patch_json())["diffs"]]
    while stack:
        d = stack.pop()
        if d["type"] == "text":
            return d["objectId"]
        for values in d.get("props", {}).values():
            stack.extend(v for v in values.values() if "objectId" in v)
    raise RuntimeError("no Text in the document")


def fetch(eng, ir):
    eng._check(eng._L.am355_fetch_ir(eng._h, ctypes.byref(ir)))


def rank_of(ir, actor):
    off = view(ir.actor_off, ir.n_actors + 1, np.dtype("<u4"))
    raw = view(ir.actor_bytes, int(off[-1]), np.dtype("u1")).tobytes()
    return [raw[off[k]:off[k + 1]] for k in range(ir.n_actors)].index(actor)


def document(lib, name, log, reps, tail_calls):
    """(a), (b) and -- tail_calls > 0 -- (c) on one document. The last tail_calls changes of the log are applied one per call."""
    changes = log.changes()
    head = changes[:len(changes) - tail_calls] if tail_calls else changes
    eng = engine.Engine(0, lib)
    ir = PatchIR()
    eng.load_changes(ChangeLog.from_changes(head))
    eng.replay()
    oid = text_id(eng)
    ctr, actor = int(oid.split("@")[0]), bytes.fromhex(oid.split("@")[1])
    fetch(eng, ir)
    rank = rank_of(ir, actor)
    want, info = eng.object_text(oid)
    got, n = fold(ir, ctr, rank)
    assert got == want and n == info.n_elements, "the numpy fold and the device read differ"
    st = eng.stats()
    print(f"## {name}: {st.n_ops} ops, {st.n_changes} changes, {ir.n_edits} edit records, Text of {info.n_elements} elements, {len(want)} bytes")
    t = {k: [] for k in ("text_first", "text_again", "ir_first", "fold", "ir_again")}
    for _ in range(reps):   # alternating, each behind a replay of its own
        eng.replay()
        t["text_first"].append(timed(lambda: eng.object_text(oid))[0])
        t["text_again"].append(timed(lambda: eng.object_text(oid))[0])
        eng.replay()
        a = timed(lambda: fetch(eng, ir))[0]
        b = timed(lambda: fold(ir, ctr, rank))[0]
        t["ir_first"].append(a + b)
        t["fold"].append(b)
        t["ir_again"].append(timed(lambda: (fetch(eng, ir), fold(ir, ctr, rank)))[0])
    print(f"(a) object_text behind a replay       {med(t['text_first'])}")
    print(f"(a) object_text again                 {med(t['text_again'])}")
    print(f"(b) fetch_ir + fold behind a replay   {med(t['ir_first'])}")
    print(f"(b)   of which the numpy fold         {med(t['fold'])}")
    print(f"(b) fetch_ir (cached) + fold again    {med(t['ir_again'])}")
    row = [statistics.median(t[k]) for k in ("text_first", "text_again", "ir_first", "ir_again")]
    if tail_calls:
        eng.close()
        eng = engine.Engine(0, lib)   # (a context whose state Backend.applyChanges built: the next calls are served on it)
        for sw in ("set_resident_new_actors", "set_resident_new_objects", "set_resident_counters"):
            getattr(eng, sw)(True)
        eng.apply_changes(ChangeLog.from_changes(head))
        eng.object_text(oid)
        tc = {"apply": [], "text": [], "ir": []}
        before = eng.resident_counters()
        for k, c in enumerate(changes[len(head):]):
            tc["apply"].append(timed(lambda: eng.apply_changes(ChangeLog.from_changes([c])))[0])
            if k % 2 == 0:
                tc["text"].append(timed(lambda: eng.object_text(oid))[0])
            else:
                tc["ir"].append(timed(lambda: (fetch(eng, ir), fold(ir, ctr, rank_of(ir, actor))))[0])   # (a new author moves the ranks)
        after = eng.resident_counters()
        print(f"(c) {tail_calls} one-change calls: resident_counters (served, fell back, in place) + {tuple(x - y for x, y in zip(after, before))}")
        print(f"(c) apply_changes of one change       {med(tc['apply'])}")
        print(f"(c) object_text behind it             {med(tc['text'])}   (the rebuild of the edit tables inside)")
        print(f"(c) fetch_ir + fold behind it         {med(tc['ir'])}   (the rebuild of the edit tables inside)")
        fetch(eng, ir)
        got, n = fold(ir, ctr, rank_of(ir, actor))
        want, info = eng.object_text(oid)
        assert got == want and n == info.n_elements
        row += [statistics.median(tc["text"]), statistics.median(tc["ir"])]
    eng.close()
    return row


def pinned(lib, reps):
    """(e) the two ways down, per size of the string: one typed run of n characters."""
    print("## (e) gather into pinned memory against device memory + one copy (object_text again, host tables current)")
    for n in (64, 1024, 4096, 16384, 65536, 262144, 1048576):
        log = loggen.generate(loggen.KIND_TEXT_CONCURRENT, n_actors=1, n_rounds=1, ins_per_change=n, del_per_change=0, n_objects=1, seed=3)
        eng = engine.Engine(0, lib)
        eng.load_changes(log)
        eng.replay()
        oid = text_id(eng)
        assert len(eng.object_text(oid)[0]) == n
        t = {0: [], 1: []}
        for _ in range(reps):
            for direct in (0, 1):
                eng.set_text_pinned_max(1 << 30 if direct else 0)
                t[direct].append(timed(lambda: eng.object_text(oid))[0])
        print(f"{n:8d} bytes   device + copy {med(t[0])}   |   pinned {med(t[1])}")
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=engine.DEFAULT_LIB)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0)
    a = ap.parse_args()
    print(f"# {os.path.basename(a.lib)}: the string of a Text, am355_object_text against am355_fetch_ir + a numpy fold, alternating; scale {a.scale}")
    c4 = loggen.config("c4_text_single", a.scale, False)
    c2 = loggen.config("c2_text_typing", a.scale, False)
    rows = []
    for run in range(a.runs):
        print(f"# run {run + 1}")
        rows.append((document(a.lib, "c4_text_single", c4, a.reps, 2 * a.reps), document(a.lib, "c2_text_typing", c2, a.reps, 0)))
        pinned(a.lib, a.reps)
    print("## medians per run, ms: object_text behind a replay | again | fetch_ir + fold behind a replay | again | (c) object_text | (c) fetch_ir + fold")
    for run, (r4, r2) in enumerate(rows):
        print(f"run {run + 1}  c4_text_single  " + "  ".join(f"{x:8.3f}" for x in r4))
        print(f"run {run + 1}  c2_text_typing  " + "  ".join(f"{x:8.3f}" for x in r2))


if __name__ == "__main__":
    main()
