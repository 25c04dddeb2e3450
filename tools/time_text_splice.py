"""What an edit of a Text BY POSITION costs: on the engine (am355_text_splice: positions resolved to ids on the device, the change built
and applied) against what a caller could do before with the same library -- am355_fetch_ir (the record tables to the host), a numpy
fold of the edit records to find the elemIds and preds, the request built in Python, am355_apply_local_change. Host to host through
the C ABI, one process, one GPU, two contexts that hold the same document and take the same edits, one by each route, alternating; the
two routes must return the same binary change every time. Every shape is run twice (`--runs`) so that the spread between two runs of
the same code stands beside the difference between the routes.

On the headline document (c4_text_single, 1,020,801 ops), positions in the middle of the Text:
  (a) one character typed            (b) 3 deleted + 3 inserted            (c) 100,000 characters deleted
  -- each with the whole-document edit tables fresh (an untimed read in front), and
  (d) the same three directly behind a one-change apply_changes merged in place: the rebuild of the stale edit tables (ensure_ir_fresh)
      is inside both routes.
The locate half is timed by itself (am355_text_locate of the same range, tables fresh); `--trace 1` adds one call per shape with
AM355_TRACE=1, whose laps (text_splice: located / request built / applied) go to stderr.

    python tools/time_text_splice.py [--lib libam355.so] [--reps 7] [--runs 2] [--scale 1.0] [--trace 0]
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

AUTHOR = "e5" * 16


def ids_of(ir, ctr, actor, first, n):
    """(elem_ctr, elem_actor, pred_ctr, pred_actor) of the elements [first, first + n) and the Text's length, by the rule of
    csrc/am355_locate.hip over the host's copy of the record tables: the last record with index <= j holds both ids."""
    off = view(ir.actor_off, ir.n_actors + 1, np.dtype("<u4"))
    raw = view(ir.actor_bytes, int(off[-1]), np.dtype("u1")).tobytes()
    actors = [raw[off[k]:off[k + 1]] for k in range(ir.n_actors)]
    obj = view(ir.objects, ir.n_objects, OBJ)
    oi = int(np.nonzero((obj["id_ctr"] == ctr) & (obj["id_actor"] == actors.index(actor)))[0][-1])
    eb, ee = int(obj["edit_begin"][oi]), int(obj["edit_end"][oi])
    e = view(ir.edits, ir.n_edits + 1, EDIT)[eb:ee + 1]
    rec = e[:-1]
    length = int(rec["index"][-1] + (e["first"][-1] - rec["first"][-1])) if len(rec) else 0
    j = np.arange(first, first + n, dtype=np.int64)
    hi = np.searchsorted(rec["index"], j, side="right") - 1
    d = j - rec["index"][hi]
    return (rec["elem_ctr"][hi] + d, rec["elem_actor"][hi], rec["id_ctr"][hi] + d, rec["id_actor"][hi]), length, actors


def request_by_fold(eng, ir, oid, start, deletions, values, time):
    """fetch_ir + the fold + context.splice's rule (frontend/context.js:441-502): the request am355_text_splice builds on the device"""
    fetch(eng, ir)
    ctr, actor = int(oid.split("@")[0]), bytes.fromhex(oid.split("@")[1])
    lead = 1 if start else 0
    (ec, ea, pc, pa), length, actors = ids_of(ir, ctr, actor, start - lead, deletions + lead)
    assert start + deletions <= length
    ops = []
    if deletions:
        dec, dea, dpc, dpa = ec[lead:], ea[lead:], pc[lead:], pa[lead:]
        head = np.ones(deletions, dtype=bool)
        head[1:] = ~((dea[1:] == dea[:-1]) & (dec[1:] == dec[:-1] + 1) & (dpa[1:] == dpa[:-1]) & (dpc[1:] == dpc[:-1] + 1))
        at = np.nonzero(head)[0]
        counts = np.diff(np.append(at, deletions))
        for k, n in zip(at, counts):
            op = {"action": "del", "obj": oid, "elemId": f"{int(dec[k])}@{actors[dea[k]].hex()}", "insert": False, "pred": [f"{int(dpc[k])}@{actors[dpa[k]].hex()}"]}
            if n > 1:
                op["multiOp"] = int(n)
            ops.append(op)
    if values:
        op = {"action": "set", "obj": oid, "elemId": f"{int(ec[0])}@{actors[ea[0]].hex()}" if lead else "_head", "insert": True}
        if len(values) > 1:
            op["values"] = list(values)
        else:
            op["value"] = values[0]
        op["pred"] = []
        ops.append(op)
    clock = dict(zip(view(ir.clock_actor, ir.n_clock, np.dtype("<u4")).tolist(), view(ir.clock_seq, ir.n_clock, np.dtype("<u8")).tolist()))
    me = actors.index(bytes.fromhex(AUTHOR)) if bytes.fromhex(AUTHOR) in actors else None
    heads = view(ir.heads, 32 * ir.n_heads, np.dtype("u1")).tobytes()
    # (the deps are the heads: apply_local_change adds the author's last hash itself and keeps every hash once)
    return {"actor": AUTHOR, "seq": int(clock.get(me, 0)) + 1, "startOp": int(ir.max_op) + 1, "time": time, "message": "",
            "deps": [heads[32 * k:32 * k + 32].hex() for k in range(ir.n_heads)], "ops": ops}


SHAPES = (("(a) one character typed", 0, ["x"]), ("(b) 3 deleted + 3 inserted", 3, ["a", "b", "c"]), ("(c) 100,000 deleted", 100000, []))


def session(lib, log, reps, tail):
    """Two contexts built by apply_changes (the in-place paths serve what follows); `tail` changes of the log are kept back and fed one
    per call for (d)."""
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
    st = a.stats()
    length = a.text_locate(oid, 0, 0)[1]
    print(f"## {st.n_ops} ops, {st.n_changes} changes, Text {oid[:10]}... of {length} elements")
    t = {}
    clock = [0]

    def one(label, asked, values, behind_apply, n_reps):
        deletions = asked
        key_a, key_b, key_l = (label, "splice"), (label, "fold"), (label, "locate")
        for k in (key_a, key_b, key_l):
            t.setdefault(k, [])
        for _ in range(n_reps):
            clock[0] += 1
            n = a.text_locate(oid, 0, 0)[1]
            start = n // 2
            deletions = min(deletions, n // 4)   # (only smaller than asked for at a reduced --scale)
            if behind_apply:
                c = rest.pop(0)
                for eng in (a, b):
                    eng.apply_changes(ChangeLog.from_changes([c]))
            else:
                for eng in (a, b):
                    eng.object_text(oid)   # (untimed: the edit tables are fresh for both routes)
                t[key_l].append(timed(lambda: a.text_locate(oid, start - 1, deletions + 1))[0])
            before = a.text_splice_calls()[2]
            ta, got = timed(lambda: a.text_splice(oid, start, deletions, values, AUTHOR, time=clock[0]))
            launches = a.text_splice_calls()[2] - before
            tb, want = timed(lambda: b.apply_local_change(request_by_fold(b, ir, oid, start, deletions, values, clock[0])))
            assert got == want, f"{label}: the two routes made different changes"
            t[key_a].append(ta)
            t[key_b].append(tb)
        tag = " behind an in-place apply_changes" if behind_apply else ""
        print(f"{label}{tag}: change of {len(got)} bytes, {launches} launches of the locate half")
        print(f"    text_splice                          {med(t[key_a])}")
        if t[key_l]:
            print(f"      of which am355_text_locate alone   {med(t[key_l])}")
        print(f"    fetch_ir + fold + apply_local_change {med(t[key_b])}")
        return statistics.median(t[key_a]), statistics.median(t[key_b])

    row = []
    for label, deletions, values in SHAPES:
        row += one(label, deletions, values, False, reps if deletions < 1000 else 3)
    for label, deletions, values in SHAPES:
        row += one("(d) " + label[4:], deletions, values, True, reps if deletions < 1000 else 2)
    served = a.resident_counters()
    print(f"resident_counters of the text_splice context (served, fell back, in place): {served}; local_small_calls {a.local_small_calls()}; "
          f"text_splice_calls {a.text_splice_calls()}")
    assert a.object_text(oid)[0] == b.object_text(oid)[0]
    return a, b, oid, row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=engine.DEFAULT_LIB)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--trace", type=int, default=0)
    arg = ap.parse_args()
    print(f"# {os.path.basename(arg.lib)}: a Text edited by position, am355_text_splice against am355_fetch_ir + a numpy fold + am355_apply_local_change, "
          f"alternating; scale {arg.scale}")
    log = loggen.config("c4_text_single", arg.scale, False)
    rows = []
    for run in range(arg.runs):
        print(f"# run {run + 1}")
        a, b, oid, row = session(arg.lib, log, arg.reps, 2 * arg.reps + 8)
        rows.append(row)
        if arg.trace and run + 1 == arg.runs:
            print("# one call per shape with AM355_TRACE=1 (laps on stderr)", flush=True)
            os.environ["AM355_TRACE"] = "1"
            for label, deletions, values in SHAPES:
                print(f"# traced: {label}", file=sys.stderr, flush=True)
                n = a.text_locate(oid, 0, 0)[1]
                a.text_splice(oid, n // 2, min(deletions, n // 4), values, AUTHOR, time=999)
            del os.environ["AM355_TRACE"]
        a.close()
        b.close()
    print("## medians per run, ms, text_splice | fetch_ir + fold + apply_local_change, for (a) (b) (c) with fresh tables, then (d) behind an in-place apply_changes")
    for run, row in enumerate(rows):
        print(f"run {run + 1}  " + "  ".join(f"{x:8.3f}" for x in row))


if __name__ == "__main__":
    main()
