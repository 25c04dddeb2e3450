"""What an edit of a plain LIST by position costs: on the engine (am355_list_splice / am355_list_set: positions resolved to elemIds and
every pred on the device, the change built and applied) against what a caller could do before with the same library -- am355_fetch_ir
(the record tables to the host), a numpy fold of the edit records (both searches of csrc/am355_list_locate.hip), the request built in
Python, am355_apply_local_change. Host to host through the C ABI, one process, one GPU, two contexts that hold the same document and
take the same edits, one by each route, alternating; the two routes must return the same binary change every time. Every shape is run
twice (`--runs`) so that the spread between two runs of the same code stands beside the difference between the routes.

Documents: (L) one list of 100,000 ints of which 1,000 elements hold two concurrent values; (LT) the same list beside the headline Text
(c4_text_single, 1,020,801 ops). Positions in the middle of the list:
  (a) one element deleted and one inserted   (b) an assignment onto a conflicted element (two preds)   (c) 10,000 elements deleted
  -- each with the whole-document edit tables fresh (an untimed read in front), and
  (d) the same three directly behind a one-change apply_changes merged in place (another actor's insertion at the list's head): the
      rebuild of the stale edit tables (ensure_ir_fresh) is inside both routes.

    python tools/time_list_splice.py [--lib libam355.so] [--reps 7] [--runs 2] [--scale 1.0] [--docs L,LT]
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
from time_text_read import EDIT, OBJ, PatchIR, fetch, med, timed, view  # noqa: E402

AUTHOR = "e5" * 16
ACT_A, ACT_B, ACT_C, ACT_E = "1a" * 16, "2b" * 16, "3c" * 16, "4e" * 16
LIST = f"1@{ACT_A}"
EVERY = 100   # one element in EVERY is conflicted: 50, 150, ...


def list_changes(eng, n, tail):
    """The list's history as binary changes: A makes the list of n ints; B and C assign concurrently to every EVERY-th element; then `tail`
    changes of E, each one insertion at the list's head (kept back by the caller and fed one per call)."""
    first = {"actor": ACT_A, "seq": 1, "startOp": 1, "time": 0, "message": "", "deps": [],
             "ops": [{"action": "makeList", "obj": "_root", "key": "list", "insert": False, "pred": []},
                     {"action": "set", "obj": LIST, "elemId": "_head", "insert": True, "values": list(range(n)), "datatype": "int", "pred": []}]}
    made, digest = eng.encode_change(first)
    dep = digest.hex()
    out = [made]
    for actor in (ACT_B, ACT_C):
        out.append(eng.encode_change({"actor": actor, "seq": 1, "startOp": n + 2, "time": 0, "message": "", "deps": [dep],
                                      "ops": [{"action": "set", "obj": LIST, "elemId": f"{2 + i}@{ACT_A}", "insert": False, "value": f"{actor[:2]}{i}", "pred": [f"{2 + i}@{ACT_A}"]}
                                              for i in range(EVERY // 2, n, EVERY)]})[0])
    late, last = [], dep
    for k in range(tail):
        change, digest = eng.encode_change({"actor": ACT_E, "seq": k + 1, "startOp": 0x10000000 + k, "time": 0, "message": "", "deps": [last],
                                            "ops": [{"action": "set", "obj": LIST, "elemId": "_head", "insert": True, "value": k, "datatype": "int", "pred": []}]})
        late.append(change)
        last = digest.hex()
    return out, late


def elements_of(ir, first, n):
    """elemIds, preds and shown-counter bits of the elements [first, first + n) of LIST and its length, by the rule of
    csrc/am355_list_locate.hip over the host's copy of the record tables."""
    off = view(ir.actor_off, ir.n_actors + 1, np.dtype("<u4"))
    raw = view(ir.actor_bytes, int(off[-1]), np.dtype("u1")).tobytes()
    actors = [raw[off[k]:off[k + 1]] for k in range(ir.n_actors)]
    obj = view(ir.objects, ir.n_objects, OBJ)
    oi = int(np.nonzero((obj["id_ctr"] == 1) & (obj["id_actor"] == actors.index(bytes.fromhex(ACT_A))))[0][-1])
    eb, ee = int(obj["edit_begin"][oi]), int(obj["edit_end"][oi])
    e = view(ir.edits, ir.n_edits + 1, EDIT)[eb:ee + 1]
    rec = e[:-1]
    count = (e["first"][1:] - rec["first"]).astype(np.int64)
    index = rec["index"].astype(np.int64)
    length = int(index[-1] + count[-1]) if len(rec) else 0
    j = np.arange(first, first + n, dtype=np.int64)
    hi = np.searchsorted(index, j, side="right") - 1
    lo = np.searchsorted(index + count - 1, j, side="left")
    multi = (lo != hi) & ((count[lo] > 1) | ((rec["flags"][lo] & 2) != 0))   # (behind a multi-insert edit the updates' ids alone)
    lo = lo + multi
    d = j - index[hi]
    pred_ctr = np.where(lo == hi, rec["id_ctr"][hi] + d, rec["id_ctr"][lo])
    return (rec["elem_ctr"][hi] + d, rec["elem_actor"][hi], pred_ctr, rec["id_actor"][lo], lo, hi - lo + 1), rec, length, actors


def request_by_fold(eng, ir, call, time):
    """fetch_ir + the fold + context.js's rules (splice :441-502, setListIndex :411-435): the request the engine builds on the device"""
    fetch(eng, ir)
    name = lambda ctr, a: f"{int(ctr)}@{actors[a].hex()}"   # noqa: E731
    if call[0] == "set":
        (ec, ea, pc, pa, lo, pn), rec, length, actors = elements_of(ir, call[1], 1)
        preds = [name(pc[0], pa[0])] + [name(rec["id_ctr"][lo[0] + q], rec["id_actor"][lo[0] + q]) for q in range(1, int(pn[0]))]
        ops = [{"action": "set", "obj": LIST, "elemId": name(ec[0], ea[0]), "insert": False, "value": call[2], "datatype": "int", "pred": preds}]
    else:
        _, start, deletions, values = call
        lead = 1 if start else 0
        (ec, ea, pc, pa, lo, pn), rec, length, actors = elements_of(ir, start - lead, deletions + lead)
        assert start + deletions <= length
        ops = []
        if deletions:
            dec, dea, dpc, dpa, dlo, dpn = ec[lead:], ea[lead:], pc[lead:], pa[lead:], lo[lead:], pn[lead:]
            head = np.ones(deletions, dtype=bool)
            head[1:] = ~((dpn[1:] == 1) & (dpn[:-1] == 1) & (dea[1:] == dea[:-1]) & (dec[1:] == dec[:-1] + 1) & (dpa[1:] == dpa[:-1]) & (dpc[1:] == dpc[:-1] + 1))
            at = np.nonzero(head)[0]
            for k, n in zip(at, np.diff(np.append(at, deletions))):
                preds = [name(dpc[k], dpa[k])] + [name(rec["id_ctr"][dlo[k] + q], rec["id_actor"][dlo[k] + q]) for q in range(1, int(dpn[k]))]
                op = {"action": "del", "obj": LIST, "elemId": name(dec[k], dea[k]), "insert": False, "pred": preds}
                if n > 1:
                    op["multiOp"] = int(n)
                ops.append(op)
        if values:
            op = {"action": "set", "obj": LIST, "elemId": name(ec[0], ea[0]) if lead else "_head", "insert": True, "datatype": "int", "pred": []}
            if len(values) > 1:
                op["values"] = list(values)
            else:
                op["value"] = values[0]
            ops.append(op)
    clock = dict(zip(view(ir.clock_actor, ir.n_clock, np.dtype("<u4")).tolist(), view(ir.clock_seq, ir.n_clock, np.dtype("<u8")).tolist()))
    me = actors.index(bytes.fromhex(AUTHOR)) if bytes.fromhex(AUTHOR) in actors else None
    heads = view(ir.heads, 32 * ir.n_heads, np.dtype("u1")).tobytes()
    return {"actor": AUTHOR, "seq": int(clock.get(me, 0)) + 1, "startOp": int(ir.max_op) + 1, "time": time, "message": "",
            "deps": [heads[32 * k:32 * k + 32].hex() for k in range(ir.n_heads)], "ops": ops}


def session(lib, base, n, reps):
    """Two contexts built by apply_changes (the in-place paths serve what follows)."""
    a, b = engine.Engine(0, lib), engine.Engine(0, lib)
    for eng in (a, b):
        for sw in ("set_resident_new_actors", "set_resident_new_objects", "set_resident_counters", "set_local_small"):
            getattr(eng, sw)(True)
    made, late = list_changes(a, n, 3 * (reps + 3))
    for eng in (a, b):
        if base is not None:
            eng.apply_changes(base)
        eng.apply_changes(ChangeLog.from_changes(made))
    ir = PatchIR()
    st = a.stats()
    print(f"## {st.n_ops} ops, {st.n_changes} changes, list of {a.list_locate(LIST, 0, 0)[2]} elements")
    clock, used, shifted, row = [0], [0], [0], []

    def one(label, make_call, behind_apply, n_reps):
        ts = {"engine": [], "fold": [], "locate": []}
        for _ in range(n_reps):
            clock[0] += 1
            if behind_apply:
                c = late.pop(0)
                shifted[0] += 1
                for eng in (a, b):
                    eng.apply_changes(ChangeLog.from_changes([c]))
            call = make_call(a.list_locate(LIST, 0, 0)[2] if not behind_apply else None)
            if not behind_apply:
                for eng in (a, b):
                    eng.list_locate(LIST, 0, 0)   # (untimed: the edit tables are fresh for both routes)
                first, cnt = (call[1], 1) if call[0] == "set" else (max(call[1] - 1, 0), call[2] + 1)
                ts["locate"].append(timed(lambda: a.list_locate(LIST, first, cnt))[0])
            before = a.list_splice_calls()[2]
            if call[0] == "set":
                ta, got = timed(lambda: a.list_set(LIST, call[1], call[2], AUTHOR, time=clock[0]))
            else:
                ta, got = timed(lambda: a.list_splice(LIST, call[1], call[2], call[3], AUTHOR, time=clock[0]))
            launches = a.list_splice_calls()[2] - before
            tb, want = timed(lambda: b.apply_local_change(request_by_fold(b, ir, call, clock[0])))
            assert got == want, f"{label}: the two routes made different changes"
            ts["engine"].append(ta)
            ts["fold"].append(tb)
        tag = " behind an in-place apply_changes" if behind_apply else ""
        print(f"{label}{tag}: change of {len(got)} bytes, {launches} launches of the locate half")
        print(f"    list_splice / list_set               {med(ts['engine'])}")
        if ts["locate"]:
            print(f"      of which am355_list_locate alone   {med(ts['locate'])}")
        print(f"    fetch_ir + fold + apply_local_change {med(ts['fold'])}")
        row.extend([statistics.median(ts["engine"]), statistics.median(ts["fold"])])

    length = a.list_locate(LIST, 0, 0)[2]
    big = min(10000, length // 8)   # (four calls delete that many)

    def conflicted(_):
        used[0] += 1   # (the conflicted elements of the first quarter, which no other shape touches; E's insertions at the head shift them)
        at = EVERY // 2 + EVERY * used[0] + shifted[0]
        runs = a.list_locate(LIST, at, 1)[0]
        assert int(runs[0]["pred_num"]) == 2, "not a conflicted element"
        return ("set", at, clock[0])

    mid = lambda _: a.list_locate(LIST, 0, 0)[2] // 2   # noqa: E731
    shapes = (("(a) 1 deleted + 1 inserted", lambda n_: ("splice", mid(n_), 1, [7]), reps), ("(b) assignment onto 2 values", conflicted, reps),
              (f"(c) {big} deleted", lambda n_: ("splice", mid(n_), big, []), 2))
    for label, make_call, n_reps in shapes[:2]:
        one(label, make_call, False, n_reps)
    for label, make_call, n_reps in shapes[:2]:
        one("(d) " + label[4:], make_call, True, n_reps)
    one(shapes[2][0], shapes[2][1], False, 2)
    one("(d) " + shapes[2][0][4:], shapes[2][1], True, 2)
    print(f"resident_counters of the list_splice context (served, fell back, in place): {a.resident_counters()}; local_small_calls {a.local_small_calls()}; "
          f"list_splice_calls {a.list_splice_calls()}")
    assert a.patch_json() == b.patch_json()
    a.close()
    b.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=engine.DEFAULT_LIB)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--docs", default="L,LT")
    arg = ap.parse_args()
    print(f"# {os.path.basename(arg.lib)}: a list edited by position, am355_list_splice / am355_list_set against am355_fetch_ir + a numpy fold + "
          f"am355_apply_local_change, alternating; scale {arg.scale}")
    n = max(400, int(100_000 * arg.scale))
    for doc in arg.docs.split(","):
        base = loggen.config("c4_text_single", arg.scale, False) if doc == "LT" else None
        print(f"# document {doc}: " + ("the list beside the headline Text" if base is not None else "the list alone"))
        rows = []
        for run in range(arg.runs):
            print(f"# run {run + 1}")
            rows.append(session(arg.lib, base, n, arg.reps))
        print("## medians per run, ms, engine | fetch_ir + fold + apply_local_change: (a) (b) fresh, (d)(a) (d)(b) behind an in-place apply_changes, (c), (d)(c)")
        for run, row in enumerate(rows):
            print(f"run {run + 1}  " + "  ".join(f"{x:8.3f}" for x in row))


if __name__ == "__main__":
    main()
