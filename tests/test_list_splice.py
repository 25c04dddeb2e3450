"""A plain list edited by position on the engine (include/am355.h am355_list_locate, am355_list_splice, am355_list_set;
csrc/am355_list_locate.hip klist_check, klist_locate, klist_runs): position -> (elemId, every pred) on the device, and from there exactly
the change request the reference's frontend hands to Backend.applyLocalChange for list.deleteAt / list.insertAt / list[i] = v
(frontend/context.js:441-502 splice, :370-405 insertListItems, :411-435 setListIndex).

1. The restatement, without an engine: a fold of the ORACLE's whole-document patch into (elemId, preds) per element by the rule of
   frontend/apply_patch.js:156-213, turned into a request by context.js's rules, equals the request the reference's frontend made, for
   every call of every session of tests/golden/list/list_splices.json (tools/fixtures/make_list_splices.js).
2. The fixture's sessions on the engine, call by call on one context; the set of refused calls is asserted exactly.
3. Twin contexts: list_splice / list_set against apply_local_change(the request of the fold).
4. list_locate against the fold at the kernels' switch points (am355_list_locate_limits).
5. The check pass on hand-made record tables: the element whose first record carries the update bit.
6. Edges and errors; after each refusal the state is still served.
7. list_locate changes nothing.

Each engine body runs on the emulation (CPU suite) and on the device, with AM355_RESORDER_VERIFY=1 and AM355_LOCAL_SMALL_VERIFY=1.

AN ASSIGNMENT ALWAYS EMITS ITS OP on the engine (the reference skips list[i] = v when v is the shown value and there is no conflict; the
engine holds no JS values); the fixture records only assignments the reference emits.
A CONFLICTED ELEMENT WITH A HIDDEN INCREMENTED COUNTER (session `counters`): see REFUSED below for what the engine answers there."""
import base64
import json
import os

import numpy as np
import pytest

import oracle_lib
import test_local_small as tls
from automerge_classic_amd import engine
from automerge_classic_amd.loggen import ChangeLog
from golden_util import same_patch
from test_local_change import emu_lib  # noqa: F401 (the fixture that builds the emulation)
from test_text_splice import OutOfBounds, _parse, own_last_hash, change_info

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "list", "list_splices.json")
AM355_E_ARG, AM355_E_INVALID, AM355_E_UNSUPPORTED, AM355_E_STATE = -2, -3, -4, -5
COUNTER_DELETE = "Unsupported operation: deleting a counter from a list"
COUNTER_ASSIGN = "Cannot overwrite a Counter object; use .increment() or .decrement() to change its value."
SESSION_NAMES = ["typed", "mixed_values", "two_actors", "conflicts", "holes", "children", "counters", "past_end", "bounds"]
# (session, index of the call) of every recorded call that the engine refuses although the reference's LIVE frontend served it. The rule is
# defined on a frontend made fresh from getPatch(state). `counters` call 19 deletes an element whose incremented counter was overwritten:
# the whole-document patch reports it as `remove` first and lists its value as a bare `update` edit, so a fresh frontend has no elemId for
# it (and misplaces every elemId behind it); the fold raises NoElemId there and the engine answers AM355_E_UNSUPPORTED.
# The question the fixture settles -- does the record of a counter completed by increments, hidden behind a later value of the same
# element, carry the op id the frontend sends as pred? -- is answered by `counters` call 17 (an assignment onto such an element, two
# preds) being served with the reference's bytes: it does, the id of the counter's `set` row. Such elements are not refused.
REFUSED = {("counters", 19)}
# ... and the calls after which the list holds such an element (the assignment that overwrote the incremented counter): list_locate refuses
NO_ELEM_AFTER = {("counters", 17)}


def _b64(x):
    return base64.b64decode(x)


def load_sessions():
    with open(FIXTURE) as f:
        fx = json.load(f)
    out = {}
    for s in fx["sessions"]:
        s = dict(s)
        s["changes"] = [_b64(c) for c in s["changes"]]
        out[s["name"]] = s
    return out


SESSIONS = load_sessions()
_emulated, _gpu = tls._emulated, tls._gpu


def _verify(monkeypatch):
    tls._verify(monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------------
# the rule, restated over a patch
# ---------------------------------------------------------------------------------------------------------------------------
def _is_counter(value):
    return value.get("datatype") == "counter"


def elements_of_patch(patch_json):
    """{objectId: [(elemId, [pred, ...], the shown value is a counter)]} of every plain list of a whole-document patch: updateListObject
    (apply_patch.js:156-213) applied to an empty object. insert / update: the values are the edit's and those of every `update` edit of
    the same index directly behind it, the last one is shown; multi-insert: elemIds count up from edit.elemId, the pred is the elemId."""
    out = {}

    def walk(diff):
        for values in diff.get("props", {}).values():
            for v in values.values():
                if "objectId" in v:
                    walk(v)
        if "edits" not in diff:
            return
        elems, edits, i = [], diff["edits"], 0
        while i < len(edits):
            e = edits[i]
            a, index = e["action"], e["index"]
            if a in ("insert", "update"):
                preds, shown = [e["opId"]], e["value"]
                while i + 1 < len(edits) and edits[i + 1]["index"] == index and edits[i + 1]["action"] == "update":
                    i += 1
                    preds.append(edits[i]["opId"])
                    shown = edits[i]["value"]
                    if "objectId" in shown:
                        walk(shown)
                if a == "insert":
                    elems.insert(index, (e["elemId"], preds, _is_counter(shown)))
                elif index < len(elems):   # (apply_patch.js:187-190: behind a multi-insert edit the updates REPLACE the conflicts)
                    elems[index] = (elems[index][0], preds, _is_counter(shown))
                else:   # (... and on an index nothing inserted there is no ELEM_IDS entry)
                    raise NoElemId(f"element {index} of {diff['objectId']} begins with an `update` edit")
                if "objectId" in e["value"]:
                    walk(e["value"])
            elif a == "multi-insert":
                ctr, actor = _parse(e["elemId"])
                ids = [f"{ctr + k}@{actor}" for k in range(len(e["values"]))]
                elems[index:index] = [(x, [x], e.get("datatype") == "counter") for x in ids]
            else:
                raise AssertionError(f"{a} edit in a whole-document patch")
            i += 1
        if diff["type"] == "list":
            out[diff["objectId"]] = elems

    walk(json.loads(patch_json)["diffs"])
    return out


class NoElemId(Exception):
    pass


def runs_of(elems, lead=0):
    """context.js:474-492: a deletion joins the one before it iff both have exactly one pred, and elemId and pred have equal actors and
    consecutive counters. [(elemId, preds, count, holds a counter)]; element `lead` always starts a run."""
    runs = []
    for k, (elem, preds, counter) in enumerate(elems):
        if runs and k != lead and len(preds) == 1 and len(runs[-1][1]) == 1:
            (ec, ea), (pc, pa) = _parse(elem), _parse(preds[0])
            (lec, lea), (lpc, lpa), n = _parse(runs[-1][0]), _parse(runs[-1][1][0]), runs[-1][2]
            if lea == ea and lec + n == ec and lpa == pa and lpc + n == pc:
                runs[-1] = (runs[-1][0], runs[-1][1], n + 1, runs[-1][3] or counter)
                continue
        runs.append((elem, list(preds), 1, counter))
    return runs


def request_value(pair):
    """a [class, v] pair of the fixture as the (value, datatype) of a request's op"""
    cls, v = pair
    return v, (None if cls in ("str", "bool", "null") else cls)


def engine_value(pair):
    """... and as list_splice / list_set take it"""
    cls, v = pair
    return v if cls in ("str", "bool", "null") else (cls, float(v) if cls == "float64" else v)


def insert_ops(object_id, ref_elem, values, actor, next_op):
    """insertListItems (context.js:370-405): one `set` with `values` when there are several and all carry the same datatype, else one
    inserting `set` per value, each behind the element the one before it made."""
    pairs = [request_value(v) for v in values]
    if len(pairs) > 1 and len({d for _, d in pairs}) == 1:
        op = {"action": "set", "obj": object_id, "elemId": ref_elem, "insert": True, "values": [v for v, _ in pairs], "pred": []}
        if pairs[0][1]:
            op["datatype"] = pairs[0][1]
        return [op]
    ops = []
    for v, d in pairs:
        op = {"action": "set", "obj": object_id, "elemId": ref_elem, "insert": True, "value": v, "pred": []}
        if d:
            op["datatype"] = d
        ops.append(op)
        ref_elem = f"{next_op}@{actor}"
        next_op += 1
    return ops


def splice_ops(elems, object_id, start, deletions, values, actor, next_op):
    if start < 0 or deletions < 0 or start > len(elems) - deletions:
        raise OutOfBounds(f"{deletions} deletions starting at index {start} are out of bounds for list of length {len(elems)}")
    ops = []
    for elem, preds, count, counter in runs_of(elems[start:start + deletions]):
        if counter:
            raise TypeError(COUNTER_DELETE)
        op = {"action": "del", "obj": object_id, "elemId": elem, "insert": False, "pred": preds}
        if count > 1:
            op["multiOp"] = count
        ops.append(op)
        next_op += count
    return ops + insert_ops(object_id, elems[start - 1][0] if start else "_head", values, actor, next_op)


def request_of_fold(patch_json, call, own_last=None):
    """The change request of the recorded call (kind 'splice' or 'set', or a 'throws' of either) onto the state of a whole-document patch;
    None when there is nothing to do."""
    patch = json.loads(patch_json)
    oid, actor = call["objectId"], call["actor"]
    elems = elements_of_patch(patch_json)[oid]
    next_op = patch["maxOp"] + 1
    if call.get("call", call["kind"]) == "splice":
        ops = splice_ops(elems, oid, call["start"], call["deletions"], call["values"], actor, next_op)
    else:
        index = call["index"]
        if index >= len(elems):   # setListIndex: nulls up to the index, then the value
            ops = splice_ops(elems, oid, len(elems), 0, [["null", None]] * (index - len(elems)) + [call["value"]], actor, next_op)
        else:
            elem, preds, counter = elems[index]
            if counter:
                raise RangeError(COUNTER_ASSIGN)
            v, d = request_value(call["value"])
            op = {"action": "set", "obj": oid, "elemId": elem, "insert": False, "value": v, "pred": preds}
            if d:
                op["datatype"] = d
            ops = [op]
    if not ops:
        return None
    return {"actor": actor, "seq": patch["clock"].get(actor, 0) + 1, "startOp": next_op, "deps": [h for h in patch["deps"] if h != own_last],
            "time": call["time"], "message": "", "ops": ops}


class RangeError(Exception):
    pass


THROWN = {"RangeError": (OutOfBounds, RangeError), "TypeError": (TypeError,)}


def test_the_fixture_holds_every_session():
    assert sorted(SESSIONS) == sorted(SESSION_NAMES)
    assert os.path.getsize(FIXTURE) < (1 << 20)
    calls = lambda name: [c for c in SESSIONS[name]["calls"] if c["kind"] != "apply"]   # noqa: E731
    ops = lambda name: [o for c in calls(name) if c.get("request") for o in c["request"]["ops"]]   # noqa: E731
    assert any(len(o["pred"]) == 2 for o in ops("conflicts")) and any(len(o["pred"]) == 3 for o in ops("conflicts"))
    assert any(o["action"] == "set" and not o["insert"] and len(o["pred"]) == 3 for o in ops("conflicts"))
    assert any(o.get("multiOp", 1) > 1 for o in ops("typed")) and any(o.get("multiOp", 1) > 1 for o in ops("holes"))
    first = calls("two_actors")[0]   # two actors in turns: a deletion of five elements is five ops
    assert first["deletions"] == 5 and len(first["request"]["ops"]) == 5 and all("multiOp" not in o for o in first["request"]["ops"])
    assert {o.get("datatype") for o in ops("mixed_values")} == {None, "int", "uint", "float64", "counter", "timestamp"}
    assert any(o.get("values") == ["a", True, None] for o in ops("mixed_values"))
    assert [(c["error"], c["message"]) for c in calls("counters") if c["kind"] == "throws"].count(("TypeError", COUNTER_DELETE)) >= 3
    assert ("RangeError", COUNTER_ASSIGN) in [(c["error"], c["message"]) for c in calls("counters") if c["kind"] == "throws"]
    assert any(o.get("values") == [None, None, "v"] for o in ops("past_end"))
    assert sum(c["kind"] == "throws" for c in calls("bounds")) >= 4 and any(c["kind"] == "splice" and c["request"] is None for c in calls("bounds"))
    assert any(c["kind"] == "set" for c in calls("children"))
    assert all(SESSIONS[n]["calls"][i]["kind"] == "splice" for n, i in REFUSED)
    hidden = SESSIONS["counters"]["calls"][17]   # the assignment onto [a counter with an increment, a later string]
    assert hidden["kind"] == "set" and len(hidden["request"]["ops"][0]["pred"]) == 2


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the restatement against the requests of the reference's frontend, on the oracle's patch
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SESSION_NAMES)
def test_the_fold_makes_the_requests_of_the_frontend(name):
    s = SESSIONS[name]
    session = oracle_lib.OracleSession()
    applied, checked = 0, 0
    try:
        for i, call in enumerate(s["calls"]):
            if call["kind"] == "apply":
                continue
            if call["n_before"] > applied:
                session.apply(s["changes"][applied:call["n_before"]])
                applied = call["n_before"]
            last = own_last_hash(s["changes"][:applied], call["actor"])
            if (name, i) in REFUSED:
                with pytest.raises(NoElemId):
                    request_of_fold(session.patch_json(), call, last)
            elif call["kind"] == "throws":
                with pytest.raises(THROWN[call["error"]]) as e:
                    request_of_fold(session.patch_json(), call, last)
                assert str(e.value) == call["message"], f"{name} call {i}"
            else:
                want = dict(call["request"], deps=[h for h in call["request"]["deps"] if h != last]) if call["request"] else None
                assert request_of_fold(session.patch_json(), call, last) == want, f"{name} call {i}"
            checked += 1
        assert checked >= 5
    finally:
        session.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the fixture's sessions on the engine
# ---------------------------------------------------------------------------------------------------------------------------
def engine_call(eng, call):
    if call.get("call", call["kind"]) == "splice":
        return eng.list_splice(call["objectId"], call["start"], call["deletions"], [engine_value(v) for v in call["values"]], call["actor"], time=call["time"])
    return eng.list_set(call["objectId"], call["index"], engine_value(call["value"]), call["actor"], time=call["time"])


def check_call_outcome(eng, call, where, no_elem_after=False):
    """One recorded call on a context that holds the state before it. Returns True when the engine refused a call the reference served."""
    if call["kind"] == "throws":
        with pytest.raises(engine.EngineError) as e:
            engine_call(eng, call)
        code = AM355_E_ARG if "out of bounds" in call["message"] else AM355_E_INVALID   # (the bounds | the two counter rules)
        assert e.value.code == code and call["message"] in str(e.value), where
        return False
    if call["request"] is None:
        assert engine_call(eng, call) == b"", where
    else:
        try:
            got = engine_call(eng, call)
        except engine.UnsupportedChanges as e:
            assert "first edit is an `update`" in str(e), where
            return True
        assert got == _b64(call["change"]), f"{where}:\n got  {got.hex()}\n want {_b64(call['change']).hex()}"
        assert same_patch(eng.apply_patch_json(), call["patch"]), f"{where}:\n got  {eng.apply_patch_json()}\n want {call['patch']}"
    if no_elem_after:
        with pytest.raises(engine.UnsupportedChanges, match="first edit is an `update`"):
            eng.list_locate(call["objectId"], 0, 0)
    else:
        assert eng.list_locate(call["objectId"], 0, 0)[2] == call["length"], where
    return False


def check_whole_session(make_engine, name):
    """Call after call on one context: the resident path and the one-workgroup build serve every call."""
    s = SESSIONS[name]
    eng = make_engine()
    try:
        at, served, refused, unsupported = 0, 0, 0, set()
        for i, call in enumerate(s["calls"]):
            where = f"{name} call {i}"
            assert call["n_before"] == at, where
            if call["kind"] == "apply":
                eng.apply_changes(ChangeLog.from_changes(s["changes"][at:at + call["n"]]))
                at += call["n"]
                continue
            resident, small = eng.resident_counters()[0], eng.local_small_calls()
            if check_call_outcome(eng, call, where, (name, i) in NO_ELEM_AFTER):
                unsupported.add((name, i))
                refused += 1
                at += 1   # the session goes on with the reference's change (from a fresh replay: the resident path does not take it either)
                eng.load_changes(ChangeLog.from_changes(s["changes"][:at]))
                eng.replay()
                continue
            made = call["kind"] != "throws" and call["request"] is not None
            served += call["kind"] != "throws"
            refused += call["kind"] == "throws"
            at += made
            assert eng.list_splice_calls()[:2] == (served, refused), where
            assert eng.resident_counters()[0] == resident + made, f"{where}: not merged into the resident state"
            assert eng.local_small_calls() == (small[0] + made, small[1]), f"{where}: not built by the one workgroup"
        assert unsupported == {r for r in REFUSED if r[0] == name}
        assert same_patch(eng.patch_json(), s["whole_patch"])
    finally:
        eng.close()


@pytest.mark.parametrize("name", SESSION_NAMES)
def test_whole_session_emulated(emu_lib, monkeypatch, name):  # noqa: F811
    _verify(monkeypatch)
    check_whole_session(_emulated(emu_lib), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SESSION_NAMES)
def test_whole_session_gpu(monkeypatch, name):
    _verify(monkeypatch)
    check_whole_session(_gpu, name)


def check_calls_from_a_fresh_replay(make_engine, name):
    s = SESSIONS[name]
    eng = make_engine()
    try:
        for i, call in enumerate(s["calls"]):
            if call["kind"] == "apply":
                continue
            eng.load_changes(ChangeLog.from_changes(s["changes"][:call["n_before"]]))
            eng.replay()
            assert check_call_outcome(eng, call, f"{name} call {i}", (name, i) in NO_ELEM_AFTER) == ((name, i) in REFUSED)
    finally:
        eng.close()


@pytest.mark.parametrize("name", ["conflicts", "counters", "children"])
def test_calls_from_a_fresh_replay_emulated(emu_lib, monkeypatch, name):  # noqa: F811
    _verify(monkeypatch)
    check_calls_from_a_fresh_replay(_emulated(emu_lib), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["conflicts", "counters", "children"])
def test_calls_from_a_fresh_replay_gpu(monkeypatch, name):
    _verify(monkeypatch)
    check_calls_from_a_fresh_replay(_gpu, name)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. twin contexts: the list calls against apply_local_change(the request of the fold)
# ---------------------------------------------------------------------------------------------------------------------------
def check_twins(make_engine, name):
    s = SESSIONS[name]
    a, b = make_engine(), make_engine()
    try:
        at, n = 0, 0
        for i, call in enumerate(s["calls"]):
            if call["kind"] == "apply":
                for eng in (a, b):
                    eng.apply_changes(ChangeLog.from_changes(s["changes"][at:at + call["n"]]))
                at += call["n"]
                continue
            if call["kind"] == "throws" or call["request"] is None:
                continue
            request = request_of_fold(b.patch_json(), call, own_last_hash(s["changes"][:at], call["actor"]))
            got, want = engine_call(a, call), b.apply_local_change(request)
            at += 1
            n += 1
            assert got == want, f"{name} call {i}"
            assert a.apply_patch_json() == b.apply_patch_json(), f"{name} call {i}"
            assert a.patch_json() == b.patch_json(), f"{name} call {i}"
        assert n >= 5
        assert bytes(a.save()) == bytes(b.save())
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("name", ["typed", "conflicts", "holes"])
def test_twins_emulated(emu_lib, monkeypatch, name):  # noqa: F811
    _verify(monkeypatch)
    check_twins(_emulated(emu_lib), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["typed", "conflicts", "holes"])
def test_twins_gpu(monkeypatch, name):
    _verify(monkeypatch)
    check_twins(_gpu, name)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. list_locate against the fold at the switch points
# ---------------------------------------------------------------------------------------------------------------------------
def locate_limits():
    import ctypes
    out = (ctypes.c_uint32 * 3)()
    assert engine.load_library().am355_list_locate_limits(out) == 0
    return tuple(int(x) for x in out)


ACT_A, ACT_B, ACT_C, ACT_D = "2a" * 16, "b7" * 16, "c1" * 16, "d9" * 16
LIST = f"1@{ACT_A}"


def _make_list(n):
    return {"actor": ACT_A, "seq": 1, "startOp": 1, "time": 0, "message": "", "deps": [],
            "ops": [{"action": "makeList", "obj": "_root", "key": "list", "insert": False, "pred": []},
                    {"action": "set", "obj": LIST, "elemId": "_head", "insert": True, "values": list(range(n)), "datatype": "int", "pred": []}]}


def _assigns(actor, start_op, dep, targets):
    """one change of `actor`: for (index, keep) in targets a `set` onto element index of _make_list's list, overwriting the first value
    (pred = its id) or, keep, standing beside it (pred = [])"""
    return {"actor": actor, "seq": 1, "startOp": start_op, "time": 0, "message": "", "deps": [dep],
            "ops": [{"action": "set", "obj": LIST, "elemId": f"{2 + i}@{ACT_A}", "insert": False, "value": f"{actor[:2]}{i}", "pred": [] if keep else [f"{2 + i}@{ACT_A}"]}
                    for i, keep in targets]}


def conflicted_requests(n, two, three, kept):
    """_make_list(n); the elements `two` get two concurrent values (B and C overwrite the first), `three` three (B, C, D), and those of
    `kept` keep their first value beside B's and C's (a `set` without pred, which no frontend makes): the last value of a record of
    several values, with records behind it -- where the reference's frontend keeps the ids of the updates alone (apply_patch.js:187-190)."""
    first = _make_list(n)
    b = sorted([(i, False) for i in two + three] + [(i, True) for i in kept])
    c = b
    d = sorted((i, False) for i in three)
    return [first, lambda dep: _assigns(ACT_B, n + 2, dep, b), lambda dep: _assigns(ACT_C, n + 2, dep, c), lambda dep: _assigns(ACT_D, n + 2, dep, d)]


def alternating_requests(half):
    """A inserts `half` values; B, who has seen them, inserts one behind each: a0 b0 a1 b1 ... -- every element is a run of its own."""
    return [_make_list(half), lambda dep: {"actor": ACT_B, "seq": 1, "startOp": half + 2, "time": 0, "message": "", "deps": [dep],
                                           "ops": [{"action": "set", "obj": LIST, "elemId": f"{2 + k}@{ACT_A}", "insert": True, "value": "b", "pred": []} for k in range(half)]}]


def two_valued_requests(n, m):
    """the first m of n elements keep their value beside B's: two preds each"""
    return [_make_list(n), lambda dep: _assigns(ACT_B, n + 2, dep, [(i, True) for i in range(m)])]


_shapes = {}


def shape(make_engine, key):
    """(log, the list's elements by the fold of the ORACLE's patch, actor ranks): made once, shared by the emulated and the device run."""
    if key not in _shapes:
        b, s, p = locate_limits()
        n = s + 40
        requests = {"conflicted": lambda: conflicted_requests(n, [0, b - 1, 2 * b, n - 1], [b, 2 * b - 1, s - 1], [40, s]),
                    "alternating": lambda: alternating_requests(p // 2 + 4),
                    "two_valued": lambda: two_valued_requests(p // 2 + 8, p // 2 + 2),
                    "empty": lambda: [_make_list(0)]}[key]()
        if key == "empty":
            requests[0]["ops"] = requests[0]["ops"][:1]
        eng = make_engine()
        try:
            changes, dep = [], None
            for r in requests:
                change, digest = eng.encode_change(r if dep is None else r(dep))
                changes.append(change)
                dep = dep or digest.hex()   # (every later change depends on the first alone: they are concurrent)
        finally:
            eng.close()
        log = ChangeLog.from_changes(changes)
        elems = elements_of_patch(oracle_lib.OracleDoc(log).patch_json())[LIST]
        _shapes[key] = (log, elems, {a: k for k, a in enumerate(sorted([ACT_A, ACT_B, ACT_C, ACT_D][:max(2, len(requests))]))})
    return _shapes[key]


def as_tuples(runs, rank):
    """[(elem ctr, elem actor rank, count, counter, [(pred ctr, pred actor rank)])]"""
    out = []
    for elem, preds, count, counter in runs:
        ec, ea = _parse(elem)
        out.append((ec, rank[ea], count, 1 if counter else 0, [(pc, rank[pa]) for pc, pa in map(_parse, preds)]))
    return out


def located(eng, oid, first, n):
    runs, preds, length = eng.list_locate(oid, first, n)
    out, at = [], 0
    for r in runs:
        assert int(r["pred_first"]) == at, "the preds of the runs follow each other"
        at += int(r["pred_num"])
        out.append((int(r["elem_ctr"]), int(r["elem_actor"]), int(r["count"]), int(r["flags"]),
                    [(int(p["ctr"]), int(p["actor"])) for p in preds[int(r["pred_first"]):at]]))
    assert at == len(preds)
    return out, length


def check_locate(make_engine, key, queries):
    """queries(limits, total) -> [(first, n)]"""
    log, elems, rank = shape(make_engine, key)
    eng = make_engine()
    try:
        eng.load_changes(log)
        eng.replay()
        for first, n in queries(locate_limits(), len(elems)):
            got, length = located(eng, LIST, first, n)
            assert length == len(elems)
            assert got == as_tuples(runs_of(elems[first:first + n]), rank), f"{key}: [{first}, {first} + {n})"
    finally:
        eng.close()


def _conflicted_queries(limits, total):
    b, s, p = limits
    sizes = [1, b - 1, b, b + 1, 2 * b + 1, s - 1, s, s + 1, total]
    return [(0, n) for n in sizes] + [(1, b), (1, s), (b - 1, 2), (b, b), (39, 3), (40, 1), (41, s - 41), (total - 1, 1), (total - 2, 2), (0, 0), (total, 0)]


LOCATE_SHAPES = {
    # conflicted elements of two and three values as element 0, as the last thread of a workgroup and the first of the next (b - 1, b), at
    # the same places one element later (first = 1), as the last element; at 40 and s the last value of a record of several values
    "conflicted": _conflicted_queries,
    # every element is a run: P + 1 runs straddle the pinned bound of the run buffer
    "alternating": lambda limits, total: [(0, limits[2] - 1), (0, limits[2]), (0, limits[2] + 1), (3, limits[2] + 1), (0, total)],
    # two preds per element: P - 1 .. P + 2 preds straddle the pinned bound of the pred buffer
    "two_valued": lambda limits, total: [(0, limits[2] // 2), (0, limits[2] // 2 + 1), (1, limits[2] // 2 + 1), (0, limits[2] // 2 + 2), (0, limits[2] // 2 + 3), (0, total)],
    "empty": lambda limits, total: [(0, 0)],
}


def test_the_shapes_are_what_they_say(emu_lib):  # noqa: F811
    b, s, p = locate_limits()
    assert b < p < s, "else the shapes no longer straddle the bounds: add shapes for them"
    _, elems, _ = shape(_emulated(emu_lib), "conflicted")
    n = len(elems)
    assert n == s + 40
    assert [len(elems[i][1]) for i in (0, b - 1, 2 * b, n - 1)] == [2] * 4 and [len(elems[i][1]) for i in (b, 2 * b - 1, s - 1)] == [3] * 3
    # (element 40 ends a multi-insert edit: the updates' ids alone; element s stands behind a conflicted one, as an insert edit of its own)
    assert [len(elems[i][1]) for i in (40, s)] == [2, 3] and elems[40][0] not in elems[40][1] and elems[s][0] == elems[s][1][0]
    assert sum(len(e[1]) for e in elems) == n + 4 + 6 + 1 + 2
    _, elems, _ = shape(_emulated(emu_lib), "alternating")
    assert len(runs_of(elems)) == len(elems) >= p + 2
    _, elems, _ = shape(_emulated(emu_lib), "two_valued")
    assert [len(e[1]) for e in elems] == [2] * (p // 2 + 2) + [1] * 6
    assert shape(_emulated(emu_lib), "empty")[1] == []


@pytest.mark.parametrize("key", sorted(LOCATE_SHAPES))
def test_locate_at_the_switch_points_emulated(emu_lib, monkeypatch, key):  # noqa: F811
    _verify(monkeypatch)
    check_locate(_emulated(emu_lib), key, LOCATE_SHAPES[key])


@pytest.mark.gpu
@pytest.mark.parametrize("key", sorted(LOCATE_SHAPES))
def test_locate_at_the_switch_points_gpu(monkeypatch, key):
    _verify(monkeypatch)
    check_locate(_gpu, key, LOCATE_SHAPES[key])


def check_locate_on_the_sessions(make_engine):
    """Every range of the small documents of the fixture, counters, children and conflicts included."""
    for name in ("conflicts", "two_actors", "children", "mixed_values"):
        s = SESSIONS[name]
        at = max(c["n_before"] for c in s["calls"] if c["kind"] != "apply" and c.get("length", 1) > 0 and c["n_before"] > 0)
        changes = s["changes"][:at]
        want_all = elements_of_patch(oracle_lib.OracleDoc(ChangeLog.from_changes(changes)).patch_json())
        rank = {a: k for k, a in enumerate(sorted({change_info(c)[1] for c in changes}))}
        eng = make_engine()
        try:
            eng.load_changes(ChangeLog.from_changes(changes))
            eng.replay()
            assert want_all
            for oid, elems in want_all.items():
                for first in range(len(elems) + 1):
                    for n in range(len(elems) - first + 1):
                        got, length = located(eng, oid, first, n)
                        assert length == len(elems)
                        assert got == as_tuples(runs_of(elems[first:first + n]), rank), f"{name}: [{first}, {first} + {n})"
        finally:
            eng.close()


def test_locate_on_the_sessions_emulated(emu_lib, monkeypatch):  # noqa: F811
    _verify(monkeypatch)
    check_locate_on_the_sessions(_emulated(emu_lib))


@pytest.mark.gpu
def test_locate_on_the_sessions_gpu(monkeypatch):
    _verify(monkeypatch)
    check_locate_on_the_sessions(_gpu)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the check pass on hand-made tables: an element whose first record carries the update bit
# ---------------------------------------------------------------------------------------------------------------------------
LIF_NO_ELEM = 8
LENGTH_BEFORE = 0xDEADBEEF


def _flat_table(R, begin, updates=(), no_elem=()):
    """R records of one value each at `begin`: record k opens index k -- but a record of `updates` replaces the value before it (a
    conflict, well-formed) and one of `no_elem` opens its index WITH the update bit (the element that was reported as `remove` first).
    In front stand `begin` foreign records whose last one ends on index 0, as if record 0 of the object replaced its value."""
    t = np.zeros(begin + R + 1, dtype=engine.IR_EDIT_DTYPE)
    first = 0
    for k in range(begin):
        t[k]["index"], t[k]["first"] = 0, first
        first += 1
    index = 0
    for k in range(R):
        rec = t[begin + k]
        if k in updates:
            rec["flags"], rec["index"] = engine.EDIT_UPDATE, index - 1
        else:
            rec["flags"], rec["index"] = (engine.EDIT_UPDATE if k in no_elem else 0), index
            index += 1
        rec["first"] = first
        first += 1
    t[begin + R]["first"] = first
    t[begin + R]["flags"], t[begin + R]["index"] = engine.EDIT_UPDATE, index - 1
    return t, first, index


def check_list_premises(make_engine):
    b = locate_limits()[0]
    R = 2 * b + 3
    eng = make_engine()
    try:
        for begin in (0, 3):
            # well-formed, conflicts at the workgroup boundary included: as the Text pass answers, and the length
            for updates in ((), (1,), (b - 1, b), (b, b + 1, R - 1)):
                t, nv, length = _flat_table(R, begin, updates)
                assert eng.prim_list_premises(t, begin, R, nv) == (0, length) == eng.prim_text_premises(t, begin, R, nv), (begin, updates)
            for p in (0, b - 1, b, R - 1):
                t, nv, length = _flat_table(R, begin, updates=(5,), no_elem=(p,))
                flags, left = eng.prim_list_premises(t, begin, R, nv)
                assert flags == LIF_NO_ELEM, (begin, p)
                assert left == (LENGTH_BEFORE if p == R - 1 else length), (begin, p)
                assert eng.prim_text_premises(t, begin, R, nv) == (0, length), "the Text pass takes such an element (am355_textrec.h (f))"
            # behind an update record of the index before: still no element of its own
            t, nv, length = _flat_table(R, begin, updates=(b - 1,), no_elem=(b,))
            assert eng.prim_list_premises(t, begin, R, nv)[0] == LIF_NO_ELEM
            # a single record
            t, nv, length = _flat_table(1, begin, no_elem=(0,))
            assert eng.prim_list_premises(t, begin, 1, nv) == (LIF_NO_ELEM, LENGTH_BEFORE)
            t, nv, length = _flat_table(1, begin)
            assert eng.prim_list_premises(t, begin, 1, nv) == (0, 1)
            # a `remove` record and a broken table keep their bits
            t, nv, length = _flat_table(R, begin)
            t[begin + 7]["flags"] |= engine.EDIT_REMOVE
            assert eng.prim_list_premises(t, begin, R, nv)[0] == 2
            t, nv, length = _flat_table(R, begin)
            t[begin + b]["index"] += 2
            assert eng.prim_list_premises(t, begin, R, nv)[0] & 1
    finally:
        eng.close()


def test_list_premises_emulated(emu_lib):  # noqa: F811
    check_list_premises(_emulated(emu_lib))


@pytest.mark.gpu
def test_list_premises_gpu():
    check_list_premises(_gpu)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. edges and errors; after each refusal the state is still served
# ---------------------------------------------------------------------------------------------------------------------------
OBJECTS = {"actor": ACT_A, "seq": 1, "startOp": 1, "time": 0, "message": "", "deps": [],
           "ops": [{"action": "makeList", "obj": "_root", "key": "list", "insert": False, "pred": []},
                   {"action": "set", "obj": LIST, "elemId": "_head", "insert": True, "values": list("hello"), "pred": []},
                   {"action": "makeText", "obj": "_root", "key": "text", "insert": False, "pred": []},
                   {"action": "makeList", "obj": "_root", "key": "empty", "insert": False, "pred": []},
                   {"action": "makeMap", "obj": "_root", "key": "map", "insert": False, "pred": []},
                   {"action": "set", "obj": f"7@{ACT_A}", "elemId": "_head", "insert": True, "values": list("text"), "pred": []}]}
TEXT, EMPTY, MAP = f"7@{ACT_A}", f"8@{ACT_A}", f"9@{ACT_A}"


def check_errors(make_engine):
    asked, twin = make_engine(), make_engine()
    try:
        for call in (lambda: asked.list_splice(LIST, 0, 0, ["x"], ACT_B), lambda: asked.list_set(LIST, 0, "x", ACT_B), lambda: asked.list_locate(LIST, 0, 0)):
            with pytest.raises(engine.EngineError) as e:   # no state
                call()
            assert e.value.code == AM355_E_STATE
        made, _ = twin.encode_change(OBJECTS)
        for eng in (asked, twin):
            eng.apply_changes(ChangeLog.from_changes([made]))
        refused = 2   # (splices and assignments refused: list_locate is not counted)
        step = [0]

        def still_served(where):
            """an insertion, an assignment and a deletion on both contexts: the same changes, the same patch"""
            step[0] += 3
            for call in (lambda e: e.list_splice(LIST, 0, 0, ["é", step[0], ("counter", 3)], ACT_B, time=step[0]), lambda e: e.list_set(LIST, 0, 2.5, ACT_B, time=step[0]),
                         lambda e: e.list_splice(LIST, 0, 1, [], ACT_B, time=step[0])):
                got, want = call(asked), call(twin)
                assert got and got == want and asked.apply_patch_json() == twin.apply_patch_json(), where
            assert asked.patch_json() == twin.patch_json(), where
            assert asked.list_splice_calls()[:2] == (step[0], refused), where

        still_served("after the calls without a state")
        length = asked.list_locate(LIST, 0, 0)[2]
        assert length == 7
        # the empty list, and n == 0
        assert asked.list_locate(EMPTY, 0, 0)[2] == 0 and len(asked.list_locate(EMPTY, 0, 0)[0]) == 0
        runs, preds, _ = asked.list_locate(LIST, 2, 0)
        assert len(runs) == 0 and len(preds) == 0
        assert asked.list_locate(LIST, length, 0)[2] == length
        assert asked.list_splice(EMPTY, 0, 0, [], ACT_B) == b"" and asked.list_splice(LIST, 3, 0, [], ACT_B) == b""   # nothing to do
        step[0] += 2   # (both are served)
        for oid, first, n in ((EMPTY, 0, 1), (LIST, length, 1), (LIST, 0, length + 1), (LIST, length + 1, 0), (LIST, 2 ** 40, 1), (LIST, 1, 2 ** 64 - 1)):
            with pytest.raises(engine.EngineError, match="out of bounds") as e:
                asked.list_locate(oid, first, n)
            assert e.value.code == AM355_E_ARG
        # out of bounds, and the wrap-around of start + deletions
        for start, deletions in ((length + 1, 0), (length, 1), (0, length + 1), (2 ** 33, 2), (2, 2 ** 64 - 2), (2 ** 64 - 1, 1), (2 ** 63, 2 ** 63)):
            with pytest.raises(engine.EngineError) as e:
                asked.list_splice(LIST, start, deletions, ["x"], ACT_B)
            assert e.value.code == AM355_E_ARG
            assert f"{deletions} deletions starting at index {start} are out of bounds for list of length {length}" in str(e.value)
            refused += 1
        still_served("after the calls out of bounds")
        # a counter: no deletion reaches it, no assignment lands on it (still_served put one in: find it)
        counters = [i for i in range(asked.list_locate(LIST, 0, 0)[2]) if asked.list_locate(LIST, i, 1)[0][0]["flags"] & 1]
        assert counters and counters[0] > 0
        with pytest.raises(engine.InvalidChanges, match=COUNTER_DELETE):
            asked.list_splice(LIST, counters[0] - 1, 2, [], ACT_B)
        with pytest.raises(engine.InvalidChanges, match="Cannot overwrite a Counter object"):
            asked.list_set(LIST, counters[0], 1, ACT_B)
        with pytest.raises(engine.UnsupportedChanges):   # a byte array: refused as am355_apply_local_change refuses it
            asked.list_splice(LIST, 0, 0, [b"bytes"], ACT_B)
        refused += 3
        still_served("after the calls onto a counter")
        ctr, actor = LIST.split("@")
        for oid, text in ((TEXT, "not a list object"), (MAP, "not a list object"), ("_root", "not a list object"), (f"99@{actor}", f"no such object: 99@{actor}"),
                          (f"{ctr}@{'0' * 32}", "no such object"), (f"{ctr}@{actor}ff", "no such object")):
            with pytest.raises(engine.EngineError, match=text) as e:
                asked.list_splice(oid, 0, 0, ["x"], ACT_B)
            assert e.value.code == AM355_E_ARG
            with pytest.raises(engine.EngineError, match=text) as e:
                asked.list_set(oid, 0, "x", ACT_B)
            assert e.value.code == AM355_E_ARG
            with pytest.raises(engine.EngineError, match=text) as e:
                asked.list_locate(oid, 0, 0)
            assert e.value.code == AM355_E_ARG
            refused += 2
        # a list given to the Text calls: as before
        for call in (lambda: asked.text_locate(LIST, 0, 0), lambda: asked.text_splice(LIST, 0, 0, ["x"], ACT_B), lambda: asked.object_text(LIST)):
            with pytest.raises(engine.EngineError, match="not a Text object") as e:
                call()
            assert e.value.code == AM355_E_ARG
        assert asked.text_locate(TEXT, 0, 0)[1] == 4
        still_served("after the calls that name no list")
        # everything deleted, then inserted into again from _head; an assignment past the end of the emptied list
        for eng in (asked, twin):
            n = eng.list_locate(LIST, 0, 0)[2]
            keep = [i for i in range(n) if eng.list_locate(LIST, i, 1)[0][0]["flags"] & 1]
            assert keep, "the counters stay: delete around them"
            spans = [(a + 1, b - a - 1) for a, b in zip([-1] + keep, keep + [n]) if b - a > 1]
            for first, count in reversed(spans):
                assert eng.list_splice(LIST, first, count, [], ACT_B)
            assert eng.list_locate(LIST, 0, 0)[2] == len(keep)
            assert eng.list_set(EMPTY, 2, "z", ACT_B) and eng.list_locate(EMPTY, 0, 0)[2] == 3
            assert eng.list_splice(EMPTY, 0, 3, ["a"], ACT_B) and eng.list_splice(EMPTY, 1, 0, ["b", "c"], ACT_B)
        step[0] += len(spans) + 3
        still_served("after the list was emptied")
        # queued changes: a change whose dependency is missing waits in the state
        other = dict(OBJECTS, actor="c3" * 16, ops=[{"action": "set", "obj": "_root", "key": "k", "insert": False, "value": 1, "pred": []}], startOp=500)
        base, base_hash = twin.encode_change(other)
        late, _ = twin.encode_change(dict(other, seq=2, startOp=501, deps=[base_hash.hex()]))
        asked.apply_changes(ChangeLog.from_changes([late]))
        with pytest.raises(engine.UnsupportedChanges, match="queued changes"):
            asked.list_splice(LIST, 0, 0, ["x"], ACT_B)
        with pytest.raises(engine.UnsupportedChanges, match="queued changes"):
            asked.list_set(LIST, 0, "x", ACT_B)
        refused += 2
        asked.apply_changes(ChangeLog.from_changes([base]))
        twin.apply_changes(ChangeLog.from_changes([base, late]))
        still_served("after the calls onto queued changes")
    finally:
        asked.close()
        twin.close()
    eng = make_engine()
    try:
        eng.set_shard(0, 2)
        eng.load_changes(ChangeLog.from_changes([made]))
        eng.replay()
        for call in (lambda: eng.list_locate(LIST, 0, 1), lambda: eng.list_splice(LIST, 0, 0, ["x"], ACT_B), lambda: eng.list_set(LIST, 0, "x", ACT_B)):
            with pytest.raises(engine.UnsupportedChanges, match="sharded"):
                call()
    finally:
        eng.close()


def test_edges_and_errors_emulated(emu_lib, monkeypatch):  # noqa: F811
    _verify(monkeypatch)
    check_errors(_emulated(emu_lib))


@pytest.mark.gpu
def test_edges_and_errors_gpu(monkeypatch):
    _verify(monkeypatch)
    check_errors(_gpu)


def check_document_context(make_engine):
    """A context made by backend_load: locate reads it as it is; a splice turns it into the state of its rebuilt changes first."""
    s = SESSIONS["typed"]
    last = max(i for i, c in enumerate(s["calls"]) if c["kind"] == "splice" and c["request"])
    call = s["calls"][last]
    eng, twin = make_engine(), make_engine()
    try:
        twin.load_changes(ChangeLog.from_changes(s["changes"][:call["n_before"]]))
        twin.replay()
        eng.backend_load(bytes(twin.save()))
        elems = elements_of_patch(twin.patch_json())[call["objectId"]]
        runs, preds, length = eng.list_locate(call["objectId"], 0, len(elems))
        assert length == len(elems) and sum(int(r["count"]) for r in runs) == len(elems) and len(runs) == len(runs_of(elems))
        assert engine_call(eng, call) == _b64(call["change"])
        assert same_patch(eng.apply_patch_json(), call["patch"])
    finally:
        eng.close()
        twin.close()


def test_document_context_emulated(emu_lib, monkeypatch):  # noqa: F811
    _verify(monkeypatch)
    check_document_context(_emulated(emu_lib))


@pytest.mark.gpu
def test_document_context_gpu(monkeypatch):
    _verify(monkeypatch)
    check_document_context(_gpu)


# ---------------------------------------------------------------------------------------------------------------------------
# 7. locate changes nothing
# ---------------------------------------------------------------------------------------------------------------------------
def check_locate_changes_nothing(make_engine, name):
    s = SESSIONS[name]
    asked, twin = make_engine(), make_engine()
    try:
        at = 0
        for i, call in enumerate(s["calls"]):
            where = f"{name} call {i}"
            if call["kind"] == "apply":
                for eng in (asked, twin):
                    eng.apply_changes(ChangeLog.from_changes(s["changes"][at:at + call["n"]]))
                at += call["n"]
            elif call["kind"] != "throws" and call["request"]:
                assert engine_call(asked, call) == engine_call(twin, call) == _b64(call["change"]), where
                assert asked.apply_patch_json() == twin.apply_patch_json(), where
                at += 1
            else:
                continue
            oid = next(c["objectId"] for c in s["calls"] if c["kind"] != "apply")
            length = asked.list_locate(oid, 0, 0)[2]
            runs, _, _ = asked.list_locate(oid, 0, length)
            assert sum(int(r["count"]) for r in runs) == length, where
            if length > 2:
                asked.list_locate(oid, 1, length - 2)
            assert asked.resident_counters() == twin.resident_counters(), f"{where}: the query changed what serves the next call"
            assert asked.local_small_calls() == twin.local_small_calls(), where
        assert asked.list_splice_calls()[:2] == twin.list_splice_calls()[:2]
        assert asked.patch_json() == twin.patch_json()
        assert bytes(asked.save()) == bytes(twin.save())
    finally:
        asked.close()
        twin.close()


@pytest.mark.parametrize("name", ["typed", "two_actors"])
def test_locate_changes_nothing_emulated(emu_lib, monkeypatch, name):  # noqa: F811
    _verify(monkeypatch)
    check_locate_changes_nothing(_emulated(emu_lib), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["typed", "two_actors"])
def test_locate_changes_nothing_gpu(monkeypatch, name):
    _verify(monkeypatch)
    check_locate_changes_nothing(_gpu, name)
