"""A map edited by key on the engine (include/am355.h am355_map_locate, am355_map_update; csrc/am355_map_locate.hip kmap_locate,
kmap_gather): key -> (op ids of every visible value, is the shown one a counter) on the device, and from there exactly the change request
the reference's frontend hands to Backend.applyLocalChange for d.key = v / delete d.key / d.key.increment(n)
(frontend/context.js:325-346 setMapKey, :351-362 deleteMapKey, :531-540 deleteTableRow, :546-573 increment).

1. The rule without an engine: a fold of the ORACLE's whole-document patch (`props` -> preds, shown value) turned into a request equals
   the request the reference's frontend made, for every call of tests/golden/map/map_updates.json (tools/fixtures/make_map_updates.js).
2. The fixture's sessions on the engine, call by call on one context; the set of refused calls is asserted exactly: it is empty.
3. Twin contexts: map_update against apply_local_change(the request of the fold), with the in-place switches of the resident path on and
   off, and directly behind an in-place Text merge against a twin whose tables were fetched first.
4. map_locate / map_get against a fold of fetch_ir's map table at the smallest shapes that can go wrong (am355_map_locate_limits).
5. map_locate changes nothing: a twin context that is never asked.
6. Edges and errors; after each refusal the state is still served.

Each engine body runs on the emulation (CPU suite) and on the device, with AM355_LOCAL_SMALL_VERIFY=1.

AN ASSIGNMENT ALWAYS EMITS ITS OP on the engine (the reference skips d.key = v when v is the shown value and there is no conflict; the
engine holds no JS values); the fixture records only assignments the reference emits."""
import base64
import bisect
import ctypes
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
from test_text_splice import _parse, own_last_hash

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "map", "map_updates.json")
AM355_E_ARG, AM355_E_INVALID, AM355_E_UNSUPPORTED, AM355_E_STATE = -2, -3, -4, -5
EMPTY_KEY = "The key of a map entry must not be an empty string"
COUNTER_ASSIGN = "Cannot overwrite a Counter object; use .increment() or .decrement() to change its value."
NOT_A_COUNTER = "Only counter values can be incremented"
SESSION_NAMES = ["root", "nested", "nested_inner", "conflicts", "counters", "children", "table", "key_order", "mixed_values", "bounds"]
REFUSED = set()   # (session, index of the call) of recorded calls the engine refuses although the reference served them: none (check_whole_session)


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
class RangeError(Exception):
    pass


THROWN = {"RangeError": RangeError, "TypeError": TypeError}


def maps_of_patch(patch_json):
    """{objectId: (type, props)} of every map and table of a whole-document patch"""
    out = {}

    def walk(diff):
        if diff["type"] in ("map", "table"):
            out[diff["objectId"]] = (diff["type"], diff.get("props", {}))
        for values in diff.get("props", {}).values():
            for v in values.values():
                if "objectId" in v:
                    walk(v)
        for e in diff.get("edits", []):
            for v in [e.get("value", {})]:
                if "objectId" in v:
                    walk(v)

    walk(json.loads(patch_json)["diffs"])
    return out


def held_by(props, key):
    """([op ids of the key's values, the greatest first], the shown value is a counter): applyProperties (apply_patch.js:57-79) sorts by
    Lamport order and reverses; getPred (context.js:576-586) returns the keys of the conflicts object in that order."""
    held = props.get(key, {})
    ids = sorted(held, key=_parse, reverse=True)
    return ids, bool(ids) and held[ids[0]].get("datatype") == "counter"


def request_value(pair):
    cls, v = pair
    return v, (None if cls in ("str", "bool", "null") else cls)


def engine_value(pair):
    cls, v = pair
    return v if cls in ("str", "bool", "null") else (cls, float(v) if cls == "float64" else v)


def request_of_fold(patch_json, call, own_last=None):
    """The change request of the recorded call onto the state of a whole-document patch; None when no op comes of it."""
    patch = json.loads(patch_json)
    oid, actor = call["objectId"], call["actor"]
    kind, props = maps_of_patch(patch_json)[oid]
    ops = []
    for op in call["ops"]:
        what, key = op[0], op[1]
        ids, counter = held_by(props, key)
        if what == "set":
            if key == "":
                raise RangeError(EMPTY_KEY)
            if counter:
                raise RangeError(COUNTER_ASSIGN)
            v, d = request_value(op[2])
            o = {"action": "set", "obj": oid, "key": key, "insert": False, "value": v, "pred": ids}
            if d:
                o["datatype"] = d
            ops.append(o)
        elif what == "del":
            if ids:
                assert kind == "map" or len(ids) == 1
                ops.append({"action": "del", "obj": oid, "key": key, "insert": False, "pred": ids})
        else:
            if not counter:
                raise TypeError(NOT_A_COUNTER)
            ops.append({"action": "inc", "obj": oid, "key": key, "value": op[2], "insert": False, "pred": ids})
    if not ops:
        return None
    return {"actor": actor, "seq": patch["clock"].get(actor, 0) + 1, "startOp": patch["maxOp"] + 1, "deps": [h for h in patch["deps"] if h != own_last],
            "time": call["time"], "message": "", "ops": ops}


def engine_ops(call):
    return [(op[0], op[1], engine_value(op[2])) if op[0] == "set" else tuple(op) for op in call["ops"]]


def calls_of(name):
    return [c for c in SESSIONS[name]["calls"] if c["kind"] != "apply"]


def test_the_fixture_holds_every_session():
    assert sorted(SESSIONS) == sorted(SESSION_NAMES)
    assert os.path.getsize(FIXTURE) < (1 << 20)
    ops = lambda name: [o for c in calls_of(name) if c.get("request") for o in c["request"]["ops"]]   # noqa: E731
    thrown = lambda name: [(c["error"], c["message"]) for c in calls_of(name) if c["kind"] == "throws"]   # noqa: E731
    assert {len(o["pred"]) for o in ops("conflicts")} >= {0, 1, 2, 3}
    assert any(o["action"] == "del" and len(o["pred"]) == 3 for o in ops("conflicts")) and any(o["action"] == "set" and len(o["pred"]) == 3 for o in ops("conflicts"))
    assert any(c["kind"] == "update" and c["request"] is None for c in calls_of("root")), "a deletion of an absent key"
    assert any(o["action"] == "set" and o["pred"] == [] for c in calls_of("root")[3:] if c.get("request") for o in c["request"]["ops"]), "a deleted key set again"
    assert max(len(c["request"]["ops"]) for c in calls_of("root") if c.get("request")) >= 3
    assert any(o["action"] == "inc" and len(o["pred"]) == 2 for o in ops("counters")) and any(o["action"] == "inc" and o["value"] < 0 for o in ops("counters"))
    assert {("RangeError", COUNTER_ASSIGN), ("TypeError", NOT_A_COUNTER)} <= set(thrown("counters")) and thrown("counters").count(("TypeError", NOT_A_COUNTER)) >= 4
    assert ("RangeError", EMPTY_KEY) in thrown("bounds") and ("TypeError", NOT_A_COUNTER) in thrown("bounds")
    assert all(c["table"] and all(len(o["pred"]) == 1 and o["action"] == "del" for o in c["request"]["ops"]) for c in calls_of("table"))
    assert SESSIONS["nested"]["calls"][1]["objectId"] != "_root" != SESSIONS["nested_inner"]["calls"][1]["objectId"]
    assert {o.get("datatype") for o in ops("mixed_values")} == {None, "int", "uint", "float64", "counter", "timestamp"}
    keys = {o["key"] for o in ops("key_order")}
    assert {"a", "ab", "abc", "abcd"} <= keys and any(len(k.encode()) > 256 for k in keys)
    assert any(0xE000 <= ord(k[0]) <= 0xFFFF for k in keys) and any(ord(k[0]) >= 0x10000 for k in keys), "UTF-16 order differs from byte order"
    assert any(len(o["pred"]) == 2 for o in ops("children"))
    assert any(c["kind"] == "apply" and i > 2 for i, c in enumerate(SESSIONS["conflicts"]["calls"])), "remote changes between the calls"


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the restatement against the requests of the reference's frontend, on the oracle's patch
# ---------------------------------------------------------------------------------------------------------------------------
EMPTY_PATCH = json.dumps({"clock": {}, "deps": [], "maxOp": 0, "pendingChanges": 0, "diffs": {"objectId": "_root", "type": "map", "props": {}}})


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
            patch = session.patch_json() if applied else EMPTY_PATCH
            if call["kind"] == "throws":
                with pytest.raises(THROWN[call["error"]]) as e:
                    request_of_fold(patch, call, last)
                assert str(e.value) == call["message"], f"{name} call {i}"
            else:
                want = dict(call["request"], deps=[h for h in call["request"]["deps"] if h != last]) if call["request"] else None
                assert request_of_fold(patch, call, last) == want, f"{name} call {i}"
            checked += 1
        assert checked >= 2
    finally:
        session.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the fixture's sessions on the engine
# ---------------------------------------------------------------------------------------------------------------------------
def engine_call(eng, call):
    return eng.map_update(call["objectId"], engine_ops(call), call["actor"], time=call["time"])


def check_call_outcome(eng, call, where):
    if call["kind"] == "throws":
        with pytest.raises(engine.EngineError) as e:
            engine_call(eng, call)
        assert e.value.code == (AM355_E_ARG if call["message"] == EMPTY_KEY else AM355_E_INVALID) and call["message"] in str(e.value), where
    elif call["request"] is None:
        assert engine_call(eng, call) == b"", where
    else:
        got = engine_call(eng, call)
        assert got == _b64(call["change"]), f"{where}:\n got  {got.hex()}\n want {_b64(call['change']).hex()}"
        assert same_patch(eng.apply_patch_json(), call["patch"]), f"{where}:\n got  {eng.apply_patch_json()}\n want {call['patch']}"


def object_of(held_values):
    """the JSON the frontend shows for a map, from map_get's answer for all its keys: the value of the greatest op id per key"""
    out = {}
    for key, held in held_values.items():
        if held:
            out[key] = held[max(held, key=_parse)]
    return out


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
            try:
                check_call_outcome(eng, call, where)
            except engine.UnsupportedChanges:
                unsupported.add((name, i))   # (the set is asserted below; the session cannot go on without the change)
                break
            made = call["kind"] != "throws" and call["request"] is not None
            served += call["kind"] != "throws"
            refused += call["kind"] == "throws"
            assert eng.map_calls()[:2] == (served, refused), where
            if at:   # (the first change of a document has no resident state to go onto)
                assert eng.resident_counters()[0] == resident + made, f"{where}: not merged into the resident state"
            assert eng.local_small_calls() == (small[0] + made, small[1]), f"{where}: not built by the one workgroup"
            at += made
            if call["kind"] == "update" and at and not call["table"]:
                # what the keys of the call hold afterwards, against the object the reference's frontend shows
                shown = json.loads(call["object"])
                held = eng.map_get(call["objectId"], [op[1] for op in call["ops"]])
                for key, values in held.items():
                    assert bool(values) == (key in shown), f"{where}: {key!r}"
                    top = values[max(values, key=_parse)] if values else None
                    if values and "objectId" not in top and top.get("datatype") not in ("timestamp", "counter"):
                        assert top["value"] == shown[key], f"{where}: {key!r}"
                    if values and top.get("datatype") == "counter":
                        assert top["value"] == shown[key], f"{where}: {key!r}"
        assert unsupported == {r for r in REFUSED if r[0] == name}
        want = oracle_lib.OracleDoc(ChangeLog.from_changes(s["changes"])).patch_json()
        assert same_patch(eng.patch_json(), want)
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
            if call["kind"] == "apply" or not call["n_before"]:
                continue
            eng.load_changes(ChangeLog.from_changes(s["changes"][:call["n_before"]]))
            eng.replay()
            check_call_outcome(eng, call, f"{name} call {i}")
    finally:
        eng.close()


@pytest.mark.parametrize("name", ["conflicts", "counters", "key_order"])
def test_calls_from_a_fresh_replay_emulated(emu_lib, monkeypatch, name):  # noqa: F811
    _verify(monkeypatch)
    check_calls_from_a_fresh_replay(_emulated(emu_lib), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["conflicts", "counters", "key_order"])
def test_calls_from_a_fresh_replay_gpu(monkeypatch, name):
    _verify(monkeypatch)
    check_calls_from_a_fresh_replay(_gpu, name)


def check_document_context(make_engine):
    """a saved document loaded (Backend.load): map_locate reads it as it is, map_update turns it into the state of its rebuilt changes"""
    s = SESSIONS["conflicts"]
    i, call = next((i, c) for i, c in enumerate(s["calls"]) if c["kind"] == "update" and len(c["request"]["ops"][0]["pred"]) == 3)
    eng = make_engine()
    try:
        eng.load_changes(ChangeLog.from_changes(s["changes"][:call["n_before"]]))
        eng.replay()
        doc = eng.save()
        key = call["ops"][0][1]
        before = eng.map_get("_root", [key])
        eng.load_document(doc)
        eng.replay()
        assert eng.map_get("_root", [key]) == before and len(before[key]) == 3
        check_call_outcome(eng, call, f"conflicts call {i} on the loaded document")
    finally:
        eng.close()


def test_document_context_emulated(emu_lib, monkeypatch):  # noqa: F811
    _verify(monkeypatch)
    check_document_context(_emulated(emu_lib))


@pytest.mark.gpu
def test_document_context_gpu(monkeypatch):
    _verify(monkeypatch)
    check_document_context(_gpu)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. twin contexts: map_update against apply_local_change(the request of the fold)
# ---------------------------------------------------------------------------------------------------------------------------
SWITCHES = {"off": (False, False, False), "map_merge": (True, False, False), "counters": (False, True, False), "all": (True, True, True)}


def _switched(make_engine, which):
    merge, counters, new_objects = SWITCHES[which]
    eng = make_engine()
    eng.set_resident_map_merge(merge)
    eng.set_resident_counters(counters)
    eng.set_resident_new_objects(new_objects)
    return eng


def check_twins(make_engine, name, which):
    s = SESSIONS[name]
    a, b = _switched(make_engine, which), _switched(make_engine, which)
    try:
        at, n = 0, 0
        for i, call in enumerate(s["calls"]):
            if call["kind"] == "apply":
                for eng in (a, b):
                    eng.apply_changes(ChangeLog.from_changes(s["changes"][at:at + call["n"]]))
                at += call["n"]
                continue
            if call["kind"] == "throws" or call["request"] is None or not at:
                continue
            request = request_of_fold(b.patch_json(), call, own_last_hash(s["changes"][:at], call["actor"]))
            got, want = engine_call(a, call), b.apply_local_change(request)
            at += 1
            n += 1
            assert got == want == _b64(call["change"]), f"{name} call {i}"
            assert a.apply_patch_json() == b.apply_patch_json(), f"{name} call {i}"
            assert a.patch_json() == b.patch_json(), f"{name} call {i}"
        assert n >= 4
        assert bytes(a.save()) == bytes(b.save())
        assert a.resident_map_merge_calls() == b.resident_map_merge_calls() and a.resident_counter_calls() == b.resident_counter_calls()
        if which in ("map_merge", "all") and name == "conflicts":
            assert a.resident_map_merge_calls()[0] > 0, "the in-place map merge served none of the calls"
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("which", sorted(SWITCHES))
@pytest.mark.parametrize("name", ["conflicts", "counters"])
def test_twins_emulated(emu_lib, monkeypatch, name, which):  # noqa: F811
    _verify(monkeypatch)
    check_twins(_emulated(emu_lib), name, which)


@pytest.mark.gpu
@pytest.mark.parametrize("which", sorted(SWITCHES))
@pytest.mark.parametrize("name", ["conflicts", "counters"])
def test_twins_gpu(monkeypatch, name, which):
    _verify(monkeypatch)
    check_twins(_gpu, name, which)


ACT_A, ACT_B = "2a" * 16, "b7" * 16
TEXT = f"1@{ACT_A}"


def _text_document():
    """a Text of 41 characters (one op of 41 values), a counter and a few keys on _root, one change"""
    keys = [("alpha", "a"), ("beta", "b"), ("title", "t"), ("zeta", "z")]
    ops = [{"action": "makeText", "obj": "_root", "key": "text", "insert": False, "pred": []},
           {"action": "set", "obj": TEXT, "elemId": "_head", "insert": True, "values": list("the quick brown fox jumps over the lazy d"), "pred": []},
           {"action": "set", "obj": "_root", "key": "votes", "insert": False, "value": 3, "datatype": "counter", "pred": []}]
    ops += [{"action": "set", "obj": "_root", "key": k, "insert": False, "value": v, "pred": []} for k, v in keys]
    return {"actor": ACT_A, "seq": 1, "startOp": 1, "time": 0, "message": "", "deps": [], "ops": ops}


def check_behind_a_text_merge(make_engine, which):
    """A keystroke merged into the resident state in place leaves the edit tables stale; the map call behind it is served from the
    object and map tables as they stand, and makes what a twin makes whose tables were rebuilt and fetched first."""
    a, b = _switched(make_engine, which), _switched(make_engine, which)
    try:
        first, _ = a.encode_change(_text_document())
        for eng in (a, b):
            eng.apply_changes(ChangeLog.from_changes([first]))
        changes = [first]
        calls = [[("set", "title", "x")], [("inc", "votes", 2)], [("set", "title", "y"), ("inc", "votes", -1), ("del", "beta"), ("set", "new", 5)]]
        for k, ops in enumerate(calls):
            for eng in (a, b):
                typed = eng.text_splice(TEXT, 5 + k, 1, ["Q"], ACT_B, time=k)
            changes.append(typed)
            assert a.resident_counters()[2] == k + 1, "the keystroke was not merged in place"
            launches = a.text_splice_calls()[2], a.map_calls()[2]
            b.fetch_ir()   # (the twin: edit tables rebuilt, every table on the host)
            call = {"objectId": "_root", "actor": ACT_B, "time": 100 + k,
                    "ops": [[o[0], o[1], ["int" if isinstance(o[2], int) else "str", o[2]]] if o[0] == "set" else list(o) for o in ops]}
            request = request_of_fold(b.patch_json(), call, own_last_hash(changes, ACT_B))
            got, want = a.map_update("_root", ops, ACT_B, time=100 + k), b.apply_local_change(request)
            changes.append(got)
            assert got == want, f"call {k}"
            assert a.apply_patch_json() == b.apply_patch_json(), f"call {k}"
            # _root needs no lookup, and the call has: the search, the scan, the gather, the signal
            assert (a.text_splice_calls()[2], a.map_calls()[2]) == (launches[0], launches[1] + 4), f"call {k}"
        assert a.patch_json() == b.patch_json()
        assert a.object_text(TEXT)[0] == b.object_text(TEXT)[0]
        assert bytes(a.save()) == bytes(b.save())
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("which", ["off", "all"])
def test_behind_a_text_merge_emulated(emu_lib, monkeypatch, which):  # noqa: F811
    _verify(monkeypatch)
    check_behind_a_text_merge(_emulated(emu_lib), which)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["off", "all"])
def test_behind_a_text_merge_gpu(monkeypatch, which):
    _verify(monkeypatch)
    check_behind_a_text_merge(_gpu, which)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. map_locate / map_get against a fold of fetch_ir's map table at the switch points
# ---------------------------------------------------------------------------------------------------------------------------
class PatchIR(ctypes.Structure):   # am355_patch_ir (include/am355.h)
    _fields_ = [("n_objects", ctypes.c_uint32), ("n_map", ctypes.c_uint32), ("n_edits", ctypes.c_uint32), ("n_values", ctypes.c_uint32),
                ("objects", ctypes.c_void_p), ("map", ctypes.c_void_p), ("edits", ctypes.c_void_p), ("max_op", ctypes.c_uint64),
                ("n_actors", ctypes.c_uint32), ("actor_off", ctypes.c_void_p), ("actor_bytes", ctypes.c_void_p), ("n_clock", ctypes.c_uint32),
                ("clock_actor", ctypes.c_void_p), ("clock_seq", ctypes.c_void_p), ("n_heads", ctypes.c_uint32), ("heads", ctypes.c_void_p),
                ("pending", ctypes.c_uint32), ("arena", ctypes.c_void_p), ("arena_len", ctypes.c_uint64)]


OBJ_DTYPE = np.dtype([(n, "<u4") for n in ("id_ctr", "id_actor", "type", "map_begin", "map_end", "edit_begin", "edit_end", "make_row")])


def _view(ptr, count, dtype):
    return np.frombuffer((ctypes.c_uint8 * (count * dtype.itemsize)).from_address(ptr), dtype=dtype, count=count).copy() if count else np.zeros(0, dtype)


_ORDER = bytes(x - 2 if 0xF0 <= x <= 0xF4 else x + 5 if x in (0xEE, 0xEF) else x for x in range(256))   # utf16_order_byte (csrc/am355_rows.h)


def table_fold(eng):
    """fetch_ir's object and map tables as {object index: (sorted keys in the table's order, their records)} + the object table"""
    ir = PatchIR()
    eng._check(eng._L.am355_fetch_ir(eng._h, ctypes.byref(ir)))
    obj, recs = _view(ir.objects, ir.n_objects, OBJ_DTYPE), _view(ir.map, ir.n_map, engine.IR_MAP_DTYPE)
    arena = _view(ir.arena, ir.arena_len, np.dtype("u1")).tobytes()
    out = {}
    for oi, o in enumerate(obj):
        if int(o["type"]) not in (0, 6):
            continue
        r = recs[int(o["map_begin"]):int(o["map_end"])]
        keys = [arena[int(x["key_off"]):int(x["key_off"]) + int(x["key_len"])].translate(_ORDER) for x in r]
        assert keys == sorted(keys), "the map table is in UTF-16 order"
        out[oi] = (keys, r)
    return obj, out


def fold_locate(folded, key):
    keys, recs = folded
    k = key.encode("utf-8").translate(_ORDER)
    lb, ub = bisect.bisect_left(keys, k), bisect.bisect_right(keys, k)
    return recs[lb:ub]


def check_against_fold(eng, object_id, folded, keys, where):
    hits, recs = eng.map_locate(object_id, keys)
    assert len(hits) == len(keys)
    at = 0
    for key, h in zip(keys, hits):
        want = fold_locate(folded, key)
        assert int(h["first"]) == at and int(h["num"]) == len(want), f"{where}: {key!r}: {h} against {len(want)} records"
        got = recs[at:at + len(want)]
        assert got.tobytes() == want.tobytes(), f"{where}: {key!r}"
        shown = 0 if not len(want) else 2 if int(want[-1]["flags"]) & 2 else 1 if int(want[-1]["flags"]) & 1 or int(want[-1]["val_tl"]) & 15 == 8 else 0
        assert int(h["flags"]) == shown, f"{where}: {key!r}"
        if len(want) > 1:
            ids = [(int(r["id_ctr"]), int(r["id_actor"])) for r in got]
            assert ids == sorted(ids) and len(set(ids)) == len(ids), f"{where}: {key!r}"
        at += len(want)
    assert at == len(recs)


def locate_limits():
    out = (ctypes.c_uint32 * 4)()
    assert engine.load_library().am355_map_locate_limits(out) == 0
    return tuple(int(x) for x in out)


def _key(j):
    return f"k{j:05d}"


def shape_sizes():
    last, pinned_keys, pinned, first_gather = locate_limits()
    return sorted({0, 1, 2, 63, 64, 65, last - 1, last, last + 1, last + 2, last + 3, 4095, 4096, 4097, pinned - 1, pinned, pinned + 1})


N_WRITERS = 65
WIDE_ALL, WIDE_SINGLE = 70, 200   # the map `wide`: its first 70 keys hold the values of all 65 writers, the 200 behind them one value each
WRITERS = [f"{0x40 + k:02x}" * 16 for k in range(N_WRITERS)]
_shape = {}


def big_shape(make_engine):
    """One document, made once and shared by the emulated and the device run. Change 1 (ACT_A): on _root the keys k00000, k00002 and
    zz; then for every size R of shape_sizes() a map m<R> of the R keys k00000, k00002, ... (so that k<odd> lies between two, `a`
    before the first and `z` behind the last, and every neighbour holds the keys that are asked of it); then the map `conf` of 200 such
    keys and the map `tiny` of 3; in front of them the map `wide`, whose first 70 keys every writer overwrites (4,550 records from 70 keys:
    more than the first gather has room for). Changes 2 .. 66 (65 writers, concurrent): every writer overwrites conf[k00200] (a group of 65 in the
    middle), conf[k00398] (65 as the last records of the object) and tiny[k00000] (65 as the first records of an object of 69, the
    last of the table); the first two writers also conf[k00000] (2 values), the first three conf[k00100] and tiny[k00004] (3)."""
    if "log" in _shape:
        return _shape
    sizes = shape_sizes()
    ops, ids, set_id, ctr = [], {}, {}, 1

    def put(op):
        nonlocal ctr
        ops.append(op)
        ctr += 1
        return f"{ctr - 1}@{ACT_A}"

    for k in ("k00000", "k00002", "zz"):
        put({"action": "set", "obj": "_root", "key": k, "insert": False, "value": "root", "pred": []})
    for name, n in [(f"m{r}", r) for r in sizes] + [("wide", WIDE_ALL + WIDE_SINGLE), ("conf", 200), ("tiny", 3)]:
        ids[name] = put({"action": "makeMap", "obj": "_root", "key": name, "insert": False, "pred": []})
        for j in range(n):
            set_id[name, _key(2 * j)] = put({"action": "set", "obj": ids[name], "key": _key(2 * j), "insert": False, "value": j, "pred": []})
    eng = make_engine()
    try:
        first, digest = eng.encode_change({"actor": ACT_A, "seq": 1, "startOp": 1, "time": 0, "message": "", "deps": [], "ops": ops})
        changes = [first]
        for w, actor in enumerate(WRITERS):
            targets = [("conf", _key(200)), ("conf", _key(398)), ("tiny", _key(0))]
            targets += [("conf", _key(0))] if w < 2 else []
            targets += [("conf", _key(100)), ("tiny", _key(4))] if w < 3 else []
            targets += [("wide", _key(2 * j)) for j in range(WIDE_ALL)]
            wops = [{"action": "set", "obj": ids[m], "key": k, "insert": False, "value": f"{w}", "pred": [set_id[m, k]]} for m, k in targets]
            changes.append(eng.encode_change({"actor": actor, "seq": 1, "startOp": ctr, "time": 0, "message": "", "deps": [digest.hex()], "ops": wops})[0])
    finally:
        eng.close()
    _shape.update(log=ChangeLog.from_changes(changes), ids=ids, sizes=sizes)
    return _shape


def queries_for(n):
    """before the first, behind the last, between two, the first, the last, and a few inside, of a map of n keys k00000, k00002, ..."""
    q = ["a", "z", "k", "k0000", "k000000", _key(1), _key(2 * n - 1), _key(2 * n)]
    q += [_key(2 * j) for j in sorted({0, 1, n // 2, n - 2, n - 1}) if 0 <= j < n]
    return q


def check_locate_shapes(make_engine):
    sh = big_shape(make_engine)
    last, pinned_keys, pinned, first_gather = locate_limits()
    ref, eng = make_engine(), make_engine()
    try:
        for e in (ref, eng):
            e.load_changes(sh["log"])
            e.replay()
        obj, folded = table_fold(ref)
        index = {f"{int(o['id_ctr'])}@{ACT_A}": oi for oi, o in enumerate(obj) if oi}
        index["_root"] = 0
        assert len(folded[0][0]) == 3 + len(sh["ids"])
        # ---- every size: the object first in the table (_root), inside it, and last (conf); its neighbours hold the same keys ----
        check_against_fold(eng, "_root", folded[0], queries_for(2) + ["zz", "m0", "conf", "tiny", "tin", "tinyy"], "_root")
        for r in sh["sizes"]:
            oid = sh["ids"][f"m{r}"]
            assert len(folded[index[oid]][0]) == r
            check_against_fold(eng, oid, folded[index[oid]], queries_for(r), f"m{r}")
        served_before = eng.map_calls()[2]
        hits, recs = eng.map_locate(sh["ids"]["m0"], ["a", _key(0)])
        assert [int(h["num"]) for h in hits] == [0, 0] and len(recs) == 0
        hits, recs = eng.map_locate(sh["ids"]["m2"], [])
        assert len(hits) == 0 and len(recs) == 0
        # (nothing is launched for an object without records or for no key, beyond the object lookup)
        assert eng.map_calls()[2] - served_before <= 4
        # ---- groups of 1, 2, 3 and 65 values: in the middle, as the last records of the table, as the first of their object ----
        conf, tiny = sh["ids"]["conf"], sh["ids"]["tiny"]
        assert index[conf] == len(obj) - 2 and index[tiny] == len(obj) - 1
        sizes = lambda oid, keys: [int(h["num"]) for h in eng.map_locate(oid, keys)[0]]   # noqa: E731
        assert sizes(conf, [_key(0), _key(100), _key(200), _key(398), _key(2), _key(399)]) == [2, 3, 65, 65, 1, 0]
        assert sizes(tiny, [_key(0), _key(2), _key(4), _key(1)]) == [65, 1, 3, 0]
        check_against_fold(eng, conf, folded[index[conf]], queries_for(200) + [_key(100), _key(200), _key(199), _key(201), _key(202)], "conf")
        check_against_fold(eng, tiny, folded[index[tiny]], queries_for(3), "tiny")
        # ---- n = 1, 63, 64, 65 keys and the pinned limits +- 1, absent keys among them; a key asked for twice ----
        big = sh["ids"][f"m{pinned + 1}"]
        for n in sorted({1, 63, 64, 65, pinned_keys - 1, pinned_keys, pinned_keys + 1}):
            keys = [_key(j) for j in range(n)]   # (every second one is absent)
            check_against_fold(eng, big, folded[index[big]], keys, f"{n} keys")
        check_against_fold(eng, big, folded[index[big]], [_key(2 * j) for j in range(pinned + 1)], "every key: the records pass the pinned limit by one")
        check_against_fold(eng, big, folded[index[big]], [_key(2 * j) for j in range(pinned)] , "the records reach the pinned limit")
        check_against_fold(eng, conf, folded[index[conf]], [_key(200), _key(0), _key(200), _key(398)], "a key asked for twice")
        with pytest.raises(engine.EngineError, match="ask for a key once") as e:
            eng.map_locate(tiny, [_key(0)] * 8)   # 8 x 65 records > 69 + 8
        assert e.value.code == AM355_E_ARG
        check_against_fold(eng, tiny, folded[index[tiny]], [_key(0)], "served after the refusal")
        # ---- more records than the first gather has room for (2 n + G): the gather runs a second time, two launches more ----
        wide = sh["ids"]["wide"]
        a = (first_gather + 2 * 62 + 62) // 63   # 65 a + b = 2 (a + b) + G  <=>  63 a - b = G, with b single-valued keys
        b = 63 * a - first_gather
        assert a <= WIDE_ALL and 1 <= b < WIDE_SINGLE
        # (every call also looks the object up: two launches, the host's tables are not current here)
        for singles, again in ((b + 1, False), (b, False), (b - 1, True)):   # room to spare, exactly full, one record too many
            keys = [_key(2 * j) for j in range(a)] + [_key(2 * (WIDE_ALL + j)) for j in range(singles)]
            assert (65 * a + singles > 2 * len(keys) + first_gather) == again
            before = eng.map_calls()[2]
            check_against_fold(eng, wide, folded[index[wide]], keys, f"wide, {singles} single keys")
            assert eng.map_calls()[2] - before == 2 + (6 if again else 4), f"wide, {singles} single keys"
        check_against_fold(eng, wide, folded[index[wide]], [_key(2 * j) for j in range(WIDE_ALL + WIDE_SINGLE)], "wide, every key")
        # ---- the host's copy of the object and map tables current (a fetch in front): the lookup and _root's range come from it ----
        eng.fetch_ir()
        before = eng.map_calls()[2]
        check_against_fold(eng, conf, folded[index[conf]], queries_for(200) + [_key(200)], "conf, host tables current")
        check_against_fold(eng, "_root", folded[0], queries_for(2) + ["zz", "conf"], "_root, host tables current")
        assert eng.map_calls()[2] - before == 8, "a lookup was launched although the host's object table is current"
        assert eng.map_locate(sh["ids"]["m0"], ["a"])[0]["num"].tolist() == [0] and eng.map_calls()[2] - before == 8, "an empty object launches nothing"
        # ---- map_get: values, op ids, the shown one ----
        got = eng.map_get(conf, [_key(100), _key(2), "absent"])
        assert got["absent"] == {} and got[_key(2)] == {f"{_parse(conf)[0] + 2}@{ACT_A}": {"value": 1, "datatype": "int"}}
        assert sorted(v["value"] for v in got[_key(100)].values()) == ["0", "1", "2"] and {_parse(k)[1] for k in got[_key(100)]} == set(WRITERS[:3])
        assert eng.map_get("_root", ["conf", "zz"]) == {"conf": {conf: {"objectId": conf}}, "zz": {f"3@{ACT_A}": {"value": "root"}}}
        # ---- one thread per key: the same answers ----
        eng.set_map_locate_thread(True)
        check_against_fold(eng, conf, folded[index[conf]], queries_for(200) + [_key(100), _key(200)], "conf, thread per key")
        check_against_fold(eng, tiny, folded[index[tiny]], queries_for(3), "tiny, thread per key")
        check_against_fold(eng, big, folded[index[big]], [_key(j) for j in range(70)], "thread per key")
    finally:
        ref.close()
        eng.close()


def test_the_shape_is_what_it_says():
    last, pinned_keys, pinned, first_gather = locate_limits()
    assert last < 64 < pinned_keys == pinned == 4096, "else the sizes no longer straddle the limits: add sizes for them"
    assert {0, 1, 2, 63, 64, 65, 4095, 4096, 4097, last, last + 1} <= set(shape_sizes())


def test_locate_at_the_switch_points_emulated(emu_lib, monkeypatch):  # noqa: F811
    _verify(monkeypatch)
    check_locate_shapes(_emulated(emu_lib))


@pytest.mark.gpu
def test_locate_at_the_switch_points_gpu(monkeypatch):
    _verify(monkeypatch)
    check_locate_shapes(_gpu)


def check_locate_on_the_sessions(make_engine):
    """every key of the small documents of the fixture (prefixes, UTF-16 order, keys past the LDS bound), and keys around them"""
    for name in ("key_order", "conflicts", "children", "nested"):
        s = SESSIONS[name]
        for at in sorted({c["n_before"] for c in s["calls"] if c["n_before"]}):
            changes = s["changes"][:at]
            ref, eng = make_engine(), make_engine()
            try:
                for e in (ref, eng):
                    e.load_changes(ChangeLog.from_changes(changes))
                    e.replay()
                obj, folded = table_fold(ref)
                for oi, f in folded.items():
                    oid = "_root" if oi == 0 else f"{int(obj[oi]['id_ctr'])}@{ref.actor_of_rank(int(obj[oi]['id_actor']))}"
                    keys = sorted({c_op[1] for c in calls_of(name) for c_op in c["ops"]} | {"", "a", "ab\0", "", "\U00010000", "k" * 257, "~"})
                    check_against_fold(eng, oid, f, keys, f"{name} at {at}, object {oid}")
                assert folded
            finally:
                ref.close()
                eng.close()


def test_locate_on_the_sessions_emulated(emu_lib, monkeypatch):  # noqa: F811
    _verify(monkeypatch)
    check_locate_on_the_sessions(_emulated(emu_lib))


@pytest.mark.gpu
def test_locate_on_the_sessions_gpu(monkeypatch):
    _verify(monkeypatch)
    check_locate_on_the_sessions(_gpu)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. map_locate changes nothing
# ---------------------------------------------------------------------------------------------------------------------------
def check_locate_changes_nothing(make_engine):
    """Twin contexts through one session; one is asked before and after every call, the other never: same changes, patches, counters."""
    s = SESSIONS["conflicts"]
    a, b = make_engine(), make_engine()
    try:
        at = 0
        keys = ["k2", "k3", "fresh", "solo", "absent"]
        for i, call in enumerate(s["calls"]):
            if at:
                a.map_locate("_root", keys)
                a.map_get("_root", keys[:2])
            if call["kind"] == "apply":
                for eng in (a, b):
                    eng.apply_changes(ChangeLog.from_changes(s["changes"][at:at + call["n"]]))
                at += call["n"]
            else:
                assert engine_call(a, call) == engine_call(b, call), f"call {i}"
                at += 1
            assert a.apply_patch_json() == b.apply_patch_json(), f"call {i}"
            assert a.resident_counters() == b.resident_counters() and a.resident_maps_only_calls() == b.resident_maps_only_calls(), f"call {i}"
            assert a.map_calls()[:2] == b.map_calls()[:2] and a.map_calls()[2] >= b.map_calls()[2]
        assert a.map_calls()[2] > b.map_calls()[2]
        assert a.patch_json() == b.patch_json()
        assert bytes(a.save()) == bytes(b.save())
    finally:
        a.close()
        b.close()


def test_locate_changes_nothing_emulated(emu_lib, monkeypatch):  # noqa: F811
    _verify(monkeypatch)
    check_locate_changes_nothing(_emulated(emu_lib))


@pytest.mark.gpu
def test_locate_changes_nothing_gpu(monkeypatch):
    _verify(monkeypatch)
    check_locate_changes_nothing(_gpu)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. edges and errors: after each refusal the state is still served
# ---------------------------------------------------------------------------------------------------------------------------
def check_edges(make_engine):
    eng = make_engine()
    try:
        with pytest.raises(engine.EngineError) as e:   # no state at all
            eng.map_locate("_root", ["a"])
        assert e.value.code == AM355_E_STATE
        first, _ = eng.encode_change(_text_document())
        eng.apply_changes(ChangeLog.from_changes([first]))
        served = lambda: eng.map_get("_root", ["title"])["title"]   # noqa: E731
        before = served()
        assert list(before.values()) == [{"value": "t"}]

        def refused(code, text, fn):
            n = eng.map_calls()
            with pytest.raises(engine.EngineError) as e:
                fn()
            assert e.value.code == code and text in str(e.value), str(e.value)
            return n

        n = refused(AM355_E_ARG, "not a map object", lambda: eng.map_locate(TEXT, ["a"]))
        assert eng.map_calls()[:2] == n[:2]
        refused(AM355_E_ARG, f"no such object: 9@{ACT_A}", lambda: eng.map_locate(f"9@{ACT_A}", ["a"]))
        refused(AM355_E_ARG, f"no such object: 1@{ACT_B}", lambda: eng.map_locate(f"1@{ACT_B}", ["a"]))
        n = refused(AM355_E_ARG, "not a map object", lambda: eng.map_update(TEXT, [("set", "a", 1)], ACT_B))
        assert eng.map_calls()[:2] == (n[0], n[1] + 1)
        refused(AM355_E_ARG, "no such object", lambda: eng.map_update(f"9@{ACT_A}", [("set", "a", 1)], ACT_B))
        refused(AM355_E_ARG, "named twice", lambda: eng.map_update("_root", [("set", "a", 1), ("del", "a")], ACT_B))
        refused(AM355_E_ARG, EMPTY_KEY, lambda: eng.map_update("_root", [("set", "", 1)], ACT_B))
        refused(AM355_E_INVALID, COUNTER_ASSIGN, lambda: eng.map_update("_root", [("set", "votes", 1)], ACT_B))
        refused(AM355_E_INVALID, NOT_A_COUNTER, lambda: eng.map_update("_root", [("inc", "title", 1)], ACT_B))
        refused(AM355_E_INVALID, NOT_A_COUNTER, lambda: eng.map_update("_root", [("set", "fine", 1), ("inc", "nothing", 1)], ACT_B))
        refused(AM355_E_UNSUPPORTED, "", lambda: eng.map_update("_root", [("set", "a", b"bytes")], ACT_B))
        assert served() == before and eng.map_get("_root", ["fine"]) == {"fine": {}}
        assert json.loads(eng.patch_json())["maxOp"] == len(_text_document()["ops"]) + 40, "a refused call applied something"
        # nothing to do: no change, counted as served
        n = eng.map_calls()
        assert eng.map_update("_root", [], ACT_B) == b"" and eng.map_update("_root", [("del", "absent"), ("del", "")], ACT_B) == b""
        assert eng.map_calls()[:2] == (n[0] + 2, n[1])
        # and the state is still served
        assert eng.map_update("_root", [("set", "title", "T"), ("inc", "votes", 4)], ACT_B, message="hello")
        assert list(served().values()) == [{"value": "T"}]
        assert list(eng.map_get("_root", ["votes"])["votes"].values()) == [{"value": 7, "datatype": "counter"}]
        # a state with a queued change: refused before anything is touched
        orphan, _ = eng.encode_change({"actor": "ee" * 16, "seq": 1, "startOp": 60, "time": 0, "message": "", "deps": ["00" * 32],
                                       "ops": [{"action": "set", "obj": "_root", "key": "q", "insert": False, "value": 1, "pred": []}]})
        eng.apply_changes(ChangeLog.from_changes([orphan]))
        refused(AM355_E_UNSUPPORTED, "queued changes", lambda: eng.map_update("_root", [("set", "title", "U")], ACT_B))
        assert list(served().values()) == [{"value": "T"}]   # (a read is served all the same)
    finally:
        eng.close()


def test_edges_emulated(emu_lib, monkeypatch):  # noqa: F811
    _verify(monkeypatch)
    check_edges(_emulated(emu_lib))


@pytest.mark.gpu
def test_edges_gpu(monkeypatch):
    _verify(monkeypatch)
    check_edges(_gpu)
