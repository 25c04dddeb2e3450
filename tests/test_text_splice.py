"""A Text edited by position on the engine (include/am355.h am355_text_locate, am355_text_splice; csrc/am355_locate.hip kl_check,
kl_locate, kl_runs): position -> (elemId, pred) on the device, and from there exactly the change request the reference's frontend hands
to Backend.applyLocalChange for text.deleteAt / text.insertAt (frontend/context.js:441-502 splice).

1. The restatement, without an engine: a fold of the ORACLE's whole-document patch into (elemId, pred) per element by the rule of
   frontend/apply_patch.js:231-255, turned into a request by context.js's rule, equals the request the reference's frontend made, for
   every call of every session of tests/golden/text/text_splices.json (tools/fixtures/make_text_splices.js).
2. The fixture's sessions on the engine: call by call from a fresh replay, and the whole session on one context.
3. Twin contexts: text_splice against apply_local_change(the request of the fold).
4. text_locate against the fold at the kernels' switch points (am355_text_locate_limits).
5. Edges and errors; after each refusal the state is still served.
6. text_locate changes nothing.

Each engine body runs on the emulation (CPU suite) and on the device, with AM355_RESORDER_VERIFY=1 and AM355_LOCAL_SMALL_VERIFY=1.

A COUNTER INSIDE A TEXT. context.js:455-471 throws a TypeError when a deletion reaches a Counter, and am355_text_splice refuses such a
call with that text (AM355_E_INVALID). The reference's frontend itself only throws for a LIST: it looks the element up as
object[index], which a Text object does not have, so text.deleteAt over a counter deletes it. The fixture records what the reference
did (calls of kind 'counter', made on a copy of the replica); the fold reproduces those requests too; the engine refuses them."""
import base64
import ctypes
import hashlib
import json
import os
import zlib

import pytest

import oracle_lib
import test_local_small as tls
from automerge_classic_amd import engine
from automerge_classic_amd.loggen import ChangeLog
from golden_util import same_patch
from test_local_change import emu_lib  # noqa: F401 (the fixture that builds the emulation)

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "text", "text_splices.json")
AM355_E_ARG, AM355_E_INVALID, AM355_E_UNSUPPORTED, AM355_E_STATE = -2, -3, -4, -5
COUNTER_TEXT = "Unsupported operation: deleting a counter from a list"
SESSION_NAMES = ["typed", "two_actors", "conflicts", "holes", "edges", "counters"]


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
_emulated, _gpu = tls._emulated, tls._gpu   # (the switches the JS host turns on, and the one-workgroup build of small changes)


def _verify(monkeypatch):
    tls._verify(monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------------
# the rule, restated over a patch
# ---------------------------------------------------------------------------------------------------------------------------
def _parse(op_id):
    ctr, actor = op_id.split("@")
    return int(ctr), actor


def _is_counter(value):
    return value.get("datatype") == "counter"


def elements_of_patch(patch_json):
    """{objectId: [(elemId, pred, is a counter)]} of every Text of a whole-document patch: updateTextObject (apply_patch.js:231-255)
    applied to an empty object. insert: pred = opId; multi-insert: elemIds count up from edit.elemId, pred = the elemId; update: the
    element is replaced, pred = opId, the elemId kept."""
    out = {}

    def walk(diff):
        for values in diff.get("props", {}).values():
            for v in values.values():
                if "objectId" in v:
                    walk(v)
        if "edits" not in diff:
            return
        elems = []
        for e in diff["edits"]:
            a, i = e["action"], e["index"]
            if a == "insert":
                elems.insert(i, (e["elemId"], e["opId"], _is_counter(e["value"])))
            elif a == "multi-insert":
                ctr, actor = _parse(e["elemId"])
                ids = [f"{ctr + k}@{actor}" for k in range(len(e["values"]))]
                elems[i:i] = [(x, x, e.get("datatype") == "counter") for x in ids]
            elif a == "update":
                elems[i] = (elems[i][0], e["opId"], _is_counter(e["value"]))
            else:
                raise AssertionError(f"{a} edit in a whole-document patch")
            if isinstance(e.get("value"), dict) and "objectId" in e["value"]:
                walk(e["value"])
        if diff["type"] == "text":
            out[diff["objectId"]] = elems

    walk(json.loads(patch_json)["diffs"])
    return out


def runs_of(elems, lead=0):
    """context.js:474-492: a deletion joins the one before it iff elemId and pred have equal actors and consecutive counters.
    [(elemId, pred, count, holds a counter)]; element `lead` (1: the first element is no deletion) always starts a run."""
    runs = []
    for k, (elem, pred, counter) in enumerate(elems):
        (ec, ea), (pc, pa) = _parse(elem), _parse(pred)
        if runs and k != lead:
            (lec, lea), (lpc, lpa), n = _parse(runs[-1][0]), _parse(runs[-1][1]), runs[-1][2]
            if lea == ea and lec + n == ec and lpa == pa and lpc + n == pc:
                runs[-1] = (runs[-1][0], runs[-1][1], n + 1, runs[-1][3] or counter)
                continue
        runs.append((elem, pred, 1, counter))
    return runs


class OutOfBounds(Exception):
    pass


def request_of_fold(patch_json, object_id, start, deletions, values, actor, time, own_last_hash=None, refuse_counters=False):
    """The change request of context.splice(path, start, deletions, values) (context.js:441-502, :370-405 insertListItems) onto the
    state of a whole-document patch, or None when there is nothing to do. own_last_hash: the hash of the author's last change, which the
    frontend's deps do not hold (backend.js:88-89)."""
    patch = json.loads(patch_json)
    elems = elements_of_patch(patch_json)[object_id]
    if start < 0 or deletions < 0 or start > len(elems) - deletions:
        raise OutOfBounds(f"{deletions} deletions starting at index {start} are out of bounds for list of length {len(elems)}")
    if deletions == 0 and not values:
        return None
    ops = []
    for elem, pred, count, counter in runs_of(elems[start:start + deletions]):
        if counter and refuse_counters:
            raise TypeError(COUNTER_TEXT)
        op = {"action": "del", "obj": object_id, "elemId": elem, "insert": False, "pred": [pred]}
        if count > 1:
            op["multiOp"] = count
        ops.append(op)
    if values:
        op = {"action": "set", "obj": object_id, "elemId": elems[start - 1][0] if start else "_head", "insert": True}
        if len(values) > 1:
            op["values"] = list(values)
        else:
            op["value"] = values[0]
        op["pred"] = []
        ops.append(op)
    return {"actor": actor, "seq": patch["clock"].get(actor, 0) + 1, "startOp": patch["maxOp"] + 1, "deps": [h for h in patch["deps"] if h != own_last_hash],
            "time": time, "message": "", "ops": ops}


def _uleb(b, off):
    v = shift = 0
    while True:
        x = b[off]
        off += 1
        v |= (x & 127) << shift
        shift += 7
        if not x & 128:
            return v, off


def change_info(change):
    """(hash, author, seq) of a binary change (columnar.js:693-760): the hash is over the uncompressed chunk."""
    kind, (n, off) = change[8], _uleb(change, 9)
    body = change[off:off + n]
    if kind == 2:
        body = zlib.decompress(body, -15)
        head = bytearray([1])
        n = len(body)
        while True:
            head.append((n & 127) | (128 if n > 127 else 0))
            n >>= 7
            if not n:
                break
        chunk = bytes(head) + body
    else:
        chunk = change[8:]
    n_deps, at = _uleb(body, 0)
    at += 32 * n_deps
    alen, at = _uleb(body, at)
    actor = body[at:at + alen].hex()
    seq, _ = _uleb(body, at + alen)
    return hashlib.sha256(chunk).hexdigest(), actor, seq


def own_last_hash(changes, actor):
    best = None
    for c in changes:
        h, a, seq = change_info(c)
        if a == actor and (best is None or seq > best[0]):
            best = (seq, h)
    return best[1] if best else None


def test_the_fixture_holds_every_session():
    assert sorted(SESSIONS) == sorted(SESSION_NAMES)
    assert os.path.getsize(FIXTURE) < (1 << 20)
    kinds = lambda name: [c["kind"] for c in SESSIONS[name]["calls"]]   # noqa: E731
    ops = lambda name: [len(c["request"]["ops"]) for c in SESSIONS[name]["calls"] if c["kind"] == "splice" and c["request"]]   # noqa: E731
    assert max(ops("typed")) >= 3 and max(ops("holes")) >= 3
    # two actors in turns: a deletion of five elements is five ops
    first = next(c for c in SESSIONS["two_actors"]["calls"] if c["kind"] == "splice")
    assert first["deletions"] == 5 and len(first["request"]["ops"]) == 5 and all("multiOp" not in o for o in first["request"]["ops"])
    assert "throws" in kinds("edges") and any(c["kind"] == "splice" and c["request"] is None for c in SESSIONS["edges"]["calls"])
    assert any(c["kind"] == "splice" and c["request"] and c["request"]["ops"][-1].get("elemId") == "_head" for c in SESSIONS["edges"]["calls"])
    assert any(c["kind"] == "splice" and c["length"] == 0 and c["deletions"] for c in SESSIONS["edges"]["calls"]), "the whole text deleted"
    assert any(len(v.encode()) == 4 for c in SESSIONS["edges"]["calls"] if c["kind"] == "splice" for v in c["values"]), "an astral character"
    assert kinds("counters").count("counter") == 4
    # the pred of a conflicting element is the last update's: a deletion in `conflicts` whose pred is no elemId of the typed run
    assert any(o["action"] == "del" and o["pred"][0].split("@")[1] != o["elemId"].split("@")[1]
               for c in SESSIONS["conflicts"]["calls"] if c["kind"] == "splice" for o in c["request"]["ops"])


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
            args = (session.patch_json(), call["objectId"], call["start"], call["deletions"], call["values"], call["actor"], call["time"])
            last = own_last_hash(s["changes"][:applied], call["actor"])
            if call["kind"] == "throws":
                assert call["error"] == "RangeError"
                with pytest.raises(OutOfBounds) as e:
                    request_of_fold(*args, own_last_hash=last)
                assert str(e.value) == call["message"], f"{name} call {i}"
            else:
                # (the frontend's deps are those of the last patch it saw: without the author's last hash behind applyLocalChange,
                # backend.js:88-89, with it behind an applyChanges that left it a head. applyLocalChange adds that hash itself and
                # keeps each hash once, backend.js:73-81: the change is the same, and the comparison leaves the hash out on both sides)
                want = dict(call["request"], deps=[h for h in call["request"]["deps"] if h != last]) if call["request"] else None
                assert request_of_fold(*args, own_last_hash=last) == want, f"{name} call {i}"
                if call["kind"] == "counter":
                    with pytest.raises(TypeError):
                        request_of_fold(*args, own_last_hash=last, refuse_counters=True)
            checked += 1
        assert checked >= 6
    finally:
        session.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the fixture's sessions on the engine
# ---------------------------------------------------------------------------------------------------------------------------
def splice_call(eng, call):
    return eng.text_splice(call["objectId"], call["start"], call["deletions"], call["values"], call["actor"], time=call["time"])


def check_call_outcome(eng, call, where):
    """One recorded call on a context that holds the state before it."""
    if call["kind"] == "throws":
        with pytest.raises(engine.EngineError) as e:
            splice_call(eng, call)
        assert e.value.code == AM355_E_ARG and call["message"] in str(e.value), where
    elif call["kind"] == "counter":
        with pytest.raises(engine.InvalidChanges, match=COUNTER_TEXT):
            splice_call(eng, call)
    elif call["request"] is None:
        assert splice_call(eng, call) == b"", where
    else:
        got = splice_call(eng, call)
        assert got == _b64(call["change"]), f"{where}:\n got  {got.hex()}\n want {_b64(call['change']).hex()}"
        assert same_patch(eng.apply_patch_json(), call["patch"]), f"{where}:\n got  {eng.apply_patch_json()}\n want {call['patch']}"
    if call["kind"] == "splice":
        text, info = eng.object_text(call["objectId"])
        assert text.decode("utf-8") == call["text"] and info.n_elements == call["length"], where


def check_calls_from_a_fresh_replay(make_engine, name):
    s = SESSIONS[name]
    eng = make_engine()
    try:
        for i, call in enumerate(s["calls"]):
            if call["kind"] == "apply":
                continue
            eng.load_changes(ChangeLog.from_changes(s["changes"][:call["n_before"]]))
            eng.replay()
            check_call_outcome(eng, call, f"{name} call {i}")
    finally:
        eng.close()


@pytest.mark.parametrize("name", SESSION_NAMES)
def test_calls_from_a_fresh_replay_emulated(emu_lib, monkeypatch, name):  # noqa: F811
    _verify(monkeypatch)
    check_calls_from_a_fresh_replay(_emulated(emu_lib), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SESSION_NAMES)
def test_calls_from_a_fresh_replay_gpu(monkeypatch, name):
    _verify(monkeypatch)
    check_calls_from_a_fresh_replay(_gpu, name)


def check_whole_session(make_engine, name):
    """Call after call on one context: the resident path and the one-workgroup build serve every splice."""
    s = SESSIONS[name]
    eng = make_engine()
    try:
        at, served, refused = 0, 0, 0
        for i, call in enumerate(s["calls"]):
            where = f"{name} call {i}"
            assert call["n_before"] == at, where
            if call["kind"] == "apply":
                eng.apply_changes(ChangeLog.from_changes(s["changes"][at:at + call["n"]]))
                at += call["n"]
                continue
            resident, small = eng.resident_counters()[0], eng.local_small_calls()
            check_call_outcome(eng, call, where)
            made = call["kind"] == "splice" and call["request"] is not None
            served += call["kind"] == "splice"
            refused += call["kind"] != "splice"
            at += made
            assert eng.text_splice_calls()[:2] == (served, refused), where
            assert eng.resident_counters()[0] == resident + made, f"{where}: not merged into the resident state"
            assert eng.local_small_calls() == (small[0] + made, small[1]), f"{where}: not built by the one workgroup"
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


# ---------------------------------------------------------------------------------------------------------------------------
# 3. twin contexts: text_splice against apply_local_change(the request of the fold)
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
            if call["kind"] != "splice" or call["request"] is None:
                continue
            request = request_of_fold(b.patch_json(), call["objectId"], call["start"], call["deletions"], call["values"], call["actor"], call["time"],
                                      own_last_hash=own_last_hash(s["changes"][:at], call["actor"]))
            got, want = splice_call(a, call), b.apply_local_change(request)
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
# 4. text_locate against the fold at the switch points
# ---------------------------------------------------------------------------------------------------------------------------
def locate_limits():
    out = (ctypes.c_uint32 * 3)()
    assert engine.load_library().am355_text_locate_limits(out) == 0
    return tuple(int(x) for x in out)


ACT_A, ACT_B = "2a" * 16, "b7" * 16
TEXT = f"1@{ACT_A}"


def query_sizes():
    b, s, _ = locate_limits()
    return [1, b - 1, b, b + 1, 2 * b + 1, s, s + 1]


def _make_text(values):
    return {"actor": ACT_A, "seq": 1, "startOp": 1, "time": 0, "message": "", "deps": [],
            "ops": [{"action": "makeText", "obj": "_root", "key": "text", "insert": False, "pred": []},
                    {"action": "set", "obj": TEXT, "elemId": "_head", "insert": True, "values": values, "pred": []}]}


def alternating_requests(half):
    """A pastes `half` characters; B, who has seen them, types one character behind each: a0 b0 a1 b1 ... -- neighbours have different
    actors, so every element is a record and a run of its own."""
    first = _make_text(["a"] * half)
    second = lambda dep: {"actor": ACT_B, "seq": 1, "startOp": half + 2, "time": 0, "message": "", "deps": [dep],   # noqa: E731
                          "ops": [{"action": "set", "obj": TEXT, "elemId": f"{2 + k}@{ACT_A}", "insert": True, "value": "b", "pred": []} for k in range(half)]}
    return [first, second]


def updated_requests(n):
    """A pastes n characters, B assigns to the LAST of them, A pastes n more behind it: the element at index n - 1 is an updated last
    value of a record."""
    first = _make_text(["u"] * n)
    second = lambda dep: {"actor": ACT_B, "seq": 1, "startOp": n + 2, "time": 0, "message": "", "deps": [dep],   # noqa: E731
                          "ops": [{"action": "set", "obj": TEXT, "elemId": f"{n + 1}@{ACT_A}", "insert": False, "value": "W", "pred": [f"{n + 1}@{ACT_A}"]}]}
    third = lambda dep: {"actor": ACT_A, "seq": 2, "startOp": n + 3, "time": 0, "message": "", "deps": [dep],   # noqa: E731
                         "ops": [{"action": "set", "obj": TEXT, "elemId": f"{n + 1}@{ACT_A}", "insert": True, "values": ["v"] * n, "pred": []}]}
    return [first, second, third]


_shapes = {}


def shape(make_engine, key):
    """(log, the Text's elements by the fold of the ORACLE's patch, actor ranks): made once, shared by the emulated and the device run."""
    if key not in _shapes:
        s = locate_limits()[1]
        requests = {"alternating": lambda: alternating_requests(s // 2 + 4), "pasted": lambda: [_make_text(["p"] * (s + 40))],
                    "updated": lambda: updated_requests(s + 8)}[key]()
        eng = make_engine()
        try:
            changes, dep = [], None
            for r in requests:
                change, digest = eng.encode_change(r if dep is None else r(dep))
                changes.append(change)
                dep = digest.hex()
        finally:
            eng.close()
        log = ChangeLog.from_changes(changes)
        elems = elements_of_patch(oracle_lib.OracleDoc(log).patch_json())[TEXT]
        _shapes[key] = (log, elems, {a: k for k, a in enumerate(sorted([ACT_A, ACT_B]))})
    return _shapes[key]


def as_tuples(runs, rank):
    out = []
    for elem, pred, count, counter in runs:
        (ec, ea), (pc, pa) = _parse(elem), _parse(pred)
        out.append((ec, rank[ea], pc, rank[pa], count, 1 if counter else 0))
    return out


def check_locate(make_engine, key, ranges, expect_runs=None):
    """ranges(elements, n) -> the first position of a query of n elements."""
    log, elems, rank = shape(make_engine, key)
    eng = make_engine()
    try:
        eng.load_changes(log)
        eng.replay()
        for n in query_sizes():
            for first in ranges(len(elems), n):
                runs, length = eng.text_locate(TEXT, first, n)
                want = as_tuples(runs_of(elems[first:first + n]), rank)
                assert length == len(elems)
                assert [tuple(int(x) for x in r) for r in runs] == want, f"{key}: [{first}, {first} + {n})"
                if expect_runs:
                    assert len(runs) == expect_runs(n), f"{key}: [{first}, {first} + {n})"
    finally:
        eng.close()


LOCATE_SHAPES = {
    # every element is a run: n_runs == n, a run boundary on every workgroup edge; n == S + ... straddles the pinned bound of the run buffer
    "alternating": (lambda total, n: [0, 3], lambda n: n),
    # one pasted record longer than the query: one run, the range begins and ends inside the record
    "pasted": (lambda total, n: [5], lambda n: 1),
    # the updated last value of a record as the first element of the range, and as the last one
    "updated": (lambda total, n: [total // 2 - 1, total // 2 - n], None),
}


def test_the_pinned_bound_of_the_run_buffer_lies_below_the_scan_limit():
    b, s, pinned = locate_limits()
    assert b < pinned < s, "else the alternating shape no longer straddles the bound: add a shape for it"


def test_the_updated_shape_is_what_it_says(emu_lib):  # noqa: F811
    _, elems, _ = shape(_emulated(emu_lib), "updated")
    k = len(elems) // 2 - 1
    assert elems[k][1].endswith(ACT_B) and elems[k][0].endswith(ACT_A) and elems[k - 1][0] == elems[k - 1][1] and elems[k + 1][0] == elems[k + 1][1]
    assert len(runs_of(elems[k - 2:k + 3])) == 3


@pytest.mark.parametrize("key", sorted(LOCATE_SHAPES))
def test_locate_at_the_switch_points_emulated(emu_lib, monkeypatch, key):  # noqa: F811
    _verify(monkeypatch)
    check_locate(_emulated(emu_lib), key, *LOCATE_SHAPES[key])


@pytest.mark.gpu
@pytest.mark.parametrize("key", sorted(LOCATE_SHAPES))
def test_locate_at_the_switch_points_gpu(monkeypatch, key):
    _verify(monkeypatch)
    check_locate(_gpu, key, *LOCATE_SHAPES[key])


def check_locate_on_the_sessions(make_engine):
    """Every range of the small documents of the fixture, counters and conflicts included."""
    for name in ("conflicts", "counters", "two_actors"):
        s = SESSIONS[name]
        want_all = elements_of_patch(s["whole_patch"])
        actors = sorted({change_info(c)[1] for c in s["changes"]})
        rank = {a: k for k, a in enumerate(actors)}
        eng = make_engine()
        try:
            eng.load_changes(ChangeLog.from_changes(s["changes"]))
            eng.replay()
            for oid, elems in want_all.items():
                for first in range(len(elems) + 1):
                    for n in range(len(elems) - first + 1):
                        runs, length = eng.text_locate(oid, first, n)
                        assert length == len(elems)
                        assert [tuple(int(x) for x in r) for r in runs] == as_tuples(runs_of(elems[first:first + n]), rank), f"{name}: [{first}, {first} + {n})"
        finally:
            eng.close()
    assert any(c for _, _, c in elements_of_patch(SESSIONS["counters"]["whole_patch"]).popitem()[1]), "a counter in the Text"


def test_locate_on_the_sessions_emulated(emu_lib, monkeypatch):  # noqa: F811
    _verify(monkeypatch)
    check_locate_on_the_sessions(_emulated(emu_lib))


@pytest.mark.gpu
def test_locate_on_the_sessions_gpu(monkeypatch):
    _verify(monkeypatch)
    check_locate_on_the_sessions(_gpu)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. edges and errors; after each refusal the state is still served
# ---------------------------------------------------------------------------------------------------------------------------
OBJECTS = {"actor": ACT_A, "seq": 1, "startOp": 1, "time": 0, "message": "", "deps": [],
           "ops": [{"action": "makeText", "obj": "_root", "key": "text", "insert": False, "pred": []},
                   {"action": "set", "obj": TEXT, "elemId": "_head", "insert": True, "values": list("hello"), "pred": []},
                   {"action": "makeList", "obj": "_root", "key": "list", "insert": False, "pred": []},
                   {"action": "makeText", "obj": "_root", "key": "empty", "insert": False, "pred": []},
                   {"action": "makeMap", "obj": "_root", "key": "map", "insert": False, "pred": []}]}
LIST, EMPTY, MAP = f"7@{ACT_A}", f"8@{ACT_A}", f"9@{ACT_A}"


def check_errors(make_engine, refused_launches=None):
    asked, twin = make_engine(), make_engine()
    try:
        with pytest.raises(engine.EngineError) as e:   # no state
            asked.text_splice(TEXT, 0, 0, ["x"], ACT_B)
        assert e.value.code == AM355_E_STATE
        with pytest.raises(engine.EngineError) as e:
            asked.text_locate(TEXT, 0, 0)
        assert e.value.code == AM355_E_STATE
        made, _ = twin.encode_change(OBJECTS)
        for eng in (asked, twin):
            eng.apply_changes(ChangeLog.from_changes([made]))
        refused = 1   # (splices refused: text_locate is not counted)
        step = [0]

        def still_served(where):
            """a valid splice on both contexts: the same change, the same patch"""
            step[0] += 1
            args = (TEXT, step[0] % 3, 1, ["é", str(step[0])], ACT_B)
            got, want = asked.text_splice(*args, time=step[0]), twin.text_splice(*args, time=step[0])
            assert got and got == want and asked.apply_patch_json() == twin.apply_patch_json(), where
            assert asked.patch_json() == twin.patch_json(), where
            assert asked.text_splice_calls()[:2] == (step[0], refused), where

        still_served("after the calls without a state")
        before = refused_launches() if refused_launches else None
        # the empty Text, and n == 0
        assert asked.text_locate(EMPTY, 0, 0)[1] == 0 and len(asked.text_locate(EMPTY, 0, 0)[0]) == 0
        runs, length = asked.text_locate(TEXT, 2, 0)
        assert len(runs) == 0 and length == 6
        assert asked.text_locate(TEXT, length, 0)[1] == 6
        assert asked.text_splice(EMPTY, 0, 0, [], ACT_B) == b"" and asked.text_splice(TEXT, 3, 0, [], ACT_B) == b""   # nothing to do
        step[0] += 2   # (both are served)
        if refused_launches:
            assert refused_launches() == before, "an empty Text or an empty range made the engine launch an empty grid"
        for oid, first, n in ((EMPTY, 0, 1), (TEXT, 6, 1), (TEXT, 0, 7), (TEXT, 7, 0), (TEXT, 2 ** 40, 1), (TEXT, 1, 2 ** 64 - 1)):
            with pytest.raises(engine.EngineError, match="out of bounds") as e:
                asked.text_locate(oid, first, n)
            assert e.value.code == AM355_E_ARG
        for start, deletions in ((7, 0), (6, 1), (0, 7), (2 ** 33, 2), (2, 2 ** 64 - 2)):
            with pytest.raises(engine.EngineError) as e:
                asked.text_splice(TEXT, start, deletions, ["x"], ACT_B)
            assert e.value.code == AM355_E_ARG
            assert f"{deletions} deletions starting at index {start} are out of bounds for list of length 6" in str(e.value)
            refused += 1
        still_served("after the calls out of bounds")
        ctr, actor = TEXT.split("@")
        for oid, text in ((LIST, "not a Text object"), (MAP, "not a Text object"), ("_root", "not a Text object"), (f"99@{actor}", f"no such object: 99@{actor}"),
                          (f"{ctr}@{'0' * 32}", "no such object"), (f"{ctr}@{actor}ff", "no such object")):
            with pytest.raises(engine.EngineError, match=text) as e:
                asked.text_splice(oid, 0, 0, ["x"], ACT_B)
            assert e.value.code == AM355_E_ARG
            with pytest.raises(engine.EngineError, match=text) as e:
                asked.text_locate(oid, 0, 0)
            assert e.value.code == AM355_E_ARG
            refused += 1
        still_served("after the calls that name no Text")
        # everything deleted, then typed into again from _head; start == length
        for eng in (asked, twin):
            n = eng.text_locate(TEXT, 0, 0)[1]
            assert eng.text_splice(TEXT, 0, n, [], ACT_B) and eng.object_text(TEXT)[0] == b""
            assert eng.text_splice(TEXT, 0, 0, ["a"], ACT_B) and eng.text_splice(TEXT, 1, 0, ["b", "c"], ACT_B)
            assert eng.object_text(TEXT)[0] == b"abc"
        step[0] += 3
        still_served("after the whole text was deleted")
        # queued changes: a change whose dependency is missing waits in the state
        other = dict(OBJECTS, actor="c3" * 16, ops=[{"action": "set", "obj": "_root", "key": "k", "insert": False, "value": 1, "pred": []}], startOp=50)
        base, base_hash = twin.encode_change(other)
        late, _ = twin.encode_change(dict(other, seq=2, startOp=51, deps=[base_hash.hex()]))
        asked.apply_changes(ChangeLog.from_changes([late]))
        with pytest.raises(engine.UnsupportedChanges, match="queued changes"):
            asked.text_splice(TEXT, 0, 0, ["x"], ACT_B)
        refused += 1
        asked.apply_changes(ChangeLog.from_changes([base]))
        twin.apply_changes(ChangeLog.from_changes([base, late]))
        still_served("after the call onto queued changes")
    finally:
        asked.close()
        twin.close()
    eng = make_engine()
    try:
        eng.set_shard(0, 2)
        eng.load_changes(ChangeLog.from_changes([made]))
        eng.replay()
        for call in (lambda: eng.text_locate(TEXT, 0, 1), lambda: eng.text_splice(TEXT, 0, 0, ["x"], ACT_B)):
            with pytest.raises(engine.UnsupportedChanges, match="sharded"):
                call()
    finally:
        eng.close()


def test_edges_and_errors_emulated(emu_lib, monkeypatch):  # noqa: F811
    _verify(monkeypatch)
    lib = engine.load_library(emu_lib)
    lib.am355_emu_refused_launches.argtypes = [ctypes.POINTER(ctypes.c_char_p)]
    lib.am355_emu_refused_launches.restype = ctypes.c_long
    check_errors(_emulated(emu_lib), lambda: int(lib.am355_emu_refused_launches(ctypes.byref(ctypes.c_char_p()))))


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
        doc = bytes(twin.save())
        eng.backend_load(doc)
        elems = elements_of_patch(twin.patch_json())[call["objectId"]]
        runs, length = eng.text_locate(call["objectId"], 0, len(elems))
        assert length == len(elems) and sum(int(r["count"]) for r in runs) == len(elems) and len(runs) == len(runs_of(elems))
        assert splice_call(eng, call) == _b64(call["change"])
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
# 6. locate changes nothing
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
            elif call["kind"] == "splice" and call["request"]:
                assert splice_call(asked, call) == splice_call(twin, call) == _b64(call["change"]), where
                assert asked.apply_patch_json() == twin.apply_patch_json(), where
                at += 1
            else:
                continue
            oid = next(c["objectId"] for c in s["calls"] if c["kind"] != "apply")
            length = asked.text_locate(oid, 0, 0)[1]
            runs, _ = asked.text_locate(oid, 0, length)
            assert sum(int(r["count"]) for r in runs) == length, where
            if length > 2:
                asked.text_locate(oid, 1, length - 2)
            assert asked.resident_counters() == twin.resident_counters(), f"{where}: the query changed what serves the next call"
            assert asked.local_small_calls() == twin.local_small_calls(), where
        assert asked.text_splice_calls()[:2] == twin.text_splice_calls()[:2]
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
