"""ElemIds of a Text resolved to positions on the engine (include/am355.h am355_text_position; csrc/am355_position.hip kp_heads,
kp_resolve): VISIBLE at the element's index, DELETED at the number of visible elements in front of where it stood, UNKNOWN for an
element no applied change inserted into the object. The reference has no cursor call; the definition is a probe on its public backend
(tools/fixtures/make_text_positions.js), recorded in tests/golden/text/text_positions.json.

1. The model, without an engine: an RGA built from the insert ops (children of an element by descending op id), visibility from the
   ORACLE's whole-document patch. It equals the fixture on every query of every checkpoint, and supplies the expectations below.
2. The fixture on the engine: every checkpoint from a fresh replay, and the whole session on one context -- behind in-place
   apply_changes (stale tables) and behind text_splice. The only refusals are the checkpoints of `remove_record`.
3. Round trip: text_positions(text_locate(j).elemId) == (VISIBLE, j) for every j.
4. The kernels' switch points (am355_text_position_limits, am355_text_locate_limits) on generated logs.
5. Edges and errors; after each refusal the state is still served.
6. The call reads only: a twin context that is never asked gives the same following patch and the same saved bytes.

Each engine body runs on the emulation (CPU suite) and on the device, with AM355_RESORDER_VERIFY=1."""
import base64
import ctypes
import json
import os

import pytest

import oracle_lib
import test_local_small as tls
from automerge_classic_amd import engine
from automerge_classic_amd.engine import POS_DELETED, POS_UNKNOWN, POS_VISIBLE
from automerge_classic_amd.loggen import ChangeLog
from test_local_change import emu_lib  # noqa: F401 (the fixture that builds the emulation)
from test_text_splice import elements_of_patch

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "text", "text_positions.json")
AM355_E_ARG, AM355_E_UNSUPPORTED, AM355_E_STATE = -2, -4, -5
SESSION_NAMES = ["typed", "two_actors", "holes", "updates", "all_deleted", "counters", "remove_record"]
STATUS = {"unknown": POS_UNKNOWN, "visible": POS_VISIBLE, "deleted": POS_DELETED}
REMOVE_TEXT = "a `remove` record"


def load_sessions():
    with open(FIXTURE) as f:
        fx = json.load(f)
    out = {}
    for s in fx["sessions"]:
        s = dict(s)
        s["changes"] = [base64.b64decode(c) for c in s["changes"]]
        out[s["name"]] = s
    return out


SESSIONS = load_sessions()
_emulated, _gpu = tls._emulated, tls._gpu


def _verify(monkeypatch):
    tls._verify(monkeypatch)


def want_of(checkpoint):
    return [(STATUS[status], position, bool(counter)) for _, status, position, counter in checkpoint["queries"]]


def ids_of(checkpoint):
    return [q[0] for q in checkpoint["queries"]]


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the model
# ---------------------------------------------------------------------------------------------------------------------------
def _op_key(op_id):
    ctr, actor = op_id.split("@")
    return int(ctr), actor   # (Lamport order: the counter, then the actor id as a string -- hex of equal length: byte order)


def document_order(inserts):
    """Every element ever inserted, tombstones included, in document order: a new element goes directly behind its reference element, in
    front of that element's children with smaller op ids -- so the children of an element stand by DESCENDING op id, each followed by
    its own subtree (backend/new.js:144-163). inserts: [(elemId, the elemId or '_head' it was inserted behind)]."""
    children = {}
    for elem, after in inserts:
        children.setdefault(after, []).append(elem)
    order, stack = [], [iter(sorted(children.get("_head", []), key=_op_key, reverse=True))]
    while stack:
        elem = next(stack[-1], None)
        if elem is None:
            stack.pop()
            continue
        order.append(elem)
        stack.append(iter(sorted(children.get(elem, []), key=_op_key, reverse=True)))
    assert len(order) == len(inserts), "an element was inserted behind one that does not exist"
    return order


def model_positions(inserts, visible, queries):
    """[(status, position, is a counter)] of the queries. visible: [(elemId, pred, is a counter)] of the Text in index order (the fold of
    the oracle's patch, test_text_splice.elements_of_patch)."""
    counter = {e: c for e, _, c in visible}
    where, in_front = {}, 0
    for elem in document_order(inserts):
        if elem in counter:
            where[elem] = (POS_VISIBLE, in_front, bool(counter[elem]))
            in_front += 1
        else:
            where[elem] = (POS_DELETED, in_front, False)
    assert in_front == len(visible) and [e for e in document_order(inserts) if e in counter] == [e for e, _, _ in visible], "the model's order is not the patch's"
    return [where.get(q, (POS_UNKNOWN, 0, False)) for q in queries]


def inserts_upto(session, n_changes):
    """The insert ops of the Text among the first n_changes changes: the fixture lists the session's, and an element is there iff the
    ORACLE's rows hold an insert row with its id."""
    doc = oracle_lib.OracleDoc(ChangeLog.from_changes(session["changes"][:n_changes]))
    try:
        rows, actors = doc.rows(), [a.hex() for a in doc.actors()]
        have = {f"{int(c)}@{actors[int(a)]}" for c, a, ins in zip(rows["id_ctr"], rows["id_actor"], rows["insert"]) if ins}
    finally:
        doc.close()
    return [(e, after) for e, after in session["inserts"] if e in have]


_oracle_visible = {}


def oracle_visible(session, n_changes):
    key = (session["name"], n_changes)
    if key not in _oracle_visible:
        doc = oracle_lib.OracleDoc(ChangeLog.from_changes(session["changes"][:n_changes]))
        try:
            _oracle_visible[key] = elements_of_patch(doc.patch_json()).get(session["objectId"], [])
        finally:
            doc.close()
    return _oracle_visible[key]


def test_the_fixture_holds_every_session():
    assert sorted(SESSIONS) == sorted(SESSION_NAMES)
    neighbours = [os.path.getsize(os.path.join(HERE, "golden", "text", f)) for f in ("text_reads.json", "text_splices.json")]
    assert os.path.getsize(FIXTURE) <= min(neighbours)
    for name, s in SESSIONS.items():
        hows = {c["how"] for c in s["checkpoints"]}
        assert hows == {"local", "remote"} or name == "typed", name
        for c in s["checkpoints"]:
            assert [q[1] for q in c["queries"][-3:]] == ["unknown"] * 3, name
    refused = [(n, c["n"]) for n, s in SESSIONS.items() for c in s["checkpoints"] if c["refused"]]
    assert refused == [("remove_record", len(SESSIONS["remove_record"]["changes"]))]
    # the issue's example: hello world, positions 3-6 deleted, XY typed at 5 by somebody who had not seen that: helXYorld
    s = SESSIONS["two_actors"]
    c = s["checkpoints"][1]
    a = s["objectId"].split("@")[1]
    ctr = int(s["objectId"].split("@")[0])
    by_id = {q[0]: (q[1], q[2]) for q in c["queries"]}
    assert c["length"] == 9
    assert [by_id[f"{ctr + k}@{a}"] for k in (4, 5, 6, 7)] == [("deleted", 3), ("deleted", 3), ("deleted", 5), ("deleted", 5)]
    # deleted elements in front of everything and behind everything; a Text with rows and no element; counters
    t = SESSIONS["typed"]["checkpoints"][-2]
    assert any(q[1:3] == ["deleted", 0] for q in t["queries"]) and any(q[1:3] == ["deleted", t["length"]] for q in t["queries"])
    assert any(c["length"] == 0 and sum(q[1] == "deleted" for q in c["queries"]) >= 9 for c in SESSIONS["all_deleted"]["checkpoints"])
    assert any(q[3] for c in SESSIONS["counters"]["checkpoints"] for q in c["queries"])


@pytest.mark.parametrize("name", SESSION_NAMES)
def test_the_model_equals_the_probe_of_the_reference(name):
    s = SESSIONS[name]
    checked = 0
    for c in s["checkpoints"]:
        if c["refused"]:
            continue   # (the whole-document patch of such a state does not list the Text as the frontend shows it: the probe alone defines it)
        visible = oracle_visible(s, c["n"])
        assert len(visible) == c["length"]
        assert model_positions(inserts_upto(s, c["n"]), visible, ids_of(c)) == want_of(c), f"{name} after {c['n']} changes"
        checked += 1
    assert checked >= 2


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the fixture on the engine
# ---------------------------------------------------------------------------------------------------------------------------
def check_checkpoint(eng, s, c, where):
    if c["refused"]:
        with pytest.raises(engine.UnsupportedChanges, match=REMOVE_TEXT) as e:
            eng.text_positions(s["objectId"], ids_of(c))
        assert e.value.code == AM355_E_UNSUPPORTED, where
        return
    got, length = eng.text_positions(s["objectId"], ids_of(c))
    assert length == c["length"], where
    assert got == want_of(c), f"{where}: {[(q, g, w) for q, g, w in zip(ids_of(c), got, want_of(c)) if g != w][:6]}"


def check_checkpoints_from_a_fresh_replay(make_engine, name):
    s = SESSIONS[name]
    eng = make_engine()
    try:
        for k, c in enumerate(s["checkpoints"]):
            eng.load_changes(ChangeLog.from_changes(s["changes"][:c["n"]]))
            eng.replay()
            check_checkpoint(eng, s, c, f"{name} after {c['n']} changes")
            assert eng.text_position_calls()[0] == k + 1 - sum(x["refused"] for x in s["checkpoints"][:k + 1])
    finally:
        eng.close()


@pytest.mark.parametrize("name", SESSION_NAMES)
def test_checkpoints_from_a_fresh_replay_emulated(emu_lib, monkeypatch, name):  # noqa: F811
    _verify(monkeypatch)
    check_checkpoints_from_a_fresh_replay(_emulated(emu_lib), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SESSION_NAMES)
def test_checkpoints_from_a_fresh_replay_gpu(monkeypatch, name):
    _verify(monkeypatch)
    check_checkpoints_from_a_fresh_replay(_gpu, name)


SPLICER = "5c" * 16


def check_whole_session(make_engine, name):
    """Change by change through apply_changes on one context (in-place merges: the tables are stale when the query comes), the
    checkpoints asked where they fall; then a text_splice by another actor, and every element asked again against the model."""
    s = SESSIONS[name]
    eng = make_engine()
    try:
        at, in_place = 0, 0
        for c in s["checkpoints"]:
            while at < c["n"]:
                before = eng.resident_counters()[2] if at else 0
                try:
                    eng.apply_changes(ChangeLog.from_changes(s["changes"][at:at + 1]))
                except engine.UnsupportedChanges:
                    # (the increment of a deleted counter: the incremental patch is the JS path's, and the refused call leaves no state --
                    # the host replays what it has applied)
                    assert name == "remove_record" and at + 1 == len(s["changes"])
                    eng.load_changes(ChangeLog.from_changes(s["changes"][:at + 1]))
                    eng.replay()
                in_place += at > 0 and eng.resident_counters()[2] > before
                at += 1
            check_checkpoint(eng, s, c, f"{name} after {c['n']} changes, one context")
            if c["refused"]:   # the state is still served: the other Text of the document answers
                other = next(q[0] for q in c["queries"] if q[1] == "unknown")
                other_text = f"1@{s['objectId'].split('@')[1]}"
                assert eng.text_positions(other_text, [other, s["inserts"][0][0]])[0] == [(POS_VISIBLE, 0, False), (POS_UNKNOWN, 0, False)]
        assert in_place >= 1, "no change of the session was merged in place: the query never met stale tables"
        last = s["checkpoints"][-1]
        if last["refused"]:
            return
        # ---- behind text_splice: delete the element at 1 (if there is one) and type two characters there ----
        start, deletions = min(1, last["length"]), 1 if last["length"] > 1 else 0
        inserts = inserts_upto(s, at)
        visible = oracle_visible(s, at)
        after = visible[start - 1][0] if start else "_head"
        change = eng.text_splice(s["objectId"], start, deletions, ["S", "T"], SPLICER)
        doc = oracle_lib.OracleDoc(ChangeLog.from_changes(s["changes"] + [change]))
        try:
            patch = doc.patch_json()
        finally:
            doc.close()
        top = json.loads(patch)["maxOp"]
        new = [f"{top - 1}@{SPLICER}", f"{top}@{SPLICER}"]
        inserts = inserts + [(new[0], after), (new[1], new[0])]
        now_visible = elements_of_patch(patch)[s["objectId"]]
        queries = [e for e, _ in inserts] + [f"{top + 1}@{SPLICER}"]
        want = model_positions(inserts, now_visible, queries)
        assert want[-3][:2] == (POS_VISIBLE, start) and want[-1][0] == POS_UNKNOWN
        got, length = eng.text_positions(s["objectId"], queries)
        assert length == len(now_visible) and got == want, f"{name} behind text_splice"
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
# 3. round trip, and 4. the switch points, on generated logs
# ---------------------------------------------------------------------------------------------------------------------------
ACT_A, ACT_B = "2a" * 16, "b7" * 16
TEXT = f"1@{ACT_A}"


def position_limits():
    out = (ctypes.c_uint32 * 2)()
    assert engine.load_library().am355_text_position_limits(out) == 0
    return tuple(int(x) for x in out)


def locate_limits():
    out = (ctypes.c_uint32 * 3)()
    assert engine.load_library().am355_text_locate_limits(out) == 0
    return tuple(int(x) for x in out)


def _delete(elem, count=1, pred=None):
    op = {"action": "del", "obj": TEXT, "elemId": elem, "insert": False, "pred": [pred or elem]}
    if count > 1:
        op["multiOp"] = count
    return op


def mixed_requests():
    """One Text that crosses every switch point. A pastes N = pinned limit + 40 characters (elements 2 .. N + 1 @A). B, who has seen
    them, types one character behind each of the first H = workgroup + 24 of them: neighbours have different actors, 2 H records of one
    value -- two workgroups of kp_heads -- and behind them one pasted record of N - H values. Then, all concurrent to nothing:
      B types Q behind pasted element H + 100 and A deletes Q: a FOREIGN TOMBSTONE between two values of the pasted record;
      B assigns to pasted element H + 50 (an UPDATE record) and A deletes element H + 51, so that the update record is the last record
        in front of a deleted element;
      A deletes the first three elements of the Text (deleted IN FRONT of the first record) and the last five (BEHIND the last record),
        and one of B's characters in the alternating part."""
    w, p = position_limits()
    n, h = p + 40, w + 24
    a = lambda k: f"{2 + k}@{ACT_A}"   # noqa: E731  pasted element k
    b0 = n + 2                          # B's first op
    b = lambda k: f"{b0 + k}@{ACT_B}"  # noqa: E731  B's character behind pasted element k
    first = {"actor": ACT_A, "seq": 1, "startOp": 1, "time": 0, "message": "", "deps": [],
             "ops": [{"action": "makeText", "obj": "_root", "key": "text", "insert": False, "pred": []},
                     {"action": "set", "obj": TEXT, "elemId": "_head", "insert": True, "values": ["p"] * n, "pred": []}]}
    q_id, w_id = f"{b0 + h}@{ACT_B}", f"{b0 + h + 1}@{ACT_B}"
    second = lambda dep: {"actor": ACT_B, "seq": 1, "startOp": b0, "time": 0, "message": "", "deps": [dep],   # noqa: E731
                          "ops": [{"action": "set", "obj": TEXT, "elemId": a(k), "insert": True, "value": "b", "pred": []} for k in range(h)] +
                                 [{"action": "set", "obj": TEXT, "elemId": a(h + 100), "insert": True, "value": "Q", "pred": []},
                                  {"action": "set", "obj": TEXT, "elemId": a(h + 50), "insert": False, "value": "W", "pred": [a(h + 50)]}]}
    third = lambda dep: {"actor": ACT_A, "seq": 2, "startOp": b0 + h + 2, "time": 0, "message": "", "deps": [dep],   # noqa: E731
                         "ops": [_delete(q_id), _delete(a(h + 51)), _delete(a(0)), _delete(b(0)), _delete(a(1)), _delete(a(n - 5), 5), _delete(b(40))]}
    inserts = [(a(0), "_head")] + [(a(k), a(k - 1)) for k in range(1, n)] + [(b(k), a(k)) for k in range(h)] + [(q_id, a(h + 100))]
    marks = {"foreign tombstone": q_id, "behind the tombstone": a(h + 101), "updated": a(h + 50), "behind the update": a(h + 51), "first": a(0), "last": a(n - 1),
             "assignment": w_id}
    return [first, second, third], inserts, marks


def emptied_requests():
    """A Text with rows and no record: w + 1 characters pasted, all deleted."""
    n = position_limits()[0] + 1
    first = {"actor": ACT_A, "seq": 1, "startOp": 1, "time": 0, "message": "", "deps": [],
             "ops": [{"action": "makeText", "obj": "_root", "key": "text", "insert": False, "pred": []},
                     {"action": "set", "obj": TEXT, "elemId": "_head", "insert": True, "values": ["g"] * n, "pred": []}]}
    second = lambda dep: {"actor": ACT_A, "seq": 2, "startOp": n + 2, "time": 0, "message": "", "deps": [dep], "ops": [_delete(f"2@{ACT_A}", n)]}   # noqa: E731
    return [first, second], [(f"2@{ACT_A}", "_head")] + [(f"{2 + k}@{ACT_A}", f"{1 + k}@{ACT_A}") for k in range(1, n)], {}


_shapes = {}


def shape(make_engine, key):
    """(log, insert ops, the visible elements by the fold of the ORACLE's patch, marked ids): made once, shared by the emulated and the
    device run."""
    if key not in _shapes:
        requests, inserts, marks = {"mixed": mixed_requests, "emptied": emptied_requests}[key]()
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
        doc = oracle_lib.OracleDoc(log)
        try:
            visible = elements_of_patch(doc.patch_json()).get(TEXT, [])
        finally:
            doc.close()
        _shapes[key] = (log, inserts, visible, marks)
    return _shapes[key]


def test_the_mixed_shape_is_what_it_says(emu_lib):  # noqa: F811
    w, p = position_limits()
    assert w < p and (w, p) == (locate_limits()[0], locate_limits()[2])
    _, inserts, visible, marks = shape(_emulated(emu_lib), "mixed")
    ids = [e for e, _ in inserts]
    assert len(ids) > p + 1
    where = dict(zip(ids, model_positions(inserts, visible, ids)))
    order = document_order(inserts)
    # a tombstone of B between two values of A that have consecutive counters and neighbouring indexes: one record, not adjacent in the order
    t = order.index(marks["foreign tombstone"])
    left, right = order[t - 1], order[t + 1]
    assert right == marks["behind the tombstone"] and where[marks["foreign tombstone"]][0] == POS_DELETED
    assert where[left][0] == where[right][0] == POS_VISIBLE and where[right][1] == where[left][1] + 1
    assert left.split("@")[1] == right.split("@")[1] == ACT_A and int(right.split("@")[0]) == int(left.split("@")[0]) + 1
    # the updated element is visible, its pred is B's assignment, and the element behind it is deleted at its index + 1
    u = where[marks["updated"]]
    assert u[0] == POS_VISIBLE and visible[u[1]][1] == marks["assignment"] and where[marks["behind the update"]] == (POS_DELETED, u[1] + 1, False)
    assert where[marks["first"]] == (POS_DELETED, 0, False) and where[marks["last"]] == (POS_DELETED, len(visible), False)
    assert model_positions(inserts, visible, [marks["assignment"]]) == [(POS_UNKNOWN, 0, False)], "an op that is no insert is no element"
    assert 2 * (w + 24) - 3 > w, "the one-value records span two workgroups of the heads pass"


def query_sets(ids):
    """Queries at the switch points: one; workgroup size - 1, the size, + 1; the pinned limit and + 1; everything. The small sets stride
    through the elements, so that each holds elements of every part of the Text."""
    w, p = position_limits()
    assert len(ids) > p + 1
    sets = []
    for n in (1, w - 1, w, w + 1, p, p + 1, len(ids)):
        step = max(1, len(ids) // n)
        pool = ids[::step] if step > 1 else ids[::-1]   # (from the end: the other actor's elements first, then the tail of the pasted run)
        picked = pool[:n]
        picked += [e for e in ids if e not in set(picked)][:n - len(picked)]
        assert len(picked) == n
        sets.append(picked)
    return sets


def check_switch_points(make_engine):
    log, inserts, visible, marks = shape(make_engine, "mixed")
    ids = [e for e, _ in inserts]
    extra = [marks["assignment"], f"1@{ACT_A}", f"999999@{ACT_A}", f"2@{'e1' * 16}", f"{2 ** 33}@{ACT_A}"]   # no insert, the Text's make op, nobody's, an unknown actor, beyond 32 bits
    eng = make_engine()
    try:
        eng.load_changes(log)
        eng.replay()
        for queries in query_sets(ids):
            queries = queries[:-len(extra)] + extra if len(queries) > 2 * len(extra) else queries
            got, length = eng.text_positions(TEXT, queries)
            want = model_positions(inserts, visible, queries)
            assert length == len(visible)
            assert got == want, f"{len(queries)} queries: {[(q, g, x) for q, g, x in zip(queries, got, want) if g != x][:6]}"
        one = [marks[k] for k in ("foreign tombstone", "behind the tombstone", "updated", "behind the update", "first", "last")]
        assert eng.text_positions(TEXT, one)[0] == model_positions(inserts, visible, one)
        # 3. the round trip over every position: locate gives the elemId, positions gives the position back
        runs, length = eng.text_locate(TEXT, 0, len(visible))
        actor = {eng.rank_of_actor(a): a for a in (ACT_A, ACT_B)}
        located = [f"{int(r['elem_ctr']) + k}@{actor[int(r['elem_actor'])]}" for r in runs for k in range(int(r["count"]))]
        assert located == [e for e, _, _ in visible]
        assert [(s, j) for s, j, _ in eng.text_positions(TEXT, located)[0]] == [(POS_VISIBLE, j) for j in range(length)]
    finally:
        eng.close()
    # a Text with rows and no record
    log, inserts, visible, _ = shape(make_engine, "emptied")
    ids = [e for e, _ in inserts]
    eng = make_engine()
    try:
        eng.load_changes(log)
        eng.replay()
        assert visible == [] and len(ids) == position_limits()[0] + 1
        got, length = eng.text_positions(TEXT, ids + [f"{len(ids) + 2}@{ACT_A}"])
        assert length == 0 and got == [(POS_DELETED, 0, False)] * len(ids) + [(POS_UNKNOWN, 0, False)]
    finally:
        eng.close()


def test_switch_points_emulated(emu_lib, monkeypatch):  # noqa: F811
    _verify(monkeypatch)
    check_switch_points(_emulated(emu_lib))


@pytest.mark.gpu
def test_switch_points_gpu(monkeypatch):
    _verify(monkeypatch)
    check_switch_points(_gpu)


def check_round_trip_on_the_sessions(make_engine):
    for name in SESSION_NAMES:
        s = SESSIONS[name]
        c = [x for x in s["checkpoints"] if not x["refused"]][-1]
        eng = make_engine()
        try:
            eng.load_changes(ChangeLog.from_changes(s["changes"][:c["n"]]))
            eng.replay()
            runs, length = eng.text_locate(s["objectId"], 0, c["length"])
            actors = {a for e, _ in s["inserts"] for a in [e.split("@")[1]]}
            actor = {eng.rank_of_actor(a): a for a in actors if eng.rank_of_actor(a) is not None}
            located = [f"{int(r['elem_ctr']) + k}@{actor[int(r['elem_actor'])]}" for r in runs for k in range(int(r["count"]))]
            counters = [bool(int(r["flags"]) & engine.RUN_COUNTER) for r in runs for k in range(int(r["count"]))]
            got = eng.text_positions(s["objectId"], located)[0]
            assert [(st, j) for st, j, _ in got] == [(POS_VISIBLE, j) for j in range(length)], name
            assert not any(is_c and not run_c for (_, _, is_c), run_c in zip(got, counters)), name   # (a counter makes its whole run a counter run)
        finally:
            eng.close()


def test_round_trip_on_the_sessions_emulated(emu_lib, monkeypatch):  # noqa: F811
    _verify(monkeypatch)
    check_round_trip_on_the_sessions(_emulated(emu_lib))


@pytest.mark.gpu
def test_round_trip_on_the_sessions_gpu(monkeypatch):
    _verify(monkeypatch)
    check_round_trip_on_the_sessions(_gpu)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. edges and errors; after each refusal the state is still served
# ---------------------------------------------------------------------------------------------------------------------------
OBJECTS = {"actor": ACT_A, "seq": 1, "startOp": 1, "time": 0, "message": "", "deps": [],
           "ops": [{"action": "makeText", "obj": "_root", "key": "text", "insert": False, "pred": []},
                   {"action": "set", "obj": TEXT, "elemId": "_head", "insert": True, "values": list("hello"), "pred": []},
                   {"action": "makeList", "obj": "_root", "key": "list", "insert": False, "pred": []},
                   {"action": "set", "obj": f"7@{ACT_A}", "elemId": "_head", "insert": True, "values": ["x", "y"], "pred": []},
                   {"action": "makeText", "obj": "_root", "key": "empty", "insert": False, "pred": []},
                   {"action": "makeMap", "obj": "_root", "key": "map", "insert": False, "pred": []}]}
LIST, EMPTY, MAP = f"7@{ACT_A}", f"10@{ACT_A}", f"11@{ACT_A}"
HELLO = [f"{2 + k}@{ACT_A}" for k in range(5)]


def check_errors(make_engine, refused_launches=None):
    eng = make_engine()
    try:
        with pytest.raises(engine.EngineError) as e:   # no state
            eng.text_positions(TEXT, [])
        assert e.value.code == AM355_E_STATE
        made, _ = eng.encode_change(OBJECTS)
        eng.apply_changes(ChangeLog.from_changes([made]))
        served = [0]

        def still_served(where):
            got, length = eng.text_positions(TEXT, HELLO + [f"8@{ACT_A}"])
            assert length == 5 and got == [(POS_VISIBLE, k, False) for k in range(5)] + [(POS_UNKNOWN, 0, False)], where   # (8@A: an element of the list)
            served[0] += 1
            assert eng.text_position_calls()[0] == served[0], where

        still_served("after the call without a state")
        # n == 0 returns the length only; an empty Text launches nothing beyond the object lookup
        assert eng.text_positions(TEXT, []) == ([], 5)
        before = (eng.text_position_calls()[1], refused_launches() if refused_launches else None)
        assert eng.text_positions(EMPTY, []) == ([], 0)
        after = (eng.text_position_calls()[1], refused_launches() if refused_launches else None)
        assert after[0] - before[0] <= 2 and after[1] == before[1], "an empty Text and no query: something beyond the object lookup was launched"
        assert eng.text_positions(EMPTY, HELLO[:2] + [f"12@{ACT_A}"]) == ([(POS_UNKNOWN, 0, False)] * 3, 0)
        if refused_launches:
            assert refused_launches() == before[1], "the engine launched an empty grid"
        served[0] += 3
        still_served("after the empty Text")
        ctr, actor = TEXT.split("@")
        for oid, text in ((LIST, "not a Text object"), (MAP, "not a Text object"), ("_root", "not a Text object"), (f"99@{actor}", f"no such object: 99@{actor}"),
                          (f"{ctr}@{'0' * 32}", "no such object"), (f"{ctr}@{actor}ff", "no such object")):
            with pytest.raises(engine.EngineError, match=text) as e:
                eng.text_positions(oid, HELLO)
            assert e.value.code == AM355_E_ARG
        still_served("after the calls that name no Text")
        assert eng.rank_of_actor(ACT_A) == 0 and eng.rank_of_actor(ACT_B) is None and eng.rank_of_actor(ACT_A + "00") is None
        # a new actor arrives and sorts in front: the ranks are renumbered, the ids asked by actor bytes stay right
        early = "0b" * 16
        typed, _ = eng.encode_change({"actor": early, "seq": 1, "startOp": 20, "time": 0, "message": "", "deps": [],
                                      "ops": [{"action": "set", "obj": TEXT, "elemId": HELLO[1], "insert": True, "value": "!", "pred": []}]})
        eng.apply_changes(ChangeLog.from_changes([typed]))
        assert (eng.rank_of_actor(early), eng.rank_of_actor(ACT_A)) == (0, 1)
        got, length = eng.text_positions(TEXT, HELLO + [f"20@{early}", f"21@{early}"])
        assert length == 6 and got == [(POS_VISIBLE, k, False) for k in (0, 1, 3, 4, 5)] + [(POS_VISIBLE, 2, False), (POS_UNKNOWN, 0, False)]
    finally:
        eng.close()
    eng = make_engine()
    try:
        eng.set_shard(0, 2)
        eng.load_changes(ChangeLog.from_changes([made]))
        eng.replay()
        with pytest.raises(engine.UnsupportedChanges, match="sharded"):
            eng.text_positions(TEXT, HELLO)
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
    """A context made by backend_load is served after it became the state of its rebuilt changes: the answers of the replayed log."""
    for name in ("holes", "updates"):
        s = SESSIONS[name]
        c = s["checkpoints"][-1]
        eng, twin = make_engine(), make_engine()
        try:
            twin.load_changes(ChangeLog.from_changes(s["changes"][:c["n"]]))
            twin.replay()
            eng.backend_load(bytes(twin.save()))
            check_checkpoint(eng, s, c, f"{name}: the loaded document")
            assert eng.text_positions(s["objectId"], ids_of(c)) == twin.text_positions(s["objectId"], ids_of(c))
            assert eng.patch_json() == twin.patch_json()
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
# 6. the call reads only
# ---------------------------------------------------------------------------------------------------------------------------
def check_positions_change_nothing(make_engine, name):
    s = SESSIONS[name]
    asked, twin = make_engine(), make_engine()
    try:
        ids = [e for e, _ in s["inserts"]]
        for at in range(len(s["changes"])):
            where = f"{name} change {at}"
            for eng in (asked, twin):
                eng.apply_changes(ChangeLog.from_changes(s["changes"][at:at + 1]))
            assert asked.apply_patch_json() == twin.apply_patch_json(), where
            assert asked.resident_counters() == twin.resident_counters(), f"{where}: the query changed what serves the next call"
            if at == 0:
                continue   # (the Text exists from the first change on)
            got, length = asked.text_positions(s["objectId"], ids)
            assert len(got) == len(ids) and sum(st == POS_VISIBLE for st, _, _ in got) == length, where
            asked.text_positions(s["objectId"], ids[:1])
        assert asked.patch_json() == twin.patch_json()
        assert bytes(asked.save()) == bytes(twin.save())
    finally:
        asked.close()
        twin.close()


@pytest.mark.parametrize("name", ["typed", "two_actors", "holes"])
def test_positions_change_nothing_emulated(emu_lib, monkeypatch, name):  # noqa: F811
    _verify(monkeypatch)
    check_positions_change_nothing(_emulated(emu_lib), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["typed", "two_actors", "holes"])
def test_positions_change_nothing_gpu(monkeypatch, name):
    _verify(monkeypatch)
    check_positions_change_nothing(_gpu, name)
