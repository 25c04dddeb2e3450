"""The string of a Text object read on the device (am355_object_text; csrc/am355_text.hip kt_find, kt_sizes, kt_gather): equal, byte
for byte, to what the reference's frontend shows as Text.toString() after applyPatch(getPatch(state)).

1. tests/golden/text/text_reads.json (tools/fixtures/make_text_reads.js: the live reference's frontend made the sessions and recorded, after
   every call, the string and the length of every Text): call by call through apply_changes with the in-place merges switched on, so
   that reads land behind them and rebuild the stale edit tables; at the end through one bulk replay and through the load of the
   reference's saved document. A twin context that is never asked ends with the same counters and the same patch.
2. Existing goldens, the ORACLE's patch as the yardstick: the expected string is a Python restatement of updateTextObject + toString
   (frontend/apply_patch.js:220-259, frontend/text.js:60-69) over the oracle's patch_json, never the engine's.
3. The kernels' edges, from their own constants (am355_text_limits): pasted records around the bytes one kt_gather workgroup owns,
   single-character records around one kt_sizes workgroup, three-byte characters across a workgroup's stretch, a Text behind another.
4. Errors, the empty Text (nothing launched, no launch refused), the counters.

Each body runs on the emulation (CPU suite) and on the device."""
import base64
import ctypes
import json
import os

import pytest

import oracle_lib
from automerge_classic_amd import engine, loggen
from automerge_classic_amd.loggen import ChangeLog
from golden_util import LIST_QUIRK_REFUSED, list_quirk_cases, load_fixture
from test_resident_limits import _emulated, emu_lib  # noqa: F401 (emu_lib: fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
AM355_E_ARG, AM355_E_STATE, AM355_E_UNSUPPORTED = -2, -5, -4


def _gpu():
    return engine.Engine(0)


# ---------------------------------------------------------------------------------------------------------------------------
# the rule, restated over a patch
# ---------------------------------------------------------------------------------------------------------------------------
class _NoString:
    """An element whose value is no JS string (a number, null, a boolean, bytes, a counter, a child object)."""


def _element(value):
    if "objectId" in value:
        return _NoString
    v = value["value"]
    return v if isinstance(v, str) and "datatype" not in value else _NoString


def texts_of_patch(patch_json):
    """{objectId: (string, length)} of every Text in a whole-document patch: updateTextObject (apply_patch.js:231-255) applied to an
    empty object, then toString (text.js:64-67). Where the reference's frontend would throw -- an `update` whose index is the list's
    length, the edits of an element that was reported as `remove` first -- the element is taken as the rule of csrc/am355_text.hip
    takes it: one element per index, the last update wins."""
    out = {}

    def walk(diff):
        if "props" in diff:
            for values in diff["props"].values():
                for v in values.values():
                    if "objectId" in v:
                        walk(v)
            return
        elems = []
        for e in diff.get("edits", []):
            a, i = e["action"], e["index"]
            if a == "insert":
                elems.insert(i, _element(e["value"]))
                if "objectId" in e["value"]:
                    walk(e["value"])
            elif a == "multi-insert":
                elems[i:i] = [v if isinstance(v, str) and not e.get("datatype") else _NoString for v in e["values"]]
            elif a == "update":
                if i < len(elems):
                    elems[i] = _element(e["value"])
                else:
                    elems.append(_element(e["value"]))
                if "objectId" in e["value"]:
                    walk(e["value"])
            elif a == "remove":
                del elems[i:i + e["count"]]
            else:
                raise AssertionError(a)
        if diff["type"] == "text":
            out[diff["objectId"]] = ("".join(x for x in elems if x is not _NoString), len(elems))

    walk(json.loads(patch_json)["diffs"])
    return out


def objects_of_patch(patch_json, kind):
    found = []

    def walk(diff):
        if diff["type"] == kind and diff["objectId"] != "_root":
            found.append(diff["objectId"])
        for values in diff.get("props", {}).values():
            for v in values.values():
                if "objectId" in v:
                    walk(v)
        for e in diff.get("edits", []):
            if isinstance(e.get("value"), dict) and "objectId" in e["value"]:
                walk(e["value"])
    walk(json.loads(patch_json)["diffs"])
    return found


def check_texts(eng, want, where):
    """want: {objectId: (string, length)}"""
    for oid, (string, length) in sorted(want.items()):
        got, info = eng.object_text(oid)
        assert got == string.encode("utf-8"), f"{where}: Text {oid}\n got  {got[:300]!r}\n want {string.encode('utf-8')[:300]!r}"
        assert info.n_elements == length, f"{where}: Text {oid}: {info.n_elements} elements, the frontend's length is {length}"
        assert info.bytes == len(got) and info.n_strings <= info.n_elements, where


def test_the_restatement_on_a_hand_made_patch():
    val = lambda v, **kw: dict({"type": "value", "value": v}, **kw)  # noqa: E731
    patch = {"diffs": {"objectId": "_root", "type": "map", "props": {"t": {"1@aa": {"objectId": "1@aa", "type": "text", "edits": [
        {"action": "multi-insert", "index": 0, "elemId": "2@aa", "values": ["a", "b", "c"]},
        {"action": "update", "index": 2, "opId": "9@aa", "value": val("X")},
        {"action": "update", "index": 2, "opId": "9@bb", "value": val(5, datatype="int")},
        {"action": "insert", "index": 3, "elemId": "5@aa", "opId": "5@aa", "value": val("d")},
        {"action": "remove", "index": 4, "count": 1},
        {"action": "update", "index": 4, "opId": "7@aa", "value": val(3, datatype="counter")},
        {"action": "multi-insert", "index": 5, "elemId": "12@aa", "datatype": "int", "values": [1, 2]},
        {"action": "insert", "index": 7, "elemId": "14@aa", "opId": "14@aa", "value": val("e")}]}}}}}
    assert texts_of_patch(json.dumps(patch)) == {"1@aa": ("abde", 8)}


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the sessions of the live reference
# ---------------------------------------------------------------------------------------------------------------------------
def load_sessions():
    with open(os.path.join(HERE, "golden", "text", "text_reads.json")) as f:
        fx = json.load(f)
    out = {}
    for s in fx["sessions"]:
        s = dict(s)
        s["batches"] = [[base64.b64decode(c) for c in b] for b in s["batches"]]
        s["save"] = base64.b64decode(s["save"])
        s["texts"] = [{t["objectId"]: (t["string"], t["length"]) for t in call} for call in s["texts"]]
        out[s["name"]] = s
    return out


SESSIONS = load_sessions()
SESSION_NAMES = ["typed", "conflicts", "mixed_values", "bom", "objects", "quirk"]


def test_the_fixture_holds_every_session():
    assert sorted(SESSIONS) == sorted(SESSION_NAMES)
    typed = SESSIONS["typed"]["texts"][-1]
    (string, length), = typed.values()
    widths = {len(ch.encode("utf-8")) for ch in string}
    assert widths == {1, 2, 3, 4} and length > 200
    assert any(length == 0 for call in SESSIONS["objects"]["texts"] for _, length in call.values()), "an empty Text"
    assert len(SESSIONS["objects"]["texts"][-1]) == 5
    (mixed, n), = SESSIONS["mixed_values"]["texts"][-1].values()
    assert n > len(mixed), "elements that are no strings"
    (bom, n), = SESSIONS["bom"]["texts"][-1].values()
    assert "\ufeff" in bom and not bom.startswith("\ufeff") and n == 10 and len(bom) < n + 3


@pytest.mark.parametrize("name", SESSION_NAMES)
def test_recorded_strings_follow_from_the_oracles_patch(name):
    """The fixture against the restatement: the strings the reference's frontend built from the incremental patches are what the rule
    gives over the oracle's whole-document patch after the same calls."""
    s = SESSIONS[name]
    session = oracle_lib.OracleSession()
    try:
        for i, batch in enumerate(s["batches"]):
            session.apply(batch)
            assert texts_of_patch(session.patch_json()) == s["texts"][i], f"{name} call {i}"
    finally:
        session.close()


def switched(make_engine):
    eng = make_engine()
    eng.set_resident_new_objects(True)
    eng.set_resident_counters(True)
    return eng


def play_session(make_engine, name):
    s = SESSIONS[name]
    asked, twin = switched(make_engine), switched(make_engine)
    try:
        served = 0
        for i, batch in enumerate(s["batches"]):
            log = ChangeLog.from_changes(batch)
            for eng in (asked, twin):
                try:
                    eng.apply_changes(log)
                except engine.UnsupportedChanges:
                    # an incremental patch the engine leaves to the JS path (an increment inside a list): the state is gone, and the host
                    # replays the changes it has retained, as js/index.js does
                    eng.load_changes(ChangeLog.from_changes([c for b in s["batches"][:i + 1] for c in b]))
                    eng.replay()
            check_texts(asked, s["texts"][i], f"{name} call {i}")
            served += len(s["texts"][i])
            assert asked.object_text_calls()[0] == served
            assert asked.resident_counters() == twin.resident_counters(), f"{name} call {i}: the read changed what serves the next call"
        assert asked.patch_json() == twin.patch_json()
        assert bytes(asked.save()) == bytes(twin.save())
    finally:
        asked.close()
        twin.close()
    final = s["texts"][-1]
    eng = make_engine()
    try:
        eng.load_changes(ChangeLog.from_changes([c for b in s["batches"] for c in b]))
        eng.replay()
        check_texts(eng, final, f"{name}: bulk replay")
        eng.fetch_ir()   # (the host's copy of the object table is current now: the lookup is the host's)
        launches = eng.object_text_calls()[1]
        check_texts(eng, final, f"{name}: bulk replay, host tables current")
        assert eng.object_text_calls()[1] - launches <= 4 * len(final)
        eng.backend_load(s["save"])
        check_texts(eng, final, f"{name}: backend_load of the reference's document")
        eng.load_document(s["save"])
        eng.replay()
        check_texts(eng, final, f"{name}: load_document + replay")
    finally:
        eng.close()


@pytest.mark.parametrize("name", SESSION_NAMES)
def test_sessions_emulated(emu_lib, monkeypatch, name):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    play_session(_emulated(emu_lib), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SESSION_NAMES)
def test_sessions_gpu(monkeypatch, name):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    play_session(_gpu, name)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. existing goldens, the oracle's patch as the yardstick
# ---------------------------------------------------------------------------------------------------------------------------
GOLDENS = ["frontend_text_4actors", "frontend_text_8actors", "frontend_multibyte_runs", "hand_conflicts", "hand_bom_values"]
_oracle_patches = {}


def oracle_patches(name):
    """(patch of the changes, patch of the loaded document) by the oracle, computed once and shared."""
    if name not in _oracle_patches:
        fx = load_fixture(name)
        _oracle_patches[name] = (fx, oracle_lib.OracleDoc(fx["log"]).patch_json(), oracle_lib.OracleDoc.load_document(fx["doc_bytes"]).patch_json())
    return _oracle_patches[name]


def check_golden(make_engine, name):
    fx, want_changes, want_doc = oracle_patches(name)
    eng = make_engine()
    try:
        eng.load_changes(fx["log"])
        eng.replay()
        texts = texts_of_patch(want_changes)
        assert texts, name
        check_texts(eng, texts, name)
        for oid in objects_of_patch(want_changes, "list") + objects_of_patch(want_changes, "map"):
            with pytest.raises(engine.EngineError, match="not a Text object") as e:
                eng.object_text(oid)
            assert e.value.code == AM355_E_ARG
        eng.load_document(fx["doc_bytes"])
        eng.replay()
        check_texts(eng, texts_of_patch(want_doc), name + " (document)")
    finally:
        eng.close()


@pytest.mark.parametrize("name", GOLDENS)
def test_goldens_emulated(emu_lib, name):
    check_golden(_emulated(emu_lib), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", GOLDENS)
def test_goldens_gpu(name):
    check_golden(_gpu, name)


_quirk_oracle = {}


def check_list_quirks(make_engine):
    """Every case of list_quirks.json: the Texts among them against the oracle's patch; a case the engine refuses is refused by
    object_text with the error patch_json gives; which cases are refused is known exactly."""
    eng = make_engine()
    refused, n_texts = [], 0
    try:
        for name, blobs, _, _, _ in list_quirk_cases():
            log = ChangeLog.from_changes(blobs, name=name)
            if name not in _quirk_oracle:
                _quirk_oracle[name] = oracle_lib.OracleDoc(log).patch_json()
            want = _quirk_oracle[name]
            texts, lists = texts_of_patch(want), objects_of_patch(want, "list")
            try:
                eng.load_changes(log)
                eng.replay()
            except engine.UnsupportedChanges:
                refused.append(name)
                with pytest.raises(engine.EngineError) as from_patch:
                    eng.patch_json()
                with pytest.raises(engine.EngineError) as from_text:
                    eng.object_text((list(texts) + lists)[0])
                assert type(from_text.value) is type(from_patch.value) and from_text.value.code == from_patch.value.code
                continue
            check_texts(eng, texts, name)
            n_texts += len(texts)
            for oid in lists:
                with pytest.raises(engine.EngineError, match="not a Text object"):
                    eng.object_text(oid)
        assert set(refused) == LIST_QUIRK_REFUSED, refused
        assert n_texts >= 6
    finally:
        eng.close()


def test_list_quirks_emulated(emu_lib):
    check_list_quirks(_emulated(emu_lib))


@pytest.mark.gpu
def test_list_quirks_gpu():
    check_list_quirks(_gpu)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the kernels' edges
# ---------------------------------------------------------------------------------------------------------------------------
def limits():
    out = (ctypes.c_uint32 * 4)()
    lib = engine.load_library()
    assert lib.am355_text_limits(out) == 0
    return tuple(int(x) for x in out)


_edge_logs = {}


def edge_log(key, make):
    """(log, {objectId: (string, length)} by the oracle): made once, shared by the emulated and the device run."""
    if key not in _edge_logs:
        log = make()
        _edge_logs[key] = (log, texts_of_patch(oracle_lib.OracleDoc(log).patch_json()))
    return _edge_logs[key]


def check_edge(make_engine, key, make, expect=None):
    log, texts = edge_log(key, make)
    if expect is not None:
        expect(texts)
    eng = make_engine()
    try:
        eng.load_changes(log)
        eng.replay()
        check_texts(eng, texts, str(key))
    finally:
        eng.close()


def pasted(n):
    """One change of one author that types n one-byte characters in a row: one edit record of n values."""
    return lambda: loggen.generate(loggen.KIND_TEXT_CONCURRENT, n_actors=1, n_rounds=1, ins_per_change=n, del_per_change=0, n_objects=1, seed=77 + n)


def typed_one_by_one(n):
    """n changes of one character each: the values of two changes are not neighbours in the arena, so every character is a record."""
    return lambda: loggen.generate(loggen.KIND_TEXT_TYPING, n_ops=n, ops_per_change=1, seed=5 + n)


def paste_sizes():
    t = limits()[0]
    return [t - 1, t, t + 1, 3 * t + 5]


def record_counts():
    b = limits()[1]
    return [b - 1, b, b + 1, 2 * b + 1]


def one_text_of(n_bytes):
    def expect(texts):
        (string, length), = texts.values()
        assert len(string.encode("utf-8")) == n_bytes and length == n_bytes, (len(string), length)
    return expect


@pytest.mark.parametrize("k", range(4))
def test_pasted_record_around_a_gather_workgroup_emulated(emu_lib, k):
    n = paste_sizes()[k]
    check_edge(_emulated(emu_lib), ("paste", n), pasted(n), one_text_of(n))


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(4))
def test_pasted_record_around_a_gather_workgroup_gpu(k):
    n = paste_sizes()[k]
    check_edge(_gpu, ("paste", n), pasted(n), one_text_of(n))


@pytest.mark.parametrize("k", range(4))
def test_single_character_records_around_a_sizes_workgroup_emulated(emu_lib, k):
    n = record_counts()[k]
    check_edge(_emulated(emu_lib), ("typed", n), typed_one_by_one(n), one_text_of(n))


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(4))
def test_single_character_records_around_a_sizes_workgroup_gpu(k):
    n = record_counts()[k]
    check_edge(_gpu, ("typed", n), typed_one_by_one(n), one_text_of(n))


ACTOR = "ab" * 16


def request_of(values_runs, start_text="", seq=1):
    """A change request that makes a Text and inserts `values_runs` (lists of one-element strings) behind each other as ONE multi-insert
    per list -- consecutive op ids: the backend reports them as one multi-insert edit whose records change with the byte width."""
    ops = [{"action": "makeText", "obj": "_root", "key": "text", "insert": False, "pred": []}]
    op, elem = 2, "_head"
    for values in values_runs:
        ops.append({"action": "set", "obj": f"1@{ACTOR}", "elemId": elem, "insert": True, "values": list(values), "pred": []})
        op += len(values)
        elem = f"{op - 1}@{ACTOR}"
    return {"actor": ACTOR, "seq": seq, "startOp": 1, "time": 0, "message": "", "deps": [], "ops": ops}


def three_byte_log(make_engine):
    """A record of three-byte characters whose bytes lie across the end of the first gather workgroup's stretch, one-byte records around
    it; a second record of three-byte characters long enough for the workgroup's own look for U+FEFF (none there), and a short one
    with U+FEFF values inside (the per-value path)."""
    t, _, inline, _ = limits()
    runs = [["a"] * (t - 31), ["€"] * 21, ["b"] * 7, ["中"] * (inline + 300), ["c"] * 5, ["あ", "\ufeff", "い", "\ufeff", "\ufeff", "う"], ["d"] * 3, ["\ufeffxy"], ["é"] * 9]
    eng = make_engine()
    try:
        change, _ = eng.encode_change(request_of(runs))
    finally:
        eng.close()
    want = "".join("".join(r) for r in runs).replace("\ufeff", "")
    return ChangeLog.from_changes([change]), want, sum(len(r) for r in runs)


def check_three_byte(make_engine):
    key = "three_byte"
    if key not in _edge_logs:
        log, want, n = three_byte_log(make_engine)
        texts = texts_of_patch(oracle_lib.OracleDoc(log).patch_json())
        assert texts == {f"1@{ACTOR}": (want, n)}, "the oracle's patch of the hand-made change"
        _edge_logs[key] = (log, texts)
    check_edge(make_engine, key, None)


def test_three_byte_characters_across_a_workgroups_stretch_emulated(emu_lib):
    check_three_byte(_emulated(emu_lib))


@pytest.mark.gpu
def test_three_byte_characters_across_a_workgroups_stretch_gpu():
    check_three_byte(_gpu)


def check_long_bom_run_is_left_to_the_caller(make_engine):
    """More values than the gather walks, one of them U+FEFF: AM355_E_UNSUPPORTED, and the state stays."""
    walk_max = limits()[3]
    runs = [["€"] * walk_max + ["\ufeff"] + ["€"] * 2]
    eng = make_engine()
    try:
        change, _ = eng.encode_change(request_of(runs))
        eng.load_changes(ChangeLog.from_changes([change]))
        eng.replay()
        with pytest.raises(engine.UnsupportedChanges, match="byte order marks"):
            eng.object_text(f"1@{ACTOR}")
        assert json.loads(eng.patch_json())["maxOp"] == walk_max + 4
    finally:
        eng.close()


def test_long_run_with_a_bom_inside_emulated(emu_lib):
    check_long_bom_run_is_left_to_the_caller(_emulated(emu_lib))


@pytest.mark.gpu
def test_long_run_with_a_bom_inside_gpu():
    check_long_bom_run_is_left_to_the_caller(_gpu)


def two_texts():
    return loggen.generate(loggen.KIND_TEXT_CONCURRENT, seed=21, n_actors=5, n_rounds=3, ins_per_change=37, del_per_change=5, n_objects=3)


def expect_three(texts):
    assert len(texts) == 3 and all(length > 50 for _, length in texts.values())


def test_a_text_behind_other_lists_emulated(emu_lib):
    check_edge(_emulated(emu_lib), "behind", two_texts, expect_three)


@pytest.mark.gpu
def test_a_text_behind_other_lists_gpu():
    check_edge(_gpu, "behind", two_texts, expect_three)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. errors, the empty Text, the counters
# ---------------------------------------------------------------------------------------------------------------------------
def check_errors(make_engine, refused_launches=None):
    s = SESSIONS["objects"]
    final = s["texts"][-1]
    empty = [oid for oid, (_, length) in final.items() if length == 0]
    assert len(empty) == 2   # one never typed into, one whose characters are all deleted
    lists = objects_of_patch(s["whole_patch"], "list")
    maps = objects_of_patch(s["whole_patch"], "map")
    assert lists and maps
    log = ChangeLog.from_changes([c for b in s["batches"] for c in b])
    eng = make_engine()
    try:
        with pytest.raises(engine.EngineError) as e:
            eng.object_text(empty[0])
        assert e.value.code == AM355_E_STATE
        eng.load_changes(log)
        with pytest.raises(engine.EngineError) as e:   # staged, not replayed
            eng.object_text(empty[0])
        assert e.value.code == AM355_E_STATE
        eng.replay()
        assert eng.object_text_calls() == (0, 0)
        before = refused_launches() if refused_launches else None
        for k, oid in enumerate(empty):
            got, info = eng.object_text(oid)
            assert got == b"" and (info.n_elements, info.n_strings, info.bytes) == (0, 0, 0)
            assert eng.object_text_calls()[0] == k + 1
        if refused_launches:
            assert refused_launches() == before, "an empty Text made the engine launch an empty grid"
        eng.fetch_ir()
        launches = eng.object_text_calls()[1]
        assert eng.object_text(empty[0])[0] == b""
        assert eng.object_text_calls() == (3, launches), "an empty Text with the host's object table current launches nothing"
        a_text = next(oid for oid in final if oid not in empty)
        ctr, actor = a_text.split("@")
        for oid in (f"{int(ctr) + 100000}@{actor}", f"{ctr}@{'0' * len(actor)}", f"{ctr}@{actor}ff"):   # no such counter, no such actor
            with pytest.raises(engine.EngineError, match="no such object: " + oid) as e:
                eng.object_text(oid)
            assert e.value.code == AM355_E_ARG
        for oid in lists + maps + ["_root"]:
            with pytest.raises(engine.EngineError, match="not a Text object") as e:
                eng.object_text(oid)
            assert e.value.code == AM355_E_ARG
        assert eng.object_text_calls()[0] == 3, "a refused call is not served"
        check_texts(eng, final, "after the errors")   # (an error leaves the state as it was)
    finally:
        eng.close()
    eng = make_engine()
    try:
        eng.set_shard(0, 2)
        eng.load_changes(log)
        eng.replay()
        with pytest.raises(engine.UnsupportedChanges, match="sharded"):
            eng.object_text(empty[0])
    finally:
        eng.close()


def test_errors_and_the_empty_text_emulated(emu_lib):
    lib = engine.load_library(emu_lib)
    lib.am355_emu_refused_launches.argtypes = [ctypes.POINTER(ctypes.c_char_p)]
    lib.am355_emu_refused_launches.restype = ctypes.c_long
    check_errors(_emulated(emu_lib), lambda: int(lib.am355_emu_refused_launches(ctypes.byref(ctypes.c_char_p()))))


@pytest.mark.gpu
def test_errors_and_the_empty_text_gpu():
    check_errors(_gpu)


def check_pinned_variant(make_engine):
    """am355_set_text_pinned_max: the gather writes into the pinned buffer itself; the same bytes."""
    s = SESSIONS["typed"]
    eng = make_engine()
    try:
        eng.load_changes(ChangeLog.from_changes([c for b in s["batches"] for c in b]))
        eng.replay()
        eng.set_text_pinned_max(1 << 20)
        check_texts(eng, s["texts"][-1], "gathered into pinned memory")
        eng.set_text_pinned_max(0)
        check_texts(eng, s["texts"][-1], "gathered into device memory and copied")
    finally:
        eng.close()


def test_pinned_variant_emulated(emu_lib):
    check_pinned_variant(_emulated(emu_lib))


@pytest.mark.gpu
def test_pinned_variant_gpu():
    check_pinned_variant(_gpu)
