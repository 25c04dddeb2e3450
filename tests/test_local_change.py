"""Backend.applyLocalChange on the engine (include/am355.h am355_encode_change / am355_apply_local_change; the device stage is kl_expand
in csrc/am355_hist.hip): a change REQUEST is expanded into rows, its numbers get their bytes and the twelve op columns are encoded on
the device, the host writes the container and hashes it, and the one-change batch goes through the resident apply path.

tests/golden/local/sessions.json (tools/fixtures/make_local_change_sessions.js) holds sessions recorded from the reference: the
requests its frontend made, and per call the binary change and the patch the reference's backend returned. Here:
  (a) the fixture against the sequential oracle (CPU only)
  (b) encode_change of every recorded request == the recorded bytes and hash
  (c) every session call by call: returned bytes, patch TEXT, whole-document patch and Backend.save at the end, the verify switches on
  (d) which path served: a local change adds to resident_counters() what the same change applied as a remote one adds
  (e) refusals: the documented code, local_change_calls()[1] + 1, the state as it was
  (f) a context destroyed after local changes leaves no HIP resource behind
and multi-inserts at the switch points of the scan the stage uses (am355_prims.hip exclusive_scan_u32 over rows + 1 values: one tile
of SCAN_TILE = 2048, one workgroup up to SCAN_SINGLE = 8192, two launches beyond) and beyond one resident chunk of 12,288 rows,
checked against the oracle. Each body runs on the emulation of tests/emu and, marked gpu, on the device."""
import base64
import ctypes
import gc
import hashlib
import json
import os
import subprocess

import pytest

import oracle_lib
from automerge_classic_amd import engine
from automerge_classic_amd.loggen import ChangeLog
from test_apply_engine import EMU_DIR, EMU_LIB, _ordered
from test_apply_vectors import same_patch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "local", "sessions.json")
with open(FIXTURE) as _f:
    SESSIONS = json.load(_f)["sessions"]
NAMES = [s["name"] for s in SESSIONS]
BY_NAME = {s["name"]: s for s in SESSIONS}
IN_PLACE = (1, 0, 1)


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-s", "-C", EMU_DIR])
    return EMU_LIB


def _emulated(lib):
    return lambda: _switched(engine.Engine(0, lib))


def _gpu():
    return _switched(engine.Engine(0))


def _switched(eng):
    # (what the JS host turns on for every context, js/index.js acquireContext)
    eng.set_resident_new_actors(True)
    eng.set_resident_new_objects(True)
    eng.set_resident_counters(True)
    return eng


def _verify(monkeypatch):
    for v in ("AM355_RESORDER_VERIFY", "AM355_MAPMERGE_VERIFY", "AM355_COUNTERS_VERIFY"):
        monkeypatch.setenv(v, "1")


def _whole(text):
    return dict(_ordered(text))["diffs"]


def _b64(x):
    return base64.b64decode(x)


def same_local_patch(got_text, want_text, own_hash):
    """The patch of a local change as the ORACLE states it against the recorded one: the oracle lists the new change's own hash among
    the deps, applyLocalChange takes it out (backend.js:88-89)."""
    got, want = dict(_ordered(got_text)), dict(_ordered(want_text))
    got["deps"] = [h for h in got["deps"] if h != own_hash]
    if list(got) != list(want):
        return False
    return all(dict(got[k]) == dict(want[k]) if k == "clock" else got[k] == want[k] for k in got)


def _oracle_for(s):
    first = s["calls"][0]
    if first["kind"] != "load":
        return oracle_lib.OracleSession()
    return oracle_lib.OracleSession(_b64(first["doc"]), bytes.fromhex(s["doc_hashes"]), graph_rebuilt=s["graph_rebuilt"])


def check_session_against_oracle(s):
    session = _oracle_for(s)
    try:
        for i, call in enumerate(s["calls"]):
            if call["kind"] == "remote":
                assert same_patch(session.apply([_b64(c) for c in call["batch"]]), call["patch"]), f"{s['name']} call {i}"
            elif call["kind"] == "local":
                got = session.apply([_b64(call["change"])], local=True)
                assert same_local_patch(got, call["patch"], call["hash"]), f"{s['name']} call {i}:\n{got[:1500]}\n{call['patch'][:1500]}"
        assert _whole(session.patch_json()) == _whole(s["whole_patch"]), f"{s['name']}: getPatch at the end"
    finally:
        session.close()


# ---------------------------------------------------------------------------------------------------------------------------
# (a) the fixture against the oracle
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_fixture_against_the_oracle(name):
    check_session_against_oracle(BY_NAME[name])


def test_fixture_holds_the_shapes():
    kinds = {c["kind"] for s in SESSIONS for c in s["calls"]}
    assert kinds == {"load", "remote", "local", "rejected"}
    below, above = BY_NAME["deflate_below"]["calls"][-1], BY_NAME["deflate_above"]["calls"][-1]
    assert _b64(below["change"])[8] == 1 and _b64(above["change"])[8] == 2   # the two sides of DEFLATE_MIN_SIZE
    runs = [len(op["values"]) for c in BY_NAME["text_runs"]["calls"] if c["kind"] == "local" for op in c["request"]["ops"] if "values" in op]
    assert {2, 64, 65} <= set(runs)
    multi = [op["multiOp"] for c in BY_NAME["deletes"]["calls"] for op in c["request"]["ops"] if op.get("multiOp", 1) > 1]
    assert multi == [2, 65]
    mixed = [op["action"] for op in BY_NAME["mixed"]["calls"][-1]["request"]["ops"]]
    assert mixed == ["set", "del", "set", "makeMap", "set", "set", "inc"]
    assert os.path.getsize(FIXTURE) < (1 << 20)


# ---------------------------------------------------------------------------------------------------------------------------
# (b) encode_change alone
# ---------------------------------------------------------------------------------------------------------------------------
def _with_own_hash(s, index):
    """The request of local call `index` with the deps applyLocalChange gave it: the author's last hash added (backend.js:73-81)."""
    call = s["calls"][index]
    req = json.loads(json.dumps(call["request"]))
    if req["seq"] > 1:
        last = None
        for c in s["calls"][:index]:
            if c["kind"] == "local" and c["request"]["actor"] == req["actor"] and c["request"]["seq"] == req["seq"] - 1:
                last = c["hash"]
        if last is None:
            return None   # (the hash lies in a loaded document or a remote batch: covered by the sessions)
        req["deps"] = sorted(set(req["deps"]) | {last})
    return req


def check_encode(make_engine):
    eng = make_engine()
    n = 0
    try:
        for s in SESSIONS:
            for i, call in enumerate(s["calls"]):
                if call["kind"] != "local":
                    continue
                req = _with_own_hash(s, i)
                if req is None:
                    continue
                got, digest = eng.encode_change(req)
                assert digest.hex() == call["hash"], f"{s['name']} call {i}: hash"
                assert got == _b64(call["change"]), f"{s['name']} call {i}:\n{got.hex()}\n{_b64(call['change']).hex()}"
                n += 1
        assert n >= 25
        assert eng.local_change_calls() == (0, 0)   # (encode_change applies nothing and is not counted)
    finally:
        eng.close()


def test_encode_change(emu_lib):
    check_encode(_emulated(emu_lib))


@pytest.mark.gpu
def test_encode_change_gpu():
    check_encode(_gpu)


# ---------------------------------------------------------------------------------------------------------------------------
# (c), (d), (e) the sessions call by call
# ---------------------------------------------------------------------------------------------------------------------------
def drive_session(make_engine, s):
    """Returns what every local call added to resident_counters(), and what the same change added as a remote one."""
    eng, twin = make_engine(), make_engine()
    local_delta, remote_delta = [], []
    served = refused = 0
    try:
        for i, call in enumerate(s["calls"]):
            where = f"{s['name']} call {i} ({call['kind']})"
            if call["kind"] == "load":
                for e in (eng, twin):
                    e.load_document(_b64(call["doc"]))
                    e.replay()
            elif call["kind"] == "remote":
                batch = ChangeLog.from_changes([_b64(c) for c in call["batch"]])
                eng.apply_changes(batch)
                assert same_patch(eng.apply_patch_json(), call["patch"]), where
                twin.apply_changes(batch)
            elif call["kind"] == "local":
                before = eng.resident_counters()
                got = eng.apply_local_change(call["request"])
                local_delta.append(tuple(a - b for a, b in zip(eng.resident_counters(), before)))
                served += 1
                assert got == _b64(call["change"]), f"{where}:\n{got.hex()}\n{_b64(call['change']).hex()}"
                assert eng.apply_patch_json() == call["patch"], f"{where}:\n{eng.apply_patch_json()[:2000]}\n{call['patch'][:2000]}"
                before = twin.resident_counters()
                twin.apply_changes(ChangeLog.from_changes([_b64(call["change"])]))
                remote_delta.append(tuple(a - b for a, b in zip(twin.resident_counters(), before)))
            else:
                with pytest.raises(engine.InvalidChanges) as ei:
                    eng.apply_local_change(call["request"])
                assert ei.value.code == engine.AM355_E_INVALID, where
                refused += 1
            assert eng.local_change_calls() == (served, refused), where
        assert _whole(eng.patch_json()) == _whole(s["whole_patch"]), f"{s['name']}: getPatch at the end"
        assert hashlib.sha256(bytes(eng.save())).hexdigest() == s["save_sha256"], f"{s['name']}: Backend.save at the end"
    finally:
        eng.close()
        twin.close()
    print(s["name"], "local calls added", local_delta, "as remote changes", remote_delta)
    return local_delta, remote_delta


def check_session(make_engine, name):
    s = BY_NAME[name]
    local_delta, remote_delta = drive_session(make_engine, s)
    if s["calls"][0]["kind"] != "load":
        # (a loaded lineage: the local call itself turns the document into its changes, the twin's does so one call later)
        assert local_delta == remote_delta, f"{name}: local changes took another path than the same changes applied as remote ones"
    if name in ("text_runs", "deletes"):
        assert local_delta.count(IN_PLACE) >= len(local_delta) - 2, f"{name}: {local_delta}"   # (all but the call that makes the Text and the first onto it)


@pytest.mark.parametrize("name", NAMES)
def test_session(emu_lib, monkeypatch, name):
    _verify(monkeypatch)
    check_session(_emulated(emu_lib), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_session_gpu(monkeypatch, name):
    _verify(monkeypatch)
    check_session(_gpu, name)


A = "7" * 32


def _request(seq, start_op, ops, deps=()):
    return {"actor": A, "seq": seq, "startOp": start_op, "time": 0, "message": "", "deps": list(deps), "ops": ops}


def check_refusals(make_engine):
    eng = make_engine()
    session = oracle_lib.OracleSession()
    try:
        first = _request(1, 1, [{"action": "makeText", "obj": "_root", "key": "text", "pred": []},
                                {"action": "set", "obj": f"1@{A}", "elemId": "_head", "insert": True, "values": ["a", "b"], "pred": []}])
        c1 = eng.apply_local_change(first)
        session.apply([c1], local=True)
        whole = eng.patch_json()
        cases = [
            (first, engine.InvalidChanges, engine.AM355_E_INVALID),   # the seq is applied already (backend.js:56)
            (_request(2, 4, [{"action": "set", "obj": f"1@{A}", "elemId": f"3@{A}", "insert": True, "values": ["x", "y"], "pred": [f"3@{A}"]}]),
             engine.InvalidChanges, engine.AM355_E_INVALID),          # multi-insert with a pred (columnar.js:451)
            (_request(2, 4, [{"action": "set", "obj": "_root", "key": "blob", "value": b"\x01\x02", "pred": []}]),
             engine.UnsupportedChanges, engine.AM355_E_UNSUPPORTED),  # a byte-array value
            (_request(2, 4, [{"action": "link", "obj": "_root", "key": "l", "child": f"1@{A}", "pred": []}]),
             engine.UnsupportedChanges, engine.AM355_E_UNSUPPORTED),  # what the flat form does not express
            (_request(3, 4, [{"action": "set", "obj": "_root", "key": "k", "value": 1, "pred": []}]),
             engine.InvalidChanges, engine.AM355_E_INVALID),          # no change with seq 2 (backend.js:44)
        ]
        for k, (req, exc, code) in enumerate(cases):
            before = eng.local_change_calls()
            with pytest.raises(exc) as ei:
                eng.apply_local_change(req)
            assert ei.value.code == code, k
            assert eng.local_change_calls() == (before[0], before[1] + 1), k
            assert eng.patch_json() == whole, f"case {k}: the state changed"
        good = _request(2, 4, [{"action": "set", "obj": f"1@{A}", "elemId": f"3@{A}", "insert": True, "value": "c", "pred": []}])
        c2 = eng.apply_local_change(good)
        assert same_local_patch(session.apply([c2], local=True), eng.apply_patch_json(), hashlib.sha256(c2[8:]).hexdigest())
        assert eng.local_change_calls() == (2, len(cases))
    finally:
        eng.close()
        session.close()


def test_refusals(emu_lib):
    check_refusals(_emulated(emu_lib))


@pytest.mark.gpu
def test_refusals_gpu():
    check_refusals(_gpu)


# ---------------------------------------------------------------------------------------------------------------------------
# multi-inserts at the scan's switch points and beyond one resident chunk, against the oracle
# ---------------------------------------------------------------------------------------------------------------------------
# rows + 1 values are scanned: 2047 rows fill one tile of 2048 exactly, 8191 rows are the last count one workgroup scans alone
SCAN_RUNS = [2047, 2048, 8191, 8192, 12289]


def check_long_run(make_engine, n):
    eng, twin = make_engine(), make_engine()
    session = oracle_lib.OracleSession()
    try:
        def local(req):
            before = eng.resident_counters()
            change = eng.apply_local_change(req)
            delta = tuple(a - b for a, b in zip(eng.resident_counters(), before))
            got = eng.apply_patch_json()
            want = session.apply([change], local=True)
            own = [h for h in json.loads(want)["deps"] if h not in json.loads(got)["deps"]]
            assert len(own) == 1, "exactly the new change's hash is taken out of the deps"
            assert same_local_patch(want, got, own[0]), f"{got[:600]}\n{want[:600]}"
            # the path: what the same change adds when it arrives as a remote one
            before = twin.resident_counters()
            twin.apply_changes(ChangeLog.from_changes([change]))
            assert delta == tuple(a - b for a, b in zip(twin.resident_counters(), before)), f"seq {req['seq']}"
            return delta
        local(_request(1, 1, [{"action": "makeText", "obj": "_root", "key": "text", "pred": []},
                              {"action": "set", "obj": f"1@{A}", "elemId": "_head", "insert": True, "values": ["s", "t"], "pred": []}]))
        values = [chr(97 + k % 26) if k % 97 else "é" for k in range(n)]   # (one- and two-byte values: the value offsets are a real scan)
        local(_request(2, 4, [{"action": "set", "obj": f"1@{A}", "elemId": f"3@{A}", "insert": True, "values": values, "pred": []}]))
        # typing behind the run's last element, and deleting across its first elements
        local(_request(3, 4 + n, [{"action": "set", "obj": f"1@{A}", "elemId": f"{3 + n}@{A}", "insert": True, "value": "!", "pred": []},
                                  {"action": "del", "obj": f"1@{A}", "elemId": f"4@{A}", "multiOp": 70, "pred": [f"4@{A}"]}]))
        # (the rows are carved with room to grow by now, whichever call outgrew the first carve: in place from here on)
        assert local(_request(4, 75 + n, [{"action": "set", "obj": f"1@{A}", "elemId": f"{4 + n}@{A}", "insert": True, "values": ["x", "y"], "pred": []}])) == IN_PLACE
        assert _whole(eng.patch_json()) == _whole(session.patch_json())
        assert eng.local_change_calls() == (4, 0)
    finally:
        eng.close()
        twin.close()
        session.close()


@pytest.mark.parametrize("n", SCAN_RUNS)
def test_long_runs(emu_lib, monkeypatch, n):
    _verify(monkeypatch)
    check_long_run(_emulated(emu_lib), n)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SCAN_RUNS)
def test_long_runs_gpu(monkeypatch, n):
    _verify(monkeypatch)
    check_long_run(_gpu, n)


# ---------------------------------------------------------------------------------------------------------------------------
# (f) nothing stays allocated
# ---------------------------------------------------------------------------------------------------------------------------
def test_destroyed_context_leaves_nothing_behind(emu_lib):
    lib = engine.load_library(emu_lib)
    lib.am355_emu_live.argtypes = [ctypes.POINTER(ctypes.c_long)]
    lib.am355_emu_live.restype = None

    def live():
        out = (ctypes.c_long * 4)()
        lib.am355_emu_live(out)
        return tuple(int(x) for x in out)
    gc.collect()
    start = live()
    for name in ("text_runs", "numbers", "rejected", "loaded_own_author"):
        eng = _emulated(emu_lib)()
        try:
            for call in BY_NAME[name]["calls"]:
                if call["kind"] == "load":
                    eng.load_document(_b64(call["doc"]))
                    eng.replay()
                elif call["kind"] == "remote":
                    eng.apply_changes(ChangeLog.from_changes([_b64(c) for c in call["batch"]]))
                elif call["kind"] == "local":
                    eng.apply_local_change(call["request"])
                else:
                    with pytest.raises(engine.InvalidChanges):
                        eng.apply_local_change(call["request"])
            busy = live()
            assert busy[0] > start[0] and busy[1] > start[1], (name, busy)
        finally:
            eng.close()
        assert live() == start, name


# ---------------------------------------------------------------------------------------------------------------------------
# the record tables keep their layout: callers compiled against am355_patch_ir (bench.py's PatchIR among them) hand the library a
# struct of that size; what a local patch adds travels through am355_apply_local_envelope
# ---------------------------------------------------------------------------------------------------------------------------
def test_patch_ir_keeps_the_layout_callers_hold(emu_lib):
    import bench
    eng = _emulated(emu_lib)()
    try:
        eng.apply_local_change(_request(1, 1, [{"action": "set", "obj": "_root", "key": "k", "value": 1, "pred": []}]))
        size = ctypes.sizeof(bench.PatchIR)
        for call in (eng._L.am355_fetch_apply_ir, eng._L.am355_fetch_ir):
            buf = (ctypes.c_uint8 * (size + 64))(*([0xA5] * (size + 64)))
            eng._check(call(eng._h, ctypes.addressof(buf)))
            assert bytes(buf[size:]) == b"\xa5" * 64, "the library wrote past the am355_patch_ir its callers were compiled against"
            assert bytes(buf[:size]) != b"\xa5" * size
    finally:
        eng.close()
