"""Small local changes built by one workgroup (include/am355.h am355_set_local_small; csrc/am355_hist.hip kl_small): with the switch on, a
change request inside the limits of csrc/am355_hist.h LOCAL_SMALL_* is expanded and its twelve columns are encoded in ONE launch that
writes them straight into pinned host memory; every other request takes the bulk path of tests/test_local_change.py.

tests/golden/local/small_edges.json (tools/fixtures/make_local_small_edges.js) holds hand-shaped requests with what the reference's own
encodeChange made of them: the smallest shapes at which the kernel can go wrong. Here, always with AM355_LOCAL_SMALL_VERIFY=1 (every small
build is repeated by the bulk path and compared column by column):
  (a) the fixture holds every shape, by name
  (b) encode_change of every entry == the recorded bytes and hash, and local_small_calls()[0] grows by one
  (c) every request the reference's FRONTEND made (tests/golden/local/sessions.json) through encode_change == the recorded bytes
  (d) every session of that fixture call by call through test_local_change.check_session: bytes, patch text, whole-document patch, save,
      which resident path served
  (e) the limits: a request exactly on each is built small, one past it goes to the bulk path; both equal the switch-off bytes and the
      recorded ones
  (f) switch off: local_small_calls() stays (0, 0)
  (g) a context destroyed after small local changes leaves no HIP resource behind
  (h) refusals and rejections are what they are with the switch off
Each body runs on the emulation of tests/emu and, marked gpu, on the device."""
import base64
import ctypes
import gc
import json
import os

import pytest

import test_local_change as tlc
from automerge_classic_amd import engine
from automerge_classic_amd.loggen import ChangeLog
from test_local_change import emu_lib  # noqa: F401  (the fixture that builds the emulation)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "local", "small_edges.json")
with open(FIXTURE) as _f:
    ENTRIES = json.load(_f)["entries"]
BY_NAME = {e["name"]: e for e in ENTRIES}
# csrc/am355_hist.h LOCAL_SMALL_*
ROWS, PREDS, OPS, BYTES = 512, 512, 256, 4096

PATTERNS = ("run2", "lit2", "abb", "aab", "run_lit_run", "null_middle", "null_leading", "null_trailing")
SHAPES = (["empty_change", "one_root_set", "type_own_elem", "type_other_elem"]
          + [f"{kind}_{p}" for kind in ("num", "delta", "key") for p in PATTERNS]
          + ["key_200_bytes", "key_multibyte", "key_same_first_16", "every_value_tag", "leb128_edges"]
          + [f"multi_insert_{n}" for n in (63, 64, 65, 128)]
          + ["multi_delete_70", "five_preds_three_actors", "counters_go_down", "make_map_and_sets", "make_text_and_insert", "make_list_and_table",
             "inc", "del_key", "container_below_256", "container_above_256"]
          + [f"limit_{what}_{side}" for what in ("rows", "preds", "ops", "bytes") for side in ("on", "past")])


def _small(make_engine):
    def make():
        eng = make_engine()
        eng.set_local_small(True)
        return eng
    return make


def _emulated(lib):
    return _small(tlc._emulated(lib))


_gpu = _small(tlc._gpu)


def _verify(monkeypatch):
    tlc._verify(monkeypatch)
    monkeypatch.setenv("AM355_LOCAL_SMALL_VERIFY", "1")


def _b64(x):
    return base64.b64decode(x)


# ---------------------------------------------------------------------------------------------------------------------------
# (a) the fixture
# ---------------------------------------------------------------------------------------------------------------------------
def test_fixture_holds_the_shapes():
    assert sorted(e["name"] for e in ENTRIES) == sorted(SHAPES)
    ops = lambda name: BY_NAME[name]["request"]["ops"]   # noqa: E731
    assert ops("empty_change") == []
    assert len(ops("key_200_bytes")[0]["key"]) == 200
    assert {len(k["key"].encode()) for k in ops("key_multibyte")} == {1, 2, 3, 4}
    assert len({k["key"][:16] for k in ops("key_same_first_16")}) == 1
    assert [len(ops(f"multi_insert_{n}")[0]["values"]) for n in (63, 64, 65, 128)] == [63, 64, 65, 128]
    assert {len(v.encode()) for v in ops("multi_insert_65")[0]["values"]} == {1, 2, 3, 4}
    assert ops("multi_delete_70")[0]["multiOp"] == 70
    preds = ops("five_preds_three_actors")[0]["pred"]
    assert len(preds) == 5 and len({p.split("@")[1] for p in preds}) == 3 and preds != sorted(preds, key=lambda p: (int(p.split("@")[0]), p.split("@")[1]))
    assert BY_NAME["type_own_elem"]["request"]["seq"] == 2 and len(BY_NAME["type_own_elem"]["request"]["deps"]) == 1
    assert [v["value"] for v in ops("leb128_edges")[:8]] == [63, 64, 127, 128, -64, -65, 2 ** 53 - 1, -(2 ** 53 - 1)]
    assert _b64(BY_NAME["container_below_256"]["change"])[8] == 1 and _b64(BY_NAME["container_above_256"]["change"])[8] == 2
    # the entries at the limits are exactly on them and one past them
    assert [len(ops(f"limit_rows_{s}")[0]["values"]) for s in ("on", "past")] == [ROWS, ROWS + 1]
    assert [sum(len(o["pred"]) for o in ops(f"limit_preds_{s}")) for s in ("on", "past")] == [PREDS, PREDS + 1]
    assert [len(ops(f"limit_ops_{s}")) for s in ("on", "past")] == [OPS, OPS + 1]
    assert [sum(len(o["key"].encode()) + len(o["value"].encode()) for o in ops(f"limit_bytes_{s}")) for s in ("on", "past")] == [BYTES, BYTES + 1]
    assert os.path.getsize(FIXTURE) < (1 << 20)


# ---------------------------------------------------------------------------------------------------------------------------
# (b) every entry
# ---------------------------------------------------------------------------------------------------------------------------
def check_entries(make_engine):
    eng = make_engine()
    try:
        for e in ENTRIES:
            before = eng.local_small_calls()
            got, digest = eng.encode_change(e["request"])
            assert got == _b64(e["change"]), f"{e['name']}:\n{got.hex()}\n{_b64(e['change']).hex()}"
            assert digest.hex() == e["hash"], e["name"]
            small = not e["name"].endswith("_past")
            assert eng.local_small_calls() == (before[0] + small, before[1] + (not small)), e["name"]
    finally:
        eng.close()


def test_entries(emu_lib, monkeypatch):  # noqa: F811
    _verify(monkeypatch)
    check_entries(_emulated(emu_lib))


@pytest.mark.gpu
def test_entries_gpu(monkeypatch):
    _verify(monkeypatch)
    check_entries(_gpu)


# ---------------------------------------------------------------------------------------------------------------------------
# (c) the requests the reference's frontend made
# ---------------------------------------------------------------------------------------------------------------------------
def check_frontend_requests(make_engine):
    eng = make_engine()
    n = 0
    try:
        for s in tlc.SESSIONS:
            for i, call in enumerate(s["calls"]):
                req = tlc._with_own_hash(s, i) if call["kind"] == "local" else None
                if req is None:
                    continue
                got, digest = eng.encode_change(req)
                assert got == _b64(call["change"]) and digest.hex() == call["hash"], f"{s['name']} call {i}"
                n += 1
        assert n >= 25
        assert eng.local_small_calls() == (n, 0)   # (none of them is beyond the limits)
    finally:
        eng.close()


def test_frontend_requests(emu_lib, monkeypatch):  # noqa: F811
    _verify(monkeypatch)
    check_frontend_requests(_emulated(emu_lib))


@pytest.mark.gpu
def test_frontend_requests_gpu(monkeypatch):
    _verify(monkeypatch)
    check_frontend_requests(_gpu)


# ---------------------------------------------------------------------------------------------------------------------------
# (d) the sessions call by call
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tlc.NAMES)
def test_session(emu_lib, monkeypatch, name):  # noqa: F811
    _verify(monkeypatch)
    tlc.check_session(_emulated(emu_lib), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", tlc.NAMES)
def test_session_gpu(monkeypatch, name):
    _verify(monkeypatch)
    tlc.check_session(_gpu, name)


def _drive(eng, name):
    for call in tlc.BY_NAME[name]["calls"]:
        if call["kind"] == "load":
            eng.load_document(_b64(call["doc"]))
            eng.replay()
        elif call["kind"] == "remote":
            eng.apply_changes(ChangeLog.from_changes([_b64(c) for c in call["batch"]]))
        elif call["kind"] == "local":
            assert eng.apply_local_change(call["request"]) == _b64(call["change"])
        else:
            with pytest.raises(engine.InvalidChanges):
                eng.apply_local_change(call["request"])


def check_sessions_are_served_small(make_engine):
    for name in ("text_runs", "rejected"):
        eng = make_engine()
        try:
            _drive(eng, name)
            n_local = sum(c["kind"] == "local" for c in tlc.BY_NAME[name]["calls"])
            assert eng.local_small_calls() == (n_local, 0), name   # (a rejected request builds nothing)
            assert eng.local_change_calls()[0] == n_local
        finally:
            eng.close()


def test_sessions_are_served_small(emu_lib, monkeypatch):  # noqa: F811
    _verify(monkeypatch)
    check_sessions_are_served_small(_emulated(emu_lib))


@pytest.mark.gpu
def test_sessions_are_served_small_gpu(monkeypatch):
    _verify(monkeypatch)
    check_sessions_are_served_small(_gpu)


# ---------------------------------------------------------------------------------------------------------------------------
# (e) the limits
# ---------------------------------------------------------------------------------------------------------------------------
def check_limits(make_on, make_off):
    on, off = make_on(), make_off()
    try:
        for what in ("rows", "preds", "ops", "bytes"):
            at, past = BY_NAME[f"limit_{what}_on"], BY_NAME[f"limit_{what}_past"]
            before = on.local_small_calls()
            got_at = on.encode_change(at["request"])
            assert on.local_small_calls() == (before[0] + 1, before[1]), f"{what}: a request exactly on the limit is built small"
            got_past = on.encode_change(past["request"])
            assert on.local_small_calls() == (before[0] + 1, before[1] + 1), f"{what}: a request one past the limit takes the bulk path"
            for got, e in ((got_at, at), (got_past, past)):
                assert got == off.encode_change(e["request"]), f"{e['name']}: differs from the switch-off bytes"
                assert got[0] == _b64(e["change"]) and got[1].hex() == e["hash"], f"{e['name']}: differs from the recorded bytes"
        assert off.local_small_calls() == (0, 0)
    finally:
        on.close()
        off.close()


def test_limits(emu_lib, monkeypatch):  # noqa: F811
    _verify(monkeypatch)
    check_limits(_emulated(emu_lib), tlc._emulated(emu_lib))


@pytest.mark.gpu
def test_limits_gpu(monkeypatch):
    _verify(monkeypatch)
    check_limits(_gpu, tlc._gpu)


# ---------------------------------------------------------------------------------------------------------------------------
# (f) switch off
# ---------------------------------------------------------------------------------------------------------------------------
def check_switch_off(make_engine):
    eng = make_engine()
    try:
        _drive(eng, "text_runs")
        assert eng.local_change_calls()[0] > 0
        assert eng.local_small_calls() == (0, 0)
        # and off again after it was on
        eng.set_local_small(True)
        eng.encode_change(BY_NAME["one_root_set"]["request"])
        assert eng.local_small_calls() == (1, 0)
        eng.set_local_small(False)
        eng.encode_change(BY_NAME["one_root_set"]["request"])
        eng.encode_change(BY_NAME["limit_rows_past"]["request"])
        assert eng.local_small_calls() == (1, 0)
    finally:
        eng.close()


def test_switch_off(emu_lib, monkeypatch):  # noqa: F811
    _verify(monkeypatch)
    check_switch_off(tlc._emulated(emu_lib))


@pytest.mark.gpu
def test_switch_off_gpu(monkeypatch):
    _verify(monkeypatch)
    check_switch_off(tlc._gpu)


# ---------------------------------------------------------------------------------------------------------------------------
# (g) nothing stays allocated
# ---------------------------------------------------------------------------------------------------------------------------
def test_destroyed_context_leaves_nothing_behind(emu_lib, monkeypatch):  # noqa: F811
    _verify(monkeypatch)
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
            _drive(eng, name)
            assert eng.local_small_calls()[0] > 0, name
            busy = live()
            assert busy[0] > start[0] and busy[1] > start[1], (name, busy)
        finally:
            eng.close()
        assert live() == start, name


# ---------------------------------------------------------------------------------------------------------------------------
# (h) refusals
# ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(emu_lib, monkeypatch):  # noqa: F811
    _verify(monkeypatch)
    tlc.check_refusals(_emulated(emu_lib))


@pytest.mark.gpu
def test_refusals_gpu(monkeypatch):
    _verify(monkeypatch)
    tlc.check_refusals(_gpu)
