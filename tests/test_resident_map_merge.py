"""Plain map rows merged into the STORED map records of the resident state (am355_set_resident_map_merge; am355_merge.hip "resident map
table", am355_replay.hip replay_resident): every batch row finds its key's records by binary search, the records whose rows no longer
emit go out, the batch's visible rows come in, one streaming pass writes the merged table beside the stored one.

Every session goes through test_resident_limits.drive: every incremental patch and the whole-document patches against the sequential
oracle (oracle_lib.OracleSession), with AM355_RESORDER_VERIFY=1 and AM355_MAPMERGE_VERIFY=1 -- behind every in-place map merge the
call rebuilds the map table and the objects' map ranges with merge_run_maps and compares them byte for byte --, and WHICH path served
each call: what it added to resident_counters() and to resident_map_merge_calls() = (merged in place, tried and declined).
All KIND_MAP_LWW logs use seed 6. Each body runs on the emulation (CPU suite) and on the device."""
import base64
import json
import os
import shutil
import subprocess

import pytest

from automerge_classic_amd import engine, loggen
from automerge_classic_amd.loggen import ChangeLog
from test_apply_engine import _changes_of, load_campaign, mixed_document_batches, run_campaign
from test_resident_limits import IN_PLACE, MERGE_RUN, NOT_ATTEMPTED, _emulated, _whole, drive, emu_lib  # noqa: F401 (emu_lib: fixture)

MAP_GROUP_MAX = 256         # am355_merge.hip: stored values of one key the walk of a group takes
MAPMERGE_ROWS_MAX = 16384   # am355_merge.h: plain map rows of one batch the stage takes
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SERVED, DECLINED, UNTRIED = (1, 0), (0, 1), (0, 0)


def _gpu():
    return engine.Engine(0)


@pytest.fixture(autouse=True)
def _verify(monkeypatch):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    monkeypatch.setenv("AM355_MAPMERGE_VERIFY", "1")


class Switched:
    """make_engine with the switch set (and am355_set_resident_new_actors when asked); of the FIRST context it makes (the session's:
    drive makes another for the bulk replay) it records what every apply_changes call added to resident_map_merge_calls(), and the
    whole-document patch the context gave last before it was closed."""

    def __init__(self, make_engine, on=True, new_actors=False):
        self.make_engine, self.on, self.new_actors, self.calls, self.last_patch = make_engine, on, new_actors, None, None

    def __call__(self):
        eng = self.make_engine()
        if self.on:
            eng.set_resident_map_merge(True)
        if self.new_actors:
            eng.set_resident_new_actors(True)
        if self.calls is None:
            self.calls = calls = []
            apply, patch = eng.apply_changes, eng.patch_json

            def tracked(log):
                before = eng.resident_map_merge_calls()
                apply(log)
                after = eng.resident_map_merge_calls()
                calls.append((after[0] - before[0], after[1] - before[1]))

            def remembered():
                self.last_patch = patch()
                return self.last_patch
            eng.apply_changes, eng.patch_json = tracked, remembered
        return eng


def map_log(n_actors, n_rounds, n_keys):
    return _changes_of(loggen.generate(loggen.KIND_MAP_LWW, n_actors=n_actors, n_rounds=n_rounds, n_keys=n_keys, seed=6))


# ---------------------------------------------------------------------------------------------------------------------------
# 1. a document without a list (the test that fails without the feature: such a document takes merge_run)
# ---------------------------------------------------------------------------------------------------------------------------
def check_pure_map_document(make_engine):
    """4 actors, 6 rounds, 64 keys. Round 1 in one call, the 8 changes of rounds 2-3 one per call, rounds 4-6 a call each: a round is 4
    concurrent changes, and two rows of one batch name the same pred. Every call behind the first is served on the resident state
    with its rows merged into the stored table; the same session with the switch off adds nothing and gives the same patches."""
    ch = map_log(4, 6, 64)
    batches = [ch[:4]] + [[c] for c in ch[4:12]] + [ch[12:16], ch[16:20], ch[20:24]]
    paths = {0: NOT_ATTEMPTED, **{i: MERGE_RUN for i in range(1, len(batches))}}
    make = Switched(make_engine)
    drive(make, batches, paths, whole_after=(1, 9), saved_log=ChangeLog.from_changes(ch), reload_saved=True)
    assert make.calls == [UNTRIED] + [SERVED] * (len(batches) - 1), make.calls
    off = Switched(make_engine, on=False)
    drive(off, batches, paths, whole_after=(1, 9))
    assert off.calls == [UNTRIED] * len(batches), off.calls


def test_pure_map_document_emulated(emu_lib):
    check_pure_map_document(_emulated(emu_lib))


def test_pure_map_document_without_verify_emulated(emu_lib, monkeypatch):
    """The same session with AM355_MAPMERGE_VERIFY unset: the verify mode runs merge_run_maps behind every in-place merge, which writes
    the table, the object ranges and the emission lists anew -- this twin goes on from the state the path itself leaves behind."""
    monkeypatch.delenv("AM355_MAPMERGE_VERIFY")
    check_pure_map_document(_emulated(emu_lib))


def test_beside_a_list_without_verify_emulated(emu_lib, monkeypatch):
    monkeypatch.delenv("AM355_MAPMERGE_VERIFY")
    check_beside_a_list(_emulated(emu_lib))


@pytest.mark.gpu
def test_pure_map_document_gpu():
    check_pure_map_document(_gpu)


@pytest.mark.gpu
def test_pure_map_document_without_verify_gpu(monkeypatch):
    monkeypatch.delenv("AM355_MAPMERGE_VERIFY")
    check_pure_map_document(_gpu)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. beside a list
# ---------------------------------------------------------------------------------------------------------------------------
def check_beside_a_list(make_engine):
    """A Text and root-map keys: maps-only calls at batches 1, 2, 5, 6, list + map calls at 4, 8 (the list rows merged in place, then
    the map rows), list-only calls at 3, 7. Exactly the six calls with map rows merge them into the stored table."""
    batches = mixed_document_batches(5, dict(n_actors=3, n_rounds=3, ins_per_change=6, del_per_change=2, n_objects=1),
                                     dict(n_actors=2, n_rounds=6, n_keys=40), held_text=4)
    assert len(batches) >= 9
    paths = {0: NOT_ATTEMPTED, 1: MERGE_RUN, 2: MERGE_RUN, 3: IN_PLACE, 4: IN_PLACE, 5: MERGE_RUN, 6: MERGE_RUN, 7: IN_PLACE, 8: IN_PLACE}
    maps_only = {1: 1, 2: 1, 3: 0, 4: 1, 5: 1, 6: 1, 7: 0, 8: 1}
    make = Switched(make_engine)
    drive(make, batches, paths, whole_after=(2, 4), maps_only=maps_only, saved_log=ChangeLog.from_changes([c for b in batches for c in b]))
    assert make.calls[:9] == [UNTRIED, SERVED, SERVED, UNTRIED, SERVED, SERVED, SERVED, UNTRIED, SERVED], make.calls
    assert all(c[1] == 0 for c in make.calls), make.calls
    off = Switched(make_engine, on=False)
    drive(off, batches, paths, maps_only=maps_only)
    assert off.calls == [UNTRIED] * len(batches), off.calls


def test_beside_a_list_emulated(emu_lib):
    check_beside_a_list(_emulated(emu_lib))


@pytest.mark.gpu
def test_beside_a_list_gpu():
    check_beside_a_list(_gpu)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. key shapes, two objects (reference-made fixtures)
# ---------------------------------------------------------------------------------------------------------------------------
KEY_FIXTURES = {"map_keys_small": (163, 177), "map_keys_mid": (406, 440), "map_keys_mixed": (810, 878)}   # records behind c1 -> at the end
DELIVERIES = ["132", "123", "1-23"]


def check_key_shapes(make_engine, name, delivery):
    """A root map and a nested map; keys equal in their first sixteen bytes, multi-byte and supplementary-plane keys, conflicts on every
    twelfth key (oracle/js/make_map_keys_golden.js). c2 is by an actor the document does not know: am355_set_resident_new_actors too."""
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        fx = json.load(f)
    c1, c2, c3 = (base64.b64decode(x) for x in fx["changes"])
    batches = {"132": [[c1], [c3], [c2]], "123": [[c1], [c2], [c3]], "1-23": [[c1], [c2, c3]]}[delivery]
    make = Switched(make_engine, new_actors=True)
    seen = drive(make, batches, {0: NOT_ATTEMPTED, **{i: MERGE_RUN for i in range(1, len(batches))}}, whole_after=(1,),
                 saved_log=ChangeLog.from_changes([c for b in batches for c in b]), reload_saved=True)
    assert make.calls == [UNTRIED] + [SERVED] * (len(batches) - 1), make.calls
    assert (seen[0][5], seen[-1][5]) == KEY_FIXTURES[name], seen
    assert _whole(make.last_patch) == _whole(fx["patch"]), "the final whole-document patch differs from the reference's"


@pytest.mark.parametrize("delivery", DELIVERIES)
@pytest.mark.parametrize("name", sorted(KEY_FIXTURES))
def test_key_shapes_emulated(emu_lib, name, delivery):
    check_key_shapes(_emulated(emu_lib), name, delivery)


@pytest.mark.gpu
@pytest.mark.parametrize("delivery", DELIVERIES)
@pytest.mark.parametrize("name", sorted(KEY_FIXTURES))
def test_key_shapes_gpu(name, delivery):
    check_key_shapes(_gpu, name, delivery)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. wide conflicts on one key
# ---------------------------------------------------------------------------------------------------------------------------
WIDE = [3, 64, 65, MAP_GROUP_MAX, MAP_GROUP_MAX + 1]


def check_wide_conflicts(make_engine, n_actors):
    """One key, n_actors concurrent values (around a wavefront, around MAP_GROUP_MAX). Rounds 1 and 2 in the first call; the first
    single change of round 3 overwrites every stored value and leaves one record, then the table grows again. A key with more than
    MAP_GROUP_MAX stored values is left to the path of before: with 257 actors that is the call that meets the 257 records of round 2
    -- no later call finds more than 256 stored. (No saved_log: Backend.save behind a bulk replay of such a log is a defect of its
    own, see the pull request that added this file.)"""
    ch = map_log(n_actors, 3, 1)
    k, step = 2 * n_actors, max(1, min(n_actors // 4, 128))
    batches = [ch[:k]] + [[c] for c in ch[k:k + 3]]
    k += 3
    while k < len(ch):
        batches.append(ch[k:k + step])
        k += step
    make = Switched(make_engine)
    seen = drive(make, batches, {0: NOT_ATTEMPTED, **{i: MERGE_RUN for i in range(1, len(batches))}}, whole_after=(1, 2), reload_saved=True)
    assert (seen[0][5], seen[1][5], seen[-1][5]) == (n_actors, 1, n_actors), seen
    first = DECLINED if n_actors > MAP_GROUP_MAX else SERVED
    assert make.calls == [UNTRIED, first] + [SERVED] * (len(batches) - 2), make.calls


@pytest.mark.parametrize("n_actors", WIDE)
def test_wide_conflicts_emulated(emu_lib, n_actors):
    check_wide_conflicts(_emulated(emu_lib), n_actors)


@pytest.mark.gpu
@pytest.mark.parametrize("n_actors", WIDE)
def test_wide_conflicts_gpu(n_actors):
    check_wide_conflicts(_gpu, n_actors)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. table sizes around a workgroup, and a large table
# ---------------------------------------------------------------------------------------------------------------------------
TABLE_KEYS = [255, 256, 257, 511, 512, 513]


def check_table_sizes(make_engine, n_keys):
    """One actor, four rounds, a change per call: every change replaces every record of the table (as many dead as new: around the
    workgroup of the streaming pass, around the small sort's 512 and its one-workgroup 256)."""
    ch = map_log(1, 4, n_keys)
    batches = [[c] for c in ch]
    make = Switched(make_engine)
    seen = drive(make, batches, {0: NOT_ATTEMPTED, 1: MERGE_RUN, 2: MERGE_RUN, 3: MERGE_RUN}, whole_after=(1,), saved_log=ChangeLog.from_changes(ch))
    assert [s[5] for s in seen] == [n_keys] * 4, seen
    assert make.calls == [UNTRIED, SERVED, SERVED, SERVED], make.calls


@pytest.mark.parametrize("n_keys", TABLE_KEYS)
def test_table_sizes_emulated(emu_lib, n_keys):
    check_table_sizes(_emulated(emu_lib), n_keys)


@pytest.mark.gpu
@pytest.mark.parametrize("n_keys", TABLE_KEYS)
def test_table_sizes_gpu(n_keys):
    check_table_sizes(_gpu, n_keys)


def check_large_table(make_engine):
    """8 actors, 4 rounds, 5000 keys: round 1 in the first call, then a change per call onto a table of thousands of records."""
    ch = map_log(8, 4, 5000)
    batches = [ch[:8]] + [[c] for c in ch[8:]]
    make = Switched(make_engine)
    drive(make, batches, {0: NOT_ATTEMPTED, **{i: MERGE_RUN for i in range(1, len(batches))}}, whole_after=(1, 9), saved_log=ChangeLog.from_changes(ch))
    assert make.calls == [UNTRIED] + [SERVED] * (len(batches) - 1), make.calls


def test_large_table_emulated(emu_lib):
    check_large_table(_emulated(emu_lib))


@pytest.mark.gpu
def test_large_table_gpu():
    check_large_table(_gpu)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. the stage's own row limit
# ---------------------------------------------------------------------------------------------------------------------------
def check_row_limit(make_engine, over):
    """One batch of exactly MAPMERGE_ROWS_MAX rows is merged in place, one of a row more is declined (on the host, before anything is
    enqueued for it) and served by the path of before. Five rounds in the first call, so that the capacity the full replay carves (rows + 25 %) holds the batch."""
    n = MAPMERGE_ROWS_MAX + over
    ch = map_log(1, 6, n)
    make = Switched(make_engine)
    seen = drive(make, [ch[:5], ch[5:]], {0: NOT_ATTEMPTED, 1: MERGE_RUN})
    assert seen[1][4] == 6 * n and seen[1][5] == n, seen
    assert make.calls == [UNTRIED, DECLINED if over else SERVED], make.calls


@pytest.mark.parametrize("over", [0, 1])
def test_row_limit_emulated(emu_lib, over):
    check_row_limit(_emulated(emu_lib), over)


@pytest.mark.gpu
@pytest.mark.parametrize("over", [0, 1])
def test_row_limit_gpu(over):
    check_row_limit(_gpu, over)


# ---------------------------------------------------------------------------------------------------------------------------
# 7. recorded sessions of the live reference (deletions, nested maps, tables) with both switches on
# ---------------------------------------------------------------------------------------------------------------------------
def check_recorded_sessions(make_engine, every, want):
    sessions, _ = load_campaign()
    names = {s["name"] for s in sessions[::every]}
    counted = []

    def make():
        eng = make_engine()
        eng.set_resident_map_merge(True)
        eng.set_resident_new_actors(True)
        close = eng.close
        eng.close = lambda: (counted.append(eng.resident_map_merge_calls()), close())
        return eng
    assert run_campaign(make, names=names) == want
    print(f"recorded sessions: {sum(c[0] for c in counted)} calls merged their map rows in place, {sum(c[1] for c in counted)} declined")


def test_recorded_sessions_emulated(emu_lib):
    check_recorded_sessions(_emulated(emu_lib), 2, (180, 0))   # (what test_apply_engine.test_campaign_sessions_emulated asserts without the switches)


@pytest.mark.gpu
def test_recorded_sessions_gpu():
    check_recorded_sessions(_gpu, 1, (447, 0))   # (test_apply_engine.test_campaign_sessions_gpu)


# ---------------------------------------------------------------------------------------------------------------------------
# 8. through the JS host
# ---------------------------------------------------------------------------------------------------------------------------
JS = os.path.join(ROOT, "automerge_classic_amd", "js")
NODE = shutil.which("node")


REF = "/root/reference"   # (the reference tree of the build container, as in tests/test_js_host.py; elsewhere the script takes the reference-made fixture)


def _run_js(**extra):
    if not os.path.exists(os.path.join(JS, "am355_napi.node")):
        import __graft_entry__ as g
        g.build_js_addon()
    env = dict(os.environ, NODE_PATH=os.path.join(ROOT, "oracle", "js_shims", "node_modules"), **extra)
    if os.path.isdir(REF):
        env.update(AUTOMERGE_REF=REF, AUTOMERGE_BACKEND_PATH=os.path.join(REF, "backend"))
    out = subprocess.run([NODE, os.path.join(JS, "test_map_merge.js")], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0 and "map merge through the JS host: ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    print(out.stdout[-600:])


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_js_host_merges_map_rows_emulated(emu_lib):
    """node -> index.js (which, with MI355X_MAP_MERGE=1 as the script sets it, switches the path on for the contexts it makes) -> addon -> the emulated engine, preloaded as
    tests/test_js_host.py does: rounds of Automerge.change key assignments by two writers applied call by call (the reference-made
    changes of a fixture where there is no reference tree), residentMapMergeCalls grows, the documents equal the reference backend's."""
    _run_js(LD_PRELOAD=" ".join(x for x in (emu_lib, os.environ.get("LD_PRELOAD")) if x))   # (in front of what the environment already preloads)


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_js_host_merges_map_rows_gpu():
    _run_js()
