"""Increments of map counters written into the resident state in place (am355_set_resident_counters; am355_resorder.hip kr_gaps,
am355_merge.hip kr_counters, am355_replay.hip resident_list_verdict): an `inc` on a string key takes no part in the list order, and one
launch over the batch rewrites the stored map record of every counter it feeds -- no merge_run, no map half of the merge.

The sessions are tests/golden/resident/counters.json (tools/fixtures/make_counter_sessions.js: the reference's frontend made the
changes, its backend the recorded patches; per call a `kind` says what the call holds). Every session goes through
test_resident_limits.drive: every incremental patch, the whole-document patch behind every increment call and at the end against the
sequential oracle, Backend.save against the bulk replay's bytes, with AM355_RESORDER_VERIFY=1 and AM355_COUNTERS_VERIFY=1 (behind every
call served the map table and ranges are rebuilt by the map half and compared byte for byte) -- and WHICH path served each call: what
it added to resident_counters(), to resident_maps_only_calls() and to resident_counter_calls() = (written in place with no merge_run and
no map half, tried and declined).

A call of increments only has no list element to merge: resident_counters() shows (1, 0, 0) like merge_run; what tells the two apart
is resident_counter_calls(). Each body runs on the emulation (CPU suite) and on the device."""
import base64
import json
import os

import pytest

import oracle_lib
from automerge_classic_amd import engine
from automerge_classic_amd.loggen import ChangeLog
from test_apply_engine import run_campaign
from test_apply_vectors import same_patch
from test_resident_limits import IN_PLACE, MERGE_RUN, NOT_ATTEMPTED, _emulated, _whole, drive, emu_lib  # noqa: F401 (emu_lib: fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
NO_LIST = (1, 0, 0)   # served on the resident state without a list merged in place: merge_run, the map half alone, or the counters alone


def _gpu():
    return engine.Engine(0)


def load_sessions():
    with open(os.path.join(HERE, "golden", "resident", "counters.json")) as f:
        fx = json.load(f)
    out = {}
    for s in fx["sessions"]:
        s = dict(s)
        s["batches"] = [[base64.b64decode(c) for c in b] for b in s["batches"]]
        out[s["name"]] = s
    return out


SESSIONS = load_sessions()

# kind of a call -> (what it adds to resident_counters(), to resident_maps_only_calls(), to resident_counter_calls()), switch on
ON = {
    "inc": (NO_LIST, 0, (1, 0)),            # increments only: the counters' records rewritten, nothing else runs
    "list+inc": (IN_PLACE, 0, (1, 0)),      # list rows merged in place, the counters' records rewritten
    "beside": (NO_LIST, 1, (0, 0)),         # beside plain map rows: the map half serves the increments too
    "beside+list": (IN_PLACE, 1, (0, 0)),   # the same behind an in-place list merge (a pushed map: am355_set_resident_new_objects)
    "declined": (NO_LIST, 1, (0, 1)),       # a key with conflicting values: declined, the map half
    "listinc": (MERGE_RUN, 0, (0, 0)),      # a counter inside a list: the list stage refuses
}
# switch off: every call with an increment is merge_run's
OFF = (MERGE_RUN, 0, (0, 0))


class Switched:
    """make_engine with the switch set (and the neighbouring ones when asked); of the FIRST context it makes (the session's: drive makes
    another for the bulk replay) it records what every apply_changes call added to resident_counter_calls(), and at its close
    resident_map_merge_calls() and resident_new_actor_calls()."""

    def __init__(self, make_engine, on=True, new_objects=False, new_actors=False, map_merge=False):
        self.make_engine, self.on, self.new_objects, self.new_actors, self.map_merge = make_engine, on, new_objects, new_actors, map_merge
        self.calls, self.at_close = None, None

    def __call__(self):
        eng = self.make_engine()
        if self.on:
            eng.set_resident_counters(True)
        if self.new_objects:
            eng.set_resident_new_objects(True)
        if self.new_actors:
            eng.set_resident_new_actors(True)
        if self.map_merge:
            eng.set_resident_map_merge(True)
        if self.calls is None:
            self.calls = calls = []
            apply, close = eng.apply_changes, eng.close

            def tracked(log):
                before = eng.resident_counter_calls()
                apply(log)
                after = eng.resident_counter_calls()
                calls.append((after[0] - before[0], after[1] - before[1]))

            def closing():
                self.at_close = {"map_merge": eng.resident_map_merge_calls(), "new_actors": eng.resident_new_actor_calls()}
                close()
            eng.apply_changes, eng.close = tracked, closing
        return eng


def play(make_engine, name, on=True, **switches):
    """One session through drive with the paths its calls must take: with the switch on as ON says, with it off every call that holds an
    increment by merge_run, adding nothing to the counters of the new stage. Setup calls (kind `setup`) are asserted nothing about but
    the first, which never asks for the resident path."""
    s = SESSIONS[name]
    batches, kinds = s["batches"], s["kinds"]
    assert len(kinds) == len(batches) == len(s["rows"]) and kinds[0] == "setup"
    paths, maps_only, want_calls = {0: NOT_ATTEMPTED}, {}, {}
    for i, kind in enumerate(kinds):
        if kind != "setup":
            paths[i], maps_only[i], want_calls[i] = ON[kind] if on else OFF
    make = Switched(make_engine, on, **switches)
    seen = drive(make, batches, paths, whole_after=sorted(want_calls), maps_only=maps_only,
                 saved_log=ChangeLog.from_changes([c for b in batches for c in b]))
    assert [x[4] - (seen[i - 1][4] if i else 0) for i, x in enumerate(seen)] == s["rows"], "the rows the recipe counted"
    for i, want in want_calls.items():
        assert make.calls[i] == want, f"{name} call {i} ({kinds[i]}): resident_counter_calls() + {make.calls[i]}, not {want}"
    assert all(c == (0, 0) for i, c in enumerate(make.calls) if i not in want_calls), make.calls
    return make


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the fixture against the oracle (CPU): the sequential oracle follows every recorded session patch for patch
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_fixture_holds_every_session():
    assert sorted(SESSIONS) == ["beside", "beside_push", "declined", "gone", "newcomer", "plain"]
    kinds = SESSIONS["plain"]["kinds"]
    assert kinds.count("inc") >= 8 and kinds.count("list+inc") >= 1 and max(len(b) for b in SESSIONS["plain"]["batches"]) == 40
    assert SESSIONS["declined"]["kinds"][-2:] == ["declined", "listinc"]


@pytest.mark.parametrize("name", sorted(SESSIONS))
def test_oracle_reproduces_the_recorded_reference_patches(name):
    s = SESSIONS[name]
    session = oracle_lib.OracleSession()
    try:
        for i, (batch, want) in enumerate(zip(s["batches"], s["patches"])):
            got = session.apply(batch)
            assert same_patch(got, want), f"{name} call {i}:\n{got[:2000]}\n{want[:2000]}"
        assert _whole(session.patch_json()) == _whole(s["whole_patch"]), f"{name}: getPatch at the end"
    finally:
        session.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the sessions, switch on and off (beside_push: with am355_set_resident_new_objects as well)
# ---------------------------------------------------------------------------------------------------------------------------
PLAIN = ["plain", "beside", "beside_push", "declined", "gone"]


def play_plain(make_engine, name, on):
    play(make_engine, name, on, new_objects=name == "beside_push")


@pytest.mark.parametrize("on", [True, False])
@pytest.mark.parametrize("name", PLAIN)
def test_sessions_emulated(emu_lib, monkeypatch, name, on):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    monkeypatch.setenv("AM355_COUNTERS_VERIFY", "1")
    play_plain(_emulated(emu_lib), name, on)


@pytest.mark.gpu
@pytest.mark.parametrize("on", [True, False])
@pytest.mark.parametrize("name", PLAIN)
def test_sessions_gpu(monkeypatch, name, on):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    monkeypatch.setenv("AM355_COUNTERS_VERIFY", "1")
    play_plain(_gpu, name, on)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the 40-change batch in chunks of five rows: the ONE launch of kr_counters covers every chunk's rows
# ---------------------------------------------------------------------------------------------------------------------------
def test_plain_in_chunks_of_five_rows_emulated(emu_lib, monkeypatch):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    monkeypatch.setenv("AM355_COUNTERS_VERIFY", "1")
    monkeypatch.setenv("AM355_RESORDER_CHUNK", "5")
    play(_emulated(emu_lib), "plain")


@pytest.mark.gpu
def test_plain_in_chunks_of_five_rows_gpu(monkeypatch):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    monkeypatch.setenv("AM355_COUNTERS_VERIFY", "1")
    monkeypatch.setenv("AM355_RESORDER_CHUNK", "5")
    play(_gpu, "plain")


# ---------------------------------------------------------------------------------------------------------------------------
# 4. beside am355_set_resident_map_merge: the stored map records' own stage never serves an increment call, the new stage does
# ---------------------------------------------------------------------------------------------------------------------------
def check_with_map_merge(make_engine):
    for name in ("plain", "beside"):
        make = play(make_engine, name, map_merge=True)
        merged, declined = make.at_close["map_merge"]
        # `plain`: no call behind the first holds a plain map row -- never attempted. `beside`: the two calls with plain rows beside the
        # increments are declined by that stage (it takes no increments) and served by the map half
        assert (merged, declined) == ((0, 0) if name == "plain" else (0, 2)), (name, merged, declined)


def test_with_map_merge_emulated(emu_lib, monkeypatch):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    monkeypatch.setenv("AM355_COUNTERS_VERIFY", "1")
    monkeypatch.setenv("AM355_MAPMERGE_VERIFY", "1")
    check_with_map_merge(_emulated(emu_lib))


@pytest.mark.gpu
def test_with_map_merge_gpu(monkeypatch):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    monkeypatch.setenv("AM355_COUNTERS_VERIFY", "1")
    monkeypatch.setenv("AM355_MAPMERGE_VERIFY", "1")
    check_with_map_merge(_gpu)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. a newcomer's first change is an increment (am355_set_resident_new_actors too: every kept rank moves in front of the merge,
#    the counters' last increments and the map records' ids among them)
# ---------------------------------------------------------------------------------------------------------------------------
def check_newcomer(make_engine, on):
    make = play(make_engine, "newcomer", on, new_actors=True)
    assert make.at_close["new_actors"] == (1, 1), make.at_close   # one call inserted an actor, and the rank rewrite ran


@pytest.mark.parametrize("on", [True, False])
def test_newcomer_increments_emulated(emu_lib, monkeypatch, on):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    monkeypatch.setenv("AM355_COUNTERS_VERIFY", "1")
    check_newcomer(_emulated(emu_lib), on)


@pytest.mark.gpu
@pytest.mark.parametrize("on", [True, False])
def test_newcomer_increments_gpu(monkeypatch, on):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    monkeypatch.setenv("AM355_COUNTERS_VERIFY", "1")
    check_newcomer(_gpu, on)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. the recorded campaigns of the live reference through a switched engine
# ---------------------------------------------------------------------------------------------------------------------------
CAMPAIGNS = ["apply_campaign.json.gz", "apply_campaign_lists.json.gz", "apply_campaign_conflicts.json.gz"]


def check_campaign(make_engine, fixture):
    """Every session of the fixture with the switch on: the patches are the live reference's, and (equal, refused) is what the same
    campaign gives without the switch. How many calls the new stage served is printed: information, not a condition."""
    counted = []

    def make():
        eng = make_engine()
        eng.set_resident_counters(True)
        close = eng.close
        eng.close = lambda: (counted.append(eng.resident_counter_calls()), close())
        return eng
    on = run_campaign(make, fixture=fixture)
    assert on == run_campaign(make_engine, fixture=fixture), fixture
    print(f"{fixture}: (equal, refused) = {on}; increment calls: {sum(c[0] for c in counted)} written in place, "
          f"{sum(c[1] for c in counted)} declined")


@pytest.mark.parametrize("fixture", CAMPAIGNS)
def test_campaigns_through_a_switched_engine_emulated(emu_lib, monkeypatch, fixture):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    monkeypatch.setenv("AM355_COUNTERS_VERIFY", "1")
    check_campaign(_emulated(emu_lib), fixture)


@pytest.mark.gpu
@pytest.mark.parametrize("fixture", CAMPAIGNS)
def test_campaigns_through_a_switched_engine_gpu(monkeypatch, fixture):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    monkeypatch.setenv("AM355_COUNTERS_VERIFY", "1")
    check_campaign(_gpu, fixture)
