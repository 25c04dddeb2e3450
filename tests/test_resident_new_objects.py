"""Batches that MAKE objects merged into the resident state in place (am355_set_resident_new_objects; am355_resorder.hip kr_new_objects,
am355_replay.hip replay_resident): the objects a batch makes take the next indexes of the stored object table and the end of the stored
list order, a list insert that makes an object is an element like any other, makes on string keys and the rows inside new maps go
through the map half of the merge -- no merge_run over the whole document.

The sessions are tests/golden/resident/new_objects.json (tools/fixtures/make_new_object_sessions.js: the reference's frontend made the
changes, its backend the recorded patches). Every session goes through test_resident_limits.drive: every incremental patch, the
whole-document patch behind every make-call and at the end against the sequential oracle, Backend.save against the bulk replay's
bytes, with AM355_RESORDER_VERIFY=1 (the next rebuild compares the order and every object's entry, first position and element count
with what the in-place calls left) -- and WHICH path served each call: what it added to resident_counters(), to
resident_maps_only_calls() and to resident_new_object_calls() = (served without merge_run, tried and declined).

A call that touches a list is IN_PLACE = (1, 0, 1). A call of map rows only -- `meta = {a: 1}`, a `set` inside a card -- has no list
element to merge: it is served by the map half alone, which resident_counters() shows as (1, 0, 0) like merge_run; what tells the two
apart is resident_maps_only_calls() (+1: the map half ran on its own, no list kernel) and, for a make-call, resident_new_object_calls().
Each body runs on the emulation (CPU suite) and on the device."""
import base64
import json
import os

import pytest

import oracle_lib
from automerge_classic_amd import engine
from automerge_classic_amd.loggen import ChangeLog
from test_apply_engine import run_campaign
from test_apply_vectors import same_patch
from test_resident_limits import FELL_BACK, IN_PLACE, MERGE_RUN, NOT_ATTEMPTED, _emulated, _whole, drive, emu_lib  # noqa: F401 (emu_lib: fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
MAPS_ALONE = (1, 0, 0)   # with resident_maps_only_calls() + 1: the map half of the merge on its own (no list kernel, no merge_run)


def _gpu():
    return engine.Engine(0)


def load_sessions():
    with open(os.path.join(HERE, "golden", "resident", "new_objects.json")) as f:
        fx = json.load(f)
    out = {}
    for s in fx["sessions"]:
        s = dict(s)
        s["batches"] = [[base64.b64decode(c) for c in b] for b in s["batches"]]
        out[s["name"]] = s
    return out


SESSIONS = load_sessions()

# Per session, for every call behind the first: (what it adds to resident_counters(), to resident_maps_only_calls()) with the switch on.
# L: list rows merged in place, no map row; LM: list rows in place and the map half behind them; M: map rows only, the map half alone.
L, LM, M = (IN_PLACE, 0), (IN_PLACE, 1), (MAPS_ALONE, 1)
SERVED = {
    # five pushes, a card at index 0, the card with a list and a text inside, meta = {a: 1}, log = Text + typing, two concurrent pushes;
    # then: a set inside a card, typing into the nested note, a card deleted, a push into tags, typing into log beside a key of meta
    "cards": [LM] * 5 + [LM, LM, M, LM, LM, M, L, L, L, LM],
    "wide": [LM, LM],
    "many": [LM, LM],
    "newcomer": [LM, LM],
}


class Switched:
    """make_engine with the switch set (and the two neighbouring ones when asked); of the FIRST context it makes (the session's: drive
    makes another for the bulk replay) it records what every apply_changes call added to resident_new_object_calls()."""

    def __init__(self, make_engine, on=True, new_actors=False, map_merge=False):
        self.make_engine, self.on, self.new_actors, self.map_merge, self.calls = make_engine, on, new_actors, map_merge, None

    def __call__(self):
        eng = self.make_engine()
        if self.on:
            eng.set_resident_new_objects(True)
        if self.new_actors:
            eng.set_resident_new_actors(True)
        if self.map_merge:
            eng.set_resident_map_merge(True)
        if self.calls is None:
            self.calls = calls = []
            apply = eng.apply_changes

            def tracked(log):
                before = eng.resident_new_object_calls()
                apply(log)
                after = eng.resident_new_object_calls()
                calls.append((after[0] - before[0], after[1] - before[1]))
            eng.apply_changes = tracked
        return eng


def play(make_engine, name, on=True, **switches):
    """One session through drive with the paths its calls must take: with the switch on as SERVED says and every make-call adding (1, 0)
    to resident_new_object_calls(); with it off every make-call by merge_run, adding nothing; the other calls alike in both."""
    s = SESSIONS[name]
    batches, makes = s["batches"], s["makes"]
    paths, maps_only = {0: NOT_ATTEMPTED}, {}
    for i, (path, alone) in enumerate(SERVED[name], 1):
        if makes[i] and not on:
            path, alone = MERGE_RUN, 0
        paths[i], maps_only[i] = path, alone
    assert len(paths) == len(batches)
    make = Switched(make_engine, on, **switches)
    seen = drive(make, batches, paths, whole_after=[i for i, m in enumerate(makes) if m], maps_only=maps_only,
                 saved_log=ChangeLog.from_changes([c for b in batches for c in b]))
    assert [x[4] - (seen[i - 1][4] if i else 0) for i, x in enumerate(seen)] == s["rows"], "the rows the recipe counted"
    assert make.calls == [(1, 0) if m and on else (0, 0) for m in makes], make.calls
    return seen


# ---------------------------------------------------------------------------------------------------------------------------
# 0. the fixture against the oracle (CPU): the sequential oracle follows every recorded session patch for patch
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SESSIONS))
def test_oracle_reproduces_the_recorded_reference_patches(name):
    s = SESSIONS[name]
    session = oracle_lib.OracleSession()
    try:
        for i, (batch, want) in enumerate(zip(s["batches"], s["patches"])):
            got = session.apply(batch)
            if want is not None:   # (a patch too large to record: 65 k characters, 300 cards)
                assert same_patch(got, want), f"{name} call {i}:\n{got[:2000]}\n{want[:2000]}"
        if s["whole_patch"] is not None:
            assert _whole(session.patch_json()) == _whole(s["whole_patch"]), f"{name}: getPatch at the end"
    finally:
        session.close()
    assert len(s["makes"]) == len(s["batches"]) == len(s["rows"]) and any(s["makes"])


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the sessions, switch on and off
# ---------------------------------------------------------------------------------------------------------------------------
PLAIN = ["cards", "wide", "many"]


@pytest.mark.parametrize("on", [True, False])
@pytest.mark.parametrize("name", PLAIN)
def test_sessions_emulated(emu_lib, monkeypatch, name, on):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    play(_emulated(emu_lib), name, on)


@pytest.mark.gpu
@pytest.mark.parametrize("on", [True, False])
@pytest.mark.parametrize("name", PLAIN)
def test_sessions_gpu(monkeypatch, name, on):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    play(_gpu, name, on)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. a make row and its children in different chunks (AM355_RESORDER_CHUNK=5: more chunks are allowed there)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cards", "wide"])
def test_sessions_in_chunks_of_five_rows_emulated(emu_lib, monkeypatch, name):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    monkeypatch.setenv("AM355_RESORDER_CHUNK", "5")
    play(_emulated(emu_lib), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cards", "wide"])
def test_sessions_in_chunks_of_five_rows_gpu(monkeypatch, name):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    monkeypatch.setenv("AM355_RESORDER_CHUNK", "5")
    play(_gpu, name)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. beside am355_set_resident_map_merge: the stored map records take no makes (declined there), later plain map calls merge in place
# ---------------------------------------------------------------------------------------------------------------------------
def check_cards_with_map_merge(make_engine):
    counted, wrapped = [], []
    switched = Switched(make_engine, map_merge=True)

    def make_counting():
        eng = switched()
        if not wrapped:   # (the session's context: the first one drive makes)
            wrapped.append(eng)
            close = eng.close
            eng.close = lambda: (counted.append(eng.resident_map_merge_calls()), close())
        return eng
    s = SESSIONS["cards"]
    paths = {0: NOT_ATTEMPTED}
    paths.update({i: p for i, (p, _) in enumerate(SERVED["cards"], 1)})
    drive(make_counting, s["batches"], paths, whole_after=[i for i, m in enumerate(s["makes"]) if m],
          saved_log=ChangeLog.from_changes([c for b in s["batches"] for c in b]))
    assert switched.calls == [(1, 0) if m else (0, 0) for m in s["makes"]], switched.calls
    merged, declined = counted[0]
    # every make-call is declined by the stored map records; the two later calls with plain map rows (a title renamed, a key of meta)
    # are merged into them in place -- on the object table the make-calls left
    assert declined == sum(s["makes"]) and merged == 2, counted


def test_cards_with_map_merge_emulated(emu_lib, monkeypatch):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    monkeypatch.setenv("AM355_MAPMERGE_VERIFY", "1")
    check_cards_with_map_merge(_emulated(emu_lib))


@pytest.mark.gpu
def test_cards_with_map_merge_gpu(monkeypatch):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    monkeypatch.setenv("AM355_MAPMERGE_VERIFY", "1")
    check_cards_with_map_merge(_gpu)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. declined on purpose: merge_run as before, counted
# ---------------------------------------------------------------------------------------------------------------------------
def check_declined(make_engine, on):
    """`list[3] = {}` (a list element ASSIGNED an object) and a counter increment beside a push: tried in place, declined, served by
    merge_run on the resident state -- (0, 1) each; without the switch never tried."""
    s = SESSIONS["declined"]
    make = Switched(make_engine, on)
    drive(make, s["batches"], {0: NOT_ATTEMPTED, 1: MERGE_RUN, 2: MERGE_RUN}, whole_after=(1, 2), maps_only={1: 0, 2: 0},
          saved_log=ChangeLog.from_changes([c for b in s["batches"] for c in b]))
    assert make.calls == [(0, 0)] + [(0, 1) if on else (0, 0)] * 2, make.calls


@pytest.mark.parametrize("on", [True, False])
def test_declined_batches_emulated(emu_lib, monkeypatch, on):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    check_declined(_emulated(emu_lib), on)


@pytest.mark.gpu
@pytest.mark.parametrize("on", [True, False])
def test_declined_batches_gpu(monkeypatch, on):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    check_declined(_gpu, on)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. a newcomer's first change pushes a card (am355_set_resident_new_actors too: every kept rank moves in front of the merge)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on", [True, False])
def test_newcomer_pushes_a_card_emulated(emu_lib, monkeypatch, on):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    play(_emulated(emu_lib), "newcomer", on, new_actors=True)


@pytest.mark.gpu
@pytest.mark.parametrize("on", [True, False])
def test_newcomer_pushes_a_card_gpu(monkeypatch, on):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    play(_gpu, "newcomer", on, new_actors=True)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. a make-call on the row capacity the first call carved
# ---------------------------------------------------------------------------------------------------------------------------
def check_make_call_at_the_row_capacity(make_engine, over):
    """The first call (4,000 rows) carves room for 4,000 + 1,000 + 65,536 rows (am355_replay.hip carve_cols); 17 changes of one typing
    run fill it up to three rows short (+ over) -- more rows than the in-place list merge takes: merge_run --; the pushed card's three
    rows then end exactly on the capacity and are merged in place, or end one row past it: the call declines on "row capacity" before
    anything of the kept state is written and the full replay serves it -- the switch is never tried. Same patches either way."""
    s = SESSIONS[f"capacity{over}"]
    assert s["capacity"] == 4000 + 1000 + 65536 and sum(s["rows"]) == s["capacity"] + over
    make = Switched(make_engine)
    seen = drive(make, s["batches"], {0: NOT_ATTEMPTED, 1: MERGE_RUN, 2: FELL_BACK if over else IN_PLACE}, whole_after=(2,),
                 saved_log=ChangeLog.from_changes([c for b in s["batches"] for c in b]))
    assert [x[4] for x in seen] == [4000, s["capacity"] - 3 + over, s["capacity"] + over]
    assert make.calls == [(0, 0), (0, 0), (0, 0) if over else (1, 0)], make.calls


@pytest.mark.parametrize("over", [0, 1])
def test_make_call_at_the_row_capacity_emulated(emu_lib, monkeypatch, over):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    check_make_call_at_the_row_capacity(_emulated(emu_lib), over)


@pytest.mark.gpu
@pytest.mark.parametrize("over", [0, 1])
def test_make_call_at_the_row_capacity_gpu(monkeypatch, over):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    check_make_call_at_the_row_capacity(_gpu, over)


# ---------------------------------------------------------------------------------------------------------------------------
# 7. the recorded campaigns of the live reference through a switched engine
# ---------------------------------------------------------------------------------------------------------------------------
CAMPAIGNS = ["apply_campaign.json.gz", "apply_campaign_lists.json.gz", "apply_campaign_conflicts.json.gz"]


def check_campaign(make_engine, fixture):
    """Every session of the fixture with the switch on: the patches are the live reference's, and (equal, refused) is what the same
    campaign gives without the switch. How many calls the new path served is printed: information, not a condition."""
    counted = []

    def make():
        eng = make_engine()
        eng.set_resident_new_objects(True)
        close = eng.close
        eng.close = lambda: (counted.append(eng.resident_new_object_calls()), close())
        return eng
    on = run_campaign(make, fixture=fixture)
    assert on == run_campaign(make_engine, fixture=fixture), fixture
    print(f"{fixture}: (equal, refused) = {on}; calls that made objects: {sum(c[0] for c in counted)} served in place, "
          f"{sum(c[1] for c in counted)} declined")


@pytest.mark.parametrize("fixture", CAMPAIGNS)
def test_campaigns_through_a_switched_engine_emulated(emu_lib, monkeypatch, fixture):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    check_campaign(_emulated(emu_lib), fixture)


@pytest.mark.gpu
@pytest.mark.parametrize("fixture", CAMPAIGNS)
def test_campaigns_through_a_switched_engine_gpu(monkeypatch, fixture):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    check_campaign(_gpu, fixture)
