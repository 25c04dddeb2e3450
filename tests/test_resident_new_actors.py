"""The first changes of a NEW actor on the resident applyChanges path (am355_set_resident_new_actors; am355_replay.hip replay_resident):
the new authors of a batch are inserted into the sorted actor table, one kernel renumbers the actor ranks the kept state holds
(am355_prims.hip k_remap_ranks) and the call goes on as a known actor's would -- instead of the full replay, whose cost grows with the
document.

Every session goes through test_resident_limits.drive: every incremental patch, the whole-document patch behind the newcomer's call and at
the end against the sequential oracle (oracle_lib.OracleSession), Backend.save against the bulk replay's bytes (actor table order, clock,
object ids), with AM355_RESORDER_VERIFY=1, and WHICH path served each call. Arrival orders are arranged by the author's id, read from the
change header. Each body runs on the emulation (CPU suite) and on the device."""
import pytest

import mutation_util
import oracle_lib
from automerge_classic_amd import engine, loggen
from automerge_classic_amd.loggen import ChangeLog
from mutation_util import _uleb
from test_apply_engine import _changes_of, load_campaign, mixed_document_batches, run_campaign
from test_resident_limits import FELL_BACK, IN_PLACE, MERGE_RUN, NOT_ATTEMPTED, _emulated, drive, emu_lib  # noqa: F401 (emu_lib: fixture)

REMAP_WG_ROWS = 1024    # am355_prims.h: ranks of a dense column one workgroup of k_remap_ranks rewrites per step
REMAP_LDS_RANKS = 4096  # am355_prims.h: the rank table is staged in LDS up to this many kept actors


def _gpu():
    return engine.Engine(0)


# ---------------------------------------------------------------------------------------------------------------------------
# change headers (columnar.js:635-652: deps, actor, seq, startOp, time, message, other actors)
# ---------------------------------------------------------------------------------------------------------------------------
def _header(change):
    assert change[8] == 1, "an uncompressed change"
    _, o = _uleb(change, 9)
    ndeps, o = _uleb(change, o)
    o += 32 * ndeps
    alen, o = _uleb(change, o)
    author = bytes(change[o:o + alen])
    o += alen
    for _ in range(3):
        _, o = _uleb(change, o)
    mlen, o = _uleb(change, o)
    o += mlen
    n_other, o = _uleb(change, o)
    others = []
    for _ in range(n_other):
        ln, o = _uleb(change, o)
        others.append(bytes(change[o:o + ln]))
        o += ln
    return author, others


def author_of(change):
    return _header(change)[0]


def other_actors_of(change):
    return _header(change)[1]


class Switched:
    """make_engine with the switch set; of the FIRST context it makes (the session's: drive makes another for the bulk replay) it records
    what every apply_changes call added to resident_new_actor_calls() and the actors the document then had."""

    def __init__(self, make_engine, on=True):
        self.make_engine, self.on, self.calls = make_engine, on, None

    def __call__(self):
        eng = self.make_engine()
        if self.on:
            eng.set_resident_new_actors(True)
        if self.calls is None:
            self.calls = calls = []
            apply = eng.apply_changes

            def tracked(log):
                before = eng.resident_new_actor_calls()
                apply(log)
                after = eng.resident_new_actor_calls()
                calls.append((after[0] - before[0], after[1] - before[1], int(eng.stats().n_actors)))
            eng.apply_changes = tracked
        return eng


def text_log(n_actors, n_rounds, ins, dele, accept=lambda ids: True, seed=7):
    """A KIND_TEXT_CONCURRENT log with one Text whose actor ids (ids[0]: the author of the setup change) pass `accept`: the first such
    seed from `seed` on. Returns (changes, ids by actor index)."""
    for s in range(seed, seed + 200):
        ch = _changes_of(loggen.generate(loggen.KIND_TEXT_CONCURRENT, n_actors=n_actors, n_rounds=n_rounds, ins_per_change=ins, del_per_change=dele,
                                         n_objects=1, seed=s))
        ids = [author_of(c) for c in ch[1:1 + n_actors]]
        assert ids[0] == author_of(ch[0]) and len(set(ids)) == n_actors
        if accept(ids):
            return ch, ids
    raise AssertionError("no seed gives such actor ids")


def first_calls_of_newcomers(batches):
    """Indexes of the batches (behind the first) that hold a change by an author no earlier batch had."""
    known = {author_of(c) for c in batches[0]}
    out = []
    for i, b in enumerate(batches[1:], 1):
        authors = {author_of(c) for c in b}
        if authors - known:
            out.append(i)
        known |= authors
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# 1. newcomers one by one, three arrival orders
# ---------------------------------------------------------------------------------------------------------------------------
ORDERS = ["generated", "ascending", "descending"]


def check_newcomers_one_by_one(make_engine, order):
    """6 actors, one Text, every change a call of its own behind the setup change (by actor 0: known from the start). The changes of the
    first round are mutually concurrent: in the generator's order; by ascending id with actor 0's the smallest -- every newcomer is
    appended to the table, no kept rank moves, no rewrite is launched --; by descending id with actor 0's the largest -- every newcomer
    takes rank 0 and every kept rank moves. No call falls back, each newcomer's is served as a known actor's would be; the same calls
    on a context without the switch take the full replay for the newcomers, as before."""
    accept = {"generated": lambda ids: True, "ascending": lambda ids: ids[0] == min(ids), "descending": lambda ids: ids[0] == max(ids)}[order]
    ch, ids = text_log(6, 3, 9, 3, accept)
    first = ch[1:7]
    if order != "generated":
        first = sorted(first, key=author_of, reverse=order == "descending")
    delivered = [ch[0]] + first + ch[7:]
    batches = [[c] for c in delivered]
    newcomer_calls = first_calls_of_newcomers(batches)
    assert len(newcomer_calls) == 5
    make = Switched(make_engine)
    seen = drive(make, batches, {0: NOT_ATTEMPTED}, whole_after=newcomer_calls, saved_log=ChangeLog.from_changes(delivered))
    assert sum(s[1] for s in seen) == 0, seen
    for i in newcomer_calls:
        assert seen[i][:3] in (IN_PLACE, MERGE_RUN), (i, seen[i])
        assert make.calls[i][0] == 1, (i, make.calls)
    inserted, rewrote = sum(c[0] for c in make.calls), sum(c[1] for c in make.calls)
    assert inserted == 5
    if order == "ascending":
        assert rewrote == 0, make.calls
    if order == "descending":
        assert rewrote == inserted, make.calls
    assert [c[2] for c in make.calls][-1] == 6
    # the same batches without the switch
    off = Switched(make_engine, on=False)
    seen = drive(off, batches, {})
    assert sum(s[1] for s in seen) >= 4 and sum(c[0] for c in off.calls) == 0, seen
    assert all(seen[i][:3] in (FELL_BACK, NOT_ATTEMPTED) for i in newcomer_calls), seen


@pytest.mark.parametrize("order", ORDERS)
def test_newcomers_one_by_one_emulated(emu_lib, monkeypatch, order):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    check_newcomers_one_by_one(_emulated(emu_lib), order)


@pytest.mark.gpu
@pytest.mark.parametrize("order", ORDERS)
def test_newcomers_one_by_one_gpu(monkeypatch, order):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    check_newcomers_one_by_one(_gpu, order)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the object and map tables a call keeps, under a moved rank
# ---------------------------------------------------------------------------------------------------------------------------
KEPT_TABLE_CASES = ["text", "map", "both"]


def check_kept_tables_under_a_moved_rank(make_engine, case):
    """A document that holds a Text and root-map keys (test_apply_engine.mixed_document_batches: a concurrent-text log and a map log side
    by side); the Text's maker, actor 0 of the text log, has the largest id of all, so every newcomer pushes its rank up -- the object
    table holds it as the Text's object id, the map records hold the ranks of the keys' writers.
    text: the newcomer's batch is its first-round text change -- merged in place, which keeps the object and map tables as they are.
    map: the newcomer's batch is its map change -- the map half of the merge alone (the kept text has three rounds: preds and deleted
    elements among the kept rows). both: one batch with a text change and a map change by two newcomers.
    The incremental patch, the whole-document patch right behind it and Backend.save equal the oracle's and the bulk replay's."""
    text_kw = dict(n_actors=4, n_rounds=3 if case == "map" else 1, ins_per_change=11, del_per_change=3, n_objects=1)
    map_kw = dict(n_actors=3, n_rounds=1, n_keys=12)
    n_text = 1 + text_kw["n_actors"] * text_kw["n_rounds"]
    for seed in range(11, 400):
        flat = [c for b in mixed_document_batches(seed, text_kw, map_kw, held_text=0) for c in b]
        text, maps = flat[:n_text], flat[n_text:]
        assert len(maps) == 3
        maker = author_of(text[0])
        if all(author_of(c) <= maker for c in flat):
            break
    else:
        raise AssertionError("no seed makes the Text's maker the largest id")
    late_text = min(text[2:5], key=author_of)   # (first-round changes of the text actors but the maker)
    late_map = min(maps, key=author_of)
    late = {"text": [late_text], "map": [late_map], "both": [late_text, late_map]}[case]
    head = [c for c in flat if c not in late]
    path = {"text": IN_PLACE, "map": MERGE_RUN, "both": IN_PLACE}[case]
    make = Switched(make_engine)
    seen = drive(make, [head, late], {0: NOT_ATTEMPTED, 1: path}, whole_after=(1,), maps_only={1: 0 if case == "text" else 1},
                 saved_log=ChangeLog.from_changes(head + late))
    assert make.calls[1][:2] == (1, 1) and make.calls[1][2] == 7, make.calls
    assert sum(s[1] for s in seen) == 0


@pytest.mark.parametrize("case", KEPT_TABLE_CASES)
def test_kept_tables_under_a_moved_rank_emulated(emu_lib, monkeypatch, case):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    check_kept_tables_under_a_moved_rank(_emulated(emu_lib), case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", KEPT_TABLE_CASES)
def test_kept_tables_under_a_moved_rank_gpu(monkeypatch, case):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    check_kept_tables_under_a_moved_rank(_gpu, case)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. shapes of the rewrite
# ---------------------------------------------------------------------------------------------------------------------------
# kept rows when the rank-moving newcomer arrives -> (changes of the first round in front of it, insertions per change): the setup
# change is one row, a first-round change has no deletions (the Text is empty). R = REMAP_WG_ROWS: one workgroup's rows per step.
KEPT_ROWS = {
    REMAP_WG_ROWS - 1: (14, 73),   # the last 16-byte word of the only workgroup is not full
    REMAP_WG_ROWS: (11, 93),       # exactly one workgroup
    REMAP_WG_ROWS + 1: (16, 64),   # a second workgroup for one row
    REMAP_WG_ROWS + 2: (25, 41),   # no multiple of the four ranks of a 16-byte word
    1: (0, 5),                     # the setup change alone: one kept row, one kept actor
}


def check_rewrite_shapes(make_engine, kept_rows):
    k, ins = KEPT_ROWS[kept_rows]
    assert 1 + k * ins == kept_rows
    # the newcomer: the smallest id among the actors but the setup's, and smaller than that one's when nobody else is kept
    ch, ids = text_log(k + 2, 1, ins, 0, (lambda ids: ids[0] != min(ids)) if k == 0 else (lambda ids: True))
    late = min(ch[2:], key=author_of)
    head = [ch[0]] + ([ch[1]] if k else []) + [c for c in ch[2:] if c is not late][:max(k - 1, 0)]
    assert len(head) == 1 + k
    make = Switched(make_engine)
    seen = drive(make, [head, [late]], {0: NOT_ATTEMPTED}, whole_after=(1,), saved_log=ChangeLog.from_changes(head + [late]))
    assert seen[0][4] == kept_rows and seen[1][4] == kept_rows + ins, seen
    assert seen[1][:3] in (IN_PLACE, MERGE_RUN) and make.calls[1][:2] == (1, 1), (seen, make.calls)


@pytest.mark.parametrize("kept_rows", sorted(KEPT_ROWS))
def test_rewrite_shapes_emulated(emu_lib, monkeypatch, kept_rows):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    check_rewrite_shapes(_emulated(emu_lib), kept_rows)


@pytest.mark.gpu
@pytest.mark.parametrize("kept_rows", sorted(KEPT_ROWS))
def test_rewrite_shapes_gpu(monkeypatch, kept_rows):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    check_rewrite_shapes(_gpu, kept_rows)


def check_rewrite_without_preds(make_engine):
    """The first round of a KIND_MAP_LWW log: the keys are new, no kept row has a pred. Three of four actors kept, the smallest id late."""
    ch = _changes_of(loggen.generate(loggen.KIND_MAP_LWW, n_actors=4, n_rounds=1, n_keys=40, seed=23))
    late = min(ch, key=author_of)
    head = [c for c in ch if c is not late]
    make = Switched(make_engine)
    seen = drive(make, [head, [late]], {0: NOT_ATTEMPTED}, whole_after=(1,), saved_log=ChangeLog.from_changes(head + [late]))
    assert seen[0][4] == 30 and seen[1][:2] == (1, 0) and make.calls[1] == (1, 1, 4), (seen, make.calls)


def test_rewrite_without_preds_emulated(emu_lib, monkeypatch):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    check_rewrite_without_preds(_emulated(emu_lib))


@pytest.mark.gpu
def test_rewrite_without_preds_gpu(monkeypatch):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    check_rewrite_without_preds(_gpu)


def check_rank_table_past_lds(make_engine):
    """REMAP_LDS_RANKS kept actors with one character each, then the two smallest ids one after the other: the first finds a rank table
    that just fits the kernel's LDS, the second one that does not and is read through L2. (A full replay of more than 4096 distinct
    actors leaves no resident state -- am355_decode.hip DISTINCT_CAP --, so such a state is only ever reached through this path.)"""
    n = REMAP_LDS_RANKS + 2
    ch, ids = text_log(n, 1, 1, 0)
    late = sorted(ch[2:], key=author_of)[:2][::-1]
    head = [c for c in ch if c is not late[0] and c is not late[1]]
    make = Switched(make_engine)
    seen = drive(make, [head, [late[0]], [late[1]]], {0: NOT_ATTEMPTED}, whole_after=(1,), saved_log=ChangeLog.from_changes(head + late))
    assert seen[0][4] == n - 1 and all(s[:3] in (IN_PLACE, MERGE_RUN) for s in seen[1:]), seen
    assert make.calls == [(0, 0, REMAP_LDS_RANKS), (1, 1, REMAP_LDS_RANKS + 1), (1, 1, REMAP_LDS_RANKS + 2)], make.calls


def test_rank_table_past_lds_emulated(emu_lib, monkeypatch):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    check_rank_table_past_lds(_emulated(emu_lib))


@pytest.mark.gpu
def test_rank_table_past_lds_gpu(monkeypatch):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    check_rank_table_past_lds(_gpu)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. several newcomers in one batch, one of them named by a later change of the batch
# ---------------------------------------------------------------------------------------------------------------------------
def _round_two_naming(ch, n_actors, known, wanted):
    """A second-round change by one of `known` whose table of other actors names one of `wanted`."""
    for c in ch[1 + n_actors:1 + 2 * n_actors]:
        if author_of(c) in known and set(other_actors_of(c)) & set(wanted):
            return c
    raise AssertionError("no second-round change names such an actor")


def check_newcomers_in_one_batch(make_engine, orphan):
    """4 actors, two kept. One batch: the first-round changes of the other two and a second-round change of a kept actor that lists one
    of them among its other actors -- served on the resident state, one call that inserts two actors. orphan: the first of the two
    newcomers' changes is delivered under an id nobody else uses (mutation_util.with_message_and_actor), so the second-round change
    names an id that nobody authored: the call takes the full replay (which queues that change, as the reference does). Same patches."""
    ch, ids = text_log(4, 2, 8, 4)
    kept, late = ids[:2], ids[2:]
    named = _round_two_naming(ch, 4, kept, late)
    late_changes = [c for c in ch[1:5] if author_of(c) in late]
    head = [ch[0]] + [c for c in ch[1:5] if author_of(c) in kept]
    make = Switched(make_engine)
    if not orphan:
        rest = [[c] for c in ch[5:] if c is not named]
        batches = [head, late_changes + [named]] + rest
        seen = drive(make, batches, {0: NOT_ATTEMPTED}, whole_after=(1,), saved_log=ChangeLog.from_changes([c for b in batches for c in b]))
        assert seen[1][:3] in (IN_PLACE, MERGE_RUN), seen
        assert make.calls[1][0] == 1 and make.calls[1][2] == 4 and sum(c[0] for c in make.calls) == 1, make.calls
        assert sum(s[1] for s in seen) == 0, seen
    else:
        who = next(a for a in other_actors_of(named) if a in late)
        stranger = bytes(b ^ 0x5a for b in who)
        assert stranger not in ids
        moved = [mutation_util.with_message_and_actor(c, b"", stranger) if author_of(c) == who else c for c in late_changes]
        seen = drive(make, [head, moved + [named]], {0: NOT_ATTEMPTED, 1: FELL_BACK})
        assert make.calls[1][0] == 0, make.calls


@pytest.mark.parametrize("orphan", [False, True])
def test_newcomers_in_one_batch_emulated(emu_lib, monkeypatch, orphan):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    check_newcomers_in_one_batch(_emulated(emu_lib), orphan)


@pytest.mark.gpu
@pytest.mark.parametrize("orphan", [False, True])
def test_newcomers_in_one_batch_gpu(monkeypatch, orphan):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    check_newcomers_in_one_batch(_gpu, orphan)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. a batch that fails behind the rewrite
# ---------------------------------------------------------------------------------------------------------------------------
def check_failure_behind_the_rewrite(make_engine):
    """4 actors, three rounds; actors 0 and 1 kept. The batch: the first-round change of a newcomer whose id moves a kept rank, and a
    second-round change of a kept actor that names only kept actors and the newcomer -- its sequence number is the next one, but it
    depends on the first-round change of the fourth actor, which has not come: the host finds that out behind the device work, rank
    rewrite included, and the call takes the full replay (which queues the change). Then the missing change, then change by change:
    resident again. Every patch equals the oracle's, and the engine counts the actors the oracle counts after every call."""
    def accept(ids):
        return min(ids[2:]) < max(ids[:2])
    for seed in range(7, 200):
        ch, ids = text_log(4, 3, 8, 1, accept, seed=seed)
        late = min(ids[2:])
        missing = next(a for a in ids[2:] if a != late)
        stuck = [c for c in ch[5:9] if author_of(c) in ids[:2] and missing not in other_actors_of(c)]
        if stuck:
            break
    else:
        raise AssertionError("no seed gives such a second-round change")
    stuck = stuck[0]
    first = {author_of(c): c for c in ch[1:5]}
    head = [ch[0], first[ids[0]], first[ids[1]]]
    batches = [head, [first[late], stuck], [first[missing]]] + [[c] for c in ch[5:] if c is not stuck]
    make = Switched(make_engine)
    seen = drive(make, batches, {0: NOT_ATTEMPTED, 1: FELL_BACK, 2: NOT_ATTEMPTED}, whole_after=(1, 2, 3))
    assert all(s[1] == 0 for s in seen[3:]) and sum(s[0] for s in seen[3:]) >= len(batches) - 4, seen
    assert make.calls[1][:2] == (0, 0), make.calls
    session = oracle_lib.OracleSession()
    try:
        for i, b in enumerate(batches):
            session.apply(b)
            assert make.calls[i][2] == oracle_lib.lib().amo_num_actors(session._h), (i, make.calls)
    finally:
        session.close()


def test_failure_behind_the_rewrite_emulated(emu_lib, monkeypatch):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    check_failure_behind_the_rewrite(_emulated(emu_lib))


@pytest.mark.gpu
def test_failure_behind_the_rewrite_gpu(monkeypatch):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    check_failure_behind_the_rewrite(_gpu)


def check_known_author_beside_a_newcomer(make_engine):
    """The per-author memo of the "other actors" table holds ranks from BEFORE an insertion. Two actors, three rounds; a resident call
    with the second actor's second-round change leaves its table in the memo; the next batch holds the setup change of an independent
    log -- a newcomer whose id sorts in front of every kept actor, so every kept rank moves -- and that actor's third-round change,
    whose table of other actors is byte for byte the one in the memo: its ranks must be looked up anew (a batch that inserts actors
    goes without the memo). One call, one insertion, one rewrite, the oracle's patches."""
    for seed in range(7, 200):
        ch, ids = text_log(2, 3, 8, 1, seed=seed)
        mine = [c for c in ch[3:] if author_of(c) == ids[1]]
        if len(mine) == 2 and other_actors_of(mine[0]) == other_actors_of(mine[1]) != []:
            break
    else:
        raise AssertionError("no seed repeats the table of other actors")
    theirs = [c for c in ch[3:] if author_of(c) == ids[0]]
    for seed in range(300, 500):
        setup = _changes_of(loggen.generate(loggen.KIND_TEXT_CONCURRENT, n_actors=1, n_rounds=1, ins_per_change=4, del_per_change=0, n_objects=1, seed=seed))[0]
        if author_of(setup) < min(ids):
            break
    else:
        raise AssertionError("no seed gives a newcomer in front of the kept actors")
    batches = [ch[:3], [theirs[0]], [mine[0]], [setup, mine[1]], [theirs[1]]]
    make = Switched(make_engine)
    seen = drive(make, batches, {0: NOT_ATTEMPTED}, whole_after=(3,))
    assert sum(s[1] for s in seen) == 0 and seen[3][:3] in (IN_PLACE, MERGE_RUN), seen
    assert make.calls[3] == (1, 1, 3), make.calls


def test_known_author_beside_a_newcomer_emulated(emu_lib, monkeypatch):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    check_known_author_beside_a_newcomer(_emulated(emu_lib))


@pytest.mark.gpu
def test_known_author_beside_a_newcomer_gpu(monkeypatch):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    check_known_author_beside_a_newcomer(_gpu)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. the actor count crosses a key width
# ---------------------------------------------------------------------------------------------------------------------------
def check_key_width_crossing(make_engine):
    """Four kept actors, ranks of two bits; the fifth makes them three bits wide (the sort keys of the list and map orders are built from
    bits(counter) + bits(actors)). Served, and the same document; then a second round of all five."""
    ch, ids = text_log(5, 2, 10, 2)
    late = min(ch[2:6], key=author_of)
    head = [c for c in ch[:6] if c is not late]
    batches = [head, [late]] + [[c] for c in ch[6:]]
    make = Switched(make_engine)
    seen = drive(make, batches, {0: NOT_ATTEMPTED}, whole_after=(1,), saved_log=ChangeLog.from_changes([c for b in batches for c in b]))
    assert seen[1][:3] in (IN_PLACE, MERGE_RUN) and make.calls[0][2] == 4 and make.calls[1] == (1, 1, 5), (seen, make.calls)
    assert sum(s[1] for s in seen) == 0


def test_key_width_crossing_emulated(emu_lib, monkeypatch):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    check_key_width_crossing(_emulated(emu_lib))


@pytest.mark.gpu
def test_key_width_crossing_gpu(monkeypatch):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    check_key_width_crossing(_gpu)


# ---------------------------------------------------------------------------------------------------------------------------
# 7. recorded sessions of the live reference with the switch on
# ---------------------------------------------------------------------------------------------------------------------------
def check_recorded_sessions(make_engine, every):
    """Sessions of tests/golden/apply_campaign.json.gz and apply_campaign_quirks.json.gz (maps, nested objects, counters and their
    increments, conflicts, lists with counters; actors that join call after call) with the switch on: the patches are the live
    reference's, and exactly the calls are served that are served without the switch -- many of them now by inserting an actor."""
    inserted = 0
    for fixture in ("apply_campaign.json.gz", "apply_campaign_quirks.json.gz"):
        sessions, _ = load_campaign(fixture)
        names = {s["name"] for s in sessions[::every]}
        made = []

        def make():
            made.append(make_engine())
            made[-1].set_resident_new_actors(True)
            close = made[-1].close
            made[-1].close = lambda eng=made[-1], close=close: (made.append(eng.resident_new_actor_calls()[0]), close())
            return made[-1]
        on = run_campaign(make, names=names, fixture=fixture)
        assert on == run_campaign(make_engine, names=names, fixture=fixture), fixture
        inserted += sum(x for x in made if isinstance(x, int))
    assert inserted >= 10, inserted


def test_recorded_sessions_emulated(emu_lib):
    check_recorded_sessions(_emulated(emu_lib), 3)


@pytest.mark.gpu
def test_recorded_sessions_gpu():
    check_recorded_sessions(_gpu, 2)


# ---------------------------------------------------------------------------------------------------------------------------
# 8. the rank inside a counter's stored last-increment id
# ---------------------------------------------------------------------------------------------------------------------------
def check_last_increment_rank(make_engine):
    """tests/golden/resident/last_inc_rank.json (oracle/js/make_last_inc_rank.js, hand-built with the reference's encodeChange). Actors
    X < A < N1 < N2 < B by id. First call: X makes the counter `cnt`, A and B increment it concurrently, both under op counter 5 -- the
    kept state stores 5@B, B of rank 2, as the id under which the completed counter is emitted (MergeBufs.last_inc). Second call: N1 and
    N2 arrive, N2 assigns `cnt` concurrently under 5@N2. The key now has two values, emitted in the order of (5@N2, 5@B): equal
    counters, so B's rank -- 4 now -- against N2's 3 decides. With the rank left at 2 the counter comes first, with the rewrite of that
    range (am355_replay.hip replay_resident) the string, as in the reference: in the patch of the call, in the whole-document patch behind
    it, and in the patch of a third call by A that leaves the key alone."""
    import base64
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resident", "last_inc_rank.json")) as f:
        fx = json.load(f)
    batches = [[base64.b64decode(c) for c in b] for b in fx["batches"]]
    ids = fx["actors"]
    assert ids["A"] < ids["N1"] < ids["N2"] < ids["B"]
    assert [author_of(c).hex() for c in batches[1]] == [ids["N1"], ids["N2"]]
    make = Switched(make_engine)
    seen = drive(make, batches, {0: NOT_ATTEMPTED}, whole_after=(1,), saved_log=ChangeLog.from_changes([c for b in batches for c in b]))
    assert all(s[:3] in (IN_PLACE, MERGE_RUN) for s in seen[1:]), seen
    assert make.calls == [(0, 0, 3), (1, 1, 5), (0, 0, 5)], make.calls   # the second call inserted actors (two at once) and rewrote the kept ranks


def test_last_increment_rank_emulated(emu_lib, monkeypatch):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    check_last_increment_rank(_emulated(emu_lib))


@pytest.mark.gpu
def test_last_increment_rank_gpu(monkeypatch):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    check_last_increment_rank(_gpu)
