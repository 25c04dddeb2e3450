"""Backend.applyChanges onto the kept state (am355_replay.hip replay_resident) with one batch exactly ON each size limit of that path
and one just past it: the rows and roots the ordering workgroup holds (am355_resorder.h), the chunks of a larger batch, the item counts
at which the delta stage switches its partition kernels (am355_delta.hip), the row capacity the last full replay carved, the small map
sort (am355_merge.hip), the number of changes the path takes at all.

Every session compares every incremental patch, the whole-document patch behind each boundary batch and at the end with the sequential
oracle's (oracle_lib.OracleSession), with AM355_RESORDER_VERIFY=1 (the order the in-place merges left == the order computed from
scratch) -- and asserts WHICH path served each boundary call, by what the call added to eng.resident_counters() = (served, fell back,
in place) and eng.resident_maps_only_calls(): a batch that quietly takes the full replay says nothing about the kernel it aims at.

Each body takes a function that makes an engine context: the CPU suite runs it on the emulation of tests/emu (a wavefront's lanes one
after the other: the logic), the GPU suite on the device (barriers, ballots under divergence, LDS, the order of workgroups)."""
import hashlib
import json
import subprocess

import pytest

import oracle_lib
from automerge_classic_amd import engine, loggen
from automerge_classic_amd.loggen import ChangeLog
from test_apply_engine import EMU_DIR, EMU_LIB, _changes_of, _ordered, mixed_document_batches
from test_apply_vectors import same_patch

# what one call adds to (served, fell_back, in_place)
IN_PLACE = (1, 0, 1)       # merged into the resident state, the new list elements into the stored order (am355_resorder.hip)
MERGE_RUN = (1, 0, 0)      # merged into the resident state, every list ordered anew by the kernels of merge_run
FELL_BACK = (0, 1, 0)      # asked for the resident path and took the full replay
NOT_ATTEMPTED = (0, 0, 0)  # never asked (the first call of a context, more changes than the path takes)


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-s", "-C", EMU_DIR])
    return EMU_LIB


def _emulated(lib):
    return lambda: engine.Engine(0, lib)


def _gpu():
    return engine.Engine(0)


def _whole(text):
    return dict(_ordered(text))["diffs"]


def drive(make_engine, batches, paths, whole_after=(), maps_only=None, saved_log=None, reload_saved=False):
    """The calls of a session, one batch each, through a fresh context and through the oracle. `paths`: {index of a batch: what the call
    must add to resident_counters()}; `maps_only`: {index: what it must add to resident_maps_only_calls()}; `whole_after`: the batches
    behind which the whole-document patch is compared as well (always at the end). `saved_log`: Backend.save of the final state == of
    the bulk replay of that log; `reload_saved`: the saved document, loaded by the oracle, is the session's document.
    Returns what every call added: [(served, fell_back, in_place, maps_only, rows of the document afterwards, its map emissions)]."""
    eng = make_engine()
    session = oracle_lib.OracleSession()
    seen = []
    try:
        for i, batch in enumerate(batches):
            want = session.apply(batch)
            before = eng.resident_counters() + (eng.resident_maps_only_calls(),)
            eng.apply_changes(ChangeLog.from_changes(batch))
            after = eng.resident_counters() + (eng.resident_maps_only_calls(),)
            got = eng.apply_patch_json()
            delta = tuple(a - b for a, b in zip(after, before))
            st = eng.stats()
            seen.append(delta + (int(st.n_ops), int(st.n_map_values)))
            print(f"batch {i}: {len(batch)} changes, counters +{delta[:3]}, map-only calls +{delta[3]}, {seen[-1][4]} rows")
            assert same_patch(got, want), f"batch {i}:\n{got[:2000]}\n{want[:2000]}"
            if i in paths:
                assert delta[:3] == paths[i], f"batch {i} ({len(batch)} changes): the call added {delta[:3]} to (served, fell_back, in_place), not {paths[i]}"
            if maps_only is not None and i in maps_only:
                assert delta[3] == maps_only[i], f"batch {i}: {delta[3]} map-only calls, not {maps_only[i]}"
            if i in whole_after:
                assert _whole(eng.patch_json()) == _whole(session.patch_json()), f"getPatch after batch {i}"
        assert _whole(eng.patch_json()) == _whole(session.patch_json()), "getPatch at the end"
        if saved_log is not None:
            doc = bytes(eng.save())
            bulk = make_engine()
            try:
                bulk.load_changes(saved_log)
                bulk.replay()
                assert doc == bytes(bulk.save()), "Backend.save of the state the calls built differs from the bulk replay's"
            finally:
                bulk.close()
        if reload_saved:
            back = oracle_lib.OracleSession(bytes(eng.save()))
            try:
                assert _whole(back.patch_json()) == _whole(session.patch_json()), "the saved document, loaded by the oracle"
            finally:
                back.close()
    finally:
        eng.close()
        session.close()
    return seen


def concurrent(seed=5, **kw):
    return loggen.generate(loggen.KIND_TEXT_CONCURRENT, seed=seed, **kw)


def round_batches(log, n_actors, head_rounds, sizes):
    """The setup change and `head_rounds` whole rounds (every actor known from then on: a new actor takes the full replay), then batches
    of `sizes` changes -- the caller keeps each inside one round: a batch that spans rounds refers to its own elements, which the
    in-place merge leaves to merge_run."""
    ch = _changes_of(log)
    k = 1 + head_rounds * n_actors
    batches = [ch[:k]]
    for s in sizes:
        assert (k - 1) // n_actors == (k - 1 + s - 1) // n_actors, "a batch spans two rounds"
        assert k + s <= len(ch)
        batches.append(ch[k:k + s])
        k += s
    return batches


# ---------------------------------------------------------------------------------------------------------------------------
# the generator: several runs per change (loggen.cpp gen_text_concurrent, runs_per_change)
# ---------------------------------------------------------------------------------------------------------------------------
# SHA-256 of arena ++ offsets of the four benchmark configurations at scale 0.1, as the generator wrote them before it knew
# runs_per_change: the option draws nothing when it is off
BENCH_LOG_SHA256 = {
    "c2_text_typing": {False: "58fe9cb52736ec043f7fb811416bcb2286ce5c0d4d46df30e38752beeae85575",
                       True: "bdcfe4a53fd6ba3db2db120033ee6496669442076c1e4a9dfcf0956d5f2edd64"},
    "c3_map_lww": {False: "9104c979127bceb786600111b98623d037604ea5bc875b72092658c690b64107",
                   True: "9318b6cc2aa69d3664e226e8ad5f2b3358eb1fb6741c618214d9032c0d07269b"},
    "c4_text_single": {False: "e996d1813f3850ec6d20fb3e957269240f794ddc495e71bdf358792ed41ff8fc",
                       True: "a8745604142fcf33ea73e303ad337b1bbf1b69da00720389274a1b33b6a72e91"},
    "c4_text_multi": {False: "475d95356a804603362273f9e044e0114add0bfb4f038e56efb0ad73a1ddf540",
                      True: "432d0ac52d4eac582991f728ae12fb10d8d5159208cae16e9c105692003863cc"},
}


@pytest.mark.parametrize("name", sorted(BENCH_LOG_SHA256))
def test_bench_config_logs_keep_their_bytes(name):
    for deflate in (False, True):
        log = loggen.config(name, 0.1, deflate)
        assert hashlib.sha256(log.arena.tobytes() + log.offsets.tobytes()).hexdigest() == BENCH_LOG_SHA256[name][deflate]


def test_runs_per_change_makes_that_many_runs():
    """runs_per_change = 0 and 1 are the log without the option; r > 1: the same number of rows, and every change of a round holds r
    runs, each behind an element of its own that the document held before the round."""
    kw = dict(n_actors=7, n_rounds=3, ins_per_change=24, del_per_change=3, n_objects=2)
    plain = concurrent(**kw)
    assert bytes(concurrent(runs_per_change=1, **kw).arena) == bytes(plain.arena)
    runs = concurrent(runs_per_change=4, **kw)
    assert runs.n_ops == plain.n_ops and runs.n_changes == plain.n_changes and bytes(runs.arena) != bytes(plain.arena)
    # the oracle's patch of one such change holds its runs: up to r insert edits (two runs at one spot are one edit), each of
    # ins_per_change / r characters or a multiple
    session = oracle_lib.OracleSession()
    try:
        ch = runs.changes()
        session.apply(ch[:1 + 7])   # (the first round types into empty lists: every run at the head)
        n_edits = []
        for c in ch[1 + 7:]:
            found = []
            interpret_inserts(json.loads(session.apply([c]))["diffs"], found)
            assert sum(found) == 24 and all(n % 6 == 0 for n in found), found
            n_edits.append(len(found))
        assert max(n_edits) == 4 and sum(n == 4 for n in n_edits) > len(n_edits) // 2, n_edits
    finally:
        session.close()


def interpret_inserts(node, found):
    """The number of values of every insert / multi-insert edit of an incremental patch, objects in patch order."""
    for e in node.get("edits", []):
        if e["action"] == "insert":
            found.append(1)
        elif e["action"] == "multi-insert":
            found.append(len(e["values"]))
    for vals in node.get("props", {}).values():
        for v in vals.values():
            if isinstance(v, dict) and "objectId" in v:
                interpret_inserts(v, found)


# ---------------------------------------------------------------------------------------------------------------------------
# (a) RESORDER_ROWS_MAX = 12288: the rows kr_order holds in LDS -- one chunk of a batch
# ---------------------------------------------------------------------------------------------------------------------------
def check_order_chunk_rows(make_engine):
    """145 actors, 80 insertions + 16 deletions = 96 rows per change, one Text. Behind the setup change and 5 rounds (67,281 rows):
    128 changes = 12,288 rows = exactly the chunk; 129 changes = 12,384 rows = a full chunk and one of 96 rows against the order the first
    left (the order ping-pongs between its two arrays: the state's order is in the first again); 144 changes = 13,824 rows. All merged
    in place; Backend.save of the final state == the bulk replay's."""
    log = concurrent(n_actors=145, n_rounds=8, ins_per_change=80, del_per_change=16, n_objects=1)
    batches = round_batches(log, 145, 5, (128, 17, 129, 16, 144, 1))
    assert sum(len(c) for c in batches[0]) and log.n_ops == 1 + 145 * 80 + 7 * 145 * 96
    seen = drive(make_engine, batches, {i: IN_PLACE for i in range(1, 7)}, whole_after=(1, 3), saved_log=log)
    assert [s[4] for s in seen] == [67281, 67281 + 12288, 81201, 81201 + 12384, 95121, 95121 + 13824, 109041]


def test_order_chunk_rows_emulated(emu_lib, monkeypatch):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    check_order_chunk_rows(_emulated(emu_lib))


@pytest.mark.gpu
def test_order_chunk_rows_gpu(monkeypatch):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    check_order_chunk_rows(_gpu)


# ---------------------------------------------------------------------------------------------------------------------------
# (b) RESORDER_CHUNKS_MAX = 3 chunks = 36864 rows: the largest batch merged in place
# ---------------------------------------------------------------------------------------------------------------------------
def check_order_chunks_max(make_engine, ins, path):
    """145 actors, 240 insertions + 16 deletions = 256 rows per change: 144 changes = 36,864 rows = three full chunks, merged in place.
    With 241 insertions (257 rows per change) 144 changes are 37,008 rows: over the limit, the lists are ordered anew by merge_run --
    on the resident state still. Head: the setup change and the first round (34,801 / 34,946 rows; the rows carved by the first call,
    carve_cols: N + N / 4 + 65,536, hold both batches: no fallback)."""
    log = concurrent(n_actors=145, n_rounds=2, ins_per_change=ins, del_per_change=16, n_objects=1)
    batches = round_batches(log, 145, 1, (144, 1))
    seen = drive(make_engine, batches, {0: NOT_ATTEMPTED, 1: path, 2: IN_PLACE}, whole_after=(1,))
    assert seen[1][4] - seen[0][4] == 144 * (ins + 16) and sum(s[1] for s in seen) == 0


CHUNKS_MAX_CASES = [(240, IN_PLACE), (241, MERGE_RUN)]


@pytest.mark.parametrize("ins,path", CHUNKS_MAX_CASES)
def test_order_chunks_max_emulated(emu_lib, monkeypatch, ins, path):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    check_order_chunks_max(_emulated(emu_lib), ins, path)


@pytest.mark.gpu
@pytest.mark.parametrize("ins,path", CHUNKS_MAX_CASES)
def test_order_chunks_max_gpu(monkeypatch, ins, path):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    check_order_chunks_max(_gpu, ins, path)


# ---------------------------------------------------------------------------------------------------------------------------
# (c) RESORDER_ROOTS_MAX = 1024: new elements whose reference element is old
# ---------------------------------------------------------------------------------------------------------------------------
def check_order_roots_max(make_engine):
    """runs_per_change = 8: every change inserts 8 runs of 8 characters, each behind an old element of its own -- 8 roots per change
    (64 insertions + 8 deletions). 128 changes = 1024 roots = one root per thread of kr_order's size scan, its R x R rank count and its
    per-object ballot loop at their full width: in place. 129 changes = 1032 roots: over, ordered anew by merge_run on the resident
    state. 127 changes = 1016 roots: in place again (the refusal left nothing behind)."""
    log = concurrent(n_actors=145, n_rounds=5, ins_per_change=64, del_per_change=8, n_objects=1, runs_per_change=8)
    batches = round_batches(log, 145, 2, (128, 17, 129, 16, 127, 18))
    drive(make_engine, batches, {1: IN_PLACE, 2: IN_PLACE, 3: MERGE_RUN, 4: IN_PLACE, 5: IN_PLACE, 6: IN_PLACE}, whole_after=(1, 3, 5))


def test_order_roots_max_emulated(emu_lib, monkeypatch):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    check_order_roots_max(_emulated(emu_lib))


@pytest.mark.gpu
def test_order_roots_max_gpu(monkeypatch):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    check_order_roots_max(_gpu)


# ---------------------------------------------------------------------------------------------------------------------------
# (d) gap scans of several steps, more than 256 objects
# ---------------------------------------------------------------------------------------------------------------------------
def check_long_gap_scans_and_300_objects(make_engine):
    """145 actors, 300 insertions + 5 deletions per change into one of 300 Text objects, 4 rounds; behind the setup change and the
    first round every later round arrives as 72 + 73 changes (~22 k rows: two chunks). Two actors that open the same empty object in
    the two batches of a round make the later root scan forward past the earlier run of 300 elements for the first smaller id: more
    than 256 positions, i.e. five steps of kr_gaps' 64-wide ballot scan. (Observed under the emulation when this test was written, with
    a temporary print at the fifth step of that loop: 11 scans of this session get there, 300-element objects scanned to their end or
    to a smaller id behind position 256. There is no counter for it, so none is asserted.) 300 objects also take objects_block over a
    second stride of 256 objects with a carry.
    The path of every call follows from the rows: the first call carves room for N + N / 4 + 65,536 rows (carve_cols); a batch that
    fits is merged in place, the one that does not falls back on "row capacity" and carves anew."""
    log = concurrent(n_actors=145, n_rounds=4, ins_per_change=300, del_per_change=5, n_objects=300)
    batches = round_batches(log, 145, 1, (72, 73, 72, 73, 72, 73))
    seen = drive(make_engine, batches, {}, whole_after=(2,))
    cap = None
    paths = []
    for served, fell_back, in_place, _, rows, _ in seen:
        want = NOT_ATTEMPTED if cap is None else IN_PLACE if rows <= cap else FELL_BACK
        if want != IN_PLACE:
            cap = rows + rows // 4 + 65536
        paths.append(want)
        assert (served, fell_back, in_place) == want, (seen, paths)
    assert paths.count(IN_PLACE) == 5 and paths.count(FELL_BACK) == 1, paths


def test_long_gap_scans_and_300_objects_emulated(emu_lib, monkeypatch):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    check_long_gap_scans_and_300_objects(_emulated(emu_lib))


@pytest.mark.gpu
def test_long_gap_scans_and_300_objects_gpu(monkeypatch):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    check_long_gap_scans_and_300_objects(_gpu)


# ---------------------------------------------------------------------------------------------------------------------------
# (e) the delta stage's partitions by item count
# ---------------------------------------------------------------------------------------------------------------------------
# (rows per change = ins + del, changes) -> rows of the boundary batch; all behind the setup change and two rounds of 145 actors
EDIT_ITEM_SHAPES = {
    1024: (12, 4, 64),    # PART_LDS_MAX: all of it in one workgroup (kd_edit_small), four items per thread
    1025: (20, 5, 41),    # one more: kd_dom_tiles / kd_dom_cross, 5 tiles, the last one holds a single item
    1280: (16, 4, 64),    # an exact multiple of the 256-item tile
    1281: (16, 5, 61),    # and one item in a sixth tile
}


def check_edit_items(make_engine, items):
    ins, dele, n = EDIT_ITEM_SHAPES[items]
    assert (ins + dele) * n == items
    log = concurrent(n_actors=145, n_rounds=3, ins_per_change=ins, del_per_change=dele, n_objects=1)
    batches = round_batches(log, 145, 2, (n, 145 - n))
    seen = drive(make_engine, batches, {1: IN_PLACE, 2: IN_PLACE}, whole_after=(1,))
    assert seen[1][4] - seen[0][4] == items


@pytest.mark.parametrize("items", sorted(EDIT_ITEM_SHAPES))
def test_edit_items_at_the_partition_limits_emulated(emu_lib, monkeypatch, items):
    """In-place batches of exactly 1024 / 1025 edit items (PART_LDS_MAX) and 1280 / 1281 (a tile edge of kd_dom_tiles)."""
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    check_edit_items(_emulated(emu_lib), items)


@pytest.mark.gpu
@pytest.mark.parametrize("items", sorted(EDIT_ITEM_SHAPES))
def test_edit_items_at_the_partition_limits_gpu(monkeypatch, items):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    check_edit_items(_gpu, items)


def check_dom_items_max(make_engine, extra):
    """DOM_ITEMS_MAX = 65,536 = 256 tiles of 256 items. One actor typing, 4096 characters per change; the head is the makeText change
    and the first change (4,097 rows: the rows the first call carves, carve_cols, then hold the batch -- a head of a few hundred rows
    does not). 16 changes = 65,536 items: kd_dom_tiles with 256 tiles and a 256 x 256 grid of kd_dom_cross. With one character more
    the batch has 17 changes = 65,537 items: the partitions go level by level. More rows than the in-place list merge takes: both are
    merged by merge_run on the resident state."""
    log = loggen.generate(loggen.KIND_TEXT_TYPING, n_ops=17 * 4096 + extra, ops_per_change=4096, seed=5)
    ch = _changes_of(log)
    assert len(ch) == 18 + extra
    seen = drive(make_engine, [ch[:2], ch[2:]], {0: NOT_ATTEMPTED, 1: MERGE_RUN})
    assert seen[0][4] == 4097 and seen[1][4] - seen[0][4] == 65536 + extra


@pytest.mark.parametrize("extra", [0, 1])
def test_dom_items_max_emulated(emu_lib, extra):
    check_dom_items_max(_emulated(emu_lib), extra)


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [0, 1])
def test_dom_items_max_gpu(extra):
    check_dom_items_max(_gpu, extra)


# ---------------------------------------------------------------------------------------------------------------------------
# (f) row capacity
# ---------------------------------------------------------------------------------------------------------------------------
def check_row_capacity(make_engine, over):
    """The rows of the kept state have the room the last full replay carved (am355_replay.hip carve_cols, in am355_apply_changes:
    N + N / 4 + 65,536). One actor typing, 3999 characters per change: the head (makeText and the first change) has 4,000 rows --
    capacity 70,536. 16 changes follow, then the last one: with 70,535 characters in all the state ends at 70,536 rows = the capacity,
    served on the resident state (by merge_run: the typist jumps behind characters of the same change, which the in-place merge does not
    take); with one more the call falls back on "row capacity" and takes the full replay. Same patches."""
    cap = 4000 + 4000 // 4 + 65536
    log = loggen.generate(loggen.KIND_TEXT_TYPING, n_ops=cap - 1 + over, ops_per_change=3999, seed=5)
    ch = _changes_of(log)
    assert len(ch) == 19
    seen = drive(make_engine, [ch[:2], ch[2:18], ch[18:]], {0: NOT_ATTEMPTED, 1: MERGE_RUN, 2: FELL_BACK if over else MERGE_RUN}, whole_after=(1,))
    assert [s[4] for s in seen] == [4000, 4000 + 16 * 3999, cap + over]


@pytest.mark.parametrize("over", [0, 1])
def test_row_capacity_emulated(emu_lib, monkeypatch, over):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    check_row_capacity(_emulated(emu_lib), over)


@pytest.mark.gpu
@pytest.mark.parametrize("over", [0, 1])
def test_row_capacity_gpu(monkeypatch, over):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    check_row_capacity(_gpu, over)


# ---------------------------------------------------------------------------------------------------------------------------
# (g) the map half alone around MAP_SORT_SMALL = 512
# ---------------------------------------------------------------------------------------------------------------------------
def check_map_half_alone(make_engine, n_keys):
    """One actor sets every one of `n_keys` root keys in every change, beside a small Text of three other actors (merge_run_maps needs a
    document that holds a list): batches of map rows alone run the map half of the merge, whose emissions -- the keys, and the key of
    the Text -- are sorted by one workgroup up to MAP_SORT_SMALL = 512 of them and by radix passes beyond. n_keys 510 .. 514 put the
    count on the limit whichever way the Text's key counts, n_keys 254 .. 257 on the 256 emissions one workgroup finishes alone
    (k_map_small_finish). The saved document is loaded by the oracle as well (save sorts the map rows
    with the same switch)."""
    batches = mixed_document_batches(5, dict(n_actors=3, n_rounds=3, ins_per_change=6, del_per_change=2, n_objects=1),
                                     dict(n_actors=1, n_rounds=4, n_keys=n_keys), held_text=2)
    maps = set(_changes_of(loggen.generate(loggen.KIND_MAP_LWW, seed=6, n_actors=1, n_rounds=4, n_keys=n_keys)))   # (the map log of these batches)
    only_maps = [i for i, b in enumerate(batches) if i and all(c in maps for c in b)]
    assert len(only_maps) >= 2
    seen = drive(make_engine, batches, {i: MERGE_RUN for i in only_maps}, whole_after=only_maps[:1], maps_only={i: 1 for i in only_maps}, reload_saved=True)
    assert sum(s[1] for s in seen) == 0
    # the emissions the map half sorted (am355_stats n_map_values): the keys and the Text's -- 255 / 256 and 511 / 512 keys are on and
    # just past the limits
    assert [seen[i][5] for i in only_maps] == [n_keys + 1] * len(only_maps)


MAP_KEYS = [254, 255, 256, 257, 510, 511, 512, 513, 514]


@pytest.mark.parametrize("n_keys", MAP_KEYS)
def test_map_half_alone_around_the_small_sort_emulated(emu_lib, monkeypatch, n_keys):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    check_map_half_alone(_emulated(emu_lib), n_keys)


@pytest.mark.gpu
@pytest.mark.parametrize("n_keys", MAP_KEYS)
def test_map_half_alone_around_the_small_sort_gpu(monkeypatch, n_keys):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    check_map_half_alone(_gpu, n_keys)


# ---------------------------------------------------------------------------------------------------------------------------
# (h) the envelope: 144 changes
# ---------------------------------------------------------------------------------------------------------------------------
def check_envelope(make_engine):
    """A batch of 144 changes is served on the resident state; a whole round of 145 is not attempted (the counters stay) and takes the
    full replay; the call behind it is resident again."""
    log = concurrent(n_actors=145, n_rounds=4, ins_per_change=6, del_per_change=2, n_objects=1)
    batches = round_batches(log, 145, 1, (144, 1, 145, 144, 1))
    drive(make_engine, batches, {0: NOT_ATTEMPTED, 1: IN_PLACE, 2: IN_PLACE, 3: NOT_ATTEMPTED, 4: IN_PLACE, 5: IN_PLACE}, whole_after=(1, 3))


def test_envelope_of_144_changes_emulated(emu_lib, monkeypatch):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    check_envelope(_emulated(emu_lib))


@pytest.mark.gpu
def test_envelope_of_144_changes_gpu(monkeypatch):
    monkeypatch.setenv("AM355_RESORDER_VERIFY", "1")
    check_envelope(_gpu)
