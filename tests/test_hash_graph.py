"""Hash-graph queries on the engine (include/am355.h am355_find_changes / am355_changes_since / am355_changes_added /
am355_missing_deps; csrc/am355_graph.hip: k_graph_insert, k_hash_probe, k_absent_ballot): what BackendDoc.getChangeByHash,
getChanges, getChangesAdded and getMissingDeps answer (new.js:1921-2028), as indexes into the engine's list of changes.

tests/golden/graph/queries.json (tools/fixtures/make_graph_queries.js) holds histories made by the reference frontend and the
reference backend's answers as hash lists. Here:
  (a) every recorded answer, content and order, with the membership tests on the device (set_graph_probe_min(1)) and on the host
      index (0xffffffff); graph_query_calls() says which ran; the queries leave the patch, the resident counters and the way the next
      apply_changes is served as they were (a twin context that is never asked anything goes through the same calls)
  (b) the indexes are kept up call by call: after every apply_changes, resident and with AM355_NO_RESIDENT=1, each answer equals that
      of a fresh context loaded with the same changes
  (c) a plain-Python restatement of the two traversals, proven on the fixture, then held against the engine on generated logs
  (d) the device table by itself (prim_hash_probe) at its edges, and changes_added at partial ballot words
  (e) refusals: the documented code and text, the state as it was
  (f) a context destroyed after such queries leaves no HIP resource behind
Each body runs on the emulation of tests/emu and, marked gpu, on the device."""
import base64
import ctypes
import gc
import hashlib
import json
import os
import subprocess
import zlib

import numpy as np
import pytest

from automerge_classic_amd import engine, loggen
from automerge_classic_amd.loggen import ChangeLog
from test_apply_engine import EMU_DIR, EMU_LIB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "graph", "queries.json")
with open(FIXTURE) as _f:
    _FX = json.load(_f)
HISTORIES = _FX["histories"]
NAMES = [h["name"] for h in HISTORIES]
BY_NAME = {h["name"]: h for h in HISTORIES}
UNKNOWN = _FX["unknown"]
NONE32 = 0xFFFFFFFF
NEVER = 0xFFFFFFFF
DEVICE, HOST = 1, NEVER


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-s", "-C", EMU_DIR])
    return EMU_LIB


def _switched(eng):
    # (what the JS host turns on for every context, js/index.js acquireContext)
    eng.set_resident_new_actors(True)
    eng.set_resident_new_objects(True)
    eng.set_resident_counters(True)
    return eng


def _emulated(lib):
    return lambda: _switched(engine.Engine(0, lib))


def _gpu():
    return _switched(engine.Engine(0))


def _changes(h):
    return [base64.b64decode(c) for c in h["changes"]]


def _batches(h):
    cs, out, at = _changes(h), [], 0
    for n in h["batches"]:
        out.append(cs[at:at + n])
        at += n
    return out


def hex_list(eng, idx):
    hs = eng.hashes()
    return [bytes(hs[int(i)]).hex() for i in idx]


def engine_answers(eng, h):
    """Every query the fixture holds for history h, asked of eng: the same structure with the engine's answers."""
    out = {"get_changes": [], "change_by_hash": [], "missing_deps": []}
    for q in h["get_changes"]:
        try:
            out["get_changes"].append({"have": q["have"], "result": hex_list(eng, eng.changes_since(q["have"]))})
        except engine.InvalidChanges as e:
            assert e.code == engine.AM355_E_INVALID
            out["get_changes"].append({"have": q["have"], "error": _error_text(e)})
    for q in h["change_by_hash"]:
        i = int(eng.find_changes([q["hash"]])[0])
        found = i != NONE32
        if found:
            assert hex_list(eng, [i]) == [q["hash"]]
        out["change_by_hash"].append({"hash": q["hash"], "found": found})
    for q in h["missing_deps"]:
        out["missing_deps"].append({"heads": q["heads"], "result": [x.hex() for x in eng.missing_deps(q["heads"])]})
    return out


def _unique(hashes):
    seen, out = set(), []
    for x in hashes:
        if x not in seen:
            seen.add(x)
            out.append(x)
    return out


def _error_text(e):
    return "hash not found" + str(e).split("hash not found", 1)[1]


# ---------------------------------------------------------------------------------------------------------------------------
# (a) the fixture
# ---------------------------------------------------------------------------------------------------------------------------
def test_fixture_holds_the_shapes():
    assert set(NAMES) == {"linear", "diamonds", "six_concurrent", "withheld", "duplicates"}
    assert os.path.getsize(FIXTURE) < 200 * 1024
    assert BY_NAME["withheld"]["queued"] and len(BY_NAME["duplicates"]["changes"]) > len(BY_NAME["duplicates"]["applied"])
    pair_names = {p["name"] for h in HISTORIES for p in h["changes_added"]}
    assert {"equal", "ahead", "diverged_bc", "diverged_cb", "empty_other", "other_superset"} <= pair_names
    for h in HISTORIES:
        assert any("error" in q and q["error"] == "hash not found: " + UNKNOWN for q in h["get_changes"])
        assert any(q["found"] for q in h["change_by_hash"]) and any(not q["found"] for q in h["change_by_hash"])


def check_fixture(make_engine, name, probe_min):
    h = BY_NAME[name]
    eng, twin = make_engine(), make_engine()
    try:
        eng.set_graph_probe_min(probe_min)
        # call by call beside a twin that is never asked anything: same patches, same path for every call
        for batch in _batches(h):
            log = ChangeLog.from_changes(batch)
            eng.apply_changes(log)
            twin.apply_changes(log)
            assert eng.apply_patch_json() == twin.apply_patch_json()
            assert eng.resident_counters() == twin.resident_counters(), "a call after a query was served another way"
            hs = eng.hashes()
            eng.find_changes(hs)                       # in between: queries of every kind
            eng.changes_since([])
            eng.changes_since([bytes(hs[int(eng.applied()[0])])])
            eng.changes_added(hs[: len(hs) // 2])
            eng.missing_deps([UNKNOWN])
        before = (eng.patch_json(), eng.resident_counters(), eng.stats().n_applied, eng.stats().n_pending)
        calls0 = eng.graph_query_calls()
        assert hex_list(eng, eng.applied()) == h["applied"]
        assert hex_list(eng, eng.pending()) == h["queued"] or sorted(hex_list(eng, eng.pending())) == sorted(h["queued"])
        got = engine_answers(eng, h)
        for kind in ("get_changes", "change_by_hash", "missing_deps"):
            for g, w in zip(got[kind], h[kind]):
                assert g == w, f"{name} {kind} {json.dumps(w)[:300]}\n got {json.dumps(g)[:600]}"
        calls1 = eng.graph_query_calls()
        if probe_min == DEVICE:
            assert calls1[0] > calls0[0] and calls1[1] == calls0[1], (calls0, calls1)
        else:
            assert calls1[1] > calls0[1] and calls1[0] == calls0[0] == 0, (calls0, calls1)
        assert (eng.patch_json(), eng.resident_counters(), eng.stats().n_applied, eng.stats().n_pending) == before
        assert eng.patch_json() == twin.patch_json()
    finally:
        eng.close()
        twin.close()
    # pairs of states cut from the history: BackendDoc(second).getChangesAdded(first)
    cs, hashes = _changes(h), h["hashes"]
    for p in h["changes_added"]:
        eng = make_engine()
        try:
            eng.set_graph_probe_min(probe_min)
            if p["second"]:
                eng.load_changes(ChangeLog.from_changes([cs[i] for i in p["second"]]))
                eng.replay()
                whole = eng.patch_json()
                calls0 = eng.graph_query_calls()
                first = _unique(hashes[i] for i in p["first"])
                got = hex_list(eng, eng.changes_added(first))
                assert got == p["result"], f"{name} pair {p['name']}"
                # (other in any order)
                assert hex_list(eng, eng.changes_added(first[::-1])) == p["result"], f"{name} pair {p['name']}, other reversed"
                calls1 = eng.graph_query_calls()
                if first:
                    assert (calls1[0] > calls0[0]) == (probe_min == DEVICE) and (calls1[1] > calls0[1]) == (probe_min == HOST), (calls0, calls1)
                assert eng.patch_json() == whole
            else:
                assert p["result"] == []
        finally:
            eng.close()


@pytest.mark.parametrize("probe_min", [DEVICE, HOST], ids=["device", "host"])
@pytest.mark.parametrize("name", NAMES)
def test_fixture(emu_lib, name, probe_min):
    check_fixture(_emulated(emu_lib), name, probe_min)


@pytest.mark.gpu
@pytest.mark.parametrize("probe_min", [DEVICE, HOST], ids=["device", "host"])
@pytest.mark.parametrize("name", NAMES)
def test_fixture_gpu(name, probe_min):
    check_fixture(_gpu, name, probe_min)


# ---------------------------------------------------------------------------------------------------------------------------
# (b) incremental upkeep
# ---------------------------------------------------------------------------------------------------------------------------
def probe_set(eng):
    """A spread of queries whose hashes come from the context itself: answers as hash lists."""
    hs = eng.hashes()
    applied = [int(i) for i in eng.applied()]
    out = [hex_list(eng, eng.changes_since([]))]
    picks = applied[:: max(1, len(applied) // 6)] + applied[-2:]
    for i in picks:
        out.append(hex_list(eng, eng.changes_since([bytes(hs[i])])))
    if len(applied) > 2:
        out.append(hex_list(eng, eng.changes_since([bytes(hs[applied[-1]]), bytes(hs[applied[0]])])))
        out.append(hex_list(eng, eng.changes_since([bytes(hs[applied[1]]), bytes(hs[applied[-2]])])))
    out.append(hex_list(eng, eng.changes_added([bytes(hs[i]) for i in applied[: len(applied) // 2]])))
    out.append(hex_list(eng, eng.changes_added([bytes(hs[i]) for i in applied[1::2]])))
    out.append(hex_list(eng, eng.changes_added([])))
    every = sorted(set(bytes(x) for x in hs))   # (the two contexts' lists differ where a change was delivered twice: each hash once)
    out.append([int(i) != NONE32 for i in eng.find_changes(every)])
    out.append(hex_list(eng, [i for i in eng.find_changes(every) if int(i) != NONE32]))
    out.append([x.hex() for x in eng.missing_deps([UNKNOWN] + [bytes(hs[i]).hex() for i in applied[:1]])])
    return out


def check_upkeep(make_engine, name, probe_min):
    h = BY_NAME[name]
    eng = make_engine()
    try:
        eng.set_graph_probe_min(probe_min)
        so_far = []
        for batch in _batches(h):
            eng.apply_changes(ChangeLog.from_changes(batch))
            so_far += batch
            fresh = make_engine()
            try:
                fresh.set_graph_probe_min(probe_min)
                fresh.load_changes(ChangeLog.from_changes(so_far))
                fresh.replay()
                assert hex_list(eng, eng.applied()) == hex_list(fresh, fresh.applied())
                assert probe_set(eng) == probe_set(fresh), f"{name} after {len(so_far)} changes"
            finally:
                fresh.close()
        return eng.resident_counters()
    finally:
        eng.close()


@pytest.mark.parametrize("probe_min", [DEVICE, HOST], ids=["device", "host"])
@pytest.mark.parametrize("name", NAMES)
def test_upkeep_resident(emu_lib, name, probe_min):
    counters = check_upkeep(_emulated(emu_lib), name, probe_min)
    if name == "linear":
        assert counters[0] >= 4, f"the resident path served too few of the calls for the extension to be tested: {counters}"


@pytest.mark.parametrize("name", NAMES)
def test_upkeep_full_replay(emu_lib, monkeypatch, name):
    monkeypatch.setenv("AM355_NO_RESIDENT", "1")
    assert check_upkeep(_emulated(emu_lib), name, DEVICE)[0] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_upkeep_resident_gpu(name):
    check_upkeep(_gpu, name, DEVICE)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_upkeep_full_replay_gpu(monkeypatch, name):
    monkeypatch.setenv("AM355_NO_RESIDENT", "1")
    check_upkeep(_gpu, name, DEVICE)


# ---------------------------------------------------------------------------------------------------------------------------
# (c) the traversals restated in plain Python (new.js:1921-1997), proven on the fixture, then held against generated logs
# ---------------------------------------------------------------------------------------------------------------------------
def _uleb(b, at):
    v = shift = 0
    while True:
        x = b[at]
        at += 1
        v |= (x & 0x7F) << shift
        shift += 7
        if not x & 0x80:
            return v, at


def change_hash_and_deps(change):
    """(hash, deps) of a binary change: columnar.js:659-739; a DEFLATEd one (chunk type 2) is hashed in its plain form (:780-790)."""
    _, at = _uleb(change, 9)
    if change[8] == 2:
        body = zlib.decompressobj(-15).decompress(change[at:])
        head, v = bytearray([1]), len(body)
        while True:
            head.append((v & 0x7F) | (0x80 if v >> 7 else 0))
            v >>= 7
            if not v:
                break
        change = change[:8] + bytes(head) + body
        _, at = _uleb(change, 9)
    assert change[8] == 1, "a change chunk"
    n, at = _uleb(change, at)
    return hashlib.sha256(change[8:]).digest(), [bytes(change[at + 32 * k:at + 32 * k + 32]) for k in range(n)]


class PyGraph:
    def __init__(self, applied_changes):
        """applied_changes: the applied changes in application order (bytes)."""
        self.order, self.deps, self.dependents = [], {}, {}
        for c in applied_changes:
            h, deps = change_hash_and_deps(c)
            self.order.append(h)
            self.deps[h] = deps
            self.dependents[h] = []
            for d in deps:
                self.dependents[d].append(h)
        self.heads = sorted(h for h in self.order if not self.dependents[h])
        self.branch = None

    def get_changes(self, have):
        if not have:
            return list(self.order)
        stack, seen, out = [], set(), []
        for h in have:
            seen.add(h)
            if h not in self.dependents:
                raise KeyError(h)
            stack.extend(self.dependents[h])
        while stack:
            h = stack.pop()
            seen.add(h)
            out.append(h)
            if not all(d in seen for d in self.deps[h]):
                break
            stack.extend(self.dependents[h])
        if not stack and all(h in seen for h in self.heads):
            self.branch = 1
            return out
        self.branch = 2
        stack, seen = list(have), set()
        while stack:
            h = stack.pop()
            if h not in seen:
                stack.extend(self.deps[h])
                seen.add(h)
        return [h for h in self.order if h not in seen]

    def changes_added(self, other):
        other = set(other)
        stack, seen, out = list(self.heads), set(), []
        while stack:
            h = stack.pop()
            if h not in seen and h not in other:
                seen.add(h)
                out.append(h)
                stack.extend(self.deps[h])
        return out[::-1]


def test_restatement_on_the_fixture():
    branches = set()
    for h in HISTORIES:
        by_hash = {x: c for x, c in zip(h["hashes"], _changes(h))}
        g = PyGraph([by_hash[x] for x in h["applied"]])
        assert [x.hex() for x in g.order] == h["applied"] and [x.hex() for x in g.heads] == h["heads"]
        for q in h["get_changes"]:
            have = [bytes.fromhex(x) for x in q["have"]]
            if "error" in q:
                with pytest.raises(KeyError) as ei:
                    g.get_changes(have)
                assert "hash not found: " + ei.value.args[0].hex() == q["error"]
            else:
                assert [x.hex() for x in g.get_changes(have)] == q["result"], (h["name"], q["have"])
                if have:
                    branches.add(g.branch)
        for p in h["changes_added"]:
            if p["second"]:
                g2 = PyGraph(_applied_in_order([_changes(h)[i] for i in p["second"]]))
                assert [x.hex() for x in g2.changes_added(bytes.fromhex(h["hashes"][i]) for i in p["first"])] == p["result"], (h["name"], p["name"])
    assert branches == {1, 2}, "the fixture must reach both branches of getChanges"


def _applied_in_order(changes):
    """The changes the reference applies, in its order, for a delivery in one call (new.js:1550-1597: passes over the queue, every
    change whose dependencies are applied goes in; duplicates are dropped)."""
    applied, order, queue = set(), [], list(changes)
    while True:
        rest, progress = [], False
        for c in queue:
            h, deps = change_hash_and_deps(c)
            if h in applied:
                continue
            if all(d in applied for d in deps):
                applied.add(h)
                order.append(c)
                progress = True
            else:
                rest.append(c)
        queue = rest
        if not progress or not queue:
            return order


def _generated(kind):
    if kind.startswith("actors64"):
        log = loggen.generate(loggen.KIND_TEXT_CONCURRENT, n_actors=64, n_rounds=8, ins_per_change=3, del_per_change=1, n_objects=1, seed=0x5EED0064)
    else:
        log = loggen.generate(loggen.KIND_TEXT_TYPING, n_ops=3000, ops_per_change=1, seed=0x5EED0001)
    changes = log.changes()
    if kind.endswith("shuffled"):
        # shuffled, and one late change left out: what depends on it stays queued
        rng = np.random.default_rng(7)
        keep = [c for k, c in enumerate(changes) if k != len(changes) - 70]
        changes = [keep[int(i)] for i in rng.permutation(len(keep))]
    return changes


GENERATED = ["actors64", "typing3000", "actors64_shuffled", "typing3000_shuffled"]
_generated_cache = {}


def check_generated(make_engine, kind, probe_min):
    if kind not in _generated_cache:
        changes = _generated(kind)
        _generated_cache[kind] = (changes, PyGraph(_applied_in_order(changes)))
    changes, g = _generated_cache[kind]
    eng = make_engine()
    try:
        eng.set_graph_probe_min(probe_min)
        eng.load_changes(ChangeLog.from_changes(changes))
        eng.replay()
        order = [bytes.fromhex(x) for x in hex_list(eng, eng.applied())]
        assert order == g.order, "application order"
        if kind.endswith("shuffled"):
            assert len(eng.pending()) > 0
        n = len(order)
        assert 400 <= n <= 3001
        rng = np.random.default_rng(11)
        haves = [[order[0]], [order[-1]], g.heads, [order[n // 2]], [order[n // 3], order[2 * n // 3]], [order[n - 5], order[5]]]
        haves += [[order[int(i)] for i in rng.integers(0, n, size=3)] for _ in range(4)]
        branches = set()
        for have in haves:
            want = g.get_changes(have)
            branches.add(g.branch)
            assert [bytes.fromhex(x) for x in hex_list(eng, eng.changes_since(have))] == want
        assert branches == ({1, 2} if kind.startswith("actors64") else {1}), "both branches of getChanges where the log has concurrent changes"
        others = [order[: n // 2], order[1::2], order[: n - 1], [order[-1]], [], order, [order[int(i)] for i in rng.permutation(n)[: n // 3]]]
        for other in others:
            assert [bytes.fromhex(x) for x in hex_list(eng, eng.changes_added(other))] == g.changes_added(other)
        pending = set(bytes.fromhex(x) for x in hex_list(eng, eng.pending()))
        known = [int(i) != NONE32 for i in eng.find_changes(eng.hashes())]
        assert known == [bytes(x) in g.deps and bytes(x) not in pending for x in eng.hashes()]
    finally:
        eng.close()


@pytest.mark.parametrize("probe_min", [DEVICE, HOST], ids=["device", "host"])
@pytest.mark.parametrize("kind", GENERATED)
def test_generated_logs(emu_lib, kind, probe_min):
    check_generated(_emulated(emu_lib), kind, probe_min)


@pytest.mark.gpu
@pytest.mark.parametrize("probe_min", [DEVICE, HOST], ids=["device", "host"])
@pytest.mark.parametrize("kind", GENERATED)
def test_generated_logs_gpu(kind, probe_min):
    check_generated(_gpu, kind, probe_min)


# ---------------------------------------------------------------------------------------------------------------------------
# (d) the device table by itself
# ---------------------------------------------------------------------------------------------------------------------------
GOLDEN = 0x9E3779B97F4A7C15
WG = 256   # threads of one workgroup of the kernels


def slots_of(n_table):
    s = 64
    while s < 2 * n_table + 64:
        s *= 2
    return s


def slot_of(h, n_table):
    """The slot rule stated in include/am355.h (am355_test_hash_probe)."""
    return (((int.from_bytes(h[:8], "little") * GOLDEN) & (2 ** 64 - 1)) >> 32) & (slots_of(n_table) - 1)


def keys_at(slot, count, n_table, salt=0):
    """`count` distinct 32-byte keys that start at `slot` in a table made for n_table hashes."""
    out, k = [], salt << 32
    while len(out) < count:
        cand = np.arange(k, k + 65536, dtype=np.uint64)
        with np.errstate(over="ignore"):
            s = ((cand * np.uint64(GOLDEN)) >> np.uint64(32)) & np.uint64(slots_of(n_table) - 1)
        for v in cand[s == slot]:
            h = int(v).to_bytes(8, "little") + bytes([len(out) & 255, salt & 255]) + b"\x5a" * 22
            assert slot_of(h, n_table) == slot
            out.append(h)
            if len(out) == count:
                break
        k += 65536
    return out


def expected(table, queries):
    first = {}
    for i, h in enumerate(table):
        first.setdefault(bytes(h), i)
    return [first.get(bytes(q), NONE32) for q in queries]


def check_hash_probe(make_engine):
    eng = make_engine()
    try:
        rng = np.random.default_rng(3)
        before = eng.graph_query_calls()
        # table sizes x query counts at the wavefront, the workgroup and beyond
        for n_table in (1, 63, 64, 65, WG - 1, WG, WG + 1, 5000):
            table = rng.integers(0, 256, size=(n_table, 32), dtype=np.uint8)
            for n_q in (0, 1, 64, 65, WG - 1, WG, WG + 1, 4097):
                present = table[rng.integers(0, n_table, size=n_q)]
                absent = rng.integers(0, 256, size=(n_q, 32), dtype=np.uint8)
                queries = np.where((np.arange(n_q) % 3 == 0)[:, None], absent, present) if n_q else np.zeros((0, 32), np.uint8)
                got = eng.prim_hash_probe(table, queries)
                assert got.tolist() == expected(table, queries), (n_table, n_q)
        # keys equal in the bytes the slot is computed from -- and in every byte but the last
        base = bytes(range(31))
        table = [base + bytes([k]) for k in range(40)]
        queries = table[::-1] + [base + bytes([200])]
        assert eng.prim_hash_probe(table, queries).tolist() == list(range(39, -1, -1)) + [NONE32]
        # a cluster that wraps behind the last slot: six keys that all start at the last slot but one of a 128-slot table
        n_table = 10
        last = slots_of(n_table) - 1
        cluster = keys_at(last - 1, 6, n_table)
        others = keys_at(40, 4, n_table, salt=1)
        table = cluster + others
        assert [slot_of(h, n_table) for h in cluster] == [last - 1] * 6
        # absent keys that land inside the full cluster: at its start, at the last slot, behind the wrap
        inside = keys_at(last - 1, 8, n_table, salt=2)[6:] + keys_at(last, 2, n_table, salt=3) + keys_at(0, 2, n_table, salt=4) + keys_at(3, 1, n_table, salt=5)
        queries = cluster + inside + others + cluster[::-1]
        assert eng.prim_hash_probe(table, queries).tolist() == list(range(6)) + [NONE32] * 7 + [6, 7, 8, 9] + list(range(5, -1, -1))
        # a key that starts at the last slot and one at slot 0 behind a cluster that ends there
        table = keys_at(last, 2, n_table) + keys_at(0, 1, n_table, salt=1)
        assert eng.prim_hash_probe(table, table + keys_at(1, 1, n_table, salt=2)).tolist() == [0, 1, 2, NONE32]
        # repeated queries; a table that holds a hash twice answers with the smaller index
        one = rng.integers(0, 256, size=(1, 32), dtype=np.uint8)
        table = np.concatenate([rng.integers(0, 256, size=(70, 32), dtype=np.uint8), one, rng.integers(0, 256, size=(70, 32), dtype=np.uint8), one])
        assert eng.prim_hash_probe(table, np.repeat(one, 300, axis=0)).tolist() == [70] * 300
        # an empty table
        assert eng.prim_hash_probe(np.zeros((0, 32), np.uint8), rng.integers(0, 256, size=(65, 32), dtype=np.uint8)).tolist() == [NONE32] * 65
        assert eng.prim_hash_probe(np.zeros((0, 32), np.uint8), np.zeros((0, 32), np.uint8)).tolist() == []
        assert eng.graph_query_calls() == before   # (the test entry is not a query)
    finally:
        eng.close()


def test_hash_probe(emu_lib):
    check_hash_probe(_emulated(emu_lib))


@pytest.mark.gpu
def test_hash_probe_gpu():
    check_hash_probe(_gpu)


BALLOT_COUNTS = [63, 64, 65, 129]


def check_ballot_words(make_engine, n):
    changes = loggen.generate(loggen.KIND_TEXT_TYPING, n_ops=n - 1, ops_per_change=1, seed=0x5EED0001).changes()   # (and the change that makes the Text)
    assert len(changes) == n
    g = PyGraph(changes)
    answers = []
    for probe_min in (DEVICE, HOST):
        eng = make_engine()
        try:
            eng.set_graph_probe_min(probe_min)
            eng.load_changes(ChangeLog.from_changes(changes))
            eng.replay()
            got = []
            # the other state lacks: the last change | the last two | everything from the last full word on | one change in the middle too
            others = (g.order[: n - 1], g.order[: n - 2], g.order[: (n - 1) // 64 * 64], g.order[: n // 2] + g.order[n // 2 + 1: n - 1], g.order[::-1], [])
            for other in others:
                r = [bytes.fromhex(x) for x in hex_list(eng, eng.changes_added(other))]
                assert r == g.changes_added(other), (n, probe_min, len(other))
                got.append(r)
            asked = sum(1 for other in others if other)   # (an empty other needs no membership test: counted nowhere)
            assert eng.graph_query_calls() == ((asked, 0) if probe_min == DEVICE else (0, asked))
            answers.append(got)
        finally:
            eng.close()
    assert answers[0] == answers[1]


@pytest.mark.parametrize("n", BALLOT_COUNTS)
def test_changes_added_ballot_words(emu_lib, n):
    check_ballot_words(_emulated(emu_lib), n)


@pytest.mark.gpu
@pytest.mark.parametrize("n", BALLOT_COUNTS)
def test_changes_added_ballot_words_gpu(n):
    check_ballot_words(_gpu, n)


# ---------------------------------------------------------------------------------------------------------------------------
# (e) refusals
# ---------------------------------------------------------------------------------------------------------------------------
def _all_queries(eng, h32):
    return [lambda: eng.find_changes([h32]), lambda: eng.changes_since([h32]), lambda: eng.changes_since([]), lambda: eng.changes_added([h32]),
            lambda: eng.missing_deps([h32])]


def check_refusals(make_engine):
    h = BY_NAME["diamonds"]
    some = bytes.fromhex(h["hashes"][3])
    # a context without a state
    eng = make_engine()
    try:
        for q in _all_queries(eng, some):
            with pytest.raises(engine.EngineError) as ei:
                q()
            assert ei.value.code == engine.AM355_E_STATE
    finally:
        eng.close()
    # a document context
    eng = make_engine()
    try:
        eng.load_changes(ChangeLog.from_changes(_changes(h)))
        eng.replay()
        doc = bytes(eng.save())
        eng.load_document(doc)
        eng.replay()
        whole = eng.patch_json()
        for q in _all_queries(eng, some):
            with pytest.raises(engine.EngineError) as ei:
                q()
            assert ei.value.code == engine.AM355_E_STATE
        assert eng.patch_json() == whole and bytes(eng.save()) == doc
        assert eng.graph_query_calls() == (0, 0)
    finally:
        eng.close()
    # a sharded context
    eng = make_engine()
    try:
        eng.set_shard(0, 2)
        eng.load_changes(ChangeLog.from_changes(_changes(h)))
        eng.replay()
        stats = eng.stats().as_dict()
        for q in _all_queries(eng, some):
            with pytest.raises(engine.UnsupportedChanges) as ei:
                q()
            assert ei.value.code == engine.AM355_E_UNSUPPORTED
        assert eng.stats().as_dict() == stats and eng.graph_query_calls() == (0, 0)
    finally:
        eng.close()
    # an unknown hash among `have`: the reference's text, for the first unknown one; the state as it was
    h = BY_NAME["linear"]
    some = bytes.fromhex(h["hashes"][3])
    for probe_min in (DEVICE, HOST):
        eng = make_engine()
        try:
            eng.set_graph_probe_min(probe_min)
            eng.apply_changes(ChangeLog.from_changes(_changes(h)[:10]))
            whole, counters = eng.patch_json(), eng.resident_counters()
            other = "0f" * 32
            with pytest.raises(engine.InvalidChanges) as ei:
                eng.changes_since([some, UNKNOWN, other])
            assert ei.value.code == engine.AM355_E_INVALID and _error_text(ei.value) == "hash not found: " + UNKNOWN
            with pytest.raises(engine.InvalidChanges) as ei:
                eng.changes_since([other, some, UNKNOWN])
            assert _error_text(ei.value) == "hash not found: " + other
            assert eng.patch_json() == whole and eng.resident_counters() == counters
            # and the next call is served as it would have been
            before = eng.resident_counters()
            eng.apply_changes(ChangeLog.from_changes(_changes(h)[10:11]))
            assert eng.resident_counters()[0] == before[0] + 1
            assert hex_list(eng, eng.changes_since([h["hashes"][9]])) == [h["hashes"][10]]
        finally:
            eng.close()


def test_refusals(emu_lib):
    check_refusals(_emulated(emu_lib))


@pytest.mark.gpu
def test_refusals_gpu():
    check_refusals(_gpu)


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
    for probe_min in (DEVICE, HOST):
        eng = _emulated(emu_lib)()
        try:
            eng.set_graph_probe_min(probe_min)
            h = BY_NAME["withheld"]
            for batch in _batches(h):
                eng.apply_changes(ChangeLog.from_changes(batch))
                engine_answers(eng, h)
                eng.changes_added(eng.hashes()[:5])
            eng.prim_hash_probe(eng.hashes(), eng.hashes())
            with pytest.raises(engine.InvalidChanges):
                eng.changes_since([UNKNOWN])
            busy = live()
            assert busy[0] > start[0] and busy[1] > start[1], busy
        finally:
            eng.close()
        assert live() == start, probe_min


# ---------------------------------------------------------------------------------------------------------------------------
# the default of set_graph_probe_min: 65,536 probes (profiles/hash_graph_timings.txt), at the threshold itself
# ---------------------------------------------------------------------------------------------------------------------------
DEFAULT_PROBE_MIN = 65536


def test_default_probe_min_leaves_small_documents_to_the_host_index(emu_lib):
    eng = _emulated(emu_lib)()
    try:
        eng.apply_changes(ChangeLog.from_changes(_changes(BY_NAME["linear"])))
        hs = eng.hashes()
        assert hex_list(eng, eng.changes_added(hs[:-1])) == [BY_NAME["linear"]["hashes"][-1]]
        assert [int(i) for i in eng.find_changes(hs)] == list(range(len(hs)))
        assert eng.graph_query_calls() == (0, 2)
    finally:
        eng.close()


@pytest.mark.gpu
def test_default_probe_min_at_the_threshold_gpu():
    changes = loggen.generate(loggen.KIND_TEXT_TYPING, n_ops=DEFAULT_PROBE_MIN - 1, ops_per_change=1, seed=0x5EED0001).changes()
    assert len(changes) == DEFAULT_PROBE_MIN
    eng = _gpu()
    try:
        eng.apply_changes(ChangeLog.from_changes(changes[:-1]))      # one change below the threshold: the host index
        hs = eng.hashes()
        last = bytes(hs[-1]).hex()
        assert hex_list(eng, eng.changes_added(hs[:-1])) == [last]
        assert eng.graph_query_calls() == (0, 1)
        eng.apply_changes(ChangeLog.from_changes(changes[-1:]))      # at it: the device, with the same answers
        hs = eng.hashes()
        assert len(hs) == DEFAULT_PROBE_MIN
        assert hex_list(eng, eng.changes_added(hs[:-2])) == [last, bytes(hs[-1]).hex()]
        assert eng.graph_query_calls() == (1, 1)
        found = eng.find_changes(hs)                                 # 65,536 probes: the device table over the context's hashes
        assert eng.graph_query_calls() == (2, 1) and (found == np.arange(DEFAULT_PROBE_MIN, dtype=np.uint32)).all()
        assert [int(i) for i in eng.find_changes(hs[:100])] == list(range(100)) and eng.graph_query_calls() == (2, 2)
        assert eng.resident_counters()[0] == 1
    finally:
        eng.close()
