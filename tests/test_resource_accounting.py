"""A context gives back every HIP resource it made (csrc/am355_ctx.h: the buffers, streams and events of am355_ctx release themselves
in their destructors; am355_destroy quiesces and deletes). The HIP-runtime emulation of tests/emu counts live device allocations,
pinned allocations, streams and events (am355_emu_live): after create -> work -> close() all four are back where they started,
exactly -- whatever the context did in between, a call that was rejected included. The same host code runs on the GPU."""
import ctypes
import gc
import os
import subprocess

import numpy as np
import pytest

from automerge_classic_amd import engine, loggen
from automerge_classic_amd.loggen import ChangeLog

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
EMU_LIB = os.path.join(EMU_DIR, "libam355_emu.so")
KINDS = ("device allocations", "pinned allocations", "streams", "events")


@pytest.fixture(scope="module")
def live():
    subprocess.check_call(["make", "-s", "-C", EMU_DIR])
    lib = engine.load_library(EMU_LIB)
    lib.am355_emu_live.argtypes = [ctypes.POINTER(ctypes.c_long)]
    lib.am355_emu_live.restype = None

    def read():
        out = (ctypes.c_long * 4)()
        lib.am355_emu_live(out)
        return dict(zip(KINDS, (int(x) for x in out)))
    return read


def _changes_of(log):
    arena, offs = bytes(log.arena), [int(x) for x in log.offsets]
    return [arena[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]


def work(eng, reject_last):
    """Every group of buffers of the context comes into being: whole-document replay on both scheduler paths, save, document load,
    history, dependency graph, Bloom filters, the primitives' test entries, and a run of single-change applyChanges calls that the
    resident path serves and merges in place. reject_last: the last call is one the engine rejects."""
    text = loggen.generate(loggen.KIND_TEXT_TYPING, n_ops=400, ops_per_change=10, seed=63)
    eng.load_changes(text)
    eng.replay()
    patch = eng.patch_json()
    assert eng.stats().fast_path == 1
    doc = eng.save()
    eng.load_document(doc)
    eng.replay()
    assert eng.patch_json() == patch
    eng.backend_load(doc)
    assert eng.patch_json() == patch
    _, offsets, hashes = eng.doc_changes()
    assert len(offsets) - 1 == text.n_changes == len(hashes)
    # sync protocol: dependency graph, Bloom filter built and probed
    eng.load_changes(text)
    eng.replay()
    first, _ = eng.dep_graph()
    assert len(first) == text.n_changes + 1
    idx = np.arange(0, text.n_changes, 3, dtype=np.uint32)
    bits = eng.bloom_build(idx)
    assert eng.bloom_probe(idx, len(idx), 10, 7, bits).all()
    # device primitives by themselves (buffers local to the call)
    vals = np.random.default_rng(1).integers(0, 5, 2049, dtype=np.uint32)
    out, total = eng.test_scan(vals)
    assert total == int(vals.sum()) and out[-1] == total - int(vals[-1])
    keys = np.random.default_rng(2).integers(0, 1 << 20, 2049, dtype=np.uint64)
    k, _ = eng.test_sort(keys, np.arange(2049, dtype=np.uint32), 20)
    assert np.array_equal(k, np.sort(keys))
    # general path: the same kind of changes in a random delivery order
    conc = loggen.generate(loggen.KIND_TEXT_CONCURRENT, seed=21, n_actors=6, n_rounds=4, ins_per_change=7, del_per_change=2, n_objects=2)
    eng.load_changes(conc.reordered(np.random.default_rng(5).permutation(conc.n_changes)))
    eng.replay()
    assert eng.stats().fast_path == 2
    eng.patch_json()
    # Backend.applyChanges change by change onto the state the context keeps
    eng.reset()
    ch = _changes_of(text)
    eng.apply_changes(ChangeLog.from_changes(ch[:3]))
    for c in ch[3:21]:
        eng.apply_changes(ChangeLog.from_changes([c]))
        eng.apply_patch_json()
    served, _, in_place = eng.resident_counters()
    assert served > 0 and in_place > 0, (served, in_place)   # (otherwise the stored list order and its scratch never exist)
    if reject_last:
        bad = bytearray(ch[21])
        bad[30] ^= 0x1   # (tests/test_engine_emu.py test_invalid_and_unsupported_inputs_are_reported: the checksum no longer matches)
        with pytest.raises(engine.InvalidChanges) as ei:
            eng.apply_changes(ChangeLog.from_changes([bytes(bad)]))
        assert "BAD_CHECKSUM" in ei.value.flag_names


def test_destroyed_contexts_leave_no_hip_resource_behind(live):
    gc.collect()   # (an Engine some earlier test dropped without close() must not be finalised in the middle of the count)
    start = live()
    for cycle in ("work", "work", "work, last call rejected", "work", "create and destroy only"):
        eng = engine.Engine(0, EMU_LIB)
        try:
            during = live()
            assert during["streams"] == start["streams"] + 4 and during["events"] > start["events"], (cycle, during)   # (the counters see this context)
            if cycle != "create and destroy only":
                work(eng, reject_last="rejected" in cycle)
                busy = live()
                assert busy["device allocations"] > start["device allocations"] and busy["pinned allocations"] > start["pinned allocations"], (cycle, busy)
        finally:
            eng.close()
        assert live() == start, cycle
