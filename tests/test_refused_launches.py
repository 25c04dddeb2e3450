"""A kernel launch the HIP runtime refuses -- an empty grid, a block of more than 1024 threads: "invalid configuration argument" -- runs
nothing and returns nothing. The error waits in the calling thread until somebody asks hipGetLastError: before csrc/am355_ctx.h
`guarded` asked at the end of every API call, that was some LATER call of some other context, which then failed for no reason of its
own (found by running tests/test_resident_limits.py behind tests/test_ref_suite_vectors.py in one process: loading a document without
ops launched kb_token_ends over 0 bytes, and the first applyChanges of the next test reported it).

The emulation of tests/emu refuses the same launches and counts them (am355_emu_refused_launches): none may happen on a tour of the
API over ordinary and degenerate inputs. On the GPU the same tour must succeed call by call -- a call that leaves an error behind now
fails itself -- and leave the next context alone."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle_lib
from automerge_classic_amd import engine, loggen
from automerge_classic_amd.loggen import ChangeLog
from test_resource_accounting import EMU_DIR, EMU_LIB, work


def degenerate_tour(make_engine):
    """Inputs at which some array of the engine is empty: no changes at all, the document saved from that, a change without ops, a
    single makeText, an empty batch onto a kept state, an empty Bloom filter."""
    eng = make_engine()
    try:
        eng.load_changes(ChangeLog.from_changes([]))
        eng.replay()
        empty_patch = eng.patch_json()
        doc = bytes(eng.save())
        eng.load_document(doc)            # a document without ops: its op columns have no bytes
        eng.replay()
        assert eng.patch_json() == empty_patch == oracle_lib.OracleDoc.load_document(doc).patch_json()
        eng.backend_load(doc)
        assert eng.patch_json() == empty_patch
        typing = loggen.generate(loggen.KIND_TEXT_TYPING, n_ops=3, ops_per_change=1, seed=3)
        ch = typing.changes()
        eng.load_changes(ChangeLog.from_changes(ch[:1]))   # one makeText: a list object without elements
        eng.replay()
        assert eng.patch_json() == oracle_lib.OracleDoc(ChangeLog.from_changes(ch[:1])).patch_json()
        doc = bytes(eng.save())
        eng.load_document(doc)
        eng.replay()
        eng.patch_json()
        eng.reset()
        session = oracle_lib.OracleSession()
        try:
            for batch in ([], ch[:1], [], ch[1:2], ch[2:], []):   # (empty batches onto no state and onto a kept one)
                want = session.apply(batch)
                eng.apply_changes(ChangeLog.from_changes(batch))
                assert eng.apply_patch_json() is not None and want
            assert eng.patch_json() == session.patch_json()
        finally:
            session.close()
        none = np.zeros(0, dtype=np.uint32)
        assert len(eng.bloom_build(none)) == 0
        assert not eng.bloom_probe(np.arange(len(ch), dtype=np.uint32), 0, 0, 0, np.zeros(0, np.uint8)).any()
    finally:
        eng.close()


def test_no_launch_is_refused_emulated():
    subprocess.check_call(["make", "-s", "-C", EMU_DIR])
    lib = engine.load_library(EMU_LIB)
    lib.am355_emu_refused_launches.argtypes = [ctypes.POINTER(ctypes.c_char_p)]
    lib.am355_emu_refused_launches.restype = ctypes.c_long

    def refused():
        name = ctypes.c_char_p()
        return int(lib.am355_emu_refused_launches(ctypes.byref(name))), (name.value or b"").decode()
    start, _ = refused()
    degenerate_tour(lambda: engine.Engine(0, EMU_LIB))
    n, kernel = refused()
    assert n == start, f"{n - start} launches refused on the degenerate inputs, the last one of {kernel}"
    eng = engine.Engine(0, EMU_LIB)
    try:
        work(eng, reject_last=True)
    finally:
        eng.close()
    n, kernel = refused()
    assert n == start, f"{n - start} launches refused on the tour of the API, the last one of {kernel}"


@pytest.mark.gpu
def test_no_call_leaves_an_error_to_the_next_one_gpu():
    degenerate_tour(lambda: engine.Engine(0))
    # the next context's first calls read the thread's last error (flush_uploads, the delta stage): nothing was left for them
    log = loggen.generate(loggen.KIND_TEXT_CONCURRENT, n_actors=3, n_rounds=2, ins_per_change=5, del_per_change=1, n_objects=1, seed=4)
    eng = engine.Engine(0)
    try:
        ch = log.changes()
        eng.apply_changes(ChangeLog.from_changes(ch[:4]))
        eng.apply_changes(ChangeLog.from_changes(ch[4:]))
        assert eng.patch_json() == oracle_lib.OracleDoc(log).patch_json()
        work(eng, reject_last=True)
    finally:
        eng.close()
