"""The device primitives of csrc/am355_prims.hip and the workgroup / carried scans of csrc/am355_scan.h, each driven by itself through the
am355_test_* hooks (am355_api.hip) at the sizes, alignments and values where its kernels change path: the launch counts of the scans,
their 16-byte and narrow loads, sums that wrap at 2^32, the fused / unfused radix sort and its buffer parity, the doubling rounds of
chain_mark inside a tile, the head / body / tail words of the range kernels. Last, the check pass of the calls on a Text
(csrc/am355_textrec.h rec_premises) on hand-made record tables, which the engine itself never builds broken.

Everything is integer work, so every comparison is exact, against NumPy or a plain Python loop over the same input -- never against a
second call of the engine. Buffers go to the device whole and come back whole with 0xA5A5A5A5 (or live values, where a stray write
of a live value would show better) around every range: the comparison is over the whole buffer.

Each body takes a function that makes an engine context: the CPU suite runs it on the emulation of tests/emu (a wavefront's lanes one
after the other: the logic), the GPU suite on the device (barriers, ballots, LDS, atomics across workgroups)."""
import os
import subprocess

import numpy as np
import pytest

from automerge_classic_amd import engine
from test_apply_engine import EMU_DIR, EMU_LIB

SENT = 0xA5A5A5A5
NONE32 = 0xFFFFFFFF
SCAN_TILE = 2048          # am355_prims.hip SCAN_TILE
SCAN_THREE = 2_097_152    # SCAN_TILE * 1024: the last size of the two-launch scan
SORT_TILE = 2048          # am355_prims.h SORT_TILE_ELEMS
CH_TILE = 4096            # am355_prims.hip CH_TILE
LAUNCH_RANGES = 8         # am355_prims.h


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-s", "-C", EMU_DIR])
    return EMU_LIB


def _emulated(lib):
    return lambda: engine.Engine(0, lib)


def _gpu():
    return engine.Engine(0)


class _lookback:
    """AM355_SCAN_LOOKBACK for the calls inside (exclusive_scan_u32 reads it per call)."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        if self.on:
            os.environ["AM355_SCAN_LOOKBACK"] = "1"

    def __exit__(self, *a):
        os.environ.pop("AM355_SCAN_LOOKBACK", None)


def _sent(words):
    return np.full(words, SENT, dtype=np.uint32)


def _ex_scan(v):
    """Exclusive prefix sums modulo 2^32 (summed in uint64) and the total."""
    c = np.cumsum(v.astype(np.uint64))
    ex = np.concatenate((np.zeros(1, np.uint64), c[:-1])) if v.size else np.zeros(0, np.uint64)
    return (ex & 0xFFFFFFFF).astype(np.uint32), int(c[-1]) & 0xFFFFFFFF if v.size else 0


# ---------------------------------------------------------------------------------------------------------------------------
# exclusive_scan_u32
# ---------------------------------------------------------------------------------------------------------------------------
def _scan_patterns(n, rng):
    yield "zero", np.zeros(n, np.uint32)
    yield "one", np.ones(n, np.uint32)
    yield "ffffffff", np.full(n, 0xFFFFFFFF, np.uint32)
    # one 0x80000000 on the last element of a tile / on the first of the next (of the last tile boundary the array has; the ends of
    # an array shorter than a tile): every prefix behind it carries the bit, none before it
    b = (n - 1) // SCAN_TILE * SCAN_TILE if n > SCAN_TILE else 0
    for name, at in (("tile_last", b - 1 if b else n - 1), ("tile_first", b)):
        if n:
            v = np.zeros(n, np.uint32)
            v[at] = 0x80000000
            yield name, v
    yield "random", rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def _scan_once(eng, v, in_place, in_off, out_off, want_total, what):
    n = v.size
    ref, ref_total = _ex_scan(v)
    a = _sent(n + 8)
    a[in_off:in_off + n] = v
    if in_place:
        got_in, got_out, total = eng.prim_scan(a, in_off, n, total=SENT if want_total else None)
        want = a.copy()
        want[in_off:in_off + n] = ref
        assert got_out is None and np.array_equal(got_in, want), f"{what}: the buffer scanned in place"
    else:
        o = _sent(n + 8)
        got_in, got_out, total = eng.prim_scan(a, in_off, n, out_buf=o, out_off=out_off, total=SENT if want_total else None)
        want = o.copy()
        want[out_off:out_off + n] = ref
        assert np.array_equal(got_in, a), f"{what}: the input was written to"
        assert np.array_equal(got_out, want), f"{what}: the output buffer"
    assert total == (ref_total if want_total else None), f"{what}: total {total}, not {ref_total}"


def scan_values(make_engine, sizes, lookback=False):
    """Every value pattern at every size, alternately in place and into a second buffer."""
    eng = make_engine()
    rng = np.random.default_rng(0x5CA0)
    try:
        with _lookback(lookback):
            for n in sizes:
                for k, (name, v) in enumerate(_scan_patterns(n, rng)):
                    _scan_once(eng, v, k % 2 == 0, 0, 0, True, f"n={n} {name} lookback={lookback}")
    finally:
        eng.close()


def scan_cross(make_engine, n, lookback=False):
    """in == out and in != out, each pointer 0..3 words off a 16-byte boundary, the total asked for or not."""
    eng = make_engine()
    v = np.random.default_rng(n).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    try:
        with _lookback(lookback):
            for want_total in (True, False):
                for in_off in range(4):
                    _scan_once(eng, v, True, in_off, in_off, want_total, f"n={n} in place +{in_off} total={want_total}")
                    for out_off in range(4):
                        _scan_once(eng, v, False, in_off, out_off, want_total, f"n={n} in +{in_off} out +{out_off} total={want_total}")
    finally:
        eng.close()


SCAN_SMALL = (0, 1, 7, 8, 9, 255, 256, 257, 2047, 2048, 2049, 8191, 8192, 8193, 8200)
SCAN_LARGE = (SCAN_THREE - 1, SCAN_THREE, SCAN_THREE + 1, SCAN_THREE + 8)
SCAN_CROSS = (2049, 8193, 8200, SCAN_THREE + 8)


def test_scan_values_small_emulated(emu_lib):
    scan_values(_emulated(emu_lib), SCAN_SMALL)


@pytest.mark.parametrize("n", SCAN_LARGE)
def test_scan_values_large_emulated(emu_lib, n):
    scan_values(_emulated(emu_lib), (n,))


@pytest.mark.parametrize("n", SCAN_LARGE[2:])
def test_scan_values_lookback_emulated(emu_lib, n):
    scan_values(_emulated(emu_lib), (n,), lookback=True)


@pytest.mark.parametrize("n", SCAN_CROSS[:3])
def test_scan_cross_emulated(emu_lib, n):
    scan_cross(_emulated(emu_lib), n)


@pytest.mark.parametrize("lookback", [False, True])
@pytest.mark.parametrize("want_total", [True, False])
@pytest.mark.parametrize("in_off", range(4))
def test_scan_cross_three_launches_emulated(emu_lib, lookback, want_total, in_off):
    # (the cross of scan_cross at 2,097,160, one slice per case: an emulated scan of two million words takes about a second)
    n = SCAN_CROSS[3]
    eng = _emulated(emu_lib)()
    v = np.random.default_rng(n).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    try:
        with _lookback(lookback):
            _scan_once(eng, v, True, in_off, in_off, want_total, f"n={n} in place +{in_off}")
            for out_off in range(4):
                _scan_once(eng, v, False, in_off, out_off, want_total, f"n={n} in +{in_off} out +{out_off}")
    finally:
        eng.close()


@pytest.mark.gpu
def test_scan_values_gpu():
    scan_values(_gpu, SCAN_SMALL + SCAN_LARGE)
    scan_values(_gpu, SCAN_LARGE[2:], lookback=True)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SCAN_CROSS)
def test_scan_cross_gpu(n):
    scan_cross(_gpu, n)
    if n > SCAN_THREE:
        scan_cross(_gpu, n, lookback=True)


# ---------------------------------------------------------------------------------------------------------------------------
# exclusive_scan2_u32
# ---------------------------------------------------------------------------------------------------------------------------
def scan2_cases(make_engine, sizes):
    eng = make_engine()
    rng = np.random.default_rng(0x5CA2)
    try:
        for n in sizes:
            va = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)   # wraps within a few elements
            vb = rng.integers(0, 9, n, dtype=np.uint64).astype(np.uint32)          # never wraps
            (ra, ta), (rb, tb) = _ex_scan(va), _ex_scan(vb)
            for k, (in_place, off, out_off, want_a, want_b) in enumerate([(True, 0, 0, True, True), (False, 0, 0, True, False), (True, 1, 1, False, True),
                                                                          (False, 2, 3, False, False), (False, 3, 0, True, True)]):
                a, b = _sent(n + 8), _sent(n + 8)
                a[off:off + n] = va
                b[off:off + n] = vb
                if k % 2:   # (which of the two wraps)
                    a, b, ra_, ta_, rb_, tb_ = b, a, rb, tb, ra, ta
                else:
                    ra_, ta_, rb_, tb_ = ra, ta, rb, tb
                what = f"n={n} in_place={in_place} +{off}/+{out_off} totals={want_a},{want_b}"
                oa, ob = (None, None) if in_place else (_sent(n + 8), _sent(n + 8))
                ga, gb, goa, gob, tot_a, tot_b = eng.prim_scan2(a, b, off, n, oa, ob, out_off, SENT if want_a else None, SENT if want_b else None)
                if in_place:
                    wa, wb = a.copy(), b.copy()
                    wa[off:off + n] = ra_
                    wb[off:off + n] = rb_
                    assert np.array_equal(ga, wa) and np.array_equal(gb, wb), what
                else:
                    wa, wb = oa.copy(), ob.copy()
                    wa[out_off:out_off + n] = ra_
                    wb[out_off:out_off + n] = rb_
                    assert np.array_equal(ga, a) and np.array_equal(gb, b), f"{what}: an input was written to"
                    assert np.array_equal(goa, wa) and np.array_equal(gob, wb), what
                assert tot_a == (ta_ if want_a else None) and tot_b == (tb_ if want_b else None), f"{what}: totals {tot_a}, {tot_b}"
    finally:
        eng.close()


SCAN2_SIZES = (0, 1, 2048, 2049, SCAN_THREE, SCAN_THREE + 1)


def test_scan2_small_emulated(emu_lib):
    scan2_cases(_emulated(emu_lib), SCAN2_SIZES[:4])


@pytest.mark.parametrize("n", SCAN2_SIZES[4:])
def test_scan2_large_emulated(emu_lib, n):
    scan2_cases(_emulated(emu_lib), (n,))


@pytest.mark.gpu
def test_scan2_gpu():
    scan2_cases(_gpu, SCAN2_SIZES)


# ---------------------------------------------------------------------------------------------------------------------------
# exclusive_scan_terminators
# ---------------------------------------------------------------------------------------------------------------------------
def _term_once(eng, data, byte_off, out_off, want_total, what):
    L = data.size
    buf = np.full(L + 16, 0x00, dtype=np.uint8)   # (bytes around the string ARE terminators: counted, if the kernel reads past an end)
    buf[byte_off:byte_off + L] = data
    out = _sent(L + 1 + 8)
    got, total = eng.prim_scan_terminators(buf, byte_off, L, out, out_off, SENT if want_total else None)
    flags = (data < 0x80).astype(np.uint64)
    c = np.concatenate((np.zeros(1, np.uint64), np.cumsum(flags))).astype(np.uint32)   # L + 1 entries, the last is the total
    want = out.copy()
    want[out_off:out_off + L + 1] = c
    assert np.array_equal(got, want), what
    assert total == (int(c[-1]) if want_total else None), f"{what}: total {total}"


def _term_patterns(L, rng):
    yield "80", np.full(L, 0x80, np.uint8)
    yield "7f", np.full(L, 0x7F, np.uint8)
    alt = np.full(L, 0x80, np.uint8)
    alt[1::2] = 0x7F
    yield "alternating", alt
    yield "random", rng.integers(0, 256, L, dtype=np.uint64).astype(np.uint8)


def terminator_cases(make_engine, sizes, offsets):
    eng = make_engine()
    rng = np.random.default_rng(0x7E63)
    try:
        for L in sizes:
            for k, (name, data) in enumerate(_term_patterns(L, rng)):
                _term_once(eng, data, 0, 0, k != 1, f"L={L} {name}")
        if offsets:
            data = rng.integers(0, 256, 2048, dtype=np.uint64).astype(np.uint8)
            for byte_off in range(8):
                for out_off in range(4):
                    _term_once(eng, data, byte_off, out_off, True, f"L=2048 bytes +{byte_off} out +{out_off}")
    finally:
        eng.close()


TERM_SMALL = (0, 1, 7, 8, 9, 2046, 2047, 2048)
TERM_LARGE = (SCAN_THREE - 1, SCAN_THREE)


def test_terminators_small_emulated(emu_lib):
    terminator_cases(_emulated(emu_lib), TERM_SMALL, True)


@pytest.mark.parametrize("L", TERM_LARGE)
def test_terminators_large_emulated(emu_lib, L):
    terminator_cases(_emulated(emu_lib), (L,), False)


@pytest.mark.gpu
def test_terminators_gpu():
    terminator_cases(_gpu, TERM_SMALL + TERM_LARGE, True)


# ---------------------------------------------------------------------------------------------------------------------------
# max_u32
# ---------------------------------------------------------------------------------------------------------------------------
def max_cases(make_engine):
    eng = make_engine()
    rng = np.random.default_rng(0x3A)
    try:
        for n in (0, 1, 256, 257, 524_288, 524_289):   # (524,288 = 2048 workgroups x 256: one more takes the grid-stride loop's second lap)
            zero = np.zeros(n, np.uint32)
            assert eng.prim_max(zero, 0) == 0 and eng.prim_max(zero, 5) == 5, f"n={n}: all zero"
            if not n:
                assert eng.prim_max(zero, SENT) == SENT
                continue
            v = rng.integers(0, 1 << 20, n, dtype=np.uint64).astype(np.uint32)
            last = v.copy()
            last[-1] = 1 << 21
            assert eng.prim_max(last, 0) == 1 << 21, f"n={n}: the maximum on the last element"
            top = v.copy()
            top[int(rng.integers(0, n))] = 0xFFFFFFFF
            assert eng.prim_max(top, 7) == 0xFFFFFFFF, f"n={n}: 0xFFFFFFFF"
            assert eng.prim_max(v, 1 << 22) == 1 << 22, f"n={n}: a value above the data stays"
            assert eng.prim_max(v, 0) == int(v.max()) and eng.prim_max(v, int(v.max()) - 1) == int(v.max()), f"n={n}: a value below the data is replaced"
    finally:
        eng.close()


def test_max_emulated(emu_lib):
    max_cases(_emulated(emu_lib))


@pytest.mark.gpu
def test_max_gpu():
    max_cases(_gpu)


# ---------------------------------------------------------------------------------------------------------------------------
# radix_sort_pairs
# ---------------------------------------------------------------------------------------------------------------------------
SORT_BITS = ((0, 0), (0, 8), (0, 16), (0, 24), (0, 64), (8, 24), (16, 17), (37, 64))
SORT_SIZES = (0, 1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 131_072, 131_073)


def _passes(begin, end):
    return (end - begin + 7) // 8 if end > begin else 0


def _sort_keys(kind, n, begin, end, rng):
    """Keys whose field [begin, end) is `kind`; the bits below begin and above the last digit are random in every key (the sort must
    not look at them), the bits between end and the top of the last digit zero (the contract of am355_prims.h). Returns (keys, field)."""
    width = end - begin
    top = begin + 8 * _passes(begin, end)
    span = 1 << width
    if kind == "equal":
        f = np.full(n, 0x5A5A5A5A5A5A5A5A % span, dtype=np.uint64)
    elif kind == "three":
        f = (rng.integers(0, 3, n, dtype=np.uint64) * np.uint64((span - 1) // 2)).astype(np.uint64)
    else:
        f = rng.integers(0, span, n, dtype=np.uint64, endpoint=False) if width < 64 else rng.integers(0, 1 << 64, n, dtype=np.uint64, endpoint=False)
        if kind == "sorted":
            f = np.sort(f)
        elif kind == "reverse":
            f = np.sort(f)[::-1].copy()
    junk = rng.integers(0, 1 << 64, n, dtype=np.uint64, endpoint=False) if n else np.zeros(0, np.uint64)
    low = junk & np.uint64((1 << begin) - 1)
    high = (junk >> np.uint64(top) << np.uint64(top)) if top < 64 else np.zeros(n, np.uint64)
    keys = low | (f << np.uint64(begin)) | high if width else low | high
    return keys.astype(np.uint64), f


def _sort_once(eng, keys, field, vals, begin, end, what, first_table=None):
    order = np.argsort(field, kind="stable")
    k, v, res = eng.prim_sort(keys, vals, begin, end, first_table)
    assert res == (_passes(begin, end) & 1 if keys.size else 0), f"{what}: the sort named buffer {res}"
    assert np.array_equal(k, keys[order]), f"{what}: keys"
    assert np.array_equal(v, vals[order]), f"{what}: values (equal keys must keep their input order)"


SORT_KINDS = ("equal", "three", "sorted", "reverse", "random")


def sort_cases(make_engine, sizes, emulated, kinds=SORT_KINDS):
    eng = make_engine()
    rng = np.random.default_rng(0x50A7)
    try:
        for n in sizes:
            for begin, end in SORT_BITS:
                if emulated and (begin, end) == (0, 64) and n > 2049:
                    continue
                for kind in kinds:
                    keys, field = _sort_keys(kind, n, begin, end, rng)
                    for vals in (np.arange(n, dtype=np.uint32), rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)):
                        _sort_once(eng, keys, field, vals, begin, end, f"n={n} bits [{begin}, {end}) {kind}")
    finally:
        eng.close()


def _first_table(keys, begin):
    """Histogram of the first digit as a caller's own kernel leaves it in sort_first_table(ws): [digit x tiles + tile]."""
    tiles = (keys.size + SORT_TILE - 1) // SORT_TILE
    d = ((keys >> np.uint64(begin)) & np.uint64(0xFF)).astype(np.int64)
    table = np.zeros((256, tiles), dtype=np.uint32)
    for t in range(tiles):
        table[:, t] = np.bincount(d[t * SORT_TILE:(t + 1) * SORT_TILE], minlength=256)
    return table


def sort_first_hist_cases(make_engine):
    """first_hist_done: the histogram the caller computed gives the same result; one with the rows of two digits exchanged a different
    one -- the sort really skipped its own histogram launch. (The exchanged rows are of two rare digits below a crowd of larger
    ones: every position the scatter computes from the wrong table stays below n, which is asserted before the call.)"""
    eng = make_engine()
    rng = np.random.default_rng(0xF157)
    try:
        for n in (2049, 131_072):
            for begin, end in ((0, 16), (8, 24)):
                first = rng.integers(10, 256, n, dtype=np.uint64)
                for t in range(0, n, SORT_TILE):   # digit 5: three per tile, digit 9: seven per tile (one and two in a last tile of one element)
                    m = min(SORT_TILE, n - t)
                    first[t:t + min(3, m)] = 5
                    first[t + m - min(7, m - min(3, m)):t + m] = 9
                field = first | (rng.integers(0, 256, n, dtype=np.uint64) << np.uint64(8))
                keys = (field << np.uint64(begin)) | (rng.integers(0, 1 << 64, n, dtype=np.uint64, endpoint=False) & np.uint64((1 << begin) - 1))
                vals = np.arange(n, dtype=np.uint32)
                table = _first_table(keys, begin)
                what = f"n={n} bits [{begin}, {end}) first_hist_done"
                _sort_once(eng, keys, field, vals, begin, end, what, first_table=table)
                wrong = table.copy()
                wrong[[5, 9]] = wrong[[9, 5]]
                assert not np.array_equal(wrong, table)
                # no other digit below 10 occurs, so from `wrong` the scatter puts a pair with digit 5 or 9 below (all pairs of both digits) +
                # (a tile's own count of one of them), and every other pair where it belongs: all below n when the crowd above is that large
                assert int(table[:10].sum()) == int(table[[5, 9]].sum()) and int(table[10:].sum()) >= int(table[[5, 9]].max())
                k, v, _ = eng.prim_sort(keys, vals, begin, end, wrong)
                order = np.argsort(field, kind="stable")
                assert not (np.array_equal(k, keys[order]) and np.array_equal(v, vals[order])), f"{what}: a wrong table changed nothing -- the histogram was computed anyway"
        with pytest.raises(engine.EngineError) as e:   # more than 64 tiles: the unfused sort scans the table in a launch of its own
            eng.prim_sort(np.zeros(131_073, np.uint64), np.zeros(131_073, np.uint32), 0, 8, np.zeros((256, 65), np.uint32))
        assert e.value.code == engine.AM355_E_ARG
    finally:
        eng.close()


def test_sort_small_emulated(emu_lib):
    sort_cases(_emulated(emu_lib), SORT_SIZES[:11], True)


@pytest.mark.parametrize("kind", SORT_KINDS)
@pytest.mark.parametrize("n", SORT_SIZES[11:])
def test_sort_fused_switch_emulated(emu_lib, n, kind):
    # (64 tiles and one more, a key set per case: an emulated pass over 131 k pairs takes a quarter of a second)
    sort_cases(_emulated(emu_lib), (n,), True, (kind,))


def test_sort_first_hist_emulated(emu_lib):
    sort_first_hist_cases(_emulated(emu_lib))


@pytest.mark.gpu
def test_sort_gpu():
    sort_cases(_gpu, SORT_SIZES, False)


@pytest.mark.gpu
def test_sort_first_hist_gpu():
    sort_first_hist_cases(_gpu)


# ---------------------------------------------------------------------------------------------------------------------------
# chain_mark
# ---------------------------------------------------------------------------------------------------------------------------
def _chain_ref(nxt, mark, n):
    """A walk from every nonzero entry. Returns the positions some walk reaches (the starts themselves not included)."""
    nx = nxt.tolist()
    reached = [False] * n
    for s in np.nonzero(mark[:n])[0].tolist():
        i = s
        while True:
            c = nx[i]
            if c >= n or c <= i:   # NONE32, past the end, itself, backwards: the chain ends
                break
            i = c
            if reached[i]:
                break
            reached[i] = True
    return np.array(reached, dtype=bool)


def _chain_once(eng, nxt, mark, n, what):
    m = _sent(n + 8)
    m[:n] = mark
    got = eng.prim_chain_mark(nxt, m, n)
    reached = _chain_ref(nxt, mark, n)
    assert np.array_equal(got[n:], m[n:]), f"{what}: words behind the marks"
    had = mark != 0
    assert np.array_equal(got[:n][had], mark[had]), f"{what}: a mark that was nonzero changed its value"
    bad = np.nonzero((got[:n][~had] != 0) != reached[~had])[0]
    assert bad.size == 0, f"{what}: {bad.size} positions wrong, the first {np.nonzero(~had)[0][bad[:5]].tolist()} (reached: {reached[~had][bad[:5]].tolist()})"


def _chain_cases(n, rng):
    """(name, next, mark) for n positions."""
    idx = np.arange(n, dtype=np.uint64)
    last_tile = (n - 1) // CH_TILE * CH_TILE

    def step(k):
        return np.minimum(idx + k, NONE32).astype(np.uint32)

    def marks(*at, value=1):
        m = np.zeros(n, np.uint32)
        for a in at:
            if 0 <= a < n:
                m[a] = value
        return m

    one = step(1)   # single steps: the worst case of the doubling inside a tile (2^12 positions, twelve rounds), and every tile is entered
    yield "i+1 from 0", one, marks(0)
    yield "i+1 no start", one, marks()
    yield "i+1 start in the last tile", one, marks(last_tile + (n - last_tile) // 2)
    yield "i+1 starts on both sides of a tile boundary", one, marks(CH_TILE - 1, CH_TILE) if n > CH_TILE else marks(0, n - 1)
    # a node marked 7 that the chain from 0 passes: it keeps 7 (and everything behind it is reached from 0 anyway)
    m = marks(0)
    m[n // 2] = 7
    yield "i+1 a 7 on the chain", one, m
    # a node marked 7 that no chain reaches: it keeps 7 -- and being nonzero it IS a start by definition, so its own chain is marked
    broken = one.copy()
    broken[n // 3] = NONE32
    m = marks(0)
    m[min(n - 1, n // 3 + 1)] = 7 if n > 2 else m[min(n - 1, n // 3 + 1)]
    yield "i+1 cut, a 7 behind the cut", broken, m
    for k in (CH_TILE, CH_TILE + 1, 5000):   # one node per tile: the exit lands on a tile's first / second position; tiles skipped
        yield f"i+{k} from 0 and 3", step(k), marks(0, 3)
        yield f"i+{k} no start", step(k), marks()
    # random forward gaps, chains merge; some entries end their chain: NONE32, >= n, == i, < i
    gap = rng.geometric(0.02, n).astype(np.uint64)
    nxt = np.minimum(idx + gap, NONE32).astype(np.uint32)
    for j, bad in enumerate(rng.integers(0, n, max(1, n // 50)).tolist()):
        nxt[bad] = (NONE32, n, bad, bad // 2, n + 7)[j % 5]
    starts = rng.integers(0, n, 6).tolist() + [CH_TILE - 1, CH_TILE, last_tile]
    yield "geometric gaps, several starts", nxt, marks(*starts)
    m = marks(*starts[:3])
    for a in rng.integers(0, n, 4).tolist():
        m[a] = 7
    yield "geometric gaps, marks of 7", nxt, m
    yield "geometric gaps, a start only in the last tile", nxt, marks(last_tile)
    yield "geometric gaps, no start", nxt, marks()


def chain_cases(make_engine, sizes):
    eng = make_engine()
    rng = np.random.default_rng(0xC4A1)
    try:
        for n in sizes:
            for name, nxt, mark in _chain_cases(n, rng):
                _chain_once(eng, nxt, mark, n, f"n={n} {name}")
    finally:
        eng.close()


CHAIN_SIZES = (1, 2, 4095, 4096, 4097, 8192, 12_293, 266_241)


def test_chain_mark_small_emulated(emu_lib):
    chain_cases(_emulated(emu_lib), CHAIN_SIZES[:7])


def test_chain_mark_65_tiles_emulated(emu_lib):
    chain_cases(_emulated(emu_lib), CHAIN_SIZES[7:])


@pytest.mark.gpu
def test_chain_mark_gpu():
    chain_cases(_gpu, CHAIN_SIZES)


# ---------------------------------------------------------------------------------------------------------------------------
# k_remap_ranks
# ---------------------------------------------------------------------------------------------------------------------------
def _remap_table(n_old, rng):
    """A random monotone injection of the old ranks into n_old + (a few) new ones."""
    return np.sort(rng.choice(n_old + 1 + n_old // 3 + 5, n_old, replace=False)).astype(np.uint32)


def _rank_words(words, n_old, rng):
    """Words that are mostly ranks (a stray rewrite outside a range would change them), with the edges n_old - 1, n_old, n_old + 1, NONE32."""
    w = rng.integers(0, n_old + 2, words, dtype=np.uint64).astype(np.uint32)
    edge = np.array([n_old - 1, n_old, n_old + 1, NONE32], dtype=np.uint32)
    at = rng.integers(0, words, max(4, words // 16))
    w[at] = edge[np.arange(at.size) % 4]
    return w


def _remap_ref(buf, base_off, ranges, table):
    out = buf.copy()
    for first, count, stride, guard, skip in ranges:
        at = base_off + first + np.arange(count, dtype=np.int64) * stride
        if stride > 1 and guard:
            at = at[buf[at + guard] != skip]
        x = buf[at]
        isrank = x < table.size
        out[at[isrank]] = table[x[isrank]]
    return out


def remap_dense_cases(make_engine, n_olds, counts):
    eng = make_engine()
    rng = np.random.default_rng(0x4E3A)
    try:
        for n_old in n_olds:
            table = _remap_table(n_old, rng)
            for count in counts:
                for base_off in range(4):
                    buf = _rank_words(8 + count + 12, n_old, rng)
                    if count:
                        buf[base_off + 8 + np.array([0, count - 1])] = n_old - 1   # (the first and the last word of the range do move)
                    ranges = [(8, count, 1, 0, 0)]
                    got, added = eng.prim_remap(buf, base_off, ranges, table)
                    assert added == (1 if count else 0)
                    want = _remap_ref(buf, base_off, ranges, table)
                    bad = np.nonzero(got != want)[0]
                    assert bad.size == 0, f"n_old={n_old} count={count} +{base_off}: words {bad[:8].tolist()} (the range starts at {8 + base_off})"
    finally:
        eng.close()


def remap_strided_cases(make_engine, n_olds):
    eng = make_engine()
    rng = np.random.default_rng(0x4E3B)
    try:
        for n_old in n_olds:
            table = _remap_table(n_old, rng)
            skip = 0x51C9
            for base_off in range(4):
                # eight ranges in one launch, each in a stretch of its own: dense ones of several lengths, records of 2 and 3 words with the guard
                # word behind / in front of the rank, and without one
                ranges, first = [], 8
                for count, stride, guard in ((5, 1, 0), (300, 2, 1), (1025, 1, 0), (300, 2, -1), (257, 3, 1), (77, 3, -1), (64, 3, 0), (1, 1, 0)):
                    ranges.append((first + (1 if guard < 0 else 0), count, stride, guard, skip))
                    first += count * stride + 9
                buf = _rank_words(first + 8, n_old, rng)
                for f, count, stride, guard, _ in ranges:   # every third record's guard word says "no rank here"; its rank word is a rank
                    if guard:
                        at = base_off + f + np.arange(0, count, 3) * stride
                        buf[at + guard] = skip
                        buf[at] = n_old - 1
                got, added = eng.prim_remap(buf, base_off, ranges, table)
                assert added == 8
                want = _remap_ref(buf, base_off, ranges, table)
                bad = np.nonzero(got != want)[0]
                assert bad.size == 0, f"n_old={n_old} +{base_off}: words {bad[:8].tolist()}"
            # RemapRanges::add(): the ninth range is refused, a range of no ranks is accepted and adds nothing, a stride of zero is refused
            buf = _rank_words(64, n_old, rng)
            with pytest.raises(engine.EngineError) as e:
                eng.prim_remap(buf, 0, [(4 * k, 2, 1, 0, 0) for k in range(9)], table)
            assert e.value.code == engine.AM355_E_ARG
            got, added = eng.prim_remap(buf, 0, [(0, 0, 1, 0, 0), (4, 0, 2, 1, 0)], table)
            assert added == 0 and np.array_equal(got, buf)
            with pytest.raises(engine.EngineError) as e:
                eng.prim_remap(buf, 0, [(0, 2, 0, 0, 0)], table)
            assert e.value.code == engine.AM355_E_ARG
    finally:
        eng.close()


REMAP_N_OLD = (1, 2, 4096, 4097)   # (4096 ranks: the table's last size in LDS)
REMAP_COUNTS = tuple(range(10)) + (1023, 1024, 1025)
REMAP_TWO_LAPS = 2_097_157         # 2048 workgroups x 1024 ranks, and five


def test_remap_dense_emulated(emu_lib):
    remap_dense_cases(_emulated(emu_lib), REMAP_N_OLD, REMAP_COUNTS)


@pytest.mark.parametrize("n_old", REMAP_N_OLD[2:])
def test_remap_second_lap_emulated(emu_lib, n_old):
    remap_dense_cases(_emulated(emu_lib), (n_old,), (REMAP_TWO_LAPS,))


def test_remap_strided_emulated(emu_lib):
    remap_strided_cases(_emulated(emu_lib), REMAP_N_OLD)


@pytest.mark.gpu
def test_remap_gpu():
    remap_dense_cases(_gpu, REMAP_N_OLD, REMAP_COUNTS)
    remap_dense_cases(_gpu, REMAP_N_OLD[2:], (REMAP_TWO_LAPS,))
    remap_strided_cases(_gpu, REMAP_N_OLD)


# ---------------------------------------------------------------------------------------------------------------------------
# k_fill_ranges
# ---------------------------------------------------------------------------------------------------------------------------
def _fill_ref(buf, base_off, ranges):
    out = buf.copy()
    for first, nbytes, value in ranges:   # in the order given: a later range wins
        out[base_off + first:base_off + first + (nbytes + 3) // 4] = value
    return out


def fill_cases(make_engine):
    eng = make_engine()
    try:
        def check(ranges, base_off, words, what, n_ranges=None):
            buf = _sent(words)
            got, added = eng.prim_fill(buf, base_off, ranges)
            assert added == (len(ranges) if n_ranges is None else n_ranges), what
            want = _fill_ref(buf, base_off, ranges)
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, f"{what}: words {bad[:8].tolist()}"

        for base_off in range(4):
            for length in (0, 1, 63, 64, 65, 66, 67, 68, 1000):
                check([(8, 4 * length, 0x11110000 + length)], base_off, 8 + length + 12, f"{length} words +{base_off}")
            # two ranges of at most 64 words that overlap, in both orders: the later one wins
            a, b = (8, 4 * 64, 0xAAAA0001), (40, 4 * 64, 0xBBBB0002)
            check([a, b], base_off, 128, f"overlap a, b +{base_off}")
            check([b, a], base_off, 128, f"overlap b, a +{base_off}")
            # FillRanges::add() rounds a byte length UP to whole words
            for nbytes, words in ((1, 1), (5, 2), (7, 2), (4 * 64 + 1, 65), (4 * 100 + 3, 101)):
                buf = _sent(8 + words + 12)
                got, _ = eng.prim_fill(buf, base_off, [(8, nbytes, 7)])
                assert int((got == 7).sum()) == words and np.array_equal(got, _fill_ref(buf, base_off, [(8, nbytes, 7)])), f"{nbytes} bytes +{base_off}"
            # eight ranges in one launch, small and long, each in a stretch of its own; the ninth is refused
            ranges, first = [], 8
            for k, length in enumerate((3, 65, 64, 1000, 1, 129, 0, 2051)):
                ranges.append((first, 4 * length, 0xC0DE0000 + k))
                first += length + 5
            check(ranges, base_off, first + 8, f"eight ranges +{base_off}")
            with pytest.raises(engine.EngineError) as e:
                eng.prim_fill(_sent(first + 8), base_off, ranges + [(0, 4, 1)])
            assert e.value.code == engine.AM355_E_ARG
    finally:
        eng.close()


def test_fill_emulated(emu_lib):
    fill_cases(_emulated(emu_lib))


@pytest.mark.gpu
def test_fill_gpu():
    fill_cases(_gpu)


# ---------------------------------------------------------------------------------------------------------------------------
# k_copy_ranges
# ---------------------------------------------------------------------------------------------------------------------------
COPY_LENGTHS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 4099)
COPY_SLOT = 4160   # a multiple of 16 that holds the longest range at any offset with bytes to spare on both sides


def copy_cases(make_engine):
    eng = make_engine()
    rng = np.random.default_rng(0xC0B1)
    try:
        def check(ranges, what, src_pinned):
            n = max(max(d + b, s + b) for d, s, b in ranges) + 64
            src = rng.integers(0, 256, n, dtype=np.uint64).astype(np.uint8)
            dst = np.full(n, 0xA5, dtype=np.uint8)
            got, added = eng.prim_copy(dst, src, ranges, src_pinned)
            assert added == len(ranges)
            want = dst.copy()
            for d, s, b in ranges:
                want[d:d + b] = src[s:s + b]
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, f"{what}: bytes {bad[:8].tolist()}"

        for src_pinned in (True, False):
            for dst_off in range(16):
                for src_shift in (0, 5):   # the source at the same offset mod 16 (16-byte words between head and tail), and at another (bytes)
                    for group in (COPY_LENGTHS[:8], COPY_LENGTHS[8:]):   # (up to eight ranges a launch, each in a slot of its own)
                        ranges = [(32 + k * COPY_SLOT + dst_off, 32 + k * COPY_SLOT + (dst_off + src_shift) % 16, b) for k, b in enumerate(group)]
                        check(ranges, f"dst +{dst_off} src +{(dst_off + src_shift) % 16} pinned={src_pinned} lengths {group}", src_pinned)
            # the bytes up to the first 16-byte boundary are more than the range has
            check([(32 + 13, 64 + 13, 2)], f"head longer than the range, pinned={src_pinned}", src_pinned)
            with pytest.raises(engine.EngineError) as e:   # CopyRanges::add(): the ninth range is refused
                eng.prim_copy(np.zeros(256, np.uint8), np.zeros(256, np.uint8), [(16 * k, 16 * k, 4) for k in range(9)], src_pinned)
            assert e.value.code == engine.AM355_E_ARG
    finally:
        eng.close()


def test_copy_emulated(emu_lib):
    copy_cases(_emulated(emu_lib))


@pytest.mark.gpu
def test_copy_gpu():
    copy_cases(_gpu)


# ---------------------------------------------------------------------------------------------------------------------------
# k_signal_words
# ---------------------------------------------------------------------------------------------------------------------------
def signal_cases(make_engine):
    eng = make_engine()
    try:
        for k, (n_a, n_b) in enumerate(((0, 0), (1, 0), (0, 1), (3, 5))):
            a = np.arange(n_a, dtype=np.uint32) + 0x1000
            b = np.arange(n_b, dtype=np.uint32) + 0x2000
            host = _sent(n_a + n_b + 4)
            got, seq = eng.prim_signal_words(a, b, 0x77 + k, host, SENT)
            want = host.copy()
            want[:n_a] = a
            want[n_a:n_a + n_b] = b
            assert np.array_equal(got, want) and seq == 0x77 + k, f"({n_a}, {n_b})"
    finally:
        eng.close()


def test_signal_words_emulated(emu_lib):
    signal_cases(_emulated(emu_lib))


@pytest.mark.gpu
def test_signal_words_gpu():
    signal_cases(_gpu)


# ---------------------------------------------------------------------------------------------------------------------------
# am355_scan.h: block_exclusive_scan_u32, carry_publish / carry_prefix
# ---------------------------------------------------------------------------------------------------------------------------
def carried_cases(make_engine, sizes):
    eng = make_engine()
    rng = np.random.default_rng(0xCA22)
    try:
        for n in sizes:
            # 0/1 flags as the replay kernels produce them, with words that wrap the sums here and there
            v = rng.integers(0, 2, n, dtype=np.uint64).astype(np.uint32)
            big = rng.integers(0, n, max(1, n // 97))
            v[big] = rng.integers(1 << 30, 1 << 32, big.size, dtype=np.uint64).astype(np.uint32)
            out, out_wg, wg_total = eng.prim_carried_scan(v)
            ref, _ = _ex_scan(v)
            pad = np.zeros((n + 255) // 256 * 256, np.uint64)
            pad[:n] = v
            rows = pad.reshape(-1, 256)
            inc = np.cumsum(rows, axis=1)
            ref_wg = ((inc - rows) & 0xFFFFFFFF).astype(np.uint32).reshape(-1)[:n]
            assert np.array_equal(wg_total, (inc[:, -1] & 0xFFFFFFFF).astype(np.uint32)), f"n={n}: workgroup sums"
            assert np.array_equal(out_wg, ref_wg), f"n={n}: block_exclusive_scan_u32"
            bad = np.nonzero(out != ref)[0]
            assert bad.size == 0, f"n={n}: carry_prefix wrong from element {bad[0]} (workgroup {bad[0] // 256}, group {bad[0] // 16384})"
    finally:
        eng.close()


CARRIED_SIZES = (1, 255, 256, 257, 16_384, 16_385, 1_048_577, 4_194_561)   # 65 groups of 64 workgroups; 257 groups: more than the 256 threads that sum them


def test_carried_scan_small_emulated(emu_lib):
    carried_cases(_emulated(emu_lib), CARRIED_SIZES[:6])


@pytest.mark.parametrize("n", CARRIED_SIZES[6:])
def test_carried_scan_groups_emulated(emu_lib, n):
    carried_cases(_emulated(emu_lib), (n,))


@pytest.mark.gpu
def test_carried_scan_gpu():
    carried_cases(_gpu, CARRIED_SIZES)


# ---------------------------------------------------------------------------------------------------------------------------
# am355_textrec.h rec_premises: the check pass of the calls on a Text (am355_locate.hip kl_check), on hand-made record tables
# ---------------------------------------------------------------------------------------------------------------------------
RF_TABLE, RF_REMOVE = 1, 2
LENGTH_BEFORE = 0xDEADBEEF   # what the length word holds before the pass: a pass that leaves no length leaves this


def _premises_ref(t, begin, R, n_values):
    """The rule, restated: (flag word, length word) for the records [begin, begin + R) of table t."""
    flags, length = 0, LENGTH_BEFORE
    for k in range(R):
        rec, nxt = t[begin + k], t[begin + k + 1]
        index, first, nfirst = int(rec["index"]), int(rec["first"]), int(nxt["first"])
        err, count = 0, 0
        if rec["flags"] & engine.EDIT_REMOVE:
            err |= RF_REMOVE
        if nfirst <= first or nfirst > n_values:          # `first` words in order and inside the table
            err |= RF_TABLE
        else:
            count = nfirst - first
        if k == 0 and index != 0:                         # record 0 has index 0
            err |= RF_TABLE
        if rec["flags"] & engine.EDIT_UPDATE and count > 1:   # an update record holds one value
            err |= RF_TABLE
        if count and index + count > 0xFFFFFFFF:
            err |= RF_TABLE
        if not err:
            if k + 1 < R:
                opens = int(nxt["index"]) == index + count
                replaces = bool(nxt["flags"] & engine.EDIT_UPDATE) and int(nxt["index"]) == index + count - 1
                if not opens and not replaces:
                    err |= RF_TABLE
            else:
                length = index + count                    # the last record leaves the length
        flags |= err
    return flags, length


def _premises_table(R, begin, behind):
    """A well-formed object of R records at `begin`: an insert record of 3 values, the update that replaces its last value, a record that
    opens the next index, and so on; `begin` foreign records in front and `behind` foreign records plus the sentinel at the end. The foreign
    records would each break the rule if the pass took them for the object's (a `remove` bit, an index out of line)."""
    t = np.zeros(begin + R + behind + 1, dtype=engine.IR_EDIT_DTYPE)
    for name in ("id_ctr", "id_actor", "elem_ctr", "elem_actor", "val_tl", "val_off", "pad"):
        t[name] = SENT
    first = 0
    for k in range(begin):
        t[k]["flags"], t[k]["index"], t[k]["first"] = engine.EDIT_REMOVE, 77, first
        first += 2
    index = 0
    for k in range(R):
        rec = t[begin + k]
        if k % 3 == 0:
            rec["flags"], rec["index"], count = 0, index, 3
            index += 3
        elif k % 3 == 1:
            rec["flags"], rec["index"], count = engine.EDIT_UPDATE, index - 1, 1
        else:
            rec["flags"], rec["index"], count = 0, index, 1 + k % 2
            index += count
        rec["first"] = first
        first += count
    for k in range(begin + R, len(t)):
        # (the record directly behind the object would pass for the update of its last value)
        t[k]["flags"], t[k]["index"], t[k]["first"] = engine.EDIT_UPDATE | engine.EDIT_REMOVE, index - 1, first
        first += 1 if k + 1 < len(t) else 0
    return t, first, index   # the table, n_values, the object's length


def _shift_index(t, begin, R, p, delta):
    for k in range(p, R):
        t[begin + k]["index"] = (int(t[begin + k]["index"]) + delta) & 0xFFFFFFFF


def _premises_defects():
    """name -> (flag word it must give, fn(t, begin, R, p, n_values) -> n_values or None where the defect has no place at record p)"""
    def index0(t, begin, R, p, nv):
        if p != 0:
            return None   # (only record 0 has a fixed index; at any other record this is the gap)
        t[begin]["index"] = 1
        return nv

    def first_order(t, begin, R, p, nv):
        t[begin + p + 1]["first"] = t[begin + p]["first"]
        return nv

    def first_past(t, begin, R, p, nv):
        return int(t[begin + p + 1]["first"]) - 1

    def update_two(t, begin, R, p, nv):
        # record p grows by one value (every `first` behind it and the indexes of the object behind it move along) and carries the bit
        t["first"][begin + p + 1:] += 1
        _shift_index(t, begin, R, p + 1, 1)
        t[begin + p]["flags"] |= engine.EDIT_UPDATE
        return nv + 1

    def gap(t, begin, R, p, nv):
        if p == 0:
            return None
        _shift_index(t, begin, R, p, 2)   # (2: an update record moved by 1 would open the next index)
        return nv

    def replaces_without_bit(t, begin, R, p, nv):
        if p == 0:
            return None
        prev = t[begin + p - 1]
        want = int(prev["index"]) + int(t[begin + p]["first"]) - int(prev["first"]) - 1
        _shift_index(t, begin, R, p, want - int(t[begin + p]["index"]))
        t[begin + p]["flags"] &= ~np.uint32(engine.EDIT_UPDATE)
        return nv

    def remove(t, begin, R, p, nv):
        t[begin + p]["flags"] |= engine.EDIT_REMOVE
        return nv

    def past_32_bits(t, begin, R, p, nv):
        # index + count == 2^32, which wraps to the index the record behind has. (In a table that passes every other check index + count
        # <= the values in front of the next record, so this defect never stands alone: here with index != 0 or a gap in front of it.)
        count = int(t[begin + p + 1]["first"]) - int(t[begin + p]["first"])
        _shift_index(t, begin, R, p, (1 << 32) - count - int(t[begin + p]["index"]))
        return nv

    return {"index0": (RF_TABLE, index0), "first_order": (RF_TABLE, first_order), "first_past": (RF_TABLE, first_past), "update_two": (RF_TABLE, update_two),
            "gap": (RF_TABLE, gap), "replaces_without_bit": (RF_TABLE, replaces_without_bit), "remove": (RF_REMOVE, remove), "past_32_bits": (RF_TABLE, past_32_bits)}


def premises_cases(make_engine):
    eng = make_engine()
    try:
        block = eng.text_locate_limits()[0]
        n_cases = 0
        # R = 1: only the last-record thread runs; R = block + 1: the last record alone in the second workgroup; begin > 0: foreign records on both sides
        for R, begin, behind in ((1, 0, 0), (2, 0, 0), (3, 0, 0), (3, 5, 4), (1, 5, 4), (block + 1, 0, 0), (block + 1, 3, 2)):
            good, n_values, length = _premises_table(R, begin, behind)
            what = f"R={R} begin={begin}"
            assert _premises_ref(good, begin, R, n_values) == (0, length), what
            assert eng.prim_text_premises(good, begin, R, n_values, LENGTH_BEFORE) == (0, length), what
            for p in sorted({0, R - 1, min(block - 1, R - 1)}):   # record 0, the last record, the last record of the first workgroup
                for name, (flags, put) in _premises_defects().items():
                    t = good.copy()
                    nv = put(t, begin, R, p, n_values)
                    if nv is None:
                        continue
                    want = _premises_ref(t, begin, R, nv)
                    assert want[0] == flags, f"{what}: {name} at record {p}: the restated rule gives flags {want[0]}"
                    assert eng.prim_text_premises(t, begin, R, nv, LENGTH_BEFORE) == want, f"{what}: {name} at record {p}"
                    n_cases += 1
        assert n_cases >= 7 * 8   # (every defect was placed)
    finally:
        eng.close()


def test_text_premises_emulated(emu_lib):
    premises_cases(_emulated(emu_lib))


@pytest.mark.gpu
def test_text_premises_gpu():
    premises_cases(_gpu)
