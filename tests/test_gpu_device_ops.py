"""The device building blocks every kernel shares, one at a time, against plain references (tests/device_ops_cases.py): the peak
lookup with its staged table and grid (csrc/device_common.hip.h: copy_peak_table, grid_build, match_rank_lds, look4 / look_rest,
match_rank_global), the per-lane arithmetic (fastdiv, charge_mz, nth_set_bit, deposit_sites, xcd_slot, nl_bump, lut_row, the rank
histogram), the wavefront helpers (wave_sum_u64, wave_min_f64 / wave_max_f64, marker_lane_f64, ion_wave_excl_scan_u64,
hist_wave_sum, ts_same_digit, ts_block_scan) and the two scans as they are launched (pya_launch_ions_scan, ts_scan) -- through
the test-only entry points of include/pyascore_debug.h (csrc/debug_ops.hip).  Everything is compared exactly: none of these
functions has a tolerance.  What the inputs are good for is proven on the CPU in tests/test_device_ops_host.py."""
import ctypes as C

import numpy as np
import pytest

import device_ops_cases as dc
from pyascore_amd import _lib

pytestmark = pytest.mark.gpu

F32 = np.float32
VP = C.c_void_p


@pytest.fixture(scope="module")
def gpu():
    from pyascore_amd import PyAscore
    return PyAscore(100.0, 10, "STY", 79.966331)


def _p(a):
    return a.ctypes.data_as(VP)


# ---------------------------------------------------------------------------------------------------------------------
# the lookup
# ---------------------------------------------------------------------------------------------------------------------
def _lookup(gpu, mz, rank, err, q, want_rc=0):
    mz, rank, q = np.ascontiguousarray(mz, F32), np.ascontiguousarray(rank, np.uint32), np.ascontiguousarray(q, F32)
    out = np.full((q.size, 4), 0xEE, np.uint8)
    cells = np.full(257, 0xEEEEEEEE, np.uint32)
    rc = gpu._lib.pya_debug_lookup(gpu._h, _p(mz), _p(rank), mz.size, float(err), _p(q), q.size, _p(out), _p(cells))
    assert rc == want_rc, gpu._lib.pya_last_error(gpu._h)
    return out, cells


def _first_bad(bad, q, got, want, what, name):
    i = int(np.flatnonzero(bad)[0])
    return "%s, %s: %d of %d queries differ, first query %d = %r (bits %#x): got %d, want %d" % (
        name, what, int(bad.sum()), q.size, i, float(q[i]), int(q[i:i + 1].view(np.uint32)[0]), int(got[i]), int(want[i]))


_cases = {}


def _group(group):
    """the cases of a group and the reference's answers, computed once and never changed"""
    if group not in _cases:
        rows = []
        for name, mz, rank, err, q, _ in dc.lookup_cases(group):
            want = dc.match_rank(mz, rank, q, err)
            for a in (mz, rank, q, want):
                a.setflags(write=False)
            rows.append((name, mz, rank, err, q, want))
        _cases[group] = rows
    return _cases[group]


@pytest.mark.parametrize("group", ("sizes", "families", "clusters"))
def test_lookup_equals_the_reference(gpu, group):
    """every table of the group at every error setting: the three device lookups give the reference's rank for every query
    (and so each other's), more() says whether the fourth entry from the grid's start is inside the window, and the grid is
    what device_ops_cases.check_grid asks of one"""
    for name, mz, rank, err, q, want in _group(group):
        out, cells = _lookup(gpu, mz, rank, err, q)
        dc.check_grid(mz, cells)
        assert not (out[:, 0] != want).any(), _first_bad(out[:, 0] != want, q, out[:, 0], want, "match_rank_lds", name)
        assert not (out[:, 2] != want).any(), _first_bad(out[:, 2] != want, q, out[:, 2], want, "match_rank_global", name)
        if F32(err) > F32(0.49):
            assert (out[:, 1] == 255).all() and (out[:, 3] == 255).all(), name
            continue
        assert not (out[:, 1] != want).any(), _first_bad(out[:, 1] != want, q, out[:, 1], want, "look4 + look_rest", name)
        # more(): the entry three behind the cell's start (a +inf entry behind the table) lies below hi
        with np.errstate(invalid="ignore", over="ignore"):
            lo, hi = (q - F32(err)).astype(F32), (q + F32(err)).astype(F32)
        start = cells[:256].astype(np.int64)[dc.grid_cell(mz, lo)] if mz.size else np.zeros(q.size, np.int64)
        fourth = np.r_[mz, np.full(4, np.inf, F32)][start + 3]
        with np.errstate(invalid="ignore"):
            more = (fourth < hi).astype(np.uint8)
        assert not (out[:, 3] != more).any(), _first_bad(out[:, 3] != more, q, out[:, 3], more, "more()", name)


def test_lookup_continues_past_the_fourth_entry(gpu):
    """the cluster queries reach look_rest and the continuation loops: more() is set for every query whose window holds five
    entries, and the rank found is the one behind the fourth (`place`: the window's first four entries have larger ranks), in
    most cases the 0 planted there"""
    hit = 0
    for name, mz, rank, err, q, want in _group("clusters"):
        if F32(err) > F32(0.49):
            continue
        count, place = dc.window_shape(mz, rank, q, err)
        out, _ = _lookup(gpu, mz, rank, err, q)
        deep = (count >= 5) & (place >= 4)
        assert (out[count >= 5, 3] == 1).all(), name
        assert (out[deep, 1] == want[deep]).all() and (out[deep, 0] == want[deep]).all() and (out[deep, 2] == want[deep]).all(), name
        hit += int((deep & (want == 0)).sum())
    assert hit >= 30


def test_lookup_refuses_what_production_could_not_build(gpu):
    mz, rank = dc.binned(8, np.random.default_rng(1))
    q = np.array([150.0], F32)
    bad = []
    for i, v in ((3, np.inf), (3, -np.inf), (3, np.nan), (7, np.inf), (0, 1e9)):       # not finite / not ascending
        m = mz.copy()
        m[i] = v
        bad.append((m, rank, 0.05))
    r = rank.copy()
    r[5] = 15
    bad.append((mz, r, 0.05))
    r = rank.copy()
    r[0] = 0xFFFFFFFF
    bad.append((mz, r, 0.05))
    bad += [(mz, rank, e) for e in (0.0, -0.5, 50.0, np.inf, np.nan)]
    big, big_rank = np.arange(8193, dtype=F32), np.zeros(8193, np.uint32)
    bad.append((big, big_rank, 0.05))
    for m, r, e in bad:
        out, cells = _lookup(gpu, m, r, e, q, want_rc=_lib.PYA_ERR_ARG)
        assert (out == 0xEE).all() and (cells == 0xEEEEEEEE).all()
    lib, h = gpu._lib, gpu._h
    out, cells = np.zeros(4, np.uint8), np.zeros(257, np.uint32)
    assert lib.pya_debug_lookup(h, None, _p(rank), 8, 0.05, _p(q), 1, _p(out), _p(cells)) == _lib.PYA_ERR_ARG
    assert lib.pya_debug_lookup(h, _p(mz), None, 8, 0.05, _p(q), 1, _p(out), _p(cells)) == _lib.PYA_ERR_ARG
    assert lib.pya_debug_lookup(h, _p(mz), _p(rank), 8, 0.05, None, 1, _p(out), _p(cells)) == _lib.PYA_ERR_ARG
    assert lib.pya_debug_lookup(h, _p(mz), _p(rank), 8, 0.05, _p(q), 1, None, _p(cells)) == _lib.PYA_ERR_ARG
    assert lib.pya_debug_lookup(h, _p(mz), _p(rank), 8, 0.05, _p(q), 1, _p(out), None) == _lib.PYA_ERR_ARG
    # ... and takes the largest table there is, and one without a query
    _lookup(gpu, big[:8192], big_rank[:8192], 0.05, q)
    _lookup(gpu, mz, rank, 0.05, np.zeros(0, F32))


# ---------------------------------------------------------------------------------------------------------------------
# one value per lane
# ---------------------------------------------------------------------------------------------------------------------
def _lane(gpu, op, a, b, want_rc=0):
    a, b = np.ascontiguousarray(a, np.uint64), np.ascontiguousarray(b, np.uint64)
    assert a.shape == b.shape
    out = np.full(a.size, 0xEEEEEEEEEEEEEEEE, np.uint64)
    rc = gpu._lib.pya_debug_lane_ops(gpu._h, op, _p(a), _p(b), a.size, _p(out))
    assert rc == want_rc, gpu._lib.pya_last_error(gpu._h)
    return out


FASTDIV_CHUNKS = 5


@pytest.mark.parametrize("chunk", range(FASTDIV_CHUNKS))
def test_fastdiv_is_the_division(gpu, chunk):
    """every divisor 2 .. 600 and the ones around 2^12, 2^16, 2^31 and 2^32; multiples, multiples - 1, every dividend up to
    70 000 and random ones up to 2^32 - 1 -- beyond e * d < 2^32 too, where the formula still holds (test_device_ops_host.py)"""
    e, d = dc.fastdiv_cases(dc.FASTDIV_D[chunk::FASTDIV_CHUNKS])
    got = _lane(gpu, _lib.PYA_DBG_FASTDIV, e, d)
    want = e // d
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%d of %d quotients differ, first %d / %d: got %d, want %d" % (bad.size, e.size, e[bad[0]], d[bad[0]], got[bad[0]],
                                                                                         want[bad[0]])


def test_fastdiv_by_one_and_by_zero(gpu):
    e = np.array([0, 1, 7, 2 ** 31, 2 ** 32 - 1], np.uint64)
    assert np.array_equal(_lane(gpu, _lib.PYA_DBG_FASTDIV, e, np.ones(5, np.uint64)), e)
    assert np.array_equal(_lane(gpu, _lib.PYA_DBG_FASTDIV, e, np.zeros(5, np.uint64)), e)      # (fastdiv_make: a divisor of 0 is 1)


def test_charge_mz_is_the_rounded_division(gpu):
    """every charge 1 .. 255: random masses, and for the charges that are no power of two the operands whose exact quotient
    lies on a float32 tie or within a float64 ulp of one -- where a wrong last bit of the float64 quotient shows"""
    m, z = dc.charge_cases()
    got = _lane(gpu, _lib.PYA_DBG_CHARGE_MZ, m.view(np.uint64), z)
    want = dc.charge_ref(m, z).view(np.uint32).astype(np.uint64)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%d of %d differ, first m = %r, z = %d: got bits %#x, want %#x" % (bad.size, m.size, m[bad[0]], z[bad[0]], got[bad[0]],
                                                                                           want[bad[0]])
    for zz in (0, 256, 2 ** 32):
        _lane(gpu, _lib.PYA_DBG_CHARGE_MZ, m[:1].view(np.uint64), np.array([zz], np.uint64), want_rc=_lib.PYA_ERR_ARG)


def test_nth_set_bit_and_deposit_sites(gpu):
    m, n = dc.nth_set_bit_cases()
    got = _lane(gpu, _lib.PYA_DBG_NTH_SET_BIT, m, n)
    want = np.array([dc.nth_set_bit_ref(int(a), int(b) if b < 2 ** 31 else int(b) - 2 ** 32) for a, b in zip(m, n)], np.uint64)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:5]
    bits, mask = dc.deposit_cases()
    got = _lane(gpu, _lib.PYA_DBG_DEPOSIT_SITES, bits, mask)
    want = np.array([dc.deposit_sites_ref(int(a), int(b)) for a, b in zip(bits, mask)], np.uint64)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:5]


def test_xcd_slot_is_a_permutation(gpu):
    """for every n in 1 .. 2049 and a few up to 1 000 003: the slots of the blocks 0 .. n - 1 are 0 .. n - 1, each once (a remap
    that is not a bijection skips PSMs), and the blocks of one XCD (b % 8) get one contiguous range in the order of b // 8"""
    b = np.concatenate([np.arange(n, dtype=np.uint64) for n in dc.XCD_N])
    n = np.concatenate([np.full(k, k, np.uint64) for k in dc.XCD_N])
    got = _lane(gpu, _lib.PYA_DBG_XCD_SLOT, b, n)
    at = 0
    for k in dc.XCD_N:
        slots = got[at:at + k].astype(np.int64)
        at += k
        assert np.array_equal(np.sort(slots), np.arange(k)), "n = %d: not a permutation" % k
        for x in range(min(8, k)):
            mine = slots[x::8]
            assert np.array_equal(mine, mine[0] + np.arange(mine.size)), "n = %d, XCD %d" % (k, x)


def test_nl_bump_lut_row_and_the_rank_histogram(gpu):
    state, cls = np.meshgrid(np.arange(65536, dtype=np.uint64), np.arange(1, 9, dtype=np.uint64))
    state, cls = state.ravel(), cls.ravel()
    sh = (cls - np.uint64(1)) * np.uint64(2)
    want = np.where((state >> sh) & np.uint64(3) < 2, state + (np.uint64(1) << sh), state)
    assert want[1 * 65536 + 5] == dc.nl_bump_ref(5, 2)
    assert np.array_equal(_lane(gpu, _lib.PYA_DBG_NL_BUMP, state, cls), want)
    _lane(gpu, _lib.PYA_DBG_NL_BUMP, state[:1], np.zeros(1, np.uint64), want_rc=_lib.PYA_ERR_ARG)
    n = np.arange(4097, dtype=np.uint64)
    want = (np.uint64(5) * n * (n + np.uint64(1))) & np.uint64(0xFFFFFFFF)
    assert [int(x) for x in want[:5]] == [dc.lut_row_ref(i) for i in range(5)]
    assert np.array_equal(_lane(gpu, _lib.PYA_DBG_LUT_ROW, n, np.zeros_like(n)), want)
    seqs = dc.hist_cases()
    a, b, want = [], [], []
    for s in seqs:
        w = dc.hist_ref(s)
        for sel in range(19):
            a.append(dc.pack_ranks(s))
            b.append(len(s) | sel << 8)
            want.append(w[sel - 16] if sel >= 16 else dc.hist_get_ref(w, sel))
    got = _lane(gpu, _lib.PYA_DBG_HIST, np.array(a, np.uint64), np.array(b, np.uint64))
    assert np.array_equal(got, np.array(want, np.uint64)), np.flatnonzero(got != np.array(want, np.uint64))[:5]


# ---------------------------------------------------------------------------------------------------------------------
# one wavefront, one workgroup
# ---------------------------------------------------------------------------------------------------------------------
def _wave(gpu, op, *words):
    vin = np.zeros(_lib.PYA_DBG_WAVE_IN, np.uint64)
    for i, w in enumerate(words):
        vin[64 * i:64 * i + 64] = np.ascontiguousarray(w).view(np.uint64)
    out = np.full(_lib.PYA_DBG_WAVE_OUT, 0xEEEEEEEEEEEEEEEE, np.uint64)
    rc = gpu._lib.pya_debug_wave64(gpu._h, op, _p(vin), _p(out))
    assert rc == 0, gpu._lib.pya_last_error(gpu._h)
    return out


def test_wave_sum_u64(gpu):
    for v in dc.wave_sum_cases():
        want = sum(int(x) for x in v) & dc.M64
        out = _wave(gpu, _lib.PYA_DBG_WAVE_SUM_U64, v)
        assert (out[:64] == np.uint64(want)).all(), (v[:4], out[:4], want)
        assert (out[64:] == 0).all()


def test_wave_min_max_f64(gpu):
    for v in dc.f64_cases():
        out = _wave(gpu, _lib.PYA_DBG_WAVE_MINMAX_F64, np.asarray(v, np.float64))
        assert (out[:64].view(np.float64) == v.min()).all() and (out[64:128].view(np.float64) == v.max()).all(), v


def test_marker_lane_f64_moves_every_bit_from_every_lane(gpu):
    v = dc.marker_case()
    out = _wave(gpu, _lib.PYA_DBG_MARKER_LANE_F64, v).reshape(64, 64)
    assert np.array_equal(out, np.repeat(v[:, None], 64, axis=1))


def test_ion_wave_excl_scan_u64(gpu):
    for v in dc.ion_scan_cases():
        inc = np.cumsum(v)
        out = _wave(gpu, _lib.PYA_DBG_ION_SCAN_U64, v)
        assert np.array_equal(out[:64], inc - v), v[:4]
        assert (out[64:128] == inc[-1]).all()


def test_hist_wave_sum(gpu):
    for words in dc.hist_wave_cases():
        out = _wave(gpu, _lib.PYA_DBG_HIST_WAVE_SUM, words[0], words[1], words[2])
        for w in range(3):
            want = sum(int(x) for x in words[w]) & dc.M64
            assert (out[64 * w:64 * w + 64] == np.uint64(want)).all()
            for fld in range(4):
                assert (want >> (16 * fld)) & 0xFFFF in (0, 65535)                     # (full, and the neighbour untouched)


def test_ts_same_digit(gpu):
    for d, inn in dc.same_digit_cases():
        out = _wave(gpu, _lib.PYA_DBG_SAME_DIGIT, d, inn)
        assert np.array_equal(out[:64], dc.same_digit_ref(d, inn))


def _block_scan(gpu, policy, entries):
    entries = np.ascontiguousarray(entries, np.uint32)
    out = np.full((257,) + entries.shape[1:], 0xEEEEEEEE, np.uint32)
    rc = gpu._lib.pya_debug_block_scan(gpu._h, policy, _p(entries), _p(out))
    assert rc == 0, gpu._lib.pya_last_error(gpu._h)
    return out


def test_ts_block_scan_is_the_sequential_fold(gpu):
    rng = np.random.default_rng(21)
    for p_flag in (0.0, 0.02, 0.1, 0.5, 1.0):
        e = dc.seg_entries(256, rng, p_flag)
        ex, total = dc.seg_fold(e)
        out = _block_scan(gpu, _lib.PYA_DBG_SCAN_SEG, e)
        assert np.array_equal(out[:256], ex) and np.array_equal(out[256], total), p_flag
    for v in (rng.integers(0, 2 ** 32, 256, dtype=np.uint64).astype(np.uint32), np.ones(256, np.uint32), np.full(256, 0xFFFFFFFF, np.uint32)):
        ex, total = dc.add_fold(v)
        out = _block_scan(gpu, _lib.PYA_DBG_SCAN_ADD, v)
        assert np.array_equal(out[:256], ex) and out[256] == total


# ---------------------------------------------------------------------------------------------------------------------
# the scans as they are launched
# ---------------------------------------------------------------------------------------------------------------------
def _ions_scan(gpu, counts):
    off = np.r_[counts, np.int64(-12345)].astype(np.int64)
    rc = gpu._lib.pya_debug_ions_scan(gpu._h, _p(off), counts.size)
    assert rc == 0, gpu._lib.pya_last_error(gpu._h)
    return off


@pytest.mark.parametrize("n", dc.IONS_SCAN_N)
def test_ions_scan_as_launched(gpu, n):
    """counts 0 .. 8 over one tile, the tile's borders, 64 and 65 tiles (the carry loop's second trip) and 200 000 entries"""
    counts = dc.ions_counts(n)
    got, want = _ions_scan(gpu, counts), dc.ions_scan_ref(counts)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "n = %d: %d offsets differ, first at %d: got %d, want %d" % (n, bad.size, bad[0], got[bad[0]], want[bad[0]])


def test_ions_scan_total_past_2_32(gpu):
    counts = dc.ions_counts(dc.IONS_SCAN_WIDE_N, wide=True)
    got, want = _ions_scan(gpu, counts), dc.ions_scan_ref(counts)
    assert want[-1] > 2 ** 32 and np.array_equal(got, want)


def _ts_scan(gpu, policy, entries):
    data = np.ascontiguousarray(entries, np.uint32).copy()
    rc = gpu._lib.pya_debug_ts_scan(gpu._h, policy, _p(data), data.shape[0])
    assert rc == 0, gpu._lib.pya_last_error(gpu._h)
    return data


@pytest.mark.parametrize("n", dc.TS_SCAN_N)
def test_ts_scan_as_launched(gpu, n):
    """one, two and three levels (65 537 entries and 70 001): a 32-bit sum, and the segmented policy that does not commute --
    whose scan is wrong when a level's offsets are combined from the wrong side"""
    rng = np.random.default_rng([22, n])
    v = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    got = _ts_scan(gpu, _lib.PYA_DBG_SCAN_ADD, v)
    assert np.array_equal(got, dc.add_fold(v)[0])
    for p_flag in (0.001, 0.3):
        e = dc.seg_entries(n, rng, p_flag)
        got = _ts_scan(gpu, _lib.PYA_DBG_SCAN_SEG, e)
        want = dc.seg_fold(e)[0]
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, "n = %d, flags %g: %d entries differ, first %d: got %s, want %s" % (n, p_flag, bad.size, bad[0], got[bad[0]],
                                                                                               want[bad[0]])
