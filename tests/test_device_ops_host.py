"""What tests/device_ops_cases.py promises, proven on the CPU: the tables and queries for the device lookup contain every size,
family and edge the GPU tests rely on, the tie operands of charge_mz are ties (in exact rational arithmetic), and the plain
references give the answers of hand-worked cases.  No GPU, no library call."""
from fractions import Fraction

import numpy as np
import pytest

import device_ops_cases as dc

F32 = np.float32


def _ordinal(x):
    """float32 values as integers that step by one from a value to the next one (both zeros at 0)"""
    b = np.asarray(x, F32).view(np.uint32).astype(np.int64)
    return np.where(b < 0x80000000, b, 0x80000000 - b)


# ---- the lookup's inputs ----
def test_every_table_size_and_family_is_present():
    sizes = dc.size_tables()
    assert sorted(t[0].size for t in sizes.values()) == [0, 1, 2, 3, 4, 5, 63, 64, 65, 640, 8191, 8192]
    for mz, rank in sizes.values():
        assert mz.dtype == F32 and rank.dtype == np.uint32 and (np.diff(mz) >= 0).all() and (rank < 10).all()
        # as the binning makes them: at most 10 peaks in any window of 100 m/z from the first one, ranks distinct inside it
        w = np.floor((mz.astype(np.float64) - 100.0) / 100.0).astype(np.int64)
        for k in np.unique(w):
            r = rank[w == k]
            assert r.size <= 10 and np.unique(r).size == r.size
    fam = dc.family_tables()
    for mz, rank in fam.values():
        assert mz.dtype == F32 and np.isfinite(mz).all() and (np.diff(mz) >= 0).all() and (rank < dc.NO_MATCH).all() and mz.size <= 8192
    for name, start in (("tail_even", 6), ("tail_odd", 7)):                            # the table ends at the fifth entry from an even index
        mz, rank = fam[name]
        assert mz.size - 1 == (start & ~1) + 4 and int(np.argmin(rank)) == mz.size - 1 and mz[-1] - mz[start] < 0.02 and mz[start] - mz[start - 1] > 16
    for n in (1, 2, 5, 7, 64, 65):
        mz = fam["all_equal_%d" % n][0]
        assert mz.size == n and (mz == mz[0]).all()                                     # a range of zero, odd and even counts
    rng = lambda name: float(fam[name][0][-1]) - float(fam[name][0][0])
    assert rng("range_below_2032") < 2032.0 == rng("range_2032") < rng("range_above_2032") < 2032.001 and rng("range_2033") == 2033.0
    assert rng("range_60000") == 60000.0
    assert fam["first_at_zero"][0][0] == 0.0 and fam["first_at_zero"][0].size > 100
    for name, base in (("cell_borders", 200.0), ("cell_borders_rescaled", 64.5)):
        mz = fam[name][0].astype(np.float64)
        assert np.array_equal(mz, base + 8.0 * np.arange(mz.size))                     # base + 8 k exactly
    assert rng("cell_borders") < 2032.0 < rng("cell_borders_rescaled")


def test_grid_rescales_exactly_above_2032():
    fam = dc.family_tables()
    for name, rescaled in (("range_below_2032", False), ("range_2032", False), ("range_above_2032", True), ("range_2033", True),
                           ("range_60000", True), ("cell_borders", False), ("cell_borders_rescaled", True)):
        inv_w, nb, last_cell = dc.grid_params(fam[name][0])
        assert (inv_w != F32(0.125)) == rescaled, name
        assert last_cell in ((253, 254) if not rescaled or name.startswith("range_above") else (253, 254, 255)), (name, last_cell)


def test_runs_of_equal_peaks_start_on_even_and_odd_indices():
    mz, rank, runs = dc.run_table()
    assert sorted(set(length for _, length in runs)) == list(range(2, 10))
    for length in range(2, 10):
        assert sorted(start % 2 for start, l in runs if l == length) == [0, 1]
    for start, length in runs:
        assert (mz[start:start + length] == mz[start]).all() and mz[start - 1] < mz[start] < mz[start + length]
        assert np.unique(rank[start:start + length]).size == length
    assert len(set(int(np.argmin(rank[s:s + l])) for s, l in runs)) >= 4               # the smallest rank anywhere in a run


@pytest.mark.parametrize("err", dc.ERRORS, ids=lambda e: "%.9g" % float(e))
def test_clusters_fill_one_window_and_hide_their_best_rank_behind_the_fourth_entry(err):
    mz, rank, clusters = dc.cluster_table(err)
    assert sorted(set(c for _, c in clusters)) == [5, 6, 9, 40]
    for c in (5, 6, 9, 40):
        assert sorted(start % 2 for start, size in clusters if size == c) == [0, 1]
    for start, c in clusters:
        centre = F32(0.5 * (float(mz[start]) + float(mz[start + c - 1])))
        i0, i1 = dc.window(mz, np.array([centre]), err)
        assert i0[0] == start and i1[0] == start + c                                  # the whole cluster and nothing else in one window
        assert int(np.argmin(rank[start:start + c])) >= 4 and rank[start:start + c].min() == 0
    q = dc.cluster_queries(mz, clusters, err)
    count, place = dc.window_shape(mz, rank, q, err)
    deep = (count >= 5) & (place >= 4)
    assert deep.sum() * 10 >= q.size, "%d of %d cluster queries" % (deep.sum(), q.size)
    assert (count > 4).sum() * 2 >= q.size and (count[::11] == [c for _, c in clusters]).all()


def test_the_error_settings_straddle_the_half_check():
    e = dc.ERRORS
    assert e[0] == F32(0.05) and e[1] == F32(0.49) and e[3] == F32(0.5) and e[4] == F32(4.0)
    assert _ordinal(e[2]) - _ordinal(e[1]) == 1 and not e[1] > F32(0.49) and e[2] > F32(0.49)


@pytest.mark.parametrize("group", ("sizes", "families", "clusters"))
def test_every_edge_query_lands_on_its_bound_or_one_step_inside(group):
    seen = set()
    for name, mz, rank, err, q, (f, idx, kind) in dc.lookup_cases(group):
        if mz.size == 0:
            assert f.size == 0
            continue
        p = mz[idx]
        with np.errstate(over="ignore"):
            lo, hi = (f - F32(err)).astype(F32), (f + F32(err)).astype(F32)
        d_lo, d_hi = _ordinal(p) - _ordinal(lo), _ordinal(hi) - _ordinal(p)
        assert ((kind == 0) == (d_lo == 0)).all() and ((kind == 1) == ((d_lo == 1) & (d_hi != 0))).all(), name
        assert ((kind == 2) == ((d_hi == 0) & (d_lo > 1))).all() and ((kind == 3) == ((d_hi == 1) & (d_lo > 1))).all(), name
        assert (kind >= 0).all() and f.size >= 4
        # each kind of edge at the first, the last and some inner peak
        for k in range(4):
            assert (kind == k).any(), (name, dc.EDGE_KINDS[k])
        # the reference takes a peak one step inside and leaves one on the bound: with the table cut down to that peak alone
        for k, inside in ((0, False), (1, True), (2, False), (3, True)):
            j = np.flatnonzero(kind == k)[0]
            one = dc.match_rank(mz[idx[j]:idx[j] + 1], np.array([7], np.uint32), f[j:j + 1], err)[0]
            if inside and not (F32(err) > F32(0.49) and float(f[j]) < float(p[j]) - 0.5):
                assert one == 7, (name, k)
            elif not inside:
                assert one == dc.NO_MATCH, (name, k)
        seen.add(name)
        # the case's queries hold them, with the far, infinite, NaN and negative ones
        assert np.isin(f.view(np.uint32), q.view(np.uint32)).all()
        assert np.isnan(q).any() and np.isposinf(q).any() and np.isneginf(q).any() and (q < 0).any()
        assert ((q < mz[0] - 900) & np.isfinite(q)).any() and ((q > mz[-1] + 900) & np.isfinite(q)).any()
    assert len(seen) >= 5


# ---- the lookup's references ----
def test_match_rank_on_a_hand_worked_table():
    mz = np.array([100.0, 100.25, 100.5, 101.0, 250.0], F32)
    rank = np.array([3, 1, 2, 0, 4], np.uint32)
    q = np.array([100.3, 99.0, 100.75, 250.0, 1e6, np.nan, np.inf, -np.inf, 100.0], F32)
    # err 0.3: (100.0, 100.6) -> peaks 100.25, 100.5 -> 1; (98.7, 99.3) none; (100.45, 101.05) -> 100.5, 101.0 -> 0; ...
    assert dc.match_rank(mz, rank, q, F32(0.3)).tolist() == [1, 15, 0, 4, 15, 15, 15, 15, 1]
    # err 1.0 with the half check: query 100.3 sees every peak of (99.3, 101.3) that is <= 100.8: not 101.0
    # (query 100.75 keeps it: 101.0 <= 101.25)
    assert dc.match_rank(mz, rank, q, F32(1.0)).tolist() == [1, 15, 0, 4, 15, 15, 15, 15, 1]
    # ... where the plain window would have taken rank 0
    i0, i1 = dc.window(mz, q[:1], F32(1.0))
    assert (i0[0], i1[0]) == (0, 4)
    assert dc.match_rank(np.zeros(0, F32), np.zeros(0, np.uint32), q, F32(0.3)).tolist() == [15] * 9
    count, place = dc.window_shape(mz, rank, q[:3], F32(0.3))
    assert count.tolist() == [2, 0, 2] and place.tolist() == [0, -1, 1]


def test_grid_reference_on_a_hand_worked_table():
    mz = np.array([100.0, 107.9, 108.0, 131.0, 132.0, 180.0], F32)      # cells of 8 m/z from 100: 0, 0, 1, 3, 4, 10
    assert dc.grid_params(mz) == (F32(0.125), F32(-12.5), 10)
    assert dc.grid_cell(mz, mz).tolist() == [0, 0, 1, 3, 4, 10]
    assert dc.grid_cell(mz, np.array([-5.0, 99.9, 1e9, np.nan, np.inf, -np.inf, 115.99], F32)).tolist() == [0, 0, 10, 0, 10, 0, 1]
    cells = np.zeros(257, np.int64)
    cells[:11] = [0, 2, 2, 2, 4, 4, 4, 4, 4, 4, 4]                     # first peak of a cell >= k: 0, 2, 3, 3, 4, 5 ... made even
    cells[256] = 10
    dc.check_grid(mz, cells)
    for k, v in ((1, 4), (1, 1), (4, 2), (10, 6)):                       # behind the first peak / odd / too early / too late
        bad = cells.copy()
        bad[k] = v
        with pytest.raises(AssertionError):
            dc.check_grid(mz, bad)
    # a rescaled grid: 254 cells over the range
    wide = np.array([0.0, 1000.0, 2540.0], F32)
    inv_w, nb, last_cell = dc.grid_params(wide)
    assert inv_w == F32(0.1) and last_cell == 254 or last_cell == 253
    assert dc.grid_params(np.array([5.0, 5.0], F32)) == (F32(0.125), F32(-0.625), 0)


def test_fma32_rounds_once():
    rng = np.random.default_rng(3)
    x = rng.uniform(0, 70000, 3000).astype(F32)
    for a, b in ((F32(0.125), F32(-12.5)), (F32(254.0) / F32(60000.0), F32(-0.21166667)), (F32(0.1), F32(-6.45))):
        got = dc.fma32(x, a, b)
        for i in range(0, x.size, 7):
            assert got[i] == dc._round_f32(Fraction(float(x[i])) * Fraction(float(a)) + Fraction(float(b)))
    # a sum exactly half way between two float32 in float64: 1 + 2^-24 (tie to even: 1), and just above it
    assert dc.fma32(np.array([2.0 ** -24], F32), F32(1.0), F32(1.0))[0] == F32(1.0)
    assert dc.fma32(np.array([1.0 + 2.0 ** -23], F32), F32(2.0 ** -24), F32(1.0))[0] == dc.up32(F32(1.0))
    assert dc.cvt_u32([-1.0, np.nan, 0.99, 1.0, 255.9, 1e20, np.inf, -np.inf]).tolist() == [0, 0, 0, 1, 255, 2 ** 32 - 1, 2 ** 32 - 1, 0]


# ---- one value per lane ----
def test_fastdiv_formula_is_the_division_on_the_whole_sample():
    """the multiplier and its one correction, restated on integers, over every divisor of the GPU test (a thinner run of small
    dividends here: the GPU test takes all of 0 .. 70 000) -- also where e * d passes 2^32, beyond the documented domain"""
    assert dc.FASTDIV_D[:599] == tuple(range(2, 601)) and set(dc.FASTDIV_D[599:]) == {4095, 4096, 4097, 65535, 65536, 65537, 2 ** 31 - 1, 2 ** 31,
                                                                                         2 ** 31 + 1, 2 ** 32 - 1}
    e, d = dc.fastdiv_cases(dc.FASTDIV_D, dense=3000)
    assert np.array_equal(dc.fastdiv_formula(e, d), e // d)
    assert (e * d >= 2 ** 32).any() and e.max() == 2 ** 32 - 1
    for dd in (2, 3, 600, 65537, 2 ** 32 - 1):
        ee = dc.fastdiv_dividends(dd, np.random.default_rng(1), dense=100)
        few = min(20, (2 ** 32 - 1) // dd)
        assert (ee % dd == 0).sum() >= few and (ee % dd == dd - 1).sum() >= few and ee.max() >= (2 ** 32 - 1) // dd * dd - 1 and ee.max() < 2 ** 32
    assert dc.fastdiv_formula([7, 7, 0, 2 ** 32 - 1], [1, 0, 5, 2 ** 32 - 1]).tolist() == [7, 7, 0, 1]
    # without the correction the sample is NOT all right: the multiplier is one too large for some operands
    m = np.ceil(4294967296.0 / d.astype(np.float64)).astype(np.uint64)
    assert (((e * m) >> np.uint64(32)) != e // d).any()


def test_charge_tie_operands_are_ties_for_every_charge():
    """in exact rational arithmetic: the dividend the device forms from m is a float64 whose quotient by z lies on a float32
    tie or within one float64 ulp of it -- at least 8 such operands for every charge that is not a power of two"""
    import math
    flips = 0
    for z in range(3, 256):
        if z & (z - 1) == 0:
            continue
        ops = dc.charge_tie_operands(z)
        assert len(ops) >= 8 and len(set(m for m, _ in ops)) >= 8
        for m, t in ops:
            assert 50.0 <= m <= 1e5
            below = F32(float(t))
            below = below if Fraction(float(below)) < t else dc.down32(below)
            assert Fraction(float(below)) < t < Fraction(float(dc.up32(below))) and Fraction(float(below)) + Fraction(float(dc.up32(below))) == 2 * t
            a = dc.charge_a(m, z)
            assert abs(Fraction(a) / z - t) <= Fraction(math.ulp(float(t)))
            # the correctly rounded float64 quotient, then float32: what the reference computes, from the rationals
            want = dc._round_f32(Fraction(a / z))
            assert dc.charge_ref(m, z) == want
            flips += F32(a * (1.0 / z)) != want
    assert flips > 50, "the operands would not tell a / z from a * (1 / z)"


def test_charge_cases_cover_every_charge():
    m, z = dc.charge_cases()
    assert np.array_equal(np.unique(z), np.arange(1, 256)) and m.min() >= 50.0 and m.max() <= 1e5
    assert np.bincount(z.astype(np.int64))[1:].min() >= 160
    assert dc.charge_ref(np.array([100.0, 100.0, 299.0]), np.array([1, 2, 3])).tolist() == [F32(101.007825), F32(51.007825), F32((299.0 + 3 * 1.007825) / 3)]


def test_bit_references_on_hand_worked_masks():
    assert [dc.nth_set_bit_ref(0b101100, n) for n in range(5)] == [2, 3, 5, 64, 64]
    assert dc.nth_set_bit_ref(1 << 63, 0) == 63 and dc.nth_set_bit_ref(0, 0) == 64 and dc.nth_set_bit_ref(2 ** 64 - 1, 63) == 63
    assert dc.deposit_sites_ref(0b101, 0b101100) == 0b100100 and dc.deposit_sites_ref(2 ** 64 - 1, 0b1010) == 0b1010
    assert dc.deposit_sites_ref(0b10, 1 << 63 | 1) == 1 << 63 and dc.deposit_sites_ref(0xDEADBEEF, 2 ** 64 - 1) == 0xDEADBEEF
    masks = dc.bit_masks()
    assert {0, 2 ** 64 - 1, 1 << 63} <= set(masks) and len(masks) > 20
    m, n = dc.nth_set_bit_cases()
    assert m.size % 64 == 0 and all(len(set(m[i:i + 64].tolist())) == 1 for i in range(0, m.size, 64))     # wave-uniform masks
    for mask in masks:
        pc = bin(mask).count("1")
        assert {pc - 1 if pc else 0, pc, pc + 1} <= set(n[m == np.uint64(mask)].tolist())                 # n at and above the popcount


def test_xcd_slot_reference_is_a_permutation_by_hand():
    assert [dc.xcd_slot_ref(b, 10) for b in range(10)] == [0, 2, 4, 5, 6, 7, 8, 9, 1, 3]
    assert [dc.xcd_slot_ref(b, 16) for b in range(16)] == [0, 2, 4, 6, 8, 10, 12, 14, 1, 3, 5, 7, 9, 11, 13, 15]
    for n in (1, 7, 8, 9, 1000, 2049):
        assert sorted(dc.xcd_slot_ref(b, n) for b in range(n)) == list(range(n))
    assert dc.XCD_N[:2049] == tuple(range(1, 2050)) and max(dc.XCD_N) == 1000003


def test_small_references_by_hand():
    assert dc.nl_bump_ref(0, 1) == 1 and dc.nl_bump_ref(1, 1) == 2 and dc.nl_bump_ref(2, 1) == 2 and dc.nl_bump_ref(0b1000, 2) == 0b1000
    assert dc.nl_bump_ref(0, 8) == 1 << 14 and dc.nl_bump_ref(3, 1) == 3
    assert [dc.lut_row_ref(n) for n in range(5)] == [0, 10, 30, 60, 100]
    w = dc.hist_ref([0, 0, 3, 4, 9, 9, 9, 10, 15])
    assert w == [2 | 1 << 48, 1, 3 << 16] and [dc.hist_get_ref(w, r) for r in range(10)] == [2, 0, 0, 1, 1, 0, 0, 0, 0, 3]
    assert dc.pack_ranks([1, 15, 2]) == 0x2F1
    d = np.zeros(64, np.uint64)
    d[[3, 9]] = 7
    inn = np.ones(64, np.uint64)
    inn[9] = 0
    ref = dc.same_digit_ref(d, inn)
    assert ref[3] == 8 and ref[9] == 8 and ref[0] == 2 ** 64 - 1 - 8 - 512


def test_scan_references_by_hand():
    e = np.array([[5, 0, 0], [7, 1, 11], [1, 0, 0], [2, 0, 0], [9, 1, 12], [4, 0, 0]], np.uint32)
    ex, total = dc.seg_fold(e)
    assert ex.tolist() == [[0, 0, 0], [5, 0, 0], [7, 1, 11], [8, 1, 11], [10, 1, 11], [9, 1, 12]] and total.tolist() == [13, 1, 12]
    a, b, c = (tuple(x) for x in e[:3].tolist())
    assert dc.seg_op(dc.seg_op(a, b), c) == dc.seg_op(a, dc.seg_op(b, c)) and dc.seg_op(a, b) != dc.seg_op(b, a)
    assert dc.seg_op((0, 0, 0), b) == b == dc.seg_op(b, (0, 0, 0))
    rng = np.random.default_rng(1)
    for p in (0.0, 0.1, 0.5, 1.0):
        x = [tuple(r) for r in dc.seg_entries(60, rng, p).tolist()]
        assert all(r[2] != 0 if r[1] else r[2] == 0 for r in x)
        for i in range(0, 57):
            assert dc.seg_op(dc.seg_op(x[i], x[i + 1]), x[i + 2]) == dc.seg_op(x[i], dc.seg_op(x[i + 1], x[i + 2]))
    ex, total = dc.add_fold(np.array([1, 2 ** 32 - 1, 5], np.uint32))
    assert ex.tolist() == [0, 1, 0] and total == 5
    assert dc.ions_scan_ref(np.array([3, 0, 8], np.int64)).tolist() == [0, 3, 3, 11]
    assert int(dc.ions_scan_ref(dc.ions_counts(dc.IONS_SCAN_WIDE_N, wide=True))[-1]) > 2 ** 32
    assert max(dc.IONS_SCAN_N) == 200000 and 66561 in dc.IONS_SCAN_N and 70001 in dc.TS_SCAN_N
    for v in dc.ion_scan_cases():
        assert int(v.max()) < 2 ** 50
    assert any(int((v & np.uint64(0xFFFFFF)).sum()) >= 2 ** 24 for v in dc.ion_scan_cases())
    for words in dc.hist_wave_cases():
        for w in range(3):
            for fld in range(4):
                assert int(((words[w] >> np.uint64(16 * fld)) & np.uint64(0xFFFF)).sum()) in (0, 65535)
