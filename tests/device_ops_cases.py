"""Inputs and plain references for the tests of the device building blocks (include/pyascore_debug.h: pya_debug_lookup,
pya_debug_lane_ops, pya_debug_wave64, pya_debug_block_scan, pya_debug_ts_scan, pya_debug_ions_scan).  Everything here is numpy
and Python: tests/test_device_ops_host.py proves on the CPU what the generators promise and holds the references against
hand-worked cases; tests/test_gpu_device_ops.py compares the kernels with them.  Every generator is deterministic."""
import math
from fractions import Fraction

import numpy as np

F32 = np.float32
INF32 = F32(np.inf)
NO_MATCH = 15
GRID_CELLS = 256
PROTON = 1.007825


def up32(x):
    return np.nextafter(np.asarray(x, F32), INF32)


def down32(x):
    return np.nextafter(np.asarray(x, F32), -INF32)


# ---------------------------------------------------------------------------------------------------------------------
# the lookup: tables
# ---------------------------------------------------------------------------------------------------------------------
ERRORS = (F32(0.05), F32(0.49), up32(F32(0.49)), F32(0.5), F32(4.0))     # (up32(0.49f): the first setting with the half check)
TABLE_SIZES = (0, 1, 2, 3, 4, 5, 63, 64, 65, 640, 8191, 8192)
CLUSTER_SIZES = (5, 6, 9, 40)
RUN_LENGTHS = tuple(range(2, 10))


def binned(n, rng, first=100.0):
    """n peaks as the binning leaves them: windows of 100 m/z from `first`, at most 10 peaks in each, ranked 0 .. 9 inside it"""
    mz, rank = [], []
    w = 0
    while len(mz) < n:
        k = min(10, n - len(mz))
        mz += sorted((first + 100.0 * w + rng.uniform(0.0, 100.0, k)).tolist())
        rank += rng.permutation(k).tolist()
        w += 1
    return np.array(mz, F32), np.array(rank, np.uint32)


def _finish(mz, rank):
    mz, rank = np.asarray(mz, F32), np.asarray(rank, np.uint32)
    order = np.argsort(mz, kind="stable")
    return np.ascontiguousarray(mz[order]), np.ascontiguousarray(rank[order])


def size_tables():
    return {"n%d" % n: binned(n, np.random.default_rng([1, n])) for n in TABLE_SIZES}


def cluster_table(err, seed=0):
    """Clusters of 5, 6, 9 and 40 peaks, each inside ONE match window of `err` (0.8 of its width) and each starting once on an
    even and once on an odd index; the smallest rank of a cluster (0) sits in its fifth or a later entry, the other ranks are
    1 .. 14.  Between the clusters: lone peaks 25 m/z apart (ranks 0 .. 9).  Returns mz, rank, clusters = [(start, size)]."""
    rng = np.random.default_rng([2, seed, int(np.asarray(err, F32).view(np.uint32))])
    err = float(err)
    mz, rank, clusters = [], [], []
    at = 300.0
    for c in CLUSTER_SIZES:
        for parity in (0, 1):
            while True:
                mz.append(at)
                rank.append(int(rng.integers(0, 10)))
                at += 25.0
                if len(mz) % 2 == parity:
                    break
            step = 1.6 * err / c
            r = rng.integers(1, NO_MATCH, c)
            r[int(rng.integers(4, c))] = 0
            clusters.append((len(mz), c))
            mz += [at + step * j for j in range(c)]
            rank += r.tolist()
            at += 25.0 + 1.6 * err
    mz.append(at)
    rank.append(3)
    mz32 = np.array(mz, F32)
    assert (np.diff(mz32) > 0).all()
    return mz32, np.array(rank, np.uint32), clusters


def cluster_queries(mz, clusters, err):
    """queries over every cluster: its centre and shifts of up to one tolerance either way"""
    out = []
    for start, c in clusters:
        centre = 0.5 * (float(mz[start]) + float(mz[start + c - 1]))
        out += [centre + float(err) * s for s in (0.0, -0.1, 0.1, -0.3, 0.3, -0.6, 0.6, -0.9, 0.9, -1.2, 1.2)]
    return np.array(out, F32)


def run_table():
    """runs of 2 .. 9 equal m/z, each once from an even and once from an odd index; distinct ranks inside a run, the smallest
    anywhere in it"""
    rng = np.random.default_rng(3)
    mz, rank, runs = [], [], []
    at = 200.0
    for length in RUN_LENGTHS:
        for parity in (0, 1):
            while True:
                mz.append(at)
                rank.append(int(rng.integers(0, 10)))
                at += 17.0
                if len(mz) % 2 == parity:
                    break
            runs.append((len(mz), length))
            mz += [at + 0.125] * length
            rank += rng.permutation(14)[:length].tolist()
            at += 17.0
    mz.append(at)
    rank.append(1)
    return np.array(mz, F32), np.array(rank, np.uint32), runs


def family_tables():
    """name -> (mz, rank): the shapes of a retained table the grid and the sentinels treat differently"""
    rng = np.random.default_rng(4)
    t = {}
    mz, rank, _ = run_table()
    t["runs"] = (mz, rank)
    # the table ends one entry behind the four a lookup fetches at once: five peaks in one window from an even index, four
    # from an odd one (the fetch starts at the even index before it), the smallest rank in the last
    for name, lone, c in (("tail_even", 6, 5), ("tail_odd", 7, 4)):
        mz = [150.0 + 40.0 * i for i in range(lone)] + [150.0 + 40.0 * lone + 0.004 * j for j in range(c)]
        t[name] = (np.array(mz, F32), np.array([2, 5, 1, 7, 3, 4, 6][:lone] + [9, 8, 6, 5, 0][-c:], np.uint32))
    for n in (1, 2, 5, 7, 64, 65):
        t["all_equal_%d" % n] = (np.full(n, 512.25, F32), (np.arange(n) % 14 + 1).astype(np.uint32)[::-1].copy())
    # the grid is rescaled when range * 0.125 > 254: range just below, at and just above 2032
    for name, last in (("range_below_2032", down32(down32(F32(2132.0)))), ("range_2032", F32(2132.0)), ("range_above_2032", up32(F32(2132.0))),
                       ("range_2033", F32(2133.0))):
        inner, r = binned(80, rng, first=110.0)
        inner = inner[inner < 2100.0]
        t[name] = _finish(np.r_[F32(100.0), inner, last], np.r_[0, r[:inner.size], 2])
    mz = np.sort(rng.uniform(50.0, 60050.0, 300)).astype(F32)
    mz[0], mz[-1] = 50.0, 60050.0
    t["range_60000"] = (mz, rng.integers(0, 10, 300).astype(np.uint32))
    mz, rank = binned(120, rng, first=0.0)
    mz[0] = 0.0
    t["first_at_zero"] = (mz, rank)
    t["cell_borders"] = ((200.0 + 8.0 * np.arange(254)).astype(F32), (np.arange(254) % 10).astype(np.uint32))
    t["cell_borders_rescaled"] = ((64.5 + 8.0 * np.arange(400)).astype(F32), (np.arange(400) % 10).astype(np.uint32))
    return t


# ---------------------------------------------------------------------------------------------------------------------
# the lookup: queries
# ---------------------------------------------------------------------------------------------------------------------
EDGE_KINDS = ("lo", "lo+", "hi", "hi-")     # the peak equals lo / the float32 above lo / hi / the float32 below hi


def edge_kind(f, p, err):
    """which of EDGE_KINDS query f is for peak p (index into EDGE_KINDS), -1: none.  Float32 throughout."""
    f, p, err = np.asarray(f, F32), np.asarray(p, F32), F32(err)
    lo, hi = (f - err).astype(F32), (f + err).astype(F32)
    kind = np.full(f.shape, -1, np.int64)
    kind[p == down32(hi)] = 3
    kind[p == hi] = 2
    kind[p == up32(lo)] = 1
    kind[p == lo] = 0
    return kind


def edge_queries(mz, err, rng, most=160):
    """queries that put a peak exactly on a bound of the window or one float32 inside it: f, index of the peak, kind.  The
    candidates are the float32 values within four steps of p + err and p - err; each is kept for what edge_kind says it is."""
    if mz.size == 0:
        return np.zeros(0, F32), np.zeros(0, np.int64), np.zeros(0, np.int64)
    pick = np.arange(mz.size) if mz.size <= most else np.unique(np.r_[0, 1, mz.size - 2, mz.size - 1, rng.choice(mz.size, most, replace=False)])
    fs, idx = [], []
    for sign in (1.0, -1.0):
        f0 = (mz[pick] + F32(sign) * F32(err)).astype(F32)
        cand = [f0]
        a = b = f0
        for _ in range(4):
            a, b = up32(a), down32(b)
            cand += [a, b]
        fs.append(np.concatenate(cand))
        idx.append(np.tile(pick, len(cand)))
    f, idx = np.concatenate(fs), np.concatenate(idx)
    kind = edge_kind(f, mz[idx], err)
    keep = kind >= 0
    return f[keep], idx[keep], kind[keep]


SPECIAL_QUERIES = np.array([np.inf, -np.inf, np.nan, -np.nan, -0.0, 0.0, -5.0, -1e30, 3e38, -3e38, 1e6, 1e-40, 7.0], F32)


def plain_queries(mz, err, rng):
    """far below and above the table, infinities, NaN, negative values, and random ones over and around it"""
    first, last = (float(mz[0]), float(mz[-1])) if mz.size else (100.0, 2000.0)
    e = float(err)
    out = [SPECIAL_QUERIES, np.array([first - 1000.0, last + 1000.0, first - 2 * e, last + 2 * e, first, last], F32),
           rng.uniform(first - 2 * e - 1.0, last + 2 * e + 1.0, 300).astype(F32)]
    if mz.size:
        near = mz[rng.integers(0, mz.size, 300)].astype(np.float64) + rng.uniform(-1.5 * e, 1.5 * e, 300)
        out.append(near.astype(F32))
    return np.concatenate(out)


def lookup_cases(group):
    """[(name, mz, rank, err, queries, (edge queries, their peaks, their kinds))] of one group: "sizes", "families" or
    "clusters", every table at every error"""
    cases = []
    for err in ERRORS:
        tag = "%s@%.9g" % ("%s", float(err))
        if group == "clusters":
            mz, rank, clusters = cluster_table(err)
            tables = {"clusters": (mz, rank)}
        else:
            tables = size_tables() if group == "sizes" else family_tables()
        for name, (mz, rank) in tables.items():
            rng = np.random.default_rng([5, len(cases)])
            edges = edge_queries(mz, err, rng)
            q = [plain_queries(mz, err, rng), edges[0]]
            if group == "clusters":
                q.append(cluster_queries(mz, clusters, err))
            cases.append((tag % name, mz, rank, err, np.concatenate(q), edges))
    return cases


# ---------------------------------------------------------------------------------------------------------------------
# the lookup: references
# ---------------------------------------------------------------------------------------------------------------------
def window(mz, f, err):
    """[i0, i1): the peaks with f32(f - err) < p < f32(f + err), float32 throughout (empty for a NaN query)"""
    f = np.asarray(f, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        lo, hi = (f - F32(err)).astype(F32), (f + F32(err)).astype(F32)
    nan = np.isnan(lo) | np.isnan(hi)
    i0 = np.searchsorted(mz, np.where(nan, INF32, lo), side="right")
    i1 = np.searchsorted(mz, np.where(nan, -INF32, hi), side="left")
    return i0, np.maximum(i0, i1)


def match_rank(mz, rank, f, err):
    """device_common.hip.h, "Match lookup": the smallest rank over the peaks p with f32(f - err) < p < f32(f + err) -- and, when
    err > 0.49, (double) f >= (double) p - 0.5 --, 15 without one"""
    f = np.asarray(f, F32)
    i0, i1 = window(mz, f, err)
    best = np.full(f.shape, NO_MATCH, np.int64)
    half = F32(err) > F32(0.49)
    pad_mz, pad_rank = np.r_[mz, F32(0)], np.r_[rank, np.uint32(NO_MATCH)].astype(np.int64)
    for j in range(int((i1 - i0).max()) if f.size else 0):
        i = np.minimum(i0 + j, mz.size)
        ok = i0 + j < i1
        if half:
            with np.errstate(invalid="ignore"):
                ok &= f.astype(np.float64) >= pad_mz[i].astype(np.float64) - 0.5
        best = np.where(ok & (pad_rank[i] < best), pad_rank[i], best)
    return best


def window_shape(mz, rank, f, err):
    """entries in each query's window, and the place inside it of the first entry with the window's smallest rank (-1: empty)"""
    i0, i1 = window(mz, f, err)
    place = np.full(i0.shape, -1, np.int64)
    for q in range(i0.size):
        if i1[q] > i0[q]:
            place[q] = int(np.argmin(rank[i0[q]:i1[q]]))
    return i1 - i0, place


def _round_f32(x):
    """a Fraction rounded to the nearest float32, ties to even (finite results only)"""
    g = F32(float(x))                                        # (within one float32 of the answer)
    cands = [down32(g), g, up32(g)]
    dist = [abs(Fraction(float(c)) - x) for c in cands]
    m = min(dist)
    near = [c for c, d in zip(cands, dist) if d == m]
    if len(near) == 2:
        near = [c for c in near if int(c.view(np.uint32)) % 2 == 0]
    return near[0]


def fma32(x, a, b):
    """fmaf(x, a, b) for a float32 array x and float32 scalars a, b: the product is exact in float64 and the sum is rounded to
    float64 first, so the few elements whose float64 sum lies exactly half way between two float32 are redone in Fractions"""
    x = np.asarray(x, F32)
    s = x.astype(np.float64) * np.float64(a) + np.float64(b)
    out = s.astype(F32)
    finite = np.isfinite(s)
    doubt = finite & ((s.view(np.uint64) & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000))
    for i in np.flatnonzero(doubt):
        out[i] = _round_f32(Fraction(float(x[i])) * Fraction(float(a)) + Fraction(float(b)))
    return out


def cvt_u32(rel):
    """v_cvt_u32_f32: truncates, NaN and negative values to 0, large ones to 2^32 - 1"""
    rel = np.asarray(rel, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(rel) | (rel <= 0), 0, np.minimum(np.floor(np.where(np.isfinite(rel), rel, 2.0 ** 32)), 2.0 ** 32 - 1)).astype(np.uint64)


def grid_params(mz):
    """(inv_w, nb, last_cell) of grid_params / grid_build for a table, in float32 as the device computes them"""
    if mz.size == 0:
        return F32(0), F32(0), 0
    first, last = F32(mz[0]), F32(mz[-1])
    rng_ = F32(last - first)
    inv_w = F32(0.125)
    if F32(rng_ * inv_w) > F32(GRID_CELLS - 2):
        inv_w = F32(F32(GRID_CELLS - 2) / rng_)
    nb = F32(-F32(first * inv_w))
    last_cell = int(min(int(cvt_u32(fma32([last], inv_w, nb))[0]), GRID_CELLS - 1))
    return inv_w, nb, last_cell


def grid_cell(mz, x):
    """grid_cell(x) of the table's grid"""
    inv_w, nb, last_cell = grid_params(mz)
    return np.minimum(cvt_u32(fma32(x, inv_w, nb)), np.uint64(last_cell)).astype(np.int64)


def check_grid(mz, cells):
    """what a grid must be (cells[0 .. 255], cells[256] = last_cell): grid_cell does not decrease over the table;
    last_cell is the last peak's cell; every cell up to it holds an even index at or before the first peak whose cell is at
    least the cell's number -- and no further before it than evenness asks (grid_build: the first peak of an occupied cell
    writes its index, an empty cell takes the next occupied one's)"""
    cells = np.asarray(cells, np.int64)
    if mz.size == 0:
        assert cells[GRID_CELLS] == 0 and cells[0] == 0
        return
    pc = grid_cell(mz, mz)
    assert (np.diff(pc) >= 0).all(), "grid_cell decreases over the sorted table"
    last_cell = grid_params(mz)[2]
    assert cells[GRID_CELLS] == last_cell == pc[-1]
    k = np.arange(last_cell + 1)
    first = np.searchsorted(pc, k, side="left")
    got = cells[:last_cell + 1]
    assert (got % 2 == 0).all(), "odd index in a cell"
    assert (got <= first).all(), "a cell starts behind the first peak of its range"
    assert np.array_equal(got, first & ~1), "a cell starts earlier than the even index at its first peak"


# ---------------------------------------------------------------------------------------------------------------------
# one value per lane
# ---------------------------------------------------------------------------------------------------------------------
FASTDIV_D = tuple(range(2, 601)) + (4095, 4096, 4097, 65535, 65536, 65537, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 32 - 1)
FASTDIV_DENSE = 70000                                       # every dividend 0 .. this


def fastdiv_dividends(d, rng, dense=FASTDIV_DENSE):
    """multiples of d and the values before them (small, random and the largest), 0 .. dense, random ones up to 2^32 - 1"""
    top = (2 ** 32 - 1) // d
    k = np.unique(np.r_[np.arange(1, min(top, 40) + 1), rng.integers(1, top + 1, 40), top]).astype(np.uint64)
    mult = k * np.uint64(d)
    return np.concatenate([mult, mult - np.uint64(1), np.arange(dense + 1, dtype=np.uint64), rng.integers(0, 2 ** 32, 200, dtype=np.uint64)])


def fastdiv_cases(ds, dense=FASTDIV_DENSE):
    """(e, d) as uint64 arrays for the divisors ds"""
    es, dd = [], []
    for d in ds:
        e = fastdiv_dividends(d, np.random.default_rng([6, d % 65521]), dense)
        es.append(e)
        dd.append(np.full(e.size, d, np.uint64))
    return np.concatenate(es), np.concatenate(dd)


def fastdiv_formula(e, d):
    """device_common.hip.h's fastdiv restated on integers: m = ceil(2^32 / d) as a 32-bit word, q = umulhi(e, m), one correction"""
    e, d = np.asarray(e, np.uint64), np.asarray(d, np.uint64)
    d = np.where(d == 0, np.uint64(1), d)
    m = np.ceil(4294967296.0 / d.astype(np.float64)).astype(np.uint64) & np.uint64(0xFFFFFFFF)    # (2^32 / d in float64 is correctly rounded; its ceil is exact for d < 2^32)
    q = (e * m) >> np.uint64(32)
    q = np.where(((q * d) & np.uint64(0xFFFFFFFF)) > e, q - np.uint64(1), q)
    return np.where(d == 1, e, q)


def charge_c(z):
    """z * 1.007825 as the device has it (float64)"""
    return float(z) * PROTON


def charge_a(m, z):
    """the dividend of charge_mz as the device computes it: m + z * 1.007825 in float64"""
    return float(m) + charge_c(z)


def charge_ref(m, z):
    """np.float32((m + z * 1.007825) / z), every step IEEE float64"""
    m, z = np.asarray(m, np.float64), np.asarray(z, np.float64)
    return ((m + z * PROTON) / z).astype(F32)


def _tie_above(f):
    """the rational half way between float32 f and the float32 above it"""
    return (Fraction(float(f)) + Fraction(float(up32(f)))) / 2


def charge_tie_operands(z, want=12):
    """m in [50, 1e5] whose dividend a = m + z * 1.007825 (float64, as the device adds) gives an exact a / z ON a float32 tie
    or within one float64 ulp of one: a = t z is exact in float64 for a tie t (25 bits times 8), and so are its neighbours.
    Returns [(m, tie as a Fraction)]."""
    rng = np.random.default_rng([7, z])
    c = charge_c(z)
    out = []
    for _ in range(100 * want):
        if len(out) >= want:
            break
        f = F32(rng.uniform((50.0 + c) / z * 1.01, (1e5 + c) / z * 0.99))
        t = _tie_above(f)
        a0 = float(t * z)
        assert Fraction(a0) == t * z
        ulp_t = Fraction(math.ulp(float(t)))
        for a in (a0, math.nextafter(a0, math.inf), math.nextafter(a0, -math.inf)):
            if abs(Fraction(a) / z - t) > ulp_t:
                continue
            m0 = a - c
            for m in (m0, math.nextafter(m0, math.inf), math.nextafter(m0, -math.inf)):
                if 50.0 <= m <= 1e5 and m + c == a:
                    out.append((m, t))
                    break
    return out


def charge_cases():
    """(m, z) float64 / uint64 arrays: every charge 1 .. 255 with 160 random masses in [50, 1e5] and its tie operands"""
    ms, zs = [], []
    for z in range(1, 256):
        rng = np.random.default_rng([8, z])
        m = rng.uniform(50.0, 1e5, 160).tolist()
        if z & (z - 1):
            m += [x for x, _ in charge_tie_operands(z)]
        ms += m
        zs += [z] * len(m)
    return np.array(ms, np.float64), np.array(zs, np.uint64)


BIT_MASKS = (0, 2 ** 64 - 1, 1 << 63, 1, 0x8000000000000001, 0x00000000FFFFFFFF, 0xFFFFFFFF00000000, 0x5555555555555555)


def bit_masks():
    rng = np.random.default_rng(9)
    dense = [int(x) for x in rng.integers(0, 2 ** 64, 12, dtype=np.uint64)]
    sparse = [int(a & b & c) for a, b, c in rng.integers(0, 2 ** 64, (8, 3), dtype=np.uint64)]
    return list(BIT_MASKS) + dense + sparse


def nth_set_bit_ref(m, n):
    j = 0
    for pos in range(64):
        if (m >> pos) & 1:
            if j == n:
                return pos
            j += 1
    return 64


def deposit_sites_ref(bits, mask):
    out, j = 0, 0
    for pos in range(64):
        if (mask >> pos) & 1:
            out |= ((bits >> j) & 1) << pos
            j += 1
    return out


def nth_set_bit_cases():
    """(mask, n): every n from 0 to two past the popcount, 64, 1000 and -1 as the int it becomes; a mask's operands fill whole
    wavefronts (the function is called with a wave-uniform mask)"""
    ms, ns = [], []
    for m in bit_masks():
        n = list(range(bin(m).count("1") + 3)) + [64, 1000, 0xFFFFFFFF]
        n += [n[-1]] * (-len(n) % 64)
        ms += [m] * len(n)
        ns += n
    return np.array(ms, np.uint64), np.array(ns, np.uint64)


def deposit_cases():
    rng = np.random.default_rng(10)
    bits, ms = [], []
    for m in bit_masks():
        b = [0, 2 ** 64 - 1, 1, 1 << 63] + [int(x) for x in rng.integers(0, 2 ** 64, 60, dtype=np.uint64)]
        bits += b
        ms += [m] * len(b)
    return np.array(bits, np.uint64), np.array(ms, np.uint64)


XCD_N = tuple(range(1, 2050)) + (4095, 4097, 65537, 100003, 1000003)


def xcd_slot_ref(b, n):
    """block b of n to its slot: XCD x = b % 8 owns n // 8 + (x < n % 8) consecutive slots, in the order of b // 8"""
    q, r, x, k = n // 8, n % 8, b % 8, b // 8
    return x * q + min(x, r) + k


def nl_bump_ref(state, cls):
    sh = (cls - 1) * 2
    return state + (1 << sh) if (state >> sh) & 3 < 2 else state


def lut_row_ref(n):
    return 10 * sum(range(1, n + 1)) & 0xFFFFFFFF           # (row n starts behind rows 0 .. n - 1 of 10 * (row + 1) floats)


def hist_ref(ranks):
    """the three words of a histogram after hist_add of `ranks`: 16-bit counts of rank 0-3 | 4-7 | 8-9, other ranks ignored"""
    w = [0, 0, 0]
    for r in ranks:
        if r < 10:
            w[r // 4] += 1 << (16 * (r % 4))
    return w


def hist_get_ref(w, r):
    return (w[0 if r < 4 else (1 if r < 8 else 2)] >> (16 * (r % 4))) & 0xFFFF


def hist_cases():
    """(packed ranks, count, [ranks]) -- every rank alone 1 .. 16 times, and random sequences of every length"""
    rng = np.random.default_rng(11)
    seqs = [[r] * k for r in range(16) for k in range(1, 17)] + [[]]
    seqs += [rng.integers(0, 16, int(k)).tolist() for k in rng.integers(0, 17, 400)]
    seqs += [rng.integers(0, 10, 16).tolist() for _ in range(100)]
    return seqs


def pack_ranks(seq):
    return sum(r << (4 * j) for j, r in enumerate(seq))


# ---------------------------------------------------------------------------------------------------------------------
# one wavefront, one workgroup, the scans
# ---------------------------------------------------------------------------------------------------------------------
M64 = 2 ** 64 - 1


def wave_sum_cases():
    rng = np.random.default_rng(12)
    c = [np.full(64, 0xFFFFFFFF, np.uint64), np.full(64, M64, np.uint64), np.zeros(64, np.uint64), np.full(64, 1 << 58, np.uint64),
         np.r_[np.uint64(M64), np.ones(63, np.uint64)], np.arange(64, dtype=np.uint64) << np.uint64(26)]
    c += [rng.integers(0, 2 ** 64, 64, dtype=np.uint64) for _ in range(10)]
    c += [rng.integers(2 ** 31, 2 ** 32, 64, dtype=np.uint64) for _ in range(10)]                 # (every addition carries across bit 32)
    return c


def f64_cases():
    """finite values and infinities (no NaN), the extremes in every lane once"""
    rng = np.random.default_rng(13)
    c = []
    for i in range(64):
        v = rng.normal(0.0, 1e6, 64)
        v[i] = -1e300 if i % 2 else 1e300
        if (i * 7 + 3) % 64 != i:
            v[(i * 7 + 3) % 64] = [np.inf, -np.inf, 1e-300, -1e-300][i % 4]
        c.append(v)
    c += [np.full(64, np.inf), np.full(64, -np.inf), np.full(64, 2.5), np.r_[np.full(63, np.inf), -np.inf], rng.normal(0, 1, 64) * 1e-9 + 1.0]
    return c


def marker_case():
    """64 doubles as bit patterns: NaNs with payloads, infinities, zeros, denormals, random bits"""
    rng = np.random.default_rng(14)
    v = rng.integers(0, 2 ** 64, 64, dtype=np.uint64)
    v[:10] = np.array([0x7FF8000000000001, 0xFFF8DEADBEEF0123, 0x7FF0000000000001, 0x7FF0000000000000, 0xFFF0000000000000, 0x0, 0x8000000000000000,
                       0x0000000000000001, 0x00000001FFFFFFFF, 0xFFFFFFFF00000000], np.uint64)
    return v


def ion_scan_cases():
    """values below 2^50 whose low 24 bits carry into the rest"""
    rng = np.random.default_rng(15)
    c = [np.full(64, 2 ** 50 - 1, np.uint64), np.full(64, 2 ** 24 - 1, np.uint64), np.full(64, 2 ** 24, np.uint64), np.zeros(64, np.uint64),
         np.r_[np.uint64(2 ** 50 - 1), np.zeros(63, np.uint64)], np.r_[np.zeros(63, np.uint64), np.uint64(2 ** 50 - 1)]]
    c += [rng.integers(0, 2 ** 50, 64, dtype=np.uint64) for _ in range(10)]
    c += [rng.integers(2 ** 23, 2 ** 24, 64, dtype=np.uint64) | (rng.integers(0, 2 ** 26, 64, dtype=np.uint64) << np.uint64(24)) for _ in range(10)]
    return c


def hist_wave_cases():
    """64 lanes x 3 words whose 16-bit fields sum to exactly 65 535 (or stay 0) over the wave"""
    rng = np.random.default_rng(16)
    cases = []
    for k in range(12):
        words = np.zeros((3, 64), np.uint64)
        for w in range(3):
            for fld in range(4 if w < 2 else 2):
                if k and rng.random() < 0.3:
                    continue                                 # (an empty field beside a full one)
                if k % 3 == 0:
                    part = rng.multinomial(65535, np.ones(64) / 64)
                elif k % 3 == 1:
                    part = np.zeros(64, np.int64)
                    part[rng.integers(64)] = 65535
                else:
                    part = np.full(64, 1023, np.int64)
                    part[rng.integers(64)] += 63
                assert part.sum() == 65535
                words[w] += part.astype(np.uint64) << np.uint64(16 * fld)
        cases.append(words)
    return cases


def same_digit_cases():
    rng = np.random.default_rng(17)
    c = []
    for k in range(24):
        pool = rng.integers(0, 256, [1, 2, 3, 8, 64, 256][k % 6])
        d = rng.choice(pool, 64).astype(np.uint64)
        inn = (rng.random(64) < [1.0, 0.9, 0.5, 0.0][k % 4]).astype(np.uint64)
        c.append((d, inn))
    c.append((np.arange(64, dtype=np.uint64) * np.uint64(4) + np.uint64(1), np.ones(64, np.uint64)))
    c.append(((np.uint64(1) << (np.arange(64, dtype=np.uint64) % np.uint64(8))), np.ones(64, np.uint64)))
    return c


def same_digit_ref(d, inn):
    return np.array([sum(1 << j for j in range(64) if inn[j] and d[j] == d[l]) for l in range(64)], np.uint64)


def seg_entries(n, rng, p_flag):
    """n entries (v, f, last) of the segmented policy: last = a tag that is never 0 where f, else 0"""
    v = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    f = (rng.random(n) < p_flag).astype(np.uint32)
    last = np.where(f != 0, rng.integers(1, 2 ** 32, n, dtype=np.uint64).astype(np.uint32), np.uint32(0))
    return np.ascontiguousarray(np.stack([v, f, last], axis=1))


def seg_op(a, b):
    """a before b"""
    return ((b[0] if b[1] else (a[0] + b[0]) & 0xFFFFFFFF), a[1] | b[1], b[2] if b[1] else a[2])


def seg_fold(entries):
    """the exclusive scan of the entries by the sequential fold from (0, 0, 0), and the total"""
    out = np.zeros((len(entries), 3), np.uint32)
    acc = (0, 0, 0)
    for i, e in enumerate(entries.tolist()):
        out[i] = acc
        acc = seg_op(acc, e)
    return out, np.array(acc, np.uint32)


def add_fold(v):
    """the exclusive 32-bit sums, and the total"""
    inc = np.cumsum(v.astype(np.uint64)) & np.uint64(0xFFFFFFFF)
    return np.r_[np.uint64(0), inc[:-1]].astype(np.uint32), np.uint32(inc[-1])


IONS_SCAN_N = (1, 1023, 1024, 1025, 65535, 65536, 65537, 66561, 200000)
IONS_SCAN_WIDE_N = 65537                                   # counts up to 2^17: the total passes 2^32
TS_SCAN_N = (1, 255, 256, 257, 65535, 65536, 65537, 70001)


def ions_counts(n, wide=False):
    rng = np.random.default_rng([18, n, int(wide)])
    return rng.integers(0, 2 ** 17 if wide else 9, n).astype(np.int64)


def ions_scan_ref(counts):
    """offsets [n + 1]: the counts before every entry, then all of them"""
    inc = np.cumsum(counts.astype(np.uint64))
    return np.r_[np.uint64(0), inc].astype(np.int64)
