"""Spectra aimed at the m/z edges of the binning stage -- TEST INFRASTRUCTURE shared by tests/test_binning_edges_host.py
(CPU copies of the window arithmetic against the reference's) and tests/test_gpu_binning_table.py (the device's
retained table against the reference's).

The reference bins a spectrum as (cpp/Spectra.cpp:43-68)
    min_mz = float(floor(min / 100.) * 100.),  max_mz = float(ceil(max / 100.) * 100.)     -- double divisions
    n_bins = ceil((max_mz - min_mz) / bin_size)                                             -- FLOAT division
    window = min(floor((mz - min_mz) / bin_size), n_bins - 1)                               -- double division
and keeps the n_top most intense peaks of every window.  A retained-table entry carries no window id, so a spectrum here
is built to make a peak on the wrong side of a border VISIBLE in the table: every populated window holds more than n_top
filler peaks, windows alternate between "bright" (fillers 1 000 .. 2 000) and "dim" (10 .. 20), and the peaks put on and
next to the borders have intensity ~500 -- retained with a high rank in a dim window, dropped from a bright one.

Every generator is deterministic (seeded) and returns a list of (settings, list of psm dicts, note).  A psm dict is what
synth.pack_batch takes; `expect_status` (PYA_PSM_NO_WINDOWS / PYA_PSM_TOO_MANY_WINDOWS), where present, marks a spectrum
the reference cannot be asked about (undefined behaviour, or beyond this library's 65 535 windows): status only.
Non-finite m/z or intensities are out of scope."""
import math
from fractions import Fraction

import numpy as np

from pyascore_amd import synth

BASE = dict(bin_size=100.0, n_top=10, mod_group="STY", mod_mass=79.966331, mz_error=0.5, fragment_types="by",
            neutral_losses=[])
PEPTIDES = ("AASPTYEKLR", "GSLTPEVYKM", "MKTAYIAKQR", "LSDEGHTPWK")
BRIGHT, DIM, EDGE = 1000.0, 10.0, 500.0


def f32(x):
    """the double that the float32 nearest to x widens to (a scorer's bin_size is a float)"""
    return float(np.float32(x))


def step(v, j, narrow=False):
    """v moved by j ulps: double ulps, or float32 ulps of the value rounded to float32 (then widened)"""
    t = np.float32 if narrow else np.float64
    v = t(v)
    for _ in range(abs(j)):
        v = np.nextafter(v, t(np.inf if j > 0 else -np.inf))
    return float(v)


def n_bins_float(span, bin_size):
    """window count as the reference computes it: float32 quotient of two floats, then ceil"""
    return int(np.ceil(np.float32(span) / np.float32(bin_size)))


def n_bins_exact(span, bin_size):
    """... and what the exact quotient of the same two floats gives"""
    return math.ceil(Fraction(float(np.float32(span))) / Fraction(f32(bin_size)))


def search_nbins_pairs(n_lo, n_hi, spans=range(100, 3100, 100), count=12):
    """(bin_size, span) pairs whose FLOAT quotient rounds across an integer, so that the reference's n_bins is one less
    than the exact ceil and the top of the span is clamped into the last window: bin_size = float32(span / n) and its float
    neighbours, n_lo <= float n_bins <= n_hi.  Brute force; `count` of the hits, spread evenly, in search order.  The two
    committed lists below are this function's output (test_binning_edges_host.py regenerates them)."""
    hits = []
    for span in spans:
        for n in range(n_lo, n_hi + 2):
            for d in (-2, -1, 0, 1, 2):
                bs = step(np.float32(span / n), d, narrow=True)
                nf = n_bins_float(span, bs)
                if nf != n_bins_exact(span, bs) and n_lo <= nf <= n_hi:
                    hits.append((bs, span))
    hits = sorted(set(hits), key=hits.index)
    pick = np.linspace(0, len(hits) - 1, count).astype(int)
    return [hits[i] for i in pick]


# search_nbins_pairs(2, 64) and search_nbins_pairs(65, 400)
NBINS_PAIRS_SMALL = ((33.33333206176758, 100), (4.255319118499756, 200), (7.017543792724609, 400), (15.217391014099121, 700),
                     (52.63157653808594, 1000), (23.52941131591797, 1200), (145.4545440673828, 1600), (633.3333129882812, 1900),
                     (35.59321975708008, 2100), (208.3333282470703, 2500), (215.38461303710938, 2800), (48.3870964050293, 3000))
NBINS_PAIRS_LARGE = ((1.5151515007019043, 100), (0.9009009003639221, 300), (2.6315789222717285, 600), (6.5217390060424805, 900),
                     (3.2738094329833984, 1100), (4.8109965324401855, 1400), (7.142857074737549, 1700), (13.793103218078613, 2000),
                     (6.0439558029174805, 2200), (11.627906799316406, 2500), (18.18181800842285, 2800), (7.518796920776367, 3000))


def psm(mz, intensity, j=0, **extra):
    mz, intensity = np.ascontiguousarray(mz, np.float64), np.ascontiguousarray(intensity, np.float64)
    assert mz.size == intensity.size and np.all(np.isfinite(mz)) and np.all(np.isfinite(intensity))
    return dict(mz=mz, intensity=intensity, peptide=PEPTIDES[j % len(PEPTIDES)], n_of_mod=1 + j % 2, max_charge=1 + (j // 2) % 2,
                **extra)


def _populated(rng, n):
    """the windows that get filler: all of up to 64, else runs of neighbours at both ends, around the fast kernels' 64
    and somewhere in the middle"""
    if n <= 64:
        return list(range(n))
    mid = int(rng.integers(70, max(71, n - 8)))
    runs = list(range(0, 4)) + list(range(61, 67)) + list(range(mid, mid + 4)) + list(range(n - 4, n))
    return sorted({k for k in runs if 0 <= k < n})


def dense(seed, lo, hi, bin_size, per_window=13, narrow=False, tie=False, first_bright=True, lo_edge="at", hi_edge="at"):
    """One spectrum (m/z ascending) meant to get the bounds [lo, hi] (multiples of 100): filler in every populated window,
    five peaks around every border between populated windows (border + j ulps, j = -2 .. 2; float32 ulps of float32 values
    when `narrow`), the stretch the float window count cuts off included.  lo_edge / hi_edge: the lowest / highest peak
    exactly "at" the bound, one ulp "inside" it, or (any other value) a few m/z inside."""
    rng = np.random.default_rng(seed)
    bsd = f32(bin_size)
    n_math = n_bins_exact(hi - lo, bin_size)                 # windows the span has room for
    windows = _populated(rng, n_math)
    mz, it = [lo + 3.7, hi - 4.1], [EDGE, EDGE]              # (anchors: the bounds do not depend on where the filler falls)
    for k in windows:
        a, b = lo + k * bsd, min(lo + (k + 1) * bsd, float(hi))
        x = np.clip(a + (b - a) * (0.1 + 0.8 * rng.random(per_window)), lo + 1e-3, hi - 1e-3)
        level = BRIGHT if (k % 2 == 0) == first_bright else DIM
        mz.extend(x)
        it.extend(np.full(per_window, level) if tie else level * (1.0 + rng.random(per_window)))
    for k in sorted({k for w in windows for k in (w, w + 1)}):
        c = float(Fraction(lo) + k * Fraction(bsd))
        c = min(c, float(hi))
        for j in range(-2, 3):
            v = step(c, j, narrow)
            if v < lo or v > hi:
                continue
            if v == lo and lo_edge != "at" or v == hi and hi_edge != "at":
                continue
            if lo_edge not in ("at", "inside") and v < lo + 1. or hi_edge not in ("at", "inside") and v > hi - 1.:
                continue
            mz.append(v)
            it.append(EDGE if tie else EDGE + 7.0 * j + 0.5 * (k % 5))
    mz, it = np.asarray(mz), np.asarray(it)
    if narrow:
        mz = mz.astype(np.float32).astype(np.float64)
        mz = np.clip(mz, lo, hi)
    o = np.argsort(mz, kind="stable")
    return mz[o], it[o]


def _settings(bin_size):
    return dict(BASE, bin_size=f32(bin_size))


# ---- the families ----------------------------------------------------------------------------------------------------

def borders():
    """for every border k of up to 64 windows: peaks at min_mz + k * bin_size + j ulp, j = -2 .. 2, among dense filler"""
    out = []
    for i, (bs, lo, hi) in enumerate([(100.0, 400, 1200), (50.0, 300, 1000), (25.0, 400, 900), (10.0, 0, 600),
                                      (np.float32(100 / 3), 400, 1100), (np.float32(7.7), 1300, 1700)]):
        psms = []
        for j, (narrow, fb) in enumerate([(False, True), (False, False), (True, True), (True, False)]):
            m, t = dense(1000 + 10 * i + j, lo, hi, bs, narrow=narrow, first_bright=fb)
            psms.append(psm(m, t, j))
        out.append((_settings(bs), psms, "borders bin_size %r [%d, %d]" % (f32(bs), lo, hi)))
    return out


BIN_SIZES = [(100.0, 1200), (50.0, 1000), (150.0, 1300), (25.0, 900), (10.0, 1000), (2000.0, 2300), (1e6, 2300),
             (np.float32(100 / 3), 500), (np.float32(100 / 3), 1000), (np.float32(100 / 7), 500), (np.float32(0.7), 1100),
             (np.float32(7.7), 800), (np.float32(99.99), 1400), (np.float32(100.01), 1400), (np.float32(0.1), 500),
             (4.761904716491699, 700), (4.615384578704834, 700)]    # (the last two: 63 and 65 windows in float, 64 and 66 exactly)


def bin_sizes():
    """the window widths: exact in float and not, divisors of 100 and not, and the (bin_size, span) pairs whose float
    window count is one less than the exact one -- each with peaks in the stretch that is cut off"""
    out = []
    todo = [(bs, 400, hi) for bs, hi in BIN_SIZES]
    todo += [(bs, 400 + 100 * (i % 7), 400 + 100 * (i % 7) + span) for i, (bs, span) in enumerate(NBINS_PAIRS_SMALL + NBINS_PAIRS_LARGE)]
    for i, (bs, lo, hi) in enumerate(todo):
        psms = []
        for j, (narrow, edges) in enumerate([(False, ("at", "at")), (False, ("inside", "inside")), (True, ("at", "at")), (False, ("in", "in"))]):
            m, t = dense(2000 + 10 * i + j, lo, hi, bs, narrow=narrow, first_bright=bool((i + j) % 2), lo_edge=edges[0],
                         hi_edge=edges[1])
            psms.append(psm(m, t, j))
        out.append((_settings(bs), psms, "bin_size %r [%d, %d]: %d windows in float, %d exactly"
                    % (f32(bs), lo, hi, n_bins_float(hi - lo, bs), n_bins_exact(hi - lo, bs))))
    return out


def extremes():
    """lowest / highest m/z on a multiple of 100 and one ulp to either side, tiny spectra, a span under 100, one m/z for
    all peaks; min == max == 100 k has no windows (status 1)"""
    out = []
    for bs in (100.0, 50.0, np.float32(100 / 3)):
        psms, names = [], []
        for narrow in (False, True):
            for fb in (True, False):
                m, t = dense(3000 + fb, 400, 1200, bs, narrow=narrow, first_bright=fb)           # lowest at 400, highest at 1200
                for name, extra in [("at", []), ("low-1", [step(400., -1, narrow)]), ("high+1", [step(1200., 1, narrow)]),
                                    ("both", [step(400., -1, narrow), step(1200., 1, narrow)])]:
                    mm = np.concatenate([m, extra])
                    tt = np.concatenate([t, np.full(len(extra), EDGE + 1.0)])
                    o = np.argsort(mm, kind="stable")
                    psms.append(psm(mm[o], tt[o], len(psms)))
                    names.append(name)
                for le, he in (("inside", "at"), ("at", "inside"), ("inside", "inside")):   # one ulp above 400 / below 1200
                    m2, t2 = dense(3010 + fb, 400, 1200, bs, narrow=narrow, first_bright=fb, lo_edge=le, hi_edge=he)
                    psms.append(psm(m2, t2, len(psms)))
        out.append((_settings(bs), psms, "extremes on and next to multiples of 100, bin_size %r" % f32(bs)))
    rng = np.random.default_rng(3100)
    small = [np.sort(412.3 + 57.8 * rng.random(40)), np.full(20, 512.3), [512.3], [step(500., 1)], [step(500., -1)],
             [450.5, 451.5], [400., 500.], [0., 100.], [399.99, 400.], [500., step(500., 1)], np.full(3, step(700., -1, True))]
    for bs in (100.0, 25.0, 10.0):
        psms = [psm(m, 100.0 + 50.0 * rng.random(len(m)), j) for j, m in enumerate(small)]
        out.append((_settings(bs), psms, "tiny spectra and spans under 100, bin_size %r" % bs))
    none = [[500.], np.full(5, 500.), [0.], np.full(2, 1200.)]
    psms = [psm(m, 100.0 + np.arange(len(m)), j, expect_status=1) for j, m in enumerate(none)]
    psms = [psm(*dense(3200, 400, 1200, 100.0), 0)] + psms + [psm(*dense(3201, 500, 900, 100.0, narrow=True), 1)]
    out.append((_settings(100.0), psms, "min == max == 100 k: no windows (between two spectra that are fine)"))
    return out


def window_counts(large=False):
    """1 .. 257 windows, or (large) 4 096 .. 65 535 -- the most the library takes"""
    out = []
    if not large:
        todo = [(100.0, 100 * n) for n in (1, 2, 63, 64, 65, 255, 256, 257)]
        todo += [(25.0, 1600), (25.0, 1700), (12.5, 800), (12.5, 700), (0.390625, 100), (np.float32(1600 / 63), 1600)]
    else:
        todo = [(100.0, 409600), (100.0, 6553400), (100.0, 6553500), (1.0, 4100), (1.0, 65500), (0.5, 32700), (np.float32(0.1), 6500)]
    for i, (bs, span) in enumerate(todo):
        psms = []
        for j, narrow in enumerate((False, True)):
            m, t = dense(4000 + 10 * i + j, 400, 400 + span, bs, narrow=narrow, first_bright=bool(j))
            psms.append(psm(m, t, j))
        out.append((_settings(bs), psms, "%d windows (bin_size %r, span %d)" % (n_bins_float(span, bs), f32(bs), span)))
    return out


def too_many_windows():
    """65 536 windows and more: status 2.  Every batch is [a spectrum that is fine, one with too many windows, another fine
    one]"""
    out = []
    for i, (bs, span) in enumerate([(100.0, 6553600), (1.0, 65600), (np.float32(0.1), 6600), (np.float32(0.01), 700)]):
        assert n_bins_float(span, bs) > 65535
        ok = max(100, span // 200 // 100 * 100)
        rng = np.random.default_rng(4500 + i)
        bad = np.sort(np.concatenate([[400.5, 400.0 + span - 0.5], 400.0 + span * rng.random(300)]))
        psms = [psm(*dense(4510 + i, 400, 400 + ok, bs), 0), psm(bad, 100.0 + rng.random(bad.size), 1, expect_status=2),
                psm(*dense(4520 + i, 700, 700 + ok, bs, first_bright=False), 2)]
        assert n_bins_float(ok, bs) <= 65535
        out.append((_settings(bs), psms, "%d windows beside %d" % (n_bins_float(span, bs), n_bins_float(ok, bs))))
    return out


def order():
    """peak order: ascending; descending; the ends in order but the true extremes in the middle (the bounds must come from
    min / max, not from the ends); shuffled -- each with and without equal intensities inside the windows"""
    out = []
    for bs in (100.0, 25.0):
        psms = []
        for tie in (False, True):
            m, t = dense(5000 + tie, 400, 1200, bs, tie=tie)
            m = np.concatenate([[step(400., -1)], m, [step(1200., 1)]])         # (the extremes decide the bounds: [300, 1300])
            t = np.concatenate([[EDGE], t, [EDGE]])
            n = m.size
            mid = n // 2
            rng = np.random.default_rng(5010 + tie)
            orders = [np.arange(n), np.arange(n)[::-1], np.concatenate([np.arange(1, mid), [0, n - 1], np.arange(mid, n - 1)]),
                      rng.permutation(n)]
            for o in orders:
                psms.append(psm(m[o], t[o], len(psms)))
        out.append((_settings(bs), psms, "peak order x ties, bin_size %r" % bs))
    return out


def intensity_variants(it, peak_off, seed=9):
    """The intensity-axis regimes of tests/test_gpu_parity.py (test_binning_keys_and_their_hand_overs,
    test_equal_intensities_follow_nth_element), built the way those tests build them."""
    rng = np.random.default_rng(seed)
    ulp = np.spacing(it)
    near = it.copy()                                          # pairs a few ulps apart: equal keys, different doubles
    idx = rng.permutation(it.size)
    half = it.size // 2
    near[idx[:half]] = np.floor(it[idx[:half]] / 64.0) * 64.0 + 1.0
    near[idx[:half]] += ulp[idx[:half]] * rng.integers(0, 4, half)
    top = it.copy()                                           # the most intense peaks of every spectrum a few ulps apart
    for a, b in zip(peak_off[:-1], peak_off[1:]):
        sel = a + np.argsort(it[a:b])[::-1][:40]
        top[sel] = 50000.0 + np.spacing(50000.0) * rng.integers(0, 6, sel.size)
    wide = it.copy()
    wide[idx[: it.size // 5]] = 0.0
    wide[idx[it.size // 5: it.size // 4]] = 5e-324
    wide[idx[it.size // 4: it.size // 3]] *= 1e-30
    wide[idx[it.size // 3: it.size // 2]] *= 1e30
    neg = it.copy()
    neg[idx[: it.size // 10]] *= -1.0
    neg[idx[it.size // 10: it.size // 8]] = -0.0
    return {"near": near, "top": top, "wide": wide, "negative": neg, "coarse": np.floor(it / np.median(it) * 3.0) + 1.0,
            "counts": np.floor(it / np.median(it) * 40.0) + 1.0, "flat": np.ones_like(it)}


def intensity_axis():
    """cfg2's synthetic spectra under every intensity regime: checked at table level too"""
    batch, settings = synth.make_batch("cfg2", n_psm=16, seed=4242)
    out = []
    for name, inten in intensity_variants(batch["intensity"], batch["peak_off"]).items():
        b2 = dict(batch, intensity=inten)
        psms = []
        for i in range(batch["n_psm"]):
            kw = synth.unpack_psm(b2, i)
            psms.append(dict(mz=kw["mz_arr"], intensity=kw["int_arr"], peptide=kw["peptide"], n_of_mod=kw["n_of_mod"],
                             max_charge=kw["max_fragment_charge"]))
        out.append((settings, psms, "intensities: %s" % name))
    return out


FAMILIES = {"borders": borders, "bin_sizes": bin_sizes, "extremes": extremes, "window_counts": window_counts, "order": order,
            "intensity_axis": intensity_axis}


def cases(family):
    """[(id, settings, psms, note)] of one family (or of the large window counts / the too-many-windows batches)"""
    if family == "window_counts_large":
        made = window_counts(large=True)
    elif family == "too_many_windows":
        made = too_many_windows()
    else:
        made = FAMILIES[family]()
    return [("%s/%d" % (family, i), s, p, note) for i, (s, p, note) in enumerate(made)]


def expected_status(settings, mz):
    """0, PYA_PSM_NO_WINDOWS (1) or PYA_PSM_TOO_MANY_WINDOWS (2) of a spectrum, from the definition at the top.  Narrowing a
    spectrum to float32 can change it (500 + 1 ulp becomes 500: a one-peak spectrum loses its window), and with no windows
    the reference writes out of bounds: it is asked only where this says 0 or 2."""
    mz = np.asarray(mz, np.float64)
    lo, hi = np.float32(np.floor(mz.min() / 100.) * 100.), np.float32(np.ceil(mz.max() / 100.) * 100.)
    nb = np.ceil((hi - lo) / np.float32(settings["bin_size"]))
    return 1 if nb < 1 else (2 if nb > 65535 else 0)


# ---- the reference's table of one spectrum --------------------------------------------------------------------------------

def reference_binned(settings, mz, intensity, kind="ref"):
    """orc_binned of one spectrum through oracle/_ref (or oracle/ascore_oracle.cpp): dict(mz, intensity, bin, rank, min_mz,
    max_mz, n_bins), retained peaks in (window, rank) order"""
    from oracle import harness, orc
    chk = harness.make_scorer(orc.OracleAscore, settings, kind=kind)
    chk.consume_spectra(np.ascontiguousarray(mz, np.float64), np.ascontiguousarray(intensity, np.float64))
    return chk.binned(cap=max(65536, len(mz)))


def expected_table(binned):
    """the retained table the device must hold: (float32 m/z, rank) sorted by (m/z, rank)"""
    m, r = binned["mz"].astype(np.float32), binned["rank"].astype(np.uint32)
    o = np.lexsort((r, m))
    return m[o], r[o]
