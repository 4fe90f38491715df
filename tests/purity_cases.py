"""Hand-made cases of the precursor-purity stage in exact binary numbers, and the inputs the host and the GPU tests share.

The numbers: step 1.0 at charge 2 is a spacing of 0.5; tol = 2^-7; the precursor at 500.0; the isolation window 499.25 .. 501.25.
Every centre, bound and intensity is a short binary fraction, so every expected record below was written down by hand and holds
bit for bit."""
import math

import numpy as np

from pyascore_amd import rollup as ru

T = 2.0 ** -7
PM, Z = 500.0, 2
WL, WH = 499.25, 501.25
P_BASE = ru.purity_params(tol=T, tol_ppm=0.0, isotopes=2, below=0, step=1.0)        # centres 500.0, 500.5, 501.0
P_ONE = ru.purity_params(tol=T, tol_ppm=0.0, isotopes=0, below=0, step=1.0)         # n_c = 1
P_16 = ru.purity_params(tol=T, tol_ppm=0.0, isotopes=11, below=4, step=1.0)         # 16 centres: 498.0 .. 505.5
P_WIDE = ru.purity_params(tol=0.5, tol_ppm=0.0, isotopes=2, below=0, step=1.0)      # neighbouring centre windows overlap
BOUNDARY_LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 4097)
NAN, INF = float("nan"), float("inf")


def up(x, t=np.float64):
    return float(np.nextafter(t(x), t(np.inf)))


def down(x, t=np.float64):
    return float(np.nextafter(t(x), t(-np.inf)))


def _case(name, params, peaks, record, query=(0, PM, Z, WL, WH), f64_only=False):
    return dict(name=name, params=params, peaks=[(float(x), float(y)) for x, y in peaks], query=query, record=record, f64_only=f64_only)


def _edges(t):
    """peaks at win_lo, win_hi, lo_1, hi_1 and one ulp of type ``t`` to either side"""
    lo1, hi1 = 500.5 - T, 500.5 + T
    window = [(down(WL, t), 1.0), (WL, 2.0), (up(WL, t), 4.0), (down(WH, t), 8.0), (WH, 16.0), (up(WH, t), 32.0)]
    centre = [(down(lo1, t), 1.0), (lo1, 2.0), (up(lo1, t), 4.0), (down(hi1, t), 8.0), (hi1, 16.0), (up(hi1, t), 32.0)]
    return window, centre, up(hi1, t)


def hand_cases():
    """[dict(name, params, peaks [(x, y)] in index order, query (survey 0 | -1, prec_mz, prec_z, win_lo, win_hi), record, f64_only)]:
    ``record`` is the expected pya_purity as a tuple in field order, pinned by hand; ``f64_only``: the m/z of the case do not fit
    float32 (every other case holds float32 values only, m/z and intensities)"""
    cases = []
    for t, f32 in ((np.float64, False), (np.float32, True)):
        tag = " (float32)" if f32 else ""
        window, centre, above_hi1 = _edges(t)
        # inside: win_lo, its upper neighbour, win_hi's lower neighbour, win_hi: 2 + 4 + 8 + 16; no centre is near
        cases.append(_case("peaks at the window bounds and one ulp to either side" + tag, P_BASE, window,
                           (30.0, 0.0, WH, 16.0, 4, 0, 0, 1), f64_only=not f32))
        # all six inside the window; in centre 1: lo_1, its upper neighbour, hi_1's lower neighbour, hi_1; the other two are others
        cases.append(_case("peaks at the bounds of centre 1 and one ulp to either side" + tag, P_BASE, centre,
                           (63.0, 30.0, above_hi1, 32.0, 6, 4, 2, 3), f64_only=not f32))
    cases += [
        _case("a centre outside the isolation window gets nothing", P_BASE, [(500.0, 4.0), (500.5, 8.0), (500.125, 2.0)],
              (6.0, 4.0, 500.125, 2.0, 2, 1, 1, 3), query=(0, PM, Z, 499.75, 500.25)),
        _case("one peak in two centre windows counts once", P_WIDE, [(500.25, 4.0), (500.5, 2.0)], (6.0, 6.0, 0.0, 0.0, 2, 2, 7, 3)),
        _case("a NaN m/z; NaN, zero and negative intensities", P_BASE,
              [(NAN, 4.0), (500.0, NAN), (500.0, 0.0), (500.0, -1.0), (500.25, -0.0), (500.0, 2.0), (500.25, -INF)],
              (2.0, 2.0, 0.0, 0.0, 1, 1, 1, 3)),
        _case("an empty window", P_BASE, [(499.0, 1.0), (502.0, 1.0)], (0.0, 0.0, 0.0, 0.0, 0, 0, 0, 1)),
        _case("no peaks at all", P_BASE, [], (0.0, 0.0, 0.0, 0.0, 0, 0, 0, 1)),
        _case("a window of one point", P_BASE, [(500.0, 1.0), (500.5, 2.0)], (2.0, 2.0, 0.0, 0.0, 1, 1, 2, 3), query=(0, PM, Z, 500.5, 500.5)),
        _case("win_lo > win_hi", P_BASE, [(500.0, 1.0)], (0.0,) * 4 + (0,) * 4, query=(0, PM, Z, WH, WL)),
        _case("a NaN bound", P_BASE, [(500.0, 1.0)], (0.0,) * 4 + (0,) * 4, query=(0, PM, Z, NAN, WH)),
        _case("an infinite bound", P_BASE, [(500.0, 1.0)], (0.0,) * 4 + (0,) * 4, query=(0, PM, Z, WL, INF)),
        _case("charge 0", P_BASE, [(500.0, 1.0)], (0.0,) * 4 + (0,) * 4, query=(0, PM, 0, WL, WH)),
        _case("charge 9", P_BASE, [(500.0, 1.0)], (0.0,) * 4 + (0,) * 4, query=(0, PM, 9, WL, WH)),
        _case("a NaN precursor", P_BASE, [(500.0, 1.0)], (0.0,) * 4 + (0,) * 4, query=(0, NAN, Z, WL, WH)),
        _case("a negative precursor", P_BASE, [(500.0, 1.0)], (0.0,) * 4 + (0,) * 4, query=(0, -500.0, Z, WL, WH)),
        _case("an infinite precursor", P_BASE, [(500.0, 1.0)], (0.0,) * 4 + (0,) * 4, query=(0, INF, Z, WL, WH)),
        _case("survey = -1", P_BASE, [(500.0, 1.0)], (0.0,) * 4 + (0,) * 4, query=(-1, PM, Z, WL, WH)),
        _case("charge 8 is a precursor", P_BASE, [(500.0, 1.0), (500.125, 2.0), (500.25, 4.0), (500.375, 8.0)],
              (15.0, 7.0, 500.375, 8.0, 4, 3, 7, 3), query=(0, PM, 8, WL, WH)),
        # 16 centres 498.0, 498.5, .. 505.5, a peak of 1.0 on each, one of 0.5 between two
        _case("below = 4 with isotopes = 11", P_16, [(498.0 + 0.5 * k, 1.0) for k in range(16)] + [(500.25, 0.5)],
              (16.5, 16.0, 500.25, 0.5, 17, 16, 0xFFFF, 3), query=(0, PM, Z, 497.75, 505.75)),
        _case("below = 4: the centres under the selected m/z alone", P_16, [(498.0, 1.0), (499.5, 2.0), (499.75, 4.0)],
              (7.0, 3.0, 499.75, 4.0, 3, 2, 0b1001, 3), query=(0, PM, Z, 497.75, 499.875)),
        _case("n_c = 1", P_ONE, [(500.0, 1.0), (500.5, 2.0)], (3.0, 1.0, 500.5, 2.0, 2, 1, 1, 3)),
        _case("the other peak: the larger y wins", P_BASE, [(500.125, 3.0), (500.25, 4.0), (500.375, 1.0)],
              (8.0, 0.0, 500.25, 4.0, 3, 0, 0, 1)),
        _case("the other peak: with equal y the smaller x, the larger x first", P_BASE, [(500.25, 4.0), (500.125, 4.0), (500.375, 3.0)],
              (11.0, 0.0, 500.125, 4.0, 3, 0, 0, 1)),
        _case("the other peak: with equal y the smaller x, the smaller x first", P_BASE, [(500.125, 4.0), (500.25, 4.0)],
              (8.0, 0.0, 500.125, 4.0, 2, 0, 0, 1)),
        _case("a duplicate peak", P_BASE, [(500.25, 4.0), (500.0, 2.0), (500.25, 4.0), (500.0, 2.0)], (12.0, 4.0, 500.25, 4.0, 4, 2, 1, 3)),
        # 2^53 + 1 rounds back to 2^53 (ties to even), twice; the other order gives 2^53 + 2
        _case("the sums run in index order: the large term first", P_BASE, [(500.0, 2.0 ** 53), (500.0, 1.0), (500.0, 1.0)],
              (2.0 ** 53, 2.0 ** 53, 0.0, 0.0, 3, 3, 1, 3)),
        _case("the sums run in index order: the large term last", P_BASE, [(500.0, 1.0), (500.0, 1.0), (500.0, 2.0 ** 53)],
              (2.0 ** 53 + 2.0, 2.0 ** 53 + 2.0, 0.0, 0.0, 3, 3, 1, 3)),
        _case("m/z that do not ascend", P_BASE, [(501.0, 1.0), (499.0, 8.0), (500.5, 2.0), (500.75, 4.0), (500.0, 16.0)],
              (23.0, 19.0, 500.75, 4.0, 4, 3, 7, 3)),
    ]
    return cases


def params_key(p):
    return tuple(sorted(p.items()))


def pack(spectra, mz_t=np.float64, it_t=np.float64):
    """[(x, y)] spectra (arrays or lists) as (mz, intensity, peak_off)"""
    lens = [len(s[0]) for s in spectra]
    mz = np.concatenate([np.asarray(s[0], np.float64) for s in spectra] + [np.zeros(0)]).astype(mz_t)
    it = np.concatenate([np.asarray(s[1], np.float64) for s in spectra] + [np.zeros(0)]).astype(it_t)
    return mz, it, np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def pack_cases(cases, mz_t=np.float64, it_t=np.float64, gaps=True):
    """the cases of one parameter set as one call: case i is survey spectrum 2 i (an empty one behind each) or i.  Returns
    (mz, it, off, survey, prec_mz, prec_z, win_lo, win_hi)"""
    spectra, sv, pm, pz, wl, wh = [], [], [], [], [], []
    for c in cases:
        s, a, b, lo, hi = c["query"]
        sv.append(len(spectra) if s >= 0 else s)
        spectra.append(([p[0] for p in c["peaks"]], [p[1] for p in c["peaks"]]))
        if gaps:
            spectra.append(([], []))
        pm.append(a), pz.append(b), wl.append(lo), wh.append(hi)
    mz, it, off = pack(spectra, mz_t, it_t)
    return mz, it, off, np.asarray(sv, np.int64), np.asarray(pm), np.asarray(pz, np.int32), np.asarray(wl), np.asarray(wh)


def as_lists(mz, it, off):
    """packed spectra as the lists tests/purity_ref.py takes (float32 widened: exact)"""
    x, y = np.asarray(mz, np.float64).tolist(), np.asarray(it, np.float64).tolist()
    return [list(zip(x[a:b], y[a:b])) for a, b in zip(off[:-1].tolist(), off[1:].tolist())]


def as_queries(sv, pm, pz, wl, wh):
    return list(zip(np.asarray(sv).tolist(), np.asarray(pm, np.float64).tolist(), np.asarray(pz).tolist(), np.asarray(wl, np.float64).tolist(),
                    np.asarray(wh, np.float64).tolist()))


def boundary_spectra(seed=0):
    """Survey spectra of BOUNDARY_LENGTHS peaks whose background lies outside the window WL .. WH and whose window peaks are
    planted as the first and the last peak and on both sides of every 64-peak boundary: (spectra, planted index lists).  The
    planted peaks alternate between centre positions and others; their intensities are small powers of two."""
    rng = np.random.default_rng(seed)
    spectra, planted = [], []
    inside = (500.0, 500.25, 500.5, 500.75, 501.0, 499.5)
    for n in BOUNDARY_LENGTHS:
        x = np.where(rng.random(n) < 0.5, rng.uniform(300.0, 499.0, size=n), rng.uniform(502.0, 900.0, size=n))
        y = rng.choice([1.0, 2.0, 3.0], size=n)
        at = sorted({k for k in [0, n - 1] + [b + d for b in range(64, n + 1, 64) for d in (-1, 0)] if 0 <= k < n})
        for j, k in enumerate(at):
            x[k] = inside[j % len(inside)]
            y[k] = float(2 ** (j % 5))
        spectra.append((x, y))
        planted.append(at)
    return spectra, planted


def random_inputs(seed, n_survey=12, n_query=60, max_peaks=200, params=None):
    """seeded random survey spectra on a grid of 1/16 m/z around 500 (so that bounds are hit exactly now and then) and queries
    over them, with inactive and out-of-range ones among them"""
    rng = np.random.default_rng(seed)
    spectra = []
    for s in range(n_survey):
        n = int(rng.integers(0, max_peaks))
        x = np.sort(rng.integers(16 * 495, 16 * 507, size=n) / 16.0) + rng.choice([0.0, 0.0, T, -T, 2.0 ** -20], size=n)
        y = rng.choice([0.0, -1.0, 0.5, 1.0, 2.0, 3.0, 1e-3, 12345.678, NAN], size=n, p=[.05, .05, .15, .2, .2, .15, .1, .05, .05])
        spectra.append((x, y))
    sv = rng.integers(-1, n_survey + 1, size=n_query).astype(np.int64)
    pm = rng.integers(16 * 498, 16 * 504, size=n_query) / 16.0
    pz = rng.integers(0, 10, size=n_query).astype(np.int32)
    half = rng.choice([0.0, 0.25, 0.75, 1.0, 2.0], size=n_query)
    wl, wh = pm - half, pm + half * rng.choice([1.0, 1.0, 1.0, -1.0, 0.5], size=n_query)
    wl[rng.random(n_query) < 0.05] = NAN
    pm[rng.random(n_query) < 0.05] = NAN
    sv[3], pm[3], pz[3], wl[3], wh[3] = n_survey, 500.0, 2, 499.0, 501.0            # one active query beyond the survey spectra for sure
    return spectra, (sv, pm, pz, wl, wh)


def planted_scan(n_background=150, seed=5):
    """One survey scan with an isotope envelope at 500.0 / 2+ and interferers inside the window WL .. WH, all intensities sums of
    powers of two, in a background outside the window.  Returns ((x, y), precursor sum, window sum)."""
    rng = np.random.default_rng(seed)
    envelope = [(500.0, 1024.0 + 256.0), (500.5, 512.0 + 64.0), (501.0, 128.0 + 32.0 + 1.0)]
    others = [(499.5, 256.0 + 16.0), (500.25, 64.0 + 2.0), (500.75, 512.0)]
    bx = np.where(rng.random(n_background) < 0.5, rng.uniform(300.0, 499.0, size=n_background), rng.uniform(502.0, 900.0, size=n_background))
    by = rng.uniform(1.0, 5000.0, size=n_background)
    x = np.concatenate([bx, [p[0] for p in envelope + others]])
    y = np.concatenate([by, [p[1] for p in envelope + others]])
    order = np.argsort(x, kind="stable")
    return (x[order], y[order]), math.fsum(p[1] for p in envelope), math.fsum(p[1] for p in envelope + others)
