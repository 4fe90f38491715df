"""Inputs of the precursor-XIC tests, shared by the host and the GPU files: the hand case of the rule, traces given as lists of
intensities, the ulp cases at the isotope bounds, and seeded batches of survey scans with eluting precursors.

Hand-made numbers are short binary fractions: the precursor at 500.0, charge 2, step 1.0 (isotopes 0.5 apart), tol = 2^-7, no
ppm term -- so every bound is exact and every expected figure was written down by hand."""
import numpy as np

from pyascore_amd import rollup as ru

T = 2.0 ** -7
PM, Z = 500.0, 2
NAN, INF = float("nan"), float("inf")
TYPES = {"f64/f64": (np.float64, np.float64), "f64/f32": (np.float64, np.float32), "f32/f32": (np.float32, np.float32)}
HAND = (10.0, 100.0, 300.0, 100.0, 20.0, 150.0, 400.0, 150.0, 10.0)


def params(**kw):
    base = dict(tol=T, tol_ppm=0.0, isotopes=0, step=1.0, rise=2.0, max_gap=1)
    base.update(kw)
    return ru.xic_params(**base)


def up(x, t=np.float64):
    return float(np.nextafter(t(x), t(np.inf)))


def down(x, t=np.float64):
    return float(np.nextafter(t(x), t(-np.inf)))


def pack(scans, mz_t=np.float64, it_t=np.float64):
    """``(mz, intensity, peak_off)`` of a list of scans, each a list of (x, y)"""
    off = np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int64)
    flat = [pk for s in scans for pk in s]
    mz = np.asarray([x for x, _ in flat], np.float64).astype(mz_t)
    it = np.asarray([y for _, y in flat], np.float64).astype(it_t)
    return mz, it, off


def unpack(mz, it, off):
    """the scans as lists of (x, y) Python floats (widened), for tests/xic_ref.py"""
    xs, ys = np.asarray(mz).astype(np.float64).tolist(), np.asarray(it).astype(np.float64).tolist()
    return [list(zip(xs[int(a):int(b)], ys[int(a):int(b)])) for a, b in zip(off[:-1], off[1:])]


def trace_scans(trace, mz=PM):
    """one peak at ``mz`` per scan with the intensities of ``trace``; None: an empty scan"""
    return [[] if y is None else [(mz, float(y))] for y in trace]


def queries(rows):
    """the five query arrays of rows (seed, scan_lo, scan_hi, prec_mz, prec_z)"""
    rows = list(rows)
    col = lambda i, t: np.asarray([r[i] for r in rows], t)          # noqa: E731
    return col(0, np.int64), col(1, np.int64), col(2, np.int64), col(3, np.float64), col(4, np.int32)


def edge_scans(t, isotopes=3):
    """For element type ``t``: scans whose only peaks sit one ulp of ``t`` outside, exactly at, and one ulp inside each of the
    2 * (isotopes + 1) bounds of the precursor 500.0 / 2+ with tol 2^-7 and step 1.0.  Returns ``(scans, expected)``: per scan the
    isotope it probes and whether the peak qualifies.  Scan k also holds a monoisotopic peak at 500.0 so that it is present."""
    scans, expected = [], []
    for i in range(isotopes + 1):
        c = PM + 0.5 * i
        for bound, inward in ((c - T, up), (c + T, down)):
            outward = down if inward is up else up
            for x, inside in ((outward(bound, t), False), (bound, True), (inward(bound, t), True)):
                scan = sorted([(PM, 64.0)] + ([(x, 8.0)] if i else []))
                if i == 0:
                    scan = [(x, 8.0)]
                scans.append(scan)
                expected.append((i, inside))
    return scans, expected


def elution(rng, n_survey, n_prec=6, background=40, dropout=0.1, unsorted=0.02):
    """A seeded survey: ``n_prec`` precursors that elute as a pair of integer-valued humps 6 to 10 scans apart (two isomers) and
    sometimes a third elsewhere, their isotope peaks jittered by a few ppm, random dropouts, ``background`` random peaks per scan,
    scans sorted by m/z but for a share of ``unsorted`` ones (two elements swapped).  Returns ``(scans, rt, precursors)`` with
    precursors [(mz, z, [hump centres])]."""
    precs, humps = [], []
    for k in range(n_prec):
        first = int(rng.integers(0, n_survey))
        centres = [first, first + int(rng.integers(6, 11))] + ([int(rng.integers(0, n_survey))] if rng.uniform() < 0.5 else [])
        humps.append([(c, float(rng.integers(100, 5000)), float(rng.uniform(1.5, 3.0))) for c in centres])
        precs.append((400.0 + 37.123 * k + float(rng.uniform(0, 1)), int(rng.integers(1, 5)), centres))
    scans = []
    for s in range(n_survey):
        peaks = [(float(x), float(np.floor(y))) for x, y in zip(rng.uniform(300.0, 900.0, background), rng.uniform(1.0, 50.0, background))]
        for (pm, z, _), hs in zip(precs, humps):
            level = sum(h * np.exp(-0.5 * ((s - c) / w) ** 2) for c, h, w in hs)
            if level < 1.0 or rng.uniform() < dropout:
                continue
            for i in range(4):
                if rng.uniform() < 0.15 * i:
                    continue
                x = (pm + i * ru.STRIP_STEP / z) * (1.0 + float(rng.uniform(-4e-6, 4e-6)))
                peaks.append((x, float(np.floor(level / (1 + i)) + 1.0)))
        peaks.sort()
        if len(peaks) > 1 and rng.uniform() < unsorted:
            peaks[0], peaks[-1] = peaks[-1], peaks[0]
        scans.append(peaks)
    rt = np.cumsum(rng.uniform(0.5, 1.5, n_survey))
    return scans, rt, precs


def elution_queries(rng, n_query, n_survey, precs, max_window=64):
    """seeded queries over an ``elution`` survey, most of them seeded within three scans of a hump: windows of every size up to
    ``max_window`` clipped to the survey, and a share of silent, out-of-range and unusable ones"""
    rows = []
    for q in range(n_query):
        pm, z, centres = precs[int(rng.integers(0, len(precs)))]
        seed = int(rng.integers(0, n_survey))
        if rng.uniform() < 0.8:
            seed = min(n_survey - 1, max(0, centres[int(rng.integers(0, len(centres)))] + int(rng.integers(-3, 4))))
        below, above = int(rng.integers(0, max_window // 2)), int(rng.integers(1, max_window // 2 + 1))
        lo, hi = max(0, seed - below), min(n_survey, seed + above)
        kind = (q + 0.5) / 100.0 if q < 10 else rng.uniform()         # (the first ten queries: one of every kind below)
        if kind < 0.03:
            seed = -1 - int(rng.integers(0, 3))
        elif kind < 0.05:
            hi = n_survey + 1
        elif kind < 0.07:
            lo, hi = seed + 1, seed + 2
        elif kind < 0.09:
            z = int(rng.choice([0, 9, -1]))
        elif kind < 0.10:
            pm = float(rng.choice([NAN, INF, 0.0, -500.0]))
        rows.append((seed, lo, hi, pm, z))
    return queries(rows)


def two_isomers():
    """Two triangular elution profiles with integer intensities at one m/z, apexes 8 scans apart, rt = 0, 1, 2, ..: scans 0 .. 16,
    t = 0 10 20 30 40 30 20 10 6 20 40 60 80 60 40 20 0 (the end scans are empty).  The valley is scan 8 (t = 6) and belongs to
    both peaks.  With unit scan spacing a peak's area is the sum of its t minus half its two end values:
    first peak scans 1 .. 8: sum 166, area 166 - (10 + 6) / 2 = 158; second peak scans 8 .. 15: sum 326, area 326 - (6 + 20) / 2
    = 313.  Returns (trace, {seed scan: (area, left, right)})."""
    trace = [None, 10, 20, 30, 40, 30, 20, 10, 6, 20, 40, 60, 80, 60, 40, 20, None]
    return trace, {3: (158.0, 1, 8), 4: (158.0, 1, 8), 6: (158.0, 1, 8), 11: (313.0, 8, 15), 12: (313.0, 8, 15), 13: (313.0, 8, 15)}
