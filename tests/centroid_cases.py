"""Hand-made spectra for the centroiding rule (include/pyascore_hip.h: pya_centroid_params), shared by
tests/test_centroid_host.py (which pins pyascore_amd.rollup.centroid on the apexes, centroids and intensities written out here
by hand) and tests/test_gpu_centroid.py (which runs the same spectra through the device), and the builders of the larger
inputs of both.  Every number of a hand case is exact in binary (and in float32): samples lie DX = 2^-6 apart, the gap is
2 DX, and the intensities of a footprint add up to a power of two wherever a centroid is computed."""
import numpy as np

from pyascore_amd import rollup as ru
from deisotope_cases import BOUNDARY_LENGTHS, pack  # noqa: F401  (pack: re-exported for the tests)

DX = 2.0 ** -6
GAP = 2.0 ** -5
NAN, INF = float("nan"), float("inf")


def _p(**kw):
    return ru.check_centroid_params(dict(dict(gap0=GAP, gap_per_mz=0.0, min_height=0.0, half_width=4, area=0), **kw))


P = _p()
P_AREA = _p(area=1)
P_W1, P_W1_AREA, P_W8_AREA = _p(half_width=1), _p(half_width=1, area=1), _p(half_width=8, area=1)
P_MIN2 = _p(min_height=2.0)
P_PPM = _p(gap0=0.0, gap_per_mz=2.0 ** -12)                                 # at m/z 128 the limit is 2^-5 = 2 DX
P_BOTH = _p(gap0=DX, gap_per_mz=2.0 ** -13)                                 # at m/z 128: DX + DX


def grid(n, base=100.0):
    return base + DX * np.arange(n)


def _c(name, params, x, y, apex, mz, height, area, dtype=np.float64, unordered=False, select=True):
    """``apex``: the indices kept; ``mz``: the output m/z; ``height`` / ``area``: the output intensity with area 0 / 1.  For
    a spectrum that is copied (unordered, not selected) all three are the input."""
    x, y = np.asarray(x, dtype), np.asarray(y, dtype)
    assert x.shape == y.shape and len(apex) == len(mz) == len(height) == len(area), name
    return dict(name=name, params=params, mz=x, intensity=y, apex=list(apex), out_mz=np.asarray(mz, dtype), height=np.asarray(height, dtype),
                area=np.asarray(area, dtype), unordered=unordered, select=select)


def _gap_edges(dtype):
    """a pair exactly gap apart (connected: one peak) and one ulp of ``dtype`` further apart (two isolated points, copied), for
    the constant term, the per-m/z term and both"""
    t = dtype
    out = []
    for tag, p, base in (("gap0", P, 100.0), ("gap_per_mz", P_PPM, 128.0), ("both", P_BOTH, 128.0)):
        far = t(base + 2 * DX)
        # y = 1, 3: the apex is the second point; sw = 4, s = -2 DX, q = -DX / 2
        out.append(_c("%s: a gap exactly at the limit %s" % (tag, np.dtype(t).name), p, [base, far], [1, 3], [1], [base + 1.5 * DX], [3], [4], t))
        above = np.nextafter(far, t(INF))
        out.append(_c("%s: a gap one ulp above the limit %s" % (tag, np.dtype(t).name), p, [base, above], [1, 3], [0, 1], [base, above], [1, 3],
                      [1, 3], t))
    return out


def hand_cases():
    """One spectrum each: dict(name, params, mz, intensity, apex, out_mz, height, area, unordered, select)."""
    g = grid
    ramp = [1, 2, 3, 4, 5, 6, 7, 8, 9, 8, 7, 6, 5, 4, 3, 2, 1]
    two_dn = np.nextafter(2.0, 0.0)
    cases = [
        # sw = 4, s = -DX + 0 + DX = 0
        _c("a symmetric triangle: c is x[i]", P, g(3), [1, 2, 1], [1], [100 + DX], [2], [4]),
        # sw = 8, s = -DX + 0 + 3 DX = 2 DX, q = DX / 4
        _c("an asymmetric peak: a dyadic centroid", P, g(3), [1, 4, 3], [1], [100 + 1.25 * DX], [4], [8]),
        # point 2 is no apex (y[1] < y[2] fails); sw = 8, s = -DX + 0 + 3 DX + 2 DX = 4 DX, q = DX / 2
        _c("a plateau: the first point wins, the whole plateau is summed", P, g(4), [1, 3, 3, 1], [1], [100 + 1.5 * DX], [3], [8]),
        # apex 1 over [0, 2]: sw = 8, s = -2 DX + 0 + 3 DX = DX, q = DX / 8; apex 3 over [2, 4] (the step 1 -> 2 does not rise
        # strictly): sw = 8, s = -3 DX + 0 + DX = -2 DX, q = -DX / 4.  Point 2 is in both footprints.
        _c("a plateau followed by a rise: two apexes", P, g(5), [2, 3, 3, 4, 1], [1, 3], [100 + 1.125 * DX, 100 + 2.75 * DX], [3, 4], [8, 8]),
        # apex 1 over [0, 2]: sw = 8, s = -DX + 2 DX = DX; apex 3 over [2, 4]: sw = 8, s = -2 DX + DX = -DX
        _c("two peaks sharing a valley point", P, g(5), [1, 5, 2, 5, 1], [1, 3], [100 + 1.125 * DX, 100 + 2.875 * DX], [5, 5], [8, 8]),
        # apex 0 over [0, 2] (equal intensities belong to the peak on their left): sw = 8, s = DX + 2 DX = 3 DX, q = 3 DX / 8;
        # apex 3 over [2, 3]: sw = 8, s = -DX, q = -DX / 8
        _c("a flat valley belongs to the left peak but for its last point", P, g(4), [6, 1, 1, 7], [0, 3], [100 + 0.375 * DX, 100 + 2.875 * DX],
           [6, 7], [8, 8]),
        _c("min_height at equality and one ulp below", P_MIN2, list(g(3)) + [101.0, 102.0], [1, 2, 1, 2, two_dn], [1, 3], [100 + DX, 101.0], [2, 2],
           [4, 2]),
        # points 0 and 2 have a connected NaN neighbour; apex 5 over [4, 6] (0 < 2 rises, 0 < 0 does not): sw = 4, s = 2 DX
        _c("NaN and zero intensities", P, list(g(7)) + [200.0, 300.0], [1, NAN, 3, 0, 0, 2, 2, 0, NAN], [5], [100 + 5.5 * DX], [2], [4]),
        # half_width 1: [2, 4], sw = 16, s = -5 DX + 0 + 3 DX = -2 DX, q = -DX / 8
        _c("a footprint cut by half_width", P_W1, g(5), [1, 2, 5, 8, 3], [3], [100 + 2.875 * DX], [8], [16]),
        _c("half_width 1 on a ramp of 17", P_W1_AREA, g(17), ramp, [8], [100 + 8 * DX], [9], [25]),
        _c("half_width 4 on a ramp of 17", P_AREA, g(17), ramp, [8], [100 + 8 * DX], [9], [61]),
        _c("half_width 8 on a ramp of 17", P_W8_AREA, g(17), ramp, [8], [100 + 8 * DX], [9], [81]),
        _c("an already centroided spectrum passes through, a zero with its sign", P, [-0.0, 100.0, 101.0, 102.5, 200.0], [9, 5, 1, 7, 2],
           [0, 1, 2, 3, 4], [-0.0, 100.0, 101.0, 102.5, 200.0], [9, 5, 1, 7, 2], [9, 5, 1, 7, 2]),
        _c("one point", P, [500.0], [1.0], [0], [500.0], [1.0], [1.0]),
        _c("one point that is no peak", P, [500.0], [0.0], [], [], [], []),
        _c("a repeated m/z is connected", P, [100.0, 100.0, 100.0], [1, 2, 1], [1], [100.0], [2], [4]),
        _c("an unselected spectrum is copied", P, g(3), [1, 2, 1], [0, 1, 2], g(3), [1, 2, 1], [1, 2, 1], select=False),
        _c("a descending pair: the spectrum is copied", P, [100 + DX, 100.0, 100 + 2 * DX], [1, 2, 1], [0, 1, 2], [100 + DX, 100.0, 100 + 2 * DX],
           [1, 2, 1], [1, 2, 1], unordered=True),
        _c("a NaN m/z: no order holds, the spectrum is copied", P, [100.0, NAN, 100 + DX], [1, 2, 1], [0, 1, 2], [100.0, NAN, 100 + DX], [1, 2, 1],
           [1, 2, 1], unordered=True),
        # THE CLAMP.  With positive finite intensities none was found that needs it, and none exists: the apex has d = 0 and
        # the largest weight of at most 17, so q stays 1/17 of the span inside [x[l] - x[i], x[r] - x[i]], far more than the
        # roundings move it.  It takes intensities a detector does not produce:
        # sw = 2 + -1 = 1, s = DX -1 = -DX, c = 100 - DX < x[l]
        _c("the clamp from below: a negative intensity on the right flank", P, g(2), [2, -1], [0], [100.0], [2], [1]),
        # sw = 1, s = (-DX)(-1) = DX, c = x[1] + DX > x[r]
        _c("the clamp from above: a negative intensity on the left flank", P, g(2), [-1, 2], [1], [100 + DX], [2], [1]),
        # p = 0 inf is NaN at k = i: c is NaN and becomes x[l]
        _c("a NaN centroid becomes x[l]: infinite intensities", P, g(3), [1, INF, INF], [1], [100.0], [INF], [INF]),
    ]
    return cases + _gap_edges(np.float64) + _gap_edges(np.float32)


def params_key(p):
    return tuple(sorted(p.items()))


def expected(case, area):
    """(mz, intensity) a case gives under its parameters with ``area`` 0 or 1, in the case's dtype"""
    return case["out_mz"], case["area"] if area else case["height"]


PLANTED = ((0, 62, 64), (63, 65))


def boundary_spectra(seed=7):
    """Spectra of the lengths at which a wavefront's stride and its ballot word begin and end, on the DX grid (exact in
    float32 up to the 4 097th point).  A step is DX (three in five), nothing (a repeated m/z) or 3 DX (not connected);
    intensities come from five values, so plateaus, valleys and equal neighbours are frequent and footprints of every shape
    straddle the stride edges.  On top, points of intensity 16 -- apexes, whatever surrounds them -- are planted at 0, 62 and 64
    of every even spectrum, at 63 and 65 of every odd one and at the last point of both (of two adjacent planted points the
    second is dropped: it would be no apex).  Returns (spectra, planted index lists)."""
    rng = np.random.default_rng(seed)
    out, planted = [], []
    for s, n in enumerate(BOUNDARY_LENGTHS):
        step = rng.choice([1.0, 1.0, 1.0, 0.0, 3.0], size=n) * DX
        x = 100.0 + np.cumsum(step)
        y = rng.choice([1.0, 2.0, 3.0, 4.0, 8.0], size=n)
        at = {k for k in PLANTED[s % 2] + (n - 1,) if 0 <= k < n}
        at = sorted(k for k in at if k - 1 not in at)                      # (of two adjacent ones only the first is an apex)
        y[at] = 16.0
        out.append((x, y))
        planted.append(at)
    return out, planted


def profile_of(batch, sigma, dx, reach=4.0):
    """``batch`` with every peak of every spectrum rendered as Gaussian samples on the grid k dx: a peak of height h at c adds
    h exp(-(x - c)^2 / (2 sigma^2)) to the grid points within ``reach`` sigma of c; the samples of overlapping peaks add up.
    The dtypes of the batch stay."""
    mz, it, off = np.asarray(batch["mz"]), np.asarray(batch["intensity"]), np.asarray(batch["peak_off"], np.int64)
    xs, ys, n = [], [], [0]
    for a, b in zip(off[:-1], off[1:]):
        c, h = mz[a:b].astype(np.float64), it[a:b].astype(np.float64)
        k0 = np.ceil((c - reach * sigma) / dx).astype(np.int64)
        cnt = np.floor((c + reach * sigma) / dx).astype(np.int64) - k0 + 1
        peak = np.repeat(np.arange(c.size), cnt)
        k = np.repeat(k0, cnt) + (np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt))
        w = h[peak] * np.exp(-((k * dx - c[peak]) ** 2) / (2.0 * sigma * sigma))
        cells, inverse = np.unique(k, return_inverse=True)
        y = np.zeros(cells.size)
        np.add.at(y, inverse, w)
        xs.append(cells * dx)
        ys.append(y)
        n.append(cells.size)
    return dict(batch, mz=np.concatenate(xs).astype(mz.dtype), intensity=np.concatenate(ys).astype(it.dtype), peak_off=np.cumsum(n).astype(np.int64))
