"""Hand-made spectra for the marker-ion rule (include/pyascore_hip.h: pya_marker_params), shared by tests/test_markers_host.py
(which pins pyascore_amd.rollup.markers on the records written out here by hand) and tests/test_gpu_markers.py (which runs the
same spectra through the device), and the builders of the larger inputs of both.

The numbers are exact in binary, so that the edges of a window can be hit and float32 holds every planted m/z: the fixed
target C = 126.125 with tol = 2^-7 has the window [126.1171875, 126.1328125]; precursor m/z 400.0 at charge 2 is M = 800.0 and
the loss 32.0 gives the centre (800 - 32) / 2 = 384.0 with the window [383.9921875, 384.0078125].  D = 2^-9 is a step inside a
window."""
import numpy as np

from deisotope_cases import BOUNDARY_LENGTHS, pack  # noqa: F401  (pack: re-exported for the tests)
from pyascore_amd import rollup as ru

NAN, INF = float("nan"), float("inf")
TOL, D = 2.0 ** -7, 2.0 ** -9
C, L = 126.125, 384.0
P_BASE = ru.marker_params(mz=(C,), losses=(32.0,), tol=TOL)
P_FIXED = ru.marker_params(mz=(C,), tol=TOL)
# two fixed targets 2^-7 apart: [126.1171875, 126.1328125] and [126.125, 126.140625] share [126.125, 126.1328125]
P_OVERLAP = ru.marker_params(mz=(C, C + TOL), tol=TOL)
# (800 - 800) / 2 = 0 and (800 - 900) / 2 = -50: not positive, inactive
P_BIG_LOSS = ru.marker_params(mz=(C,), losses=(800.0, 900.0, 32.0), tol=TOL)
# 64 targets: 63 fixed ones at 100, 104, .. 348 and the loss 32.0 in lane 63; 64 fixed ones, the last at 352
P_64 = ru.marker_params(mz=tuple(100.0 + 4.0 * k for k in range(63)), losses=(32.0,), tol=TOL)
P_64_FIXED = ru.marker_params(mz=tuple(100.0 + 4.0 * k for k in range(64)), tol=TOL)
# the loss in lane 0 of two targets is not what marker_params makes (fixed targets come first): by hand
P_LOSS_FIRST = ru.check_marker_params(dict(tol=TOL, tol_ppm=0.0, value=(32.0, C), loss_mask=0b01))
P_PPM = ru.marker_params(mz=(128.0,), tol_ppm=10.0)
P_TOL0 = ru.marker_params(mz=(C,), tol=0.0)

A, K = ru.MARKER_ACTIVE, ru.MARKER_ACTIVE | ru.MARKER_PICKED


def _c(name, params, prec_mz, prec_z, x, y, markers, spectrum, dtype=np.float64):
    """markers: per target (mz, intensity, n_peaks, flags); spectrum: (tic, base_peak, hit, n_active) -- n_peaks is len(x)"""
    x, y = np.asarray(x, dtype), np.asarray(y, dtype)
    assert x.shape == y.shape and len(markers) == len(params["value"]), name
    rec = np.zeros(len(markers), ru.MARKER_DTYPE)
    for t, m in enumerate(markers):
        rec[t] = m
    spec = np.zeros(1, ru.MARKER_SPECTRUM_DTYPE)
    spec[0] = (spectrum[0], spectrum[1], spectrum[2], x.size, spectrum[3])
    return dict(name=name, params=params, prec_mz=float(prec_mz), prec_z=int(prec_z), mz=x, intensity=y, markers=rec, spectrum=spec)


def _edges(dtype):
    """x == lo and x == hi of target 0 and one ulp (of ``dtype``) to either side of each: four peaks inside, the most intense
    of them one ulp below hi; the two outside are more intense still"""
    t = dtype
    lo, hi = C - TOL, C + TOL
    up = lambda v: np.nextafter(t(v), t(INF))                             # noqa: E731
    dn = lambda v: np.nextafter(t(v), t(-INF))                            # noqa: E731
    assert float(t(lo)) == lo and float(t(hi)) == hi                      # (the bounds exist in the type)
    x = [t(lo), dn(lo), up(lo), t(hi), up(hi), dn(hi)]
    return _c("edges of target 0, %s" % np.dtype(t).name, P_BASE, 400.0, 2, x, [1.0, 9.0, 2.0, 3.0, 9.0, 4.0],
              [(float(dn(hi)), 4.0, 4, K), (0.0, 0.0, 0, A)], (28.0, 9.0, 0b01, 2), t)


def hand_cases():
    """One spectrum each: dict(name, params, prec_mz, prec_z, mz, intensity, markers MARKER_DTYPE[n_targets], spectrum
    MARKER_SPECTRUM_DTYPE[1])."""
    none = (0.0, 0.0, 0, A)
    w_ppm = (10.0 * 1e-6) * 128.0
    lo_ppm = 128.0 - w_ppm
    zeros63 = [none] * 63
    cases = [
        _edges(np.float64),
        _edges(np.float32),
        _c("the larger intensity wins, wherever it stands", P_BASE, 400.0, 2, [C, C + 2 * D, L - D, L], [5.0, 7.0, 3.0, 2.0],
           [(C + 2 * D, 7.0, 2, K), (L - D, 3.0, 2, K)], (17.0, 7.0, 0b11, 2)),
        _c("equal intensities: the peak nearer the centre", P_BASE, 400.0, 2, [C + 2 * D, C - D, L + D, L - 2 * D], [5.0, 5.0, 6.0, 6.0],
           [(C - D, 5.0, 2, K), (L + D, 6.0, 2, K)], (22.0, 6.0, 0b11, 2)),
        _c("equal intensities at equal distances: the smaller m/z", P_BASE, 400.0, 2, [C + D, C - D, L - D, L + D], [5.0, 5.0, 6.0, 6.0],
           [(C - D, 5.0, 2, K), (L - D, 6.0, 2, K)], (22.0, 6.0, 0b11, 2)),
        _c("the three levels in one window", P_FIXED, 0.0, 0, [C + D, C - D, C + 2 * D, C - 2 * D, C, C + 3 * D],
           [5.0, 5.0, 5.0, 5.0, 4.0, 1.0], [(C - D, 5.0, 6, K)], (25.0, 5.0, 0b1, 1)),
        _c("a duplicate peak", P_BASE, 400.0, 2, [C, C, 300.0], [5.0, 5.0, 1.0], [(C, 5.0, 2, K), none], (11.0, 5.0, 0b01, 2)),
        _c("one peak in two overlapping windows", P_OVERLAP, 0.0, 0, [C + TOL / 2, C - D, C + TOL + D], [2.0, 1.0, 1.0],
           [(C + TOL / 2, 2.0, 2, K), (C + TOL / 2, 2.0, 2, K)], (4.0, 2.0, 0b11, 2)),
        _c("a NaN m/z is never inside; its intensity is ion current", P_BASE, 400.0, 2, [NAN, C, NAN], [100.0, 1.0, NAN],
           [(C, 1.0, 1, K), none], (101.0, 100.0, 0b01, 2)),
        _c("a NaN intensity is counted, not picked and no ion current", P_BASE, 400.0, 2, [C, C + D, L], [NAN, 2.0, NAN],
           [(C + D, 2.0, 2, K), (0.0, 0.0, 1, A)], (2.0, 2.0, 0b01, 2)),
        _c("nothing but NaN intensities", P_FIXED, 0.0, 0, [C], [NAN], [(0.0, 0.0, 1, A)], (0.0, 0.0, 0, 1)),
        _c("an intensity of -0.0 is picked as 0.0", P_FIXED, 0.0, 0, [C], [-0.0], [(C, 0.0, 1, K)], (0.0, 0.0, 0b1, 1)),
        _c("-0.0 beats a negative intensity and ties with 0.0", P_FIXED, 0.0, 0, [C + D, C - D, C], [-0.0, 0.0, -1.0],
           [(C - D, 0.0, 3, K)], (-1.0, 0.0, 0b1, 1)),
        _c("only negative intensities: the base peak is negative", P_FIXED, 0.0, 0, [C, 300.0], [-2.0, -3.0], [(C, -2.0, 1, K)],
           (-5.0, -2.0, 0b1, 1)),
        _c("an infinite intensity", P_FIXED, 0.0, 0, [C, C + D], [INF, 1.0], [(C, INF, 2, K)], (INF, INF, 0b1, 1)),
        _c("infinite m/z are outside", P_BASE, 400.0, 2, [INF, -INF, L], [1.0, 1.0, 1.0], [none, (L, 1.0, 1, K)], (3.0, 1.0, 0b10, 2)),
        _c("a loss at least as large as the precursor mass is inactive", P_BIG_LOSS, 400.0, 2, [0.0, -50.0, L, C], [1.0, 1.0, 2.0, 3.0],
           [(C, 3.0, 1, K), (0.0, 0.0, 0, 0), (0.0, 0.0, 0, 0), (L, 2.0, 1, K)], (7.0, 3.0, 0b1001, 2)),
        _c("target 63 of 64, a loss", P_64, 400.0, 2, [L, 348.0, 100.0, 102.0], [4.0, 3.0, 2.0, 1.0],
           [(100.0, 2.0, 1, K)] + [none] * 61 + [(348.0, 3.0, 1, K), (L, 4.0, 1, K)], (10.0, 4.0, (1 << 63) | (1 << 62) | 1, 64)),
        _c("target 63 of 64 without a precursor", P_64, 400.0, 0, [L, 348.0], [4.0, 3.0], [none] * 62 + [(348.0, 3.0, 1, K), (0.0, 0.0, 0, 0)],
           (7.0, 4.0, 1 << 62, 63)),
        _c("target 63 of 64, fixed", P_64_FIXED, 0.0, 0, [352.0, 352.0 + D], [1.0, 2.0], zeros63 + [(352.0 + D, 2.0, 2, K)],
           (3.0, 2.0, 1 << 63, 64)),
        _c("a loss in lane 0", P_LOSS_FIRST, 400.0, 2, [C, L], [1.0, 2.0], [(L, 2.0, 1, K), (C, 1.0, 1, K)], (3.0, 2.0, 0b11, 2)),
        _c("a loss in lane 0 without a precursor", P_LOSS_FIRST, NAN, 2, [C, L], [1.0, 2.0], [(0.0, 0.0, 0, 0), (C, 1.0, 1, K)],
           (3.0, 2.0, 0b10, 1)),
        _c("ppm of the centre: lo itself and one ulp below", P_PPM, 0.0, 0, [lo_ppm, np.nextafter(lo_ppm, -INF), 128.0 + w_ppm],
           [1.0, 5.0, 0.5], [(lo_ppm, 1.0, 2, K)], (6.5, 5.0, 0b1, 1)),
        _c("tol 0: the centre alone", P_TOL0, 0.0, 0, [C, np.nextafter(C, INF), np.nextafter(C, -INF)], [1.0, 2.0, 3.0], [(C, 1.0, 1, K)],
           (6.0, 3.0, 0b1, 1)),
        _c("a descending spectrum is a spectrum", P_BASE, 400.0, 2, [500.0, L, C, 100.0], [1.0, 2.0, 3.0, 4.0], [(C, 3.0, 1, K), (L, 2.0, 1, K)],
           (10.0, 4.0, 0b11, 2)),
        _c("no peaks", P_BASE, 400.0, 2, [], [], [none, none], (0.0, 0.0, 0, 2)),
        _c("no peaks and no precursor", P_BASE, 0.0, 0, [], [], [none, (0.0, 0.0, 0, 0)], (0.0, 0.0, 0, 1)),
    ]
    for tag, pm, pz in (("charge 0", 400.0, 0), ("charge -1", 400.0, -1), ("charge 9", 400.0, 9), ("a NaN precursor", NAN, 2),
                        ("an infinite precursor", INF, 2), ("a precursor of 0", 0.0, 2), ("a negative precursor", -400.0, 2)):
        cases.append(_c("no usable precursor: %s; the fixed target stays" % tag, P_BASE, pm, pz, [C, L], [3.0, 4.0],
                        [(C, 3.0, 1, K), (0.0, 0.0, 0, 0)], (7.0, 4.0, 0b01, 1)))
    return cases


def params_key(p):
    return tuple(sorted(p.items()))


def pack_cases(cases, mz_dtype=np.float64, it_dtype=np.float64, gaps=True):
    """(mz, intensity, peak_off, prec_mz, prec_z) of cases of ONE parameter set, an empty spectrum (with a precursor of its own)
    behind each when ``gaps``"""
    mz, it, off = pack([(c["mz"], c["intensity"]) for c in cases], mz_dtype, it_dtype, gaps=gaps)
    rep = 2 if gaps else 1
    return (mz, it, off, np.repeat(np.asarray([c["prec_mz"] for c in cases], np.float64), rep),
            np.repeat(np.asarray([c["prec_z"] for c in cases], np.int32), rep))


BOUNDARY_PREC = (400.0, 2)


def boundary_spectra(seed=7):
    """Spectra of the lengths at which a wavefront's stride begins and ends (deisotope_cases.BOUNDARY_LENGTHS), for P_BASE with
    the precursor 400.0 / 2 everywhere: peaks far from both windows, and PLANTED peaks inside a window -- five spots around each
    centre -- as the first and the last peak and on both sides of every 64-peak boundary, with intensities from three values:
    a target has candidates in one stride (peaks 0 and 63) and in two (63 and 64), equal ones among them.  The second spectrum
    of 64 peaks and the last spectrum (one peak) are planted throughout.  Returns (list of (mz, intensity), list of the planted
    masks)."""
    rng = np.random.default_rng(seed)
    spots = np.array([C - 2 * D, C - D, C, C + D, C + 2 * D, L - 2 * D, L - D, L, L + D, L + 2 * D])
    out, planted = [], []
    for k, n in enumerate(BOUNDARY_LENGTHS):
        x = rng.uniform(100.0, 1500.0, size=n)
        x = np.where((np.abs(x - C) < 1.0) | (np.abs(x - L) < 1.0), x + 50.0, x)
        mask = np.zeros(n, bool)
        if k >= 11:
            mask[:] = True
        elif n:
            at = np.arange(n)
            mask = (at == 0) | (at == n - 1) | (at % 64 == 63) | (at % 64 == 0)
        x[mask] = rng.choice(spots, size=int(mask.sum()))
        out.append((x, rng.choice([1.0, 2.0, 3.0], size=n)))
        planted.append(mask)
    return out, planted


def tiny_spectra(n_spec, params, seed=21, last_hit=None):
    """``n_spec`` spectra of 0 .. 3 peaks around precursors of every charge from -1 to 9, a third of the peaks at the centre of
    an active target of ``params``; ``last_hit``: the last spectrum is one peak at the centre of that (fixed) target.  Returns
    (list of (mz, intensity), prec_mz, prec_z)."""
    rng = np.random.default_rng(seed)
    pz = rng.integers(-1, 10, n_spec).astype(np.int32)
    pm = rng.uniform(300.0, 900.0, n_spec)
    pm[rng.random(n_spec) < 0.02] = np.nan
    cen, _, _, active = ru.marker_windows(pm, pz, params)
    spectra = []
    for s, n in enumerate(rng.integers(0, 4, n_spec)):
        x = rng.uniform(100.0, 2000.0, size=n)
        ts = np.flatnonzero(active[s])
        if ts.size and n:
            x = np.where(rng.random(n) < 0.33, cen[s, rng.choice(ts, size=n)], x)
        spectra.append((x, rng.choice([1.0, 2.0, 3.0], size=n)))
    if last_hit is not None:
        spectra[-1] = (np.array([params["value"][last_hit]]), np.array([7.0]))
    return spectra, pm, pz


REPORTERS = tuple(126.125 + 1.0 * k for k in range(10))                   # ten reporter-like m/z, exact in float32
LOSS_H3PO4 = 97.9769
MZ_LO = 140.0


def planted_params(tol):
    return ru.marker_params(mz=REPORTERS, losses=(LOSS_H3PO4,), tol=tol)


def with_markers(batch, tol, seed=13):
    """``batch`` with ten reporter-like peaks at REPORTERS, (10 + k) times the spectrum's base peak each, and a precursor
    - LOSS_H3PO4 peak at 21 times the base peak, for a precursor at charge 2 drawn inside the spectrum's own m/z range until no
    original peak lies within ``tol`` of the precursor or of its loss form -- that is asserted -- and the peaks sorted again per
    spectrum.  Returns (batch, prec_mz, prec_z, planted): planted[s, t] is the intensity planted for target t of
    ``planted_params``."""
    rng = np.random.default_rng(seed)
    mz, it, off = np.asarray(batch["mz"], np.float64), np.asarray(batch["intensity"], np.float64), np.asarray(batch["peak_off"], np.int64)
    xs, ys, prec, planted = [], [], [], []
    for a, b in zip(off[:-1], off[1:]):
        x, y = mz[a:b], it[a:b]
        for _ in range(1000):
            pm = float(rng.uniform(x.min() + 100.0, x.max()))
            cen = np.array([pm, (pm * 2.0 - LOSS_H3PO4) / 2.0])
            if cen.min() > MZ_LO + 1.0 and not (np.abs(x[:, None] - cen[None, :]) <= tol + 1e-9).any():
                break
        else:
            raise AssertionError("no precursor m/z leaves the spectrum's own peaks alone")
        add_x = np.concatenate([REPORTERS, cen[1:]])
        add_y = np.concatenate([(10.0 + np.arange(10.0)) * y.max(), [21.0 * y.max()]])
        x2, y2 = np.concatenate([x, add_x]), np.concatenate([y, add_y])
        order = np.argsort(x2, kind="stable")
        xs.append(x2[order])
        ys.append(y2[order])
        prec.append(pm)
        planted.append(add_y)
    new_off = np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)
    return (dict(batch, mz=np.concatenate(xs), intensity=np.concatenate(ys), peak_off=new_off), np.asarray(prec),
            np.full(len(prec), 2, np.int32), np.asarray(planted))
