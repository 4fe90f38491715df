"""Hand-made spectra for the precursor-stripping rule (include/pyascore_hip.h: pya_strip_params), shared by
tests/test_strip_host.py (which pins pyascore_amd.rollup.strip on the ``keep`` / ``hit`` / ``n_windows`` written out here by hand)
and tests/test_gpu_strip.py (which runs the same spectra through the device), and the builders of the larger inputs of both.

The numbers are exact in binary, so that the edges of a window can be hit: precursor m/z 400.0 at charge 2 is M = 800.0; the
loss 32.0 gives the centre (800 - 32) / 2 = 384.0; tol = 2^-7 gives the window [383.9921875, 384.0078125]; with step = 1.0 and
isotopes = 2 the span is 2 (1.0 / 2) = 1.0 and the upper bound 385.0078125."""
import numpy as np

from deisotope_cases import BOUNDARY_LENGTHS, pack  # noqa: F401  (pack: re-exported for the tests)
from pyascore_amd import rollup as ru

NAN, INF = float("nan"), float("inf")
TOL = 2.0 ** -7
P_BASE = ru.strip_params(TOL, losses=(32.0,), step=1.0)
P_ISO2 = ru.strip_params(TOL, losses=(32.0,), step=1.0, isotopes=2)
P_REDUCED = ru.strip_params(TOL, losses=(32.0,), step=1.0, reduced=True)
P_LAYOUT = ru.strip_params(TOL, losses=(30.0, 60.0), step=1.0, reduced=True)
# z = 8, reduced, 7 losses: all 64 windows.  M = 100 x 8 = 800; window 31 is c = 3, l = 7: (800 - 50) / 5 = 150; window 32 is
# c = 4, l = 0: 800 / 4 = 200; window 63 is c = 7, l = 7: (800 - 50) / 1 = 750
LOSSES_64 = (3.0, 7.0, 13.0, 21.0, 31.0, 43.0, 50.0)
P_64 = ru.strip_params(TOL, losses=LOSSES_64, step=1.0, reduced=True)
P_BIG_LOSS = ru.strip_params(TOL, losses=(32.0, 900.0, 800.0), step=1.0)
P_CUT = ru.strip_params(TOL, losses=(32.0,), step=1.0, mz_lo=150.0)
P_RANGE = ru.strip_params(TOL, losses=(32.0,), step=1.0, mz_lo=200.0, mz_hi=500.0)
P_IN_AND_OUT = ru.strip_params(TOL, losses=(32.0,), step=1.0, mz_lo=390.0)
P_TOL0 = ru.strip_params(0.0, losses=(32.0,), step=1.0)
P_TWICE = ru.strip_params(TOL, losses=(32.0, 32.0), step=1.0)
P_WIDE = ru.strip_params(10.0, losses=(32.0,), step=1.0)


def _c(name, params, prec_mz, prec_z, x, keep, hit, n_windows, dtype=np.float64):
    x = np.asarray(x, dtype)
    assert x.shape == (len(keep),), name
    return dict(name=name, params=params, prec_mz=float(prec_mz), prec_z=int(prec_z), mz=x, intensity=np.arange(1.0, x.size + 1.0).astype(dtype),
                keep=np.asarray(keep, bool), hit=int(hit), n_windows=int(n_windows))


def _edges(params, lo, hi, dtype, tag):
    """x == lo and x == hi of window 1 and one ulp (of ``dtype``) to either side of each"""
    t = dtype
    up = lambda v: np.nextafter(t(v), t(INF))                             # noqa: E731
    dn = lambda v: np.nextafter(t(v), t(-INF))                            # noqa: E731
    assert float(t(lo)) == lo and float(t(hi)) == hi                      # (the bounds exist in the type)
    x = [t(lo), dn(lo), up(lo), t(hi), up(hi), dn(hi)]
    return _c("edges of window 1, %s, %s" % (tag, np.dtype(t).name), params, 400.0, 2, x, [0, 1, 0, 0, 1, 0], 0b10, 2, t)


def only_window_64(w):
    """the centre of window ``w`` of P_64 at precursor 100.0 / 8 in plain Python floats, with the assertion that no other of
    the 64 windows holds it"""
    per = len(LOSSES_64) + 1
    loss = (0.0,) + LOSSES_64
    cen = [(100.0 * 8.0 - loss[v % per]) / float(8 - v // per) for v in range(64)]
    assert [v for v in range(64) if cen[v] - TOL <= cen[w] <= cen[v] + TOL] == [w], w
    return cen[w]


def hand_cases():
    """One spectrum each: dict(name, params, prec_mz, prec_z, mz, intensity, keep, hit, n_windows)."""
    assert (only_window_64(31), only_window_64(32), only_window_64(63)) == (150.0, 200.0, 750.0)
    up, dn = (lambda v: np.nextafter(v, INF)), (lambda v: np.nextafter(v, -INF))
    cases = [
        _edges(P_BASE, 383.9921875, 384.0078125, np.float64, "no isotopes"),
        _edges(P_BASE, 383.9921875, 384.0078125, np.float32, "no isotopes"),
        _edges(P_ISO2, 383.9921875, 385.0078125, np.float64, "two isotopes"),
        _edges(P_ISO2, 383.9921875, 385.0078125, np.float32, "two isotopes"),
        _c("inside a window of two isotopes, between the isotope peaks", P_ISO2, 400.0, 2, [384.25, 384.75, 400.5, 401.0078125, 401.25],
           [0, 0, 0, 0, 1], 0b11, 2),
        # z = 2 with the charge-reduced forms: w0 = 400, w1 = 384, w2 = 800 / 1, w3 = 768 / 1
        _c("reduced: the precursor and its loss at charge 2 and at charge 1", P_REDUCED, 400.0, 2, [400.0, 384.0, 800.0, 768.0, 500.0],
           [0, 0, 0, 0, 1], 0b1111, 4),
        _c("not reduced: charge 1 stays", P_BASE, 400.0, 2, [400.0, 384.0, 800.0, 768.0, 500.0], [0, 0, 1, 1, 1], 0b11, 2),
        _c("reduced at charge 1 is one charge", P_REDUCED, 400.0, 1, [400.0, 368.0, 384.0], [0, 0, 1], 0b11, 2),
        # M = 900, three windows per charge: 300 290 280 | 450 435 420 | 900 870 840
        _c("the layout w = c (n_loss + 1) + l", P_LAYOUT, 300.0, 3, [435.0, 840.0, 600.0], [0, 0, 1], (1 << 4) | (1 << 8), 9),
        _c("the layout, window 2 and window 3", P_LAYOUT, 300.0, 3, [450.0, 280.0], [0, 0], (1 << 2) | (1 << 3), 9),
        _c("window 31 alone", P_64, 100.0, 8, [150.0, 151.0], [0, 1], 1 << 31, 64),
        _c("window 32 alone", P_64, 100.0, 8, [199.0, 200.0], [1, 0], 1 << 32, 64),
        _c("window 63 alone", P_64, 100.0, 8, [750.0], [0], 1 << 63, 64),
        _c("windows 0 and 63 together", P_64, 100.0, 8, [750.0, 100.0, 98.0], [0, 0, 1], (1 << 63) | 1, 64),
        # (800 - 900) / 2 = -50 and (800 - 800) / 2 = 0: not positive, inactive, not counted
        _c("a loss larger than the precursor mass, and one equal to it", P_BIG_LOSS, 400.0, 2, [-50.0, 0.0, 384.0, 400.0, 1.0],
           [1, 1, 0, 0, 1], 0b11, 2),
        _c("a NaN and infinite m/z stay without a range", P_BASE, 400.0, 2, [NAN, INF, -INF, 400.0], [1, 1, 1, 0], 0b1, 2),
        _c("infinite m/z go with a range, a NaN stays", P_RANGE, 400.0, 2, [NAN, INF, -INF, 400.0, 384.0], [1, 0, 0, 0, 0], 0b11, 2),
        _c("mz_lo and mz_hi equal to a peak", P_RANGE, 0.0, 0, [200.0, dn(200.0), 500.0, up(500.0), 350.0], [1, 0, 1, 0, 1], 0, 0),
        _c("mz_lo and mz_hi equal to a peak, float32", P_RANGE, 0.0, 0,
           [200.0, np.nextafter(np.float32(200.0), np.float32(-INF)), 500.0, np.nextafter(np.float32(500.0), np.float32(INF))], [1, 0, 1, 0], 0, 0,
           np.float32),
        _c("inside a window and outside the range: hit, removed once", P_IN_AND_OUT, 400.0, 2, [384.0, 395.0, 389.0], [0, 1, 0], 0b10, 2),
        _c("a descending spectrum is a spectrum", P_BASE, 400.0, 2, [500.0, 400.0, 384.0, 300.0], [1, 0, 0, 1], 0b11, 2),
        _c("tol 0: the centre alone", P_TOL0, 400.0, 2, [400.0, up(400.0), dn(400.0), 384.0], [0, 1, 1, 0], 0b11, 2),
        _c("the same loss twice: two windows, one removal", P_TWICE, 400.0, 2, [384.0, 390.0], [0, 1], 0b110, 3),
        _c("windows that overlap", P_WIDE, 400.0, 2, [392.0, 380.0, 405.0, 373.0, 411.0], [0, 0, 0, 1, 1], 0b11, 2),
        _c("no peaks", P_BASE, 400.0, 2, [], [], 0, 2),
        _c("every peak goes", P_BASE, 400.0, 2, [400.0, 384.0, 400.0], [0, 0, 0], 0b11, 2),
    ]
    for tag, pm, pz in (("charge 0", 400.0, 0), ("charge -1", 400.0, -1), ("charge 9", 400.0, 9), ("a NaN precursor", NAN, 2),
                        ("an infinite precursor", INF, 2), ("a precursor of 0", 0.0, 2), ("a negative precursor", -400.0, 2)):
        cases.append(_c("no windows: %s, the range cut applies" % tag, P_CUT, pm, pz, [400.0, 384.0, 100.0], [1, 1, 0], 0, 0))
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


def boundary_spectra(seed=7):
    """Spectra of the lengths at which a wavefront's stride and its ballot word begin and end (deisotope_cases.BOUNDARY_LENGTHS),
    for P_BASE with the precursor 400.0 / 2 everywhere: peaks far from both windows, and PLANTED peaks inside a window -- at
    lo, the centre or hi of the precursor's or the loss's -- as the first and the last peak and on both sides of every 64-peak
    boundary; the second spectrum of 64 peaks and the last spectrum (one peak) are planted throughout.  Returns (list of (mz,
    intensity), list of the planted masks): the rule keeps exactly the peaks that are not planted."""
    rng = np.random.default_rng(seed)
    spots = np.array([400.0 - TOL, 400.0, 400.0 + TOL, 384.0 - TOL, 384.0, 384.0 + TOL])
    out, planted = [], []
    for k, n in enumerate(BOUNDARY_LENGTHS):
        x = rng.uniform(100.0, 1500.0, size=n)
        x = np.where((np.abs(x - 400.0) < 1.0) | (np.abs(x - 384.0) < 1.0), x + 50.0, x)
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


BOUNDARY_PREC = (400.0, 2)

LOSS_H3PO4, LOSS_WATER = 97.976896, 18.010565


def effect_params(tol):
    return ru.strip_params(tol, losses=(LOSS_H3PO4, LOSS_WATER), isotopes=1)


def with_precursors(batch, tol, seed=13):
    """``batch`` with a planted precursor at charge 2, its - H3PO4 and - H2O forms and one isotope peak of each (six peaks per
    spectrum, at ten times the spectrum's largest intensity), the peaks sorted again per spectrum.  Every precursor m/z is drawn
    inside the spectrum's own m/z range until no original peak lies in any of its windows under ``effect_params(tol)``, and
    that is asserted: stripping the result gives the original arrays back.  Returns (batch, prec_mz, prec_z)."""
    rng = np.random.default_rng(seed)
    p = effect_params(tol)
    mz, it, off = np.asarray(batch["mz"], np.float64), np.asarray(batch["intensity"], np.float64), np.asarray(batch["peak_off"], np.int64)
    xs, ys, prec = [], [], []
    for a, b in zip(off[:-1], off[1:]):
        x, y = mz[a:b], it[a:b]
        for _ in range(1000):
            pm = float(rng.uniform(x.min() + 100.0, x.max()))
            lo, hi, active = ru.strip_windows(pm, 2, p)
            assert active.sum() == 3
            if not ((lo[active][None, :] <= x[:, None]) & (x[:, None] <= hi[active][None, :])).any():
                break
        else:
            raise AssertionError("no precursor m/z leaves the spectrum's own peaks alone")
        cen = np.array([(pm * 2.0 - loss) / 2.0 for loss in p["loss"]])
        add = np.concatenate([cen, cen + p["step"] / 2.0])
        assert ((lo[active][None, :] <= add[:, None]) & (add[:, None] <= hi[active][None, :])).any(axis=1).all()
        x2, y2 = np.concatenate([x, add]), np.concatenate([y, np.full(add.size, 10.0 * y.max())])
        order = np.argsort(x2, kind="stable")
        xs.append(x2[order])
        ys.append(y2[order])
        prec.append(pm)
    new_off = np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)
    return dict(batch, mz=np.concatenate(xs), intensity=np.concatenate(ys), peak_off=new_off), np.asarray(prec), np.full(len(prec), 2, np.int32)
