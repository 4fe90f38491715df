"""Hand-made spectra for the deisotoping rule (include/pyascore_hip.h: pya_deisotope_params), shared by
tests/test_deisotope_host.py (which pins pyascore_amd.rollup.deisotope on the ``keep`` written out here by hand) and
tests/test_gpu_deisotope.py (which runs the same spectra through the device), and the builders of the larger inputs of both."""
import numpy as np

from pyascore_amd import rollup as ru, synth

S = 1.0033548378
P0 = ru.deisotope_params()                                                # tol 0.01, charges 1 .. 3, ratio 1
# spacings that are exact in binary, so that x[j] - x[i] - spacing is exact and fabs(e) == tol can be hit
TOL_EXACT = 2.0 ** -7
P_EXACT = ru.check_deisotope_params(dict(tol=TOL_EXACT, ratio0=1.0, ratio_per_mz=0.0, max_charge=3, spacing=(1.0, 0.5, 0.25)))
P_HALF = ru.deisotope_params(ratio=0.5)
P_075 = ru.deisotope_params(ratio=0.75)
P_PER_MZ = ru.deisotope_params(ratio=1.0, ratio_per_mz=0.001)
P_ONLY_PER_MZ = ru.deisotope_params(ratio=0.0, ratio_per_mz=0.001)
NAN, INF = float("nan"), float("inf")


def _c(name, params, x, y, keep, dtype=np.float64, unordered=False):
    x, y = np.asarray(x, dtype), np.asarray(y, dtype)
    assert x.shape == y.shape == (len(keep),), name
    return dict(name=name, params=params, mz=x, intensity=y, keep=np.asarray(keep, bool), unordered=unordered)


def _tol_edges(dtype):
    """fabs(e) == tol exactly on both sides of the window at charges 1 and 2, and one ulp (of ``dtype``) to either side"""
    t = dtype
    up = lambda v: np.nextafter(t(v), t(INF))                             # noqa: E731
    dn = lambda v: np.nextafter(t(v), t(-INF))                            # noqa: E731
    hi1, lo1 = 100.0 + 1.0 + TOL_EXACT, 100.0 + 1.0 - TOL_EXACT           # z = 1 against 100.0
    hi2, lo2 = 300.0 + 0.5 + TOL_EXACT, 300.0 + 0.5 - TOL_EXACT           # z = 2 against 300.0
    out = []
    for tag, a, b, base in (("z1", lo1, hi1, 100.0), ("z2", lo2, hi2, 300.0)):
        for what, x, gone in (("upper edge", b, True), ("one ulp above", up(b), False), ("one ulp inside the upper edge", dn(b), True),
                              ("lower edge", a, True), ("one ulp below", dn(a), False), ("one ulp inside the lower edge", up(a), True)):
            out.append(_c("tol %s %s %s" % (tag, what, np.dtype(t).name), P_EXACT, [base, x], [10.0, 5.0], [True, not gone], t))
    return out


def hand_cases():
    """One spectrum each: dict(name, params, mz, intensity, keep, unordered)."""
    seven_up, seven_dn = np.nextafter(7.0, INF), np.nextafter(7.0, 0.0)
    cases = [
        _c("a parent at each charge", P0, [500.0, 500.0 + S, 600.0, 600.0 + S / 2, 700.0, 700.0 + S / 3], [10, 5, 10, 5, 10, 5],
           [1, 0, 1, 0, 1, 0]),
        _c("charge 4 is not tried with max_charge 3", P0, [800.0, 800.0 + S / 4], [10, 5], [1, 1]),
        _c("charge 4 is tried with max_charge 4", ru.deisotope_params(max_charge=4), [800.0, 800.0 + S / 4], [10, 5], [1, 0]),
        _c("just outside and just inside the default tolerance", P0, [500.0, 500.0 + S + 0.0101, 600.0, 600.0 + S - 0.0099], [10, 5, 10, 5],
           [1, 1, 1, 0]),
        # M, M+1, M+2 at charge 2; M+2 meets M at charge 1.  b = 0.001 x[i] z: against M at z = 1 it is 0.5 and 8 > 5; against
        # M+1 at z = 2 it is 1.0017 and 8 <= 9.015; M+1 itself goes against M at z = 2 (b = 1.0, 9 <= 10)
        _c("the chain: M+2 fails against M and passes against the removed M+1", P_ONLY_PER_MZ, [500.0, 500.0 + S / 2, 500.0 + S], [10, 9, 8],
           [1, 0, 0]),
        _c("the chain without its middle peak", P_ONLY_PER_MZ, [500.0, 500.0 + S], [10, 8], [1, 1]),
        _c("M+2 at ratio 0.5 goes because of M+1 alone", P_HALF, [500.0, 500.0 + S, 500.0 + 2 * S], [10, 5, 2.5], [1, 0, 0]),
        _c("the ratio exactly equal", P0, [500.0, 500.0 + S], [7.0, 7.0], [1, 0]),
        _c("the ratio one ulp above", P0, [500.0, 500.0 + S], [7.0, seven_up], [1, 1]),
        _c("the ratio one ulp below", P0, [500.0, 500.0 + S], [7.0, seven_dn], [1, 0]),
        _c("the ratio 0.75 exactly equal", P_075, [500.0, 500.0 + S], [8.0, 6.0], [1, 0]),
        _c("the ratio 0.75 one ulp above", P_075, [500.0, 500.0 + S], [8.0, np.nextafter(6.0, INF)], [1, 1]),
        _c("a more intense satellite stays at ratio 1", P0, [1000.0, 1000.0 + S], [10, 12], [1, 1]),
        _c("ratio_per_mz turns the rejection into a removal", P_PER_MZ, [1000.0, 1000.0 + S], [10, 12], [1, 0]),
        _c("repeated m/z", P0, [500.0, 500.0, 500.0 + S, 500.0 + S], [3, 10, 5, 12], [1, 1, 0, 1]),
        _c("a NaN intensity stays and removes nothing", P0, [500.0, 500.0 + S, 600.0, 600.0 + S], [10, NAN, NAN, 5], [1, 1, 1, 1]),
        _c("infinite m/z at the end", P0, [500.0, 500.0 + S, INF, INF], [10, 5, 1, 1], [1, 0, 1, 1]),
        _c("an infinite parent intensity", P0, [500.0, 500.0 + S], [INF, 5], [1, 0]),
        _c("an infinite satellite intensity", P0, [500.0, 500.0 + S], [10, INF], [1, 1]),
        _c("m/z that are not positive", P0, [-5.0, -5.0 + S, 0.0, S], [10, 5, 10, 5], [1, 0, 1, 0]),
        _c("intensities that are not positive", P0, [500.0, 500.0 + S, 600.0, 600.0 + S, 700.0, 700.0 + S], [0, 0, -1, -2, -1, 0],
           [1, 0, 1, 0, 1, 1]),
        _c("a NaN m/z: no order holds, the spectrum is copied", P0, [500.0, NAN, 500.0 + S], [10, 1, 5], [1, 1, 1], unordered=True),
        _c("a descending pair: the spectrum is copied", P0, [500.0, 500.0 + S, 400.0], [10, 5, 1], [1, 1, 1], unordered=True),
        _c("a descending pair at the front", P0, [500.0, 400.0, 400.0 + S], [10, 5, 1], [1, 1, 1], unordered=True),
        _c("one peak", P0, [500.0], [1.0], [1]),
        _c("two peaks that are no pair", P0, [500.0, 501.5], [10, 1], [1, 1]),
        _c("the lowest peak stays whatever its intensity", P0, [500.0, 500.0 + S], [0.0, 0.0], [1, 0]),
    ]
    return cases + _tol_edges(np.float64) + _tol_edges(np.float32)


def params_key(p):
    return (p["tol"], p["ratio0"], p["ratio_per_mz"], p["max_charge"], p["spacing"])


def pack(spectra, mz_dtype=np.float64, it_dtype=np.float64, gaps=True):
    """(mz, intensity, peak_off) of a list of (mz, intensity) pairs, with an empty spectrum behind each when ``gaps``."""
    xs, ys, n = [], [], [0]
    for x, y in spectra:
        xs.append(np.asarray(x, mz_dtype))
        ys.append(np.asarray(y, it_dtype))
        n.append(len(x))
        if gaps:
            n.append(0)
    cat = lambda parts, t: np.concatenate(parts).astype(t) if parts else np.zeros(0, t)   # noqa: E731
    return cat(xs, mz_dtype), cat(ys, it_dtype), np.cumsum(n).astype(np.int64)


BOUNDARY_LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 4097, 0, 64, 1)


def boundary_spectra(seed=7):
    """Spectra of the lengths at which a wavefront's stride and its ballot word begin and end.  Every spectrum is a ladder:
    the step from a peak to the next is an isotope spacing (exact, or off by up to 0.012 -- inside and outside the 0.01
    tolerance), nothing at all (a repeated m/z), or a step that is no spacing; intensities come from five values, so equal
    ones are frequent.  Parents and satellites therefore sit on both sides of every 64-peak boundary."""
    rng = np.random.default_rng(seed)
    out = []
    for n in BOUNDARY_LENGTHS:
        kind = rng.integers(0, 6, size=n)
        step = np.choose(kind, [S, S / 2, S / 3, 0.7313, 0.0, 1.7])
        step = step + np.where(kind < 3, rng.uniform(-0.012, 0.012, size=n), 0.0)
        x = 100.0 + np.cumsum(step)
        y = rng.choice([1.0, 2.0, 3.0, 4.0, 8.0], size=n)
        out.append((x, y))
    return out


def dense_batch():
    """48 PSMs of the dense legs: 600 noise peaks, every peak with its two satellites"""
    desc = synth.describe("cfg2", n_psm=48, n_noise=600, isotopes=True)
    return synth.make_slice(desc), desc["settings"]


def with_satellites(batch, seed=11):
    """``batch`` with two satellites behind every peak: at +S/z and +2S/z with 0.5x / 0.2x its intensity, z drawn per peak from
    1 .. 3, the peaks sorted again per spectrum"""
    rng = np.random.default_rng(seed)
    mz, it, off = np.asarray(batch["mz"], np.float64), np.asarray(batch["intensity"], np.float64), np.asarray(batch["peak_off"], np.int64)
    z = rng.integers(1, 4, size=mz.size).astype(np.float64)
    spec = np.repeat(np.arange(off.size - 1), np.diff(off))
    x = np.concatenate([mz, mz + S / z, mz + 2 * S / z])
    y = np.concatenate([it, 0.5 * it, 0.2 * it])
    s3 = np.concatenate([spec, spec, spec])
    order = np.lexsort((x, s3))
    return dict(batch, mz=x[order], intensity=y[order], peak_off=3 * off)
