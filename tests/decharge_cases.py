"""Hand-made spectra for the charge-deconvolution rule (include/pyascore_hip.h: pya_decharge_params), shared by
tests/test_decharge_host.py (which pins pyascore_amd.rollup.decharge on the outcome written out here by hand) and
tests/test_gpu_decharge.py (which runs the same spectra through the device), and the builders of the larger inputs of both.
The deisotoping half of the rule has its own cases in tests/deisotope_cases.py; these are about charge, moving and order."""
import numpy as np

import deisotope_cases as dc
from pyascore_amd import rollup as ru, synth

S = dc.S
P0 = ru.decharge_params()                                                 # tol 0.01, charges 1 .. 3, ratio 1, witness 0.3
# everything exact in binary: spacings for charges 1 .. 4, one carrier of mass 1, a witness of one half
TOL_EXACT = 2.0 ** -7
P_EXACT = ru.check_decharge_params(dict(tol=TOL_EXACT, ratio0=1.0, ratio_per_mz=0.0, max_charge=4, spacing=(1.0, 0.5, 0.375, 0.25),
                                        carrier=1.0, witness=0.5))
P_EXACT_2 = ru.check_decharge_params(dict(P_EXACT, max_charge=2, spacing=(1.0, 0.5)))
P_HUGE = ru.check_decharge_params(dict(tol=2.0 ** 100, ratio0=1.0, ratio_per_mz=0.0, max_charge=2, spacing=(2.0 ** 125, 2.0 ** 124),
                                       carrier=1.0, witness=0.5))
NAN, INF = float("nan"), float("inf")


def _c(name, params, x, y, keep, out_mz, out_it, charge, dtype=np.float64, unordered=False):
    x, y = np.asarray(x, dtype), np.asarray(y, dtype)
    assert x.shape == y.shape == (len(keep),), name
    assert len(out_mz) == len(out_it) == len(charge) == int(np.sum(keep)), name
    return dict(name=name, params=params, mz=x, intensity=y, keep=np.asarray(keep, bool), out_mz=np.asarray(out_mz, dtype),
                out_it=np.asarray(out_it, dtype), charge=np.asarray(charge, np.uint8), unordered=unordered)


def hand_cases():
    """One spectrum each: dict(name, params, mz, intensity, keep, out_mz, out_it, charge, unordered)."""
    five_dn = np.nextafter(5.0, 0.0)
    # float32 rounding: a = 700 + 3 ulp (ulp 2^-14); 3 a - 2 = 2098 + 9 * 2^-14 lies between the float32 neighbours
    # 2098 + 2^-11 and 2098 + 2^-11 + 2^-12 and rounds DOWN to the first, the m/z of the unmoved peak behind it
    a32 = 700.0 + 3 * 2.0 ** -14
    tie = 2098.0 + 2.0 ** -11
    assert float(np.float32(a32)) == a32 and float(np.float32(tie)) == tie and float(np.float32(3 * a32 - 2)) == tie and 3 * a32 - 2 > tie
    return [
        # 50.5 at 4+ (child a quarter above) and 100.0 at 2+ (child a half above) both give 199.0; the peak with the lower raw
        # index comes first, the unmoved 199.0 last
        _c("a 4+ and a 2+ peak land on the value of an unmoved peak", P_EXACT, [50.5, 50.75, 100.0, 100.5, 199.0], [10, 6, 12, 6, 7],
           [1, 0, 1, 0, 1], [199.0, 199.0, 199.0], [10, 12, 7], [4, 2, 1]),
        _c("a moved peak passes the last peak of the spectrum", P_EXACT, [100.0, 100.5, 150.0], [10, 6, 3], [1, 0, 1], [150.0, 199.0], [3, 10],
           [1, 2]),
        # 101.0 is the child of 100.0 at z = 1 and of 100.5 at z = 2: it goes, and it testifies for 100.5 (kept: 12 > 10); 100.0
        # has no child at z >= 2 that R admits (100.5 is too intense), and z = 1 moves nothing
        _c("a child that matches z = 1 and z = 2 through different parents", P_EXACT, [100.0, 100.5, 101.0], [10, 12, 7], [1, 1, 0],
           [100.0, 200.0], [10, 12], [1, 2]),
        _c("a witness exactly at y[i] witness", P_EXACT, [100.0, 100.5], [10.0, 5.0], [1, 0], [199.0], [10.0], [2]),
        _c("a witness one ulp below y[i] witness: removed all the same, the parent stays", P_EXACT, [100.0, 100.5], [10.0, five_dn], [1, 0],
           [100.0], [10.0], [1]),
        _c("witness 0 believes any child", dict(P_EXACT, witness=0.0), [100.0, 100.5], [10.0, 0.0], [1, 0], [199.0], [10.0], [2]),
        _c("the largest witnessed charge wins", P_EXACT, [100.0, 100.375, 100.5], [10, 6, 6], [1, 0, 0], [298.0], [10], [3]),
        _c("a charge above max_charge is not tried", P_EXACT_2, [100.0, 100.25, 100.5], [10, 6, 6], [1, 1, 0], [100.25, 199.0], [6, 10], [1, 2]),
        # 0.75 at 2+ would land on 0.5, 1.0 (== carrier) at 4+ on 1.0 itself: neither is above where it was
        _c("peaks with x <= carrier stay", P_EXACT, [0.75, 1.0, 1.25, 1.5], [10, 12, 6, 6], [1, 1, 0, 0], [0.75, 1.0], [10, 12], [1, 1]),
        _c("float32: the rounding of v makes the tie, the moved peak goes first", P_EXACT, [a32, a32 + 0.375, tie], [10, 6, 3], [1, 0, 1],
           [tie, tie], [10, 3], [3, 1], np.float32),
        _c("float64: the same peaks, v stays above the unmoved peak", P_EXACT, [a32, a32 + 0.375, tie], [10, 6, 3], [1, 0, 1],
           [tie, 3 * a32 - 2], [3, 10], [1, 3]),
        _c("a NaN intensity stays, removes nothing, moves nothing and testifies to nothing", P_EXACT, [100.0, 100.5, 200.0, 200.5],
           [NAN, 5, 10, NAN], [1, 1, 1, 1], [100.0, 100.5, 200.0, 200.5], [NAN, 5, 10, NAN], [1, 1, 1, 1]),
        _c("an infinite m/z behind a moved peak", P_EXACT, [100.0, 100.5, INF], [10, 6, 1], [1, 0, 1], [199.0, INF], [10, 1], [2, 1]),
        # 2^127 at 2+ gives 2^128 - 1: beyond float32, where the peak therefore stays; 2^128 in float64
        _c("float32: a value that overflows is not stored, the peak stays", P_HUGE, [2.0 ** 127, 2.0 ** 127 + 2.0 ** 124], [10, 6], [1, 0],
           [2.0 ** 127], [10], [1], np.float32),
        _c("float64: the same peaks, the value is finite", P_HUGE, [2.0 ** 127, 2.0 ** 127 + 2.0 ** 124], [10, 6], [1, 0], [2.0 ** 128], [10], [2]),
        _c("the default parameters: a 2+ and a 3+ fragment", P0, [400.0, 400.0 + S / 3, 500.0, 500.0 + S / 2], [10, 5, 10, 5], [1, 0, 1, 0],
           [500.0 * 2.0 - 1.007825, 400.0 * 3.0 - 2.0 * 1.007825], [10, 10], [2, 3]),
        _c("the default witness of 0.3: a satellite at 0.2 testifies to nothing", P0, [500.0, 500.0 + S / 2], [10, 2], [1, 0], [500.0], [10], [1]),
        _c("a descending pair: the spectrum is copied", P_EXACT, [100.0, 100.5, 90.0], [10, 6, 3], [1, 1, 1], [100.0, 100.5, 90.0], [10, 6, 3],
           [1, 1, 1], unordered=True),
        _c("one peak", P_EXACT, [100.0], [1.0], [1], [100.0], [1.0], [1]),
    ]


def params_key(p):
    return dc.params_key(p) + (p["carrier"], p["witness"])


pack = dc.pack
BOUNDARY_LENGTHS = dc.BOUNDARY_LENGTHS


def charged_boundary_spectra(seed=7):
    """dc.boundary_spectra's ladders with about half of the steps S / 2 or S / 3 and intensities that often fall by less than
    the witness's share: parents of charge 2 and 3 on both sides of every 64-peak boundary, their moved values far up the
    ladder (or beyond its end), across many strides."""
    rng = np.random.default_rng(seed)
    out = []
    for n in BOUNDARY_LENGTHS:
        kind = rng.choice(6, size=n, p=[0.1, 0.25, 0.25, 0.15, 0.05, 0.2])
        step = np.choose(kind, [S, S / 2, S / 3, 0.7313, 0.0, 1.7])
        step = step + np.where(kind < 3, rng.uniform(-0.012, 0.012, size=n), 0.0)
        x = 100.0 + np.cumsum(step)
        y = rng.choice([1.0, 2.0, 3.0, 4.0, 8.0], size=n)
        out.append((x, y))
    return out


def all_moved_spectrum(n=150):
    """every kept peak has a satellite at S / 2 with half its intensity: all of them move"""
    base = 300.0 + 10.0 * np.arange(n)
    x = np.stack([base, base + S / 2], axis=1).reshape(-1)
    y = np.stack([np.full(n, 10.0), np.full(n, 5.0)], axis=1).reshape(-1)
    return x, y


def none_moved_spectrum(n=150):
    """every kept peak has a satellite at S: removed, and no charge above 1"""
    base = 300.0 + 10.0 * np.arange(n)
    x = np.stack([base, base + S], axis=1).reshape(-1)
    y = np.stack([np.full(n, 10.0), np.full(n, 5.0)], axis=1).reshape(-1)
    return x, y


def charged(batch, share, carrier=synth.PROTON):
    """``batch`` with its peaks as multiply charged fragments with isotope envelopes: for every peak, with ``default_rng(3)``,
    z = 2 or 3 with probability ``share``, else 1; the peak goes to (mz + (z - 1) carrier) / z and gets satellites at + S / z and
    + 2 S / z with 0.5x and 0.2x its intensity; sorted again per spectrum."""
    rng = np.random.default_rng(3)
    mz, it, off = np.asarray(batch["mz"], np.float64), np.asarray(batch["intensity"], np.float64), np.asarray(batch["peak_off"], np.int64)
    z = np.where(rng.random(mz.size) < share, rng.integers(2, 4, size=mz.size), 1).astype(np.float64)
    xz = (mz + (z - 1.0) * carrier) / z
    spec = np.repeat(np.arange(off.size - 1), np.diff(off))
    x = np.concatenate([xz, xz + S / z, xz + 2 * S / z])
    y = np.concatenate([it, 0.5 * it, 0.2 * it])
    s3 = np.concatenate([spec, spec, spec])
    order = np.lexsort((x, s3))
    return dict(batch, mz=x[order], intensity=y[order], peak_off=3 * off)


def all_pairs(x, y, p, dtype):
    """The rule with no search and no walk: every pair of peaks of one ascending spectrum as matrices (rows: parent i, columns:
    child j).  Returns (raw indices of the output peaks in output order, the stored m/z as float64 per raw peak, the charge per
    raw peak, keep)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    n = x.size
    removed, c = np.zeros(n, bool), np.ones(n, np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        d = x[None, :] - x[:, None]
        for z, sp in enumerate(p["spacing"], 1):
            e = d - sp
            b = p["ratio0"] + p["ratio_per_mz"] * (x * float(z))
            r = (np.fabs(e) <= p["tol"]) & (y[None, :] <= (y * b)[:, None])
            removed |= r.any(axis=0)
            if z >= 2:
                c[(r & (y[None, :] >= (y * p["witness"])[:, None])).any(axis=1)] = z
        keep = ~removed
        c = np.where(keep, c, 1)
        v = x * c.astype(np.float64) - (c - 1).astype(np.float64) * p["carrier"]
        stored = v.astype(dtype).astype(np.float64)
        moves = (c >= 2) & np.isfinite(stored) & (stored > x)
    value = np.where(moves, stored, x)
    kept = np.flatnonzero(keep)
    return kept[np.argsort(value[kept], kind="stable")], value, np.where(moves, c, 1), keep
