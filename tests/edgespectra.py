"""TEST INFRASTRUCTURE: spectra whose peaks sit on the ends of the match window under GENERAL settings.

The reference matches a peak to a fragment f when `f32(f - err) < peak < f32(f + err)` and visits only fragments with
`f >= peak - 0.5` (cpp/ModifiedPeptide.cpp:126-142).  A kernel that places an end one float32 ulp off -- `<=` for `<`,
`f +- err` in double, a charge quotient that is faithful but not correctly rounded, a count-node envelope one ulp too narrow
under a loss class -- stays bit-equal on spectra of uniform noise: measured with the reference's own core, moving every peak
of a general batch up by one ulp changes 0 to 7 PSMs in a hundred.  The batches made here change
for most of their PSMs (the table below; tests/test_edgespectra_host.py holds every case to at least half).

The theoretical ions are NOT restated: `edge_batch` asks the checker (`consume_peptide`, then `fragments(type, z, sig)` for
every ion type, every charge 1..max_charge and a few random site assignments) and so gets the reference's float32 m/z with
charge division and neutral-loss variants as the reference computes them.  Every peak m/z and intensity is a float32 value
held in float64, so "one ulp" means the same on the float64 and the float32 input path and `synth.narrow_batch` loses
nothing.  Peaks per fragment, mixed with every third peak of the batch's own spectrum, sorted, lognormal intensities:

    ends    f32(f - err) or f32(f + err), computed in float32 as the reference does; half of them moved by j ulps,
            j in -3..3 (0: the end itself, the last value outside), the other half by a uniform offset within +- err/4
    half    f32(f + 0.5) moved by j ulps, j in -2..2: the `- 0.5` cut, which takes part for err >= 0.5 only
    pairs   two peaks inside one window, f - err/3 and f + err/3 (random intensities decide which has the lower rank),
            and a third just outside an end (the end itself or one ulp further out: the last two values that do not
            match): the minimum over ranks

A spectrum stays below MAX_PEAKS peaks (the fast kernels' 8 192 with room to spare): where the fragments of the drawn site
assignments would make more, a random subset of them gets peaks.

PSMs of each case (24, or 4 on the general kernel) for which `nudge(+1)` changes n_sig, best_sig, best_score, alt_mask or an
Ascore, reference core alone (`sharpness`; asserted >= half by tests/test_edgespectra_host.py):

    case                  ends  half  pairs
    cfg4                    24     -     24
    bycz_z3_sty             24     -     24
    z2_st                   24     -     24
    Zc_z3_STY               24     -     24
    L30_210_z3              24     -     24
    cfg3_z2_err03           24     -     24
    z6                      24     -     24
    z7                      24     -     24
    three_losses            24     -     24
    nSTY_bycz               24     -     24
    cfg4_err05              24    24     24
    z3_sty_err075           24    24     24
    z2_err4                 21    24     24
    gk_L70                   4     -      4
    gk_n_top12               4     -      4
    gk_five_losses           4     -      4
    gk_z17                   4     -      4
"""
import numpy as np

from oracle import harness, orc
from pyascore_amd import synth

MAX_PEAKS = 6000
MIN_MZ = 50.0
KEYS = ("n_sig", "best_sig", "best_score", "alt_mask", "ascores")

_STY = ("sty", 97.9769)
_FIVE = [["st", 97.9769], ["y", 79.9663], ["ST", 18.01528], ["D", 18.0106], ["E", 17.0265]]

# name -> (config, PSMs, synth.make_batch overrides, settings overrides, site assignments drawn per PSM)
CASES = {
    "cfg4": ("cfg4", 24, {}, {}, 4),                                                     # b/y/c/z, charge <= 4, loss on s/t/y
    "bycz_z3_sty": ("cfg2", 24, dict(fragment_types="bycz", max_charge=3, neutral_loss=_STY), {}, 4),
    "z2_st": ("cfg2", 24, dict(max_charge=2, neutral_loss=("st", 97.9769)), {}, 6),       # loss classes differ: score_cntg walks
    "Zc_z3_STY": ("cfg2", 24, dict(fragment_types="Zc", max_charge=3, neutral_loss=("STY", 18.01528)), {}, 6),
    "L30_210_z3": ("cfg2", 24, dict(L=30, n_sites=10, n_mod=4, max_charge=3, neutral_loss=_STY, mz_error=0.01), {}, 4),   # C(10,4) = 210: count nodes
    "cfg3_z2_err03": ("cfg3", 24, dict(max_charge=2, neutral_loss=_STY, mz_error=0.3), {}, 6),
    "z6": ("cfg2", 24, dict(max_charge=6, mz_error=0.01), {}, 6),                          # the FMA division: charges 3, 5, 6 ...
    "z7": ("cfg2", 24, dict(max_charge=7, mz_error=0.01), {}, 6),                          # ... and 7
    "three_losses": ("cfg4", 24, {}, dict(neutral_losses=[["sty", 97.9769], ["ST", 18.01528], ["m", 63.998]]), 4),
    "nSTY_bycz": ("cfg2", 24, dict(fragment_types="bycz", max_charge=2, neutral_loss=_STY), dict(mod_group="nSTY"), 4),
    "cfg4_err05": ("cfg4", 24, dict(mz_error=0.5), {}, 4),
    "z3_sty_err075": ("cfg2", 24, dict(max_charge=3, neutral_loss=_STY, mz_error=0.75), {}, 6),
    "z2_err4": ("cfg2", 24, dict(max_charge=2, mz_error=4.0), {}, 6),
    # the general kernel (csrc/general_psm.hip)
    "gk_L70": ("cfg2", 4, dict(L=70, n_sites=4, n_mod=2, fragment_types="bycz", max_charge=2, mz_error=0.02, neutral_loss=_STY), {}, 2),
    "gk_n_top12": ("cfg2", 4, {}, dict(n_top=12), 8),
    "gk_five_losses": ("cfg2", 4, dict(L=20, n_sites=5, n_mod=2, max_charge=2, mz_error=0.02), dict(neutral_losses=_FIVE), 6),
    "gk_z17": ("cfg2", 4, dict(L=44, n_sites=5, n_mod=2, fragment_types="y", max_charge=17, neutral_loss=_STY), {}, 4),   # 43 x 17 x 3 loss sums = 2 193 fragments: above the fast kernels' 2 048 per type, inside the score table's 4 096
}


def placements(settings):
    """the placements a case is run with: the `- 0.5` cut can decide only where the tolerance reaches it"""
    return ("ends", "half", "pairs") if settings["mz_error"] >= 0.5 else ("ends", "pairs")


def base_case(name):
    """(batch, settings) of a case before its peaks are replaced"""
    cfg, n, over, st_over, _ = CASES[name]
    batch, settings = synth.make_batch(cfg, n_psm=n, seed=7100 + sorted(CASES).index(name), **over)
    return batch, dict(settings, **st_over)


_checkers = {}


def checker(settings, kind="ref"):
    """one checker per (settings, kind) and process: its first score under several loss masses takes seconds"""
    key = (repr(sorted(settings.items())), kind)
    if key not in _checkers:
        _checkers[key] = harness.make_scorer(orc.OracleAscore, settings, kind=kind)
    return _checkers[key]


def ulps(x, j):
    """float32 array `x` (positive, finite) moved by `j` float32 ulps (`j`: an integer or an integer array)"""
    x = np.ascontiguousarray(x, np.float32)
    return (x.view(np.int32) + np.asarray(j, np.int32)).view(np.float32)


def theoretical_ions(chk, settings, peptide, n_of_mod, max_charge, aux_pos, aux_mass, rng, n_assign):
    """the distinct float32 fragment m/z the checker makes for `n_assign` random site assignments of a peptide: every ion
    type, every charge 1..max_charge, neutral-loss variants included"""
    chk.consume_peptide(peptide, n_of_mod, max_charge, aux_pos if len(aux_pos) else None, aux_mass if len(aux_pos) else None)
    n_sites = int(chk.lib.orc_sig_len(chk.h))
    out = []
    for _ in range(n_assign):
        sig = np.zeros(n_sites, np.int32)
        sig[rng.choice(n_sites, size=min(n_of_mod, n_sites), replace=False)] = 1
        for t in settings["fragment_types"]:
            for z in range(1, max_charge + 1):
                out.append(chk.fragments(t, z, sig, cap=8192)[0].copy())
    f = np.unique(np.concatenate(out))
    return f[f > MIN_MZ + 8.0]


def _peaks(f, err, placement, rng):
    """float32 peak m/z for the float32 fragments `f`"""
    err32 = np.float32(err)
    n = f.size
    if placement == "ends":
        end = np.where(rng.random(n) < 0.5, f - err32, f + err32).astype(np.float32)          # float32 arithmetic, as the reference's
        by_ulp = rng.random(n) < 0.5
        wide = (end.astype(np.float64) + rng.uniform(-err / 4, err / 4, n)).astype(np.float32)
        return np.where(by_ulp, ulps(end, rng.integers(-3, 4, n)), wide)
    if placement == "half":
        return ulps((f.astype(np.float64) + 0.5).astype(np.float32), rng.integers(-2, 3, n))
    if placement == "pairs":
        inside = [(f.astype(np.float64) + s * err / 3).astype(np.float32) for s in (-1.0, 1.0)]
        out = rng.integers(0, 2, n)                                   # 0: the end itself, 1: one ulp further out -- neither matches
        outside = np.where(rng.random(n) < 0.5, ulps((f - err32).astype(np.float32), -out), ulps((f + err32).astype(np.float32), out))
        return np.concatenate(inside + [outside])
    raise ValueError(placement)


def edge_batch(batch, settings, placement, seed, n_assign=6, kind="ref"):
    """`batch` with every spectrum replaced by edge peaks of the given placement (see the module's docstring) plus every third
    peak of its own; m/z and intensities are float32 values in float64 arrays."""
    rng = np.random.default_rng(seed)
    chk = checker(settings, kind)
    per = 3 if placement == "pairs" else 1
    mzs, its, offs = [], [], [0]
    for i in range(int(batch["n_psm"])):
        kw = synth.unpack_psm(batch, i)
        f = theoretical_ions(chk, settings, kw["peptide"], kw["n_of_mod"], kw["max_fragment_charge"], kw.get("aux_mod_pos", ()),
                             kw.get("aux_mod_mass", ()), rng, n_assign)
        own = np.asarray(kw["mz_arr"], np.float64)[::3].astype(np.float32)
        room = (MAX_PEAKS - own.size) // per
        if f.size > room:
            f = np.sort(rng.choice(f, size=room, replace=False))
        m = np.concatenate([_peaks(f, settings["mz_error"], placement, rng), own])
        m = np.sort(m[m > MIN_MZ]).astype(np.float64)
        mzs.append(m)
        its.append(rng.lognormal(5.0, 1.0, m.size).astype(np.float32).astype(np.float64))
        offs.append(offs[-1] + m.size)
    return dict(batch, mz=np.concatenate(mzs), intensity=np.concatenate(its), peak_off=np.asarray(offs, np.int64))


_cache = {}


def case_batches(name, kind="ref"):
    """(settings, {placement: batch}) of a case; made once per process and shared -- do not modify"""
    if (name, kind) not in _cache:
        batch, settings = base_case(name)
        n_assign = CASES[name][4]
        _cache[name, kind] = (settings, {p: edge_batch(batch, settings, p, 7300 + 10 * sorted(CASES).index(name) + j, n_assign, kind)
                                         for j, p in enumerate(placements(settings))})
    return _cache[name, kind]


def nudge(batch, k):
    """`batch` with every peak m/z (rounded to float32 first) moved by `k` float32 ulps; the array keeps its type"""
    mz = np.asarray(batch["mz"])
    return dict(batch, mz=np.ascontiguousarray(ulps(mz.astype(np.float32), k), mz.dtype))


def changed(a, b):
    """the PSMs for which two results of `score_batch` differ in any of the five arrays"""
    bad = np.zeros(a["n_sig"].size, bool)
    for key in KEYS:
        x, y = np.asarray(a[key]), np.asarray(b[key])
        d = x.view(np.uint8).reshape(x.shape[0], -1) != y.view(np.uint8).reshape(y.shape[0], -1)
        bad |= d.any(axis=1)
    return np.flatnonzero(bad)


def sharpness(settings, batch, kind="ref", k=1):
    """how many PSMs of `batch` the checker scores differently once every peak is moved by `k` ulps"""
    chk = checker(settings, kind)
    mk = int(batch["n_of_mod"].max())
    return int(changed(chk.score_batch(batch, mk), chk.score_batch(nudge(batch, k), mk)).size)
