"""TEST INFRASTRUCTURE: PSMs with 31 to 63 modifiable residues, on both sides of every gate that keeps a kernel with 32-bit
signatures away from them.

A site assignment is a 64-bit mask over a PSM's modifiable residues; the library takes up to 63 of them.  Five gates decide
whether a PSM meets code that holds the mask in 32 bits (the count-node tables of score_cnt / score_cntg / score_big, the
count-node front end of the probability and ranked stages), and host_plan refuses 64.  The cases below put PSMs on each side of
each of them; tests/test_manysites_host.py holds the INPUTS to conditions without which equality with the reference would say
little (a 33-site PSM whose winner never uses site 32 runs the same bits as a 32-site one), and
tests/test_gpu_many_sites.py holds the device to the reference on them.

PLANTING.  synth's generator draws the truth uniformly, so the one high site of a 33-site peptide is almost never part of the
winner.  `planted` restates its spectrum synthesis (b and y ladders of the true assignment at charge 1, each kept with
`KEEP_P`, jitter within 0.4 tolerances, 300 noise peaks, the same intensity laws) PSM by PSM with a chosen truth, in three
kinds that take turns:

    straddle   one modified site (k = 1: the only one) drawn from the sites of index >= 32, the others from those below --
               for 33 sites that is bit 32 itself
    low        every modified site below 32
    high       as many modified sites of index >= 32 as there are
    (k > 32 leaves no room below 32 for the modified sites: there the kinds place the UNMODIFIED sites instead)

KEEP_P 0.6, synth's own, was enough for every condition of the host test on every case: nothing had to be raised.  The kept
share of the ladder decides the winner, and the high sites sit at the C-terminal end where the y ladder is short and dense.

CASES: name -> (L, sites, k, PSMs, settings overrides); MIXED: the batches that interleave shapes of one C(n,k) class.  Shapes with k = 0 or
k = sites have one assignment: nothing to localise, no condition on the winner applies to them.  Shapes with k > 32 cannot
keep every modified site below 32; the host test applies the winner conditions to the unmodified sites there (the
complement within the PSM's sites), which is the same question asked of the same bits.
"""
import numpy as np

from oracle import harness, orc
from pyascore_amd import synth

KEEP_P = 0.6
N_NOISE = 300
KEYS = ("n_sig", "best_sig", "best_score", "alt_mask", "ascores")
_STY = ["sty", 97.9769]
_GENERAL = dict(fragment_types="bycz", max_charge=2, neutral_losses=[_STY], mz_error=0.02)

# name -> (L, sites, k, PSMs, settings overrides)
CASES = {
    # plain cfg2 settings (b/y, charge 1, no loss, 0.05 Da)
    "p_40_31_2": (40, 31, 2, 16, {}),              # C = 465: score_cnt
    "p_40_32_2": (40, 32, 2, 16, {}),              # C = 496: score_cnt, the last site count it takes
    "p_40_33_2": (40, 33, 2, 16, {}),              # C = 528: score_signatures
    "p_40_33_1": (40, 33, 1, 16, {}),              # 33 assignments: the fused kernel's two-pass form
    "p_64_63_1": (64, 63, 1, 16, {}),              # 63 assignments
    "p_64_63_62": (64, 63, 62, 16, {}),
    "p_34_32_3": (34, 32, 3, 8, {}),               # C = 4 960: score_big with its count-node table
    "p_36_33_3": (36, 33, 3, 8, {}),               # C = 5 456: score_big without it
    "p_64_40_3": (64, 40, 3, 8, {}),               # C = 9 880
    "p_33_32_30": (33, 32, 30, 16, {}),            # k + 1 = 31: the last k the count-node tables take
    "p_33_32_31": (33, 32, 31, 16, {}),            # k + 1 = 32
    "p_34_33_31": (34, 33, 31, 16, {}),
    "p_64_48_2": (64, 48, 2, 16, {}),
    "p_64_63_2": (64, 63, 2, 16, {}),              # C = 1 953
    "p_64_63_61": (64, 63, 61, 16, {}),
    "p_64_63_3": (64, 63, 3, 4, {}),               # C = 39 711: the general kernel by assignment count
    "p_120_63_2": (120, 63, 2, 8, {}),             # ... and by length
    "p_64_63_0": (64, 63, 0, 8, {}),               # nothing to localise
    "p_64_63_63": (64, 63, 63, 8, {}),
    "p_40_33_2_ntop12": (40, 33, 2, 8, dict(n_top=12)),
    # cfg4-like settings: b/y/c/z, charge 2, the "sty" loss, 0.02 Da -- score_cntg's two gates
    "g_33_32_2": (33, 32, 2, 16, _GENERAL),        # Lm1 = 32, 32 sites: the uniform-loss fast path and the two-word form's last shape
    "g_34_32_2": (34, 32, 2, 16, _GENERAL),        # Lm1 = 33
    "g_34_33_2": (34, 33, 2, 16, _GENERAL),
    "g_40_36_2": (40, 36, 2, 16, _GENERAL),
    "g_48_40_2_err05": (48, 40, 2, 16, dict(_GENERAL, mz_error=0.5)),
}
# the mixed batches: (settings overrides, [(L, sites, k, PSMs)] interleaved PSM by PSM).  One C(n,k) class per pair so that
# the bucket-wide maxima of host_run.cpp's gate are set by the 33-site PSMs for everybody: kBucketLimits is {64, 512, 4096,
# 15000}, so C(32,2) = 496 and C(33,2) = 528 do NOT share a class; C(32,3) = 4 960 and C(33,3) = 5 456 do (score_big under
# plain settings, the bucket's own kernel under general ones), and C(16,3) = 560 / C(12,6) = 924 share C(33,2)'s.
MIXED = {
    "mixed_plain": ({}, [(34, 32, 3, 3), (36, 33, 3, 3), (40, 33, 2, 6), (20, 16, 3, 5), (20, 12, 6, 3), (20, 6, 3, 4)]),
    "mixed_general": (_GENERAL, [(34, 33, 2, 6), (20, 16, 3, 6), (34, 32, 2, 6), (20, 6, 3, 4)]),
}

BASE_SETTINGS = synth.make_batch("cfg2", n_psm=1, seed=0)[1]


def settings_of(name):
    over = MIXED[name][0] if name in MIXED else CASES[name][4]
    return dict(BASE_SETTINGS, **over)


def max_charge_of(settings):
    return 2 if settings["fragment_types"] == "bycz" else 1


def truth_of(rng, n_sites, k, kind):
    """the modified sites (indices into the PSM's modifiable residues, ascending) of a planted PSM.  The kind places the
    MARKED sites: the modified ones, or for k > 32 the unmodified ones (at most 30 then, so they fit either side)"""
    low, high = np.arange(min(n_sites, 32)), np.arange(32, n_sites)
    if k == 0 or k >= n_sites:
        return np.arange(k, dtype=np.int64)
    if high.size == 0:
        return np.sort(rng.choice(n_sites, size=k, replace=False)).astype(np.int64)
    m = k if k <= 32 else n_sites - k
    n_high = {"straddle": 1, "low": 0, "high": min(m, high.size)}[kind]
    marked = np.concatenate([rng.choice(high, size=n_high, replace=False), rng.choice(low, size=m - n_high, replace=False)])
    if k > 32:
        marked = np.setdiff1d(np.arange(n_sites), marked)
    return np.sort(marked).astype(np.int64)


def random_peptide(rng, L, n_sites):
    """(letters uint8[L], positions of its n_sites S/T/Y residues): synth's alphabet and S/T/Y shares"""
    base = np.frombuffer(synth.BASE_ALPHABET.encode(), dtype=np.uint8)
    pep = base[rng.integers(0, len(base), size=L)].copy()
    sites = np.sort(rng.choice(L, size=n_sites, replace=False))
    pep[sites] = np.frombuffer(b"STY", dtype=np.uint8)[rng.choice(3, size=n_sites, p=(0.5, 0.35, 0.15))]
    return pep, sites


def planted_psm(rng, L, n_sites, k, kind, mz_error, max_charge=1, peptide=None, truth=None):
    """one PSM dict for synth.pack_batch: the synthesis of synth._fixed_shape with the truth of `truth_of` (or a given
    peptide and truth)"""
    pep, sites = random_peptide(rng, L, n_sites) if peptide is None else peptide
    truth = truth_of(rng, n_sites, k, kind) if truth is None else np.asarray(truth, np.int64)
    mass = synth._MASS_LUT[pep].copy()
    mass[sites[truth]] += synth.PHOSPHO
    fwd = np.cumsum(mass)[: L - 1]
    rev = np.cumsum(mass[::-1])[: L - 1]
    sig = np.concatenate([fwd + synth.PROTON, rev + synth.WATER + synth.PROTON])
    keep = rng.random(sig.size) < KEEP_P
    sig = sig + rng.uniform(-0.4 * mz_error, 0.4 * mz_error, size=sig.size)
    sig_int = rng.lognormal(6.0, 1.2, size=sig.size)
    mz = np.concatenate([sig[keep], rng.uniform(100.0, 2000.0, size=N_NOISE)])
    inten = np.concatenate([sig_int[keep], rng.lognormal(4.5, 1.0, size=N_NOISE)])
    order = np.argsort(mz, kind="stable")
    return dict(mz=mz[order], intensity=inten[order], peptide=bytes(pep).decode(), n_of_mod=int(k), max_charge=int(max_charge),
                truth=truth)


KINDS = ("straddle", "low", "high")


def planted(L, n_sites, k, n, seed, mz_error, max_charge=1):
    """n planted PSM dicts of one shape; the kinds take turns"""
    rng = np.random.default_rng([int(seed), 0x3A57])
    return [planted_psm(rng, L, n_sites, k, KINDS[i % 3], mz_error, max_charge) for i in range(n)]


def isomer_batch(n_peptides=4, L=64, n_sites=63, seed=7790, mz_error=0.05):
    """for the peptidoform roll-up: every peptide against four spectra whose planted assignments (k = 2) share their low
    site and differ in the high one -- isomers of one group that differ only in the high word of sig_bits.
    -> (batch, group int32[n], planted sig_bits uint64[n])"""
    rng = np.random.default_rng([int(seed), 0x150])
    psms, group, bits = [], [], []
    for g in range(n_peptides):
        peptide = random_peptide(rng, L, n_sites)
        a = int(rng.integers(0, 32))
        h = rng.choice(np.arange(32, n_sites), size=3, replace=False)
        for hi in (h[0], h[1], h[0], h[2]):
            psms.append(planted_psm(rng, L, n_sites, 2, None, mz_error, peptide=peptide, truth=[a, int(hi)]))
            group.append(g)
            bits.append((1 << a) | (1 << int(hi)))
    return synth.pack_batch(psms), np.asarray(group, np.int32), np.asarray(bits, np.uint64)


def high_word_isomers(group, sig):
    """the groups in which two of the assignments `sig` differ, and only in the high word"""
    out = []
    for g in np.unique(group):
        s = sorted(set(int(x) for x in np.asarray(sig)[np.asarray(group) == g]))
        if any(a != b and (a ^ b) & 0xFFFFFFFF == 0 for a in s for b in s):
            out.append(int(g))
    return out


def _seed(name):
    return 7700 + sorted(list(CASES) + list(MIXED)).index(name)


_cache = {}


def case(name):
    """(settings, batch, shape of every PSM as (L, sites, k)); made once per process and shared -- do not modify"""
    if name not in _cache:
        settings = settings_of(name)
        z = max_charge_of(settings)
        if name in MIXED:
            groups = [planted(L, s, k, n, _seed(name) * 100 + j, settings["mz_error"], z) for j, (L, s, k, n) in enumerate(MIXED[name][1])]
            shapes = [sh[:3] for sh in MIXED[name][1]]
            psms, shape = [], []
            for r in range(max(len(g) for g in groups)):                       # interleaved: one PSM of every shape in turn
                for g, sh in zip(groups, shapes):
                    if r < len(g):
                        psms.append(g[r])
                        shape.append(sh)
        else:
            L, s, k, n, _ = CASES[name]
            psms = planted(L, s, k, n, _seed(name), settings["mz_error"], z)
            shape = [(L, s, k)] * n
        _cache[name] = (settings, synth.pack_batch(psms), shape)
    return _cache[name]


_checkers = {}


def checker(settings, kind="ref"):
    """one checker per (settings, kind) and process"""
    key = (repr(sorted(settings.items())), kind)
    if key not in _checkers:
        _checkers[key] = harness.make_scorer(orc.OracleAscore, settings, kind=kind)
    return _checkers[key]


_answers = {}


def answer(name, kind="ref"):
    """the checker's score_batch of a case; computed once per process and shared -- do not modify"""
    if (name, kind) not in _answers:
        settings, batch, _ = case(name)
        _answers[name, kind] = checker(settings, kind).score_batch(batch, max(1, int(batch["n_of_mod"].max())))
    return _answers[name, kind]


def changed(a, b, keys=KEYS):
    """the PSMs for which two results of `score_batch` differ in any of the arrays, byte for byte"""
    bad = np.zeros(np.asarray(a["n_sig"]).size, bool)
    for key in keys:
        x, y = np.ascontiguousarray(a[key]), np.ascontiguousarray(b[key])
        assert x.shape == y.shape and x.dtype == y.dtype, key
        bad |= (x.view(np.uint8).reshape(x.shape[0], -1) != y.view(np.uint8).reshape(y.shape[0], -1)).any(axis=1)
    return np.flatnonzero(bad)


def psm_dicts(batch, idx):
    """the PSMs `idx` of a batch as dicts for synth.pack_batch"""
    out = []
    for i in idx:
        kw = synth.unpack_psm(batch, int(i))
        out.append(dict(mz=kw["mz_arr"], intensity=kw["int_arr"], peptide=kw["peptide"], n_of_mod=kw["n_of_mod"],
                        max_charge=kw["max_fragment_charge"]))
    return out


def take(batch, idx):
    """the PSMs `idx` of a batch, in that order, as a batch"""
    return synth.pack_batch(psm_dicts(batch, idx))


def take_rows(res, idx, keys=KEYS):
    return {k: np.ascontiguousarray(np.asarray(res[k])[np.asarray(idx, np.int64)]) for k in keys}


HIGH = np.uint64(0xFFFFFFFF00000000)


def winner_masks(name, res):
    """per PSM the mask the winner conditions look at: best_sig, or where k > 32 (no assignment avoids the high sites) the
    unmodified sites, best_sig's complement within the PSM's sites"""
    _, _, shape = case(name)
    best = np.asarray(res["best_sig"], np.uint64)
    out = best.copy()
    for i, (_, s, k) in enumerate(shape):
        if k > 32:
            out[i] = np.uint64(((1 << s) - 1) & ~int(best[i]))
    return out
