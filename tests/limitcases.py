"""TEST INFRASTRUCTURE: PSMs that sit on the documented limits of the general route -- 511 residues, fragment charge 255,
n_top 16, eight neutral-loss masses, 65 535 peaks, 4 096 theoretical fragments per site assignment (PYA_MAX_LUT_N), more than
15 000 site assignments -- for the eight stages that read a run's retained tables and walk fragments again (evidence, ion
records, named localisations, site tables, site probabilities, ranked localisations, explained ion current, mass-error profile).
tests/test_limitcases_host.py holds the INPUTS to the conditions without which equality with the yardsticks would say little
(a 511-residue PSM whose sites all lie below residue 256 runs the same bits as a 255-residue one), on the reference's answers
and the CPU yardsticks; tests/test_gpu_stage_limits.py holds the device to the yardsticks on them.

2^22 site assignments, the last documented limit, are out of scope: one wavefront walks them all, and the Python yardsticks
over four million records are no test of seconds.

PLANTING.  Every limit PSM is built from a chosen peptide, chosen modifiable residues and a chosen truth: the fragments of
the truth under the case's settings (every ion type, every charge up to the PSM's, every loss variant; from this repository's
CPU restatement of the fragment walk, oracle/ascore_oracle.cpp) are kept with `keep_p`, jittered within 0.4 tolerances and laid
among noise peaks, with synth's intensity laws.  `force` keeps the fragments a case's condition needs (a b ion of size 256, a
charge-8 ion of size > 255) whatever the draw.  The n_top = 16 PSMs (`_ntop16_psm`) are laid in intensity classes so that the
conditions on ranks hold by construction:

    strong   60..80   fragments every site assignment shares, and a quarter of the others
    filler   40..50   eleven peaks in every 100-m/z window, away from the target
    target   30       the b2 ion (charge 1), which lies before the first modifiable residue and so belongs to every
                      assignment: exactly fifteen peaks of its window are made stronger, so it is retained with RANK 15
    mid      20..25   the other fragments that tell site assignments apart: ranks 11 and above behind the fillers
    low      1..5     300 noise peaks

Intensities are whole numbers (count-like, tied).  With the telling fragments mostly at ranks >= 11, the depth at which two
assignments differ most is 10 or more.

CASES: name -> builder; `case(name)` gives (settings, batch, info) with info["limit"] the limit PSMs' indices in the batch,
info["refused"] those the library must refuse, info["sig_caps"] (many_assignments) the caps the site, probability and ranked
stages are run with besides 0: n_sig - 1 of either limit PSM.
Where a case's settings are plain cfg2 ones, six ordinary cfg2 PSMs are shuffled among the limit PSMs, so that a stage's fast
launch and its general launch both run and the id lists matter.
"""
import numpy as np

from oracle import harness, orc
from pyascore_amd import synth

BASE_SETTINGS = synth.make_batch("cfg2", n_psm=1, seed=0)[1]
KEYS = ("n_sig", "best_sig", "best_score", "alt_mask", "ascores")
EIGHT_LOSSES = [["st", 97.9769], ["y", 79.9663], ["ST", 18.01528], ["D", 18.0106], ["E", 17.0265], ["K", 17.0265 + 1.0], ["R", 43.99],
                ["N", 17.5]]                                   # the masses of test_more_than_four_neutral_loss_masses
_CFG4 = dict(fragment_types="bycz", neutral_losses=[["sty", 97.9769]], mz_error=0.02)
N_ORDINARY = 6

_planters = {}


def _planter(settings):
    """this repository's CPU restatement, used for its fragment walk alone"""
    key = repr(sorted(settings.items()))
    if key not in _planters:
        _planters[key] = harness.make_scorer(orc.OracleAscore, settings, kind="oracle")
    return _planters[key]


def peptide_with_sites(rng, L, sites):
    """letters of synth's alphabet with S/T/Y (synth's shares) at the 0-based residues `sites`"""
    base = np.frombuffer(synth.BASE_ALPHABET.encode(), dtype=np.uint8)
    pep = base[rng.integers(0, len(base), size=L)].copy()
    pep[np.asarray(sites)] = np.frombuffer(b"STY", dtype=np.uint8)[rng.choice(3, size=len(sites), p=(0.5, 0.35, 0.15))]
    return bytes(pep).decode()


def truth_fragments(settings, peptide, k, z, n_sites, truth):
    """every fragment of the assignment `truth` (indices into the modifiable residues): (m/z, size, charge, type, loss) arrays"""
    chk = _planter(settings)
    chk.consume_peptide(peptide, k, z)
    sig = np.zeros(n_sites, np.int32)
    sig[np.asarray(truth, np.int64)] = 1
    out = []
    for t in settings["fragment_types"]:
        for c in range(1, z + 1):
            mz, size, loss = chk.fragments(t, c, sig, cap=16384)
            out.append((mz.astype(np.float64), size, np.full(mz.size, c), np.full(mz.size, ord(t)), loss))
    return [np.concatenate(x) for x in zip(*out)]


def _psm(mz, inten, peptide, k, z, truth):
    order = np.argsort(mz, kind="stable")
    return dict(mz=np.asarray(mz, np.float64)[order], intensity=np.asarray(inten, np.float64)[order], peptide=peptide, n_of_mod=int(k),
                max_charge=int(z), truth=np.asarray(truth, np.int64))


def planted_psm(rng, settings, L, sites, k, z, truth, keep_p=0.6, n_noise=300, force=None):
    """one PSM dict for synth.pack_batch; force(size, charge, type, loss) -> bool array of fragments kept whatever the draw"""
    peptide = peptide_with_sites(rng, L, sites)
    mz, size, charge, ftype, loss = truth_fragments(settings, peptide, k, z, len(sites), truth)
    keep = rng.random(mz.size) < keep_p
    if force is not None:
        keep |= force(size, charge, ftype, loss)
    err = settings["mz_error"]
    sig = mz + rng.uniform(-0.4 * err, 0.4 * err, size=mz.size)
    sig_int = rng.lognormal(6.0, 1.2, size=mz.size)
    lo, hi = min(100.0, 0.5 * float(mz.min())), max(2000.0, float(mz.max()) + 100.0)
    noise = rng.uniform(lo, hi, size=n_noise)
    return _psm(np.concatenate([sig[keep], noise]), np.concatenate([sig_int[keep], rng.lognormal(4.5, 1.0, size=n_noise)]), peptide, k, z, truth)


def _ntop16_psm(rng, settings, L, sites, k, z, truth):
    """the intensity classes of the module docstring; the first modifiable residue lies at index 3 or above"""
    assert min(sites) >= 3
    peptide = peptide_with_sites(rng, L, sites)
    mz, size, charge, ftype, loss = truth_fragments(settings, peptide, k, z, len(sites), truth)
    err = settings["mz_error"]
    sites = np.asarray(sites)
    # sites a fragment holds: a forward ion of size s the residues below s, a backward one those from L - s on
    fwd = np.isin(ftype, [ord(c) for c in "abc"])
    held = np.where(fwd, (sites[None, :] < size[:, None]).sum(axis=1), (sites[None, :] >= L - size[:, None]).sum(axis=1))
    telling = (held > 0) & (held < len(sites))
    target = int(np.flatnonzero((ftype == ord("b")) & (size == 2) & (charge == 1) & (loss == 0))[0])
    keep = rng.random(mz.size) < 0.8
    keep[target] = True
    strong = ~telling | (rng.random(mz.size) < 0.25)
    inten = np.where(strong, rng.integers(60, 81, size=mz.size), rng.integers(20, 26, size=mz.size)).astype(np.float64)
    inten[target] = 30.0
    sig = mz + rng.uniform(-0.4 * err, 0.4 * err, size=mz.size)
    t_mz = float(sig[target])
    p_mz, p_int = [sig[keep]], [inten[keep]]
    first, last = int(np.floor(mz.min() / 100.0)), int(np.floor(mz.max() / 100.0))
    for w in range(first, last + 1):                              # eleven fillers per window, away from the target
        f = rng.uniform(100.0 * w, 100.0 * (w + 1), size=11)
        f = f[np.abs(f - t_mz) > 1.0]
        p_mz.append(f)
        p_int.append(rng.integers(40, 51, size=f.size).astype(np.float64))
    noise = rng.uniform(100.0 * first, 100.0 * (last + 1), size=300)
    noise = noise[np.abs(noise - t_mz) > 1.0]
    p_mz.append(noise)
    p_int.append(rng.integers(1, 6, size=noise.size).astype(np.float64))
    p_mz, p_int = np.concatenate(p_mz), np.concatenate(p_int)
    # exactly fifteen peaks of the target's window above the target
    w0 = np.floor(t_mz / 100.0)
    above = np.flatnonzero((np.floor(p_mz / 100.0) == w0) & (p_int > 30.0))
    if above.size > 15:
        p_int[above[np.argsort(p_int[above], kind="stable")[: above.size - 15]]] = 2.0
    elif above.size < 15:
        more = rng.uniform(100.0 * w0, 100.0 * (w0 + 1), size=4 * (15 - above.size))
        more = more[np.abs(more - t_mz) > 1.0][: 15 - above.size]
        assert more.size == 15 - above.size
        p_mz, p_int = np.concatenate([p_mz, more]), np.concatenate([p_int, np.full(more.size, 45.0)])
    near = (np.abs(p_mz - t_mz) <= 1.0) & (p_mz != t_mz)          # nothing else near the target
    return _psm(p_mz[~near], p_int[~near], peptide, k, z, truth)


def _ordinary(seed):
    batch = synth.make_batch("cfg2", n_psm=N_ORDINARY, seed=seed)[0]
    return psm_dicts(batch, range(N_ORDINARY))


def _with_peaks(rng, psm, total, hi=2500.0):
    """a PSM with uniform noise added up to `total` peaks"""
    n = total - psm["mz"].size
    return _psm(np.concatenate([psm["mz"], rng.uniform(100.0, hi, n)]), np.concatenate([psm["intensity"], rng.lognormal(4.0, 1.0, n)]),
                psm["peptide"], psm["n_of_mod"], psm["max_charge"], psm.get("truth", ()))


# ---- the cases: rng -> (settings overrides, limit PSMs, with ordinary PSMs, extra info) -------------------------------------
def _far_positions(rng):
    """L = 511, by, charge 1: five modifiable residues, three of them at index 256 or above, the truth on at least one"""
    psms = []
    for truth in ((2, 3), (1, 4), (0, 2), (3, 4)):
        sites = [int(rng.integers(20, 120)), int(rng.integers(150, 250)), int(rng.integers(260, 330)), int(rng.integers(380, 440)),
                 int(rng.integers(470, 510))]
        psms.append(planted_psm(rng, BASE_SETTINGS, 511, sites, 2, 1, truth, keep_p=0.7, force=lambda s, c, t, l: (s > 255) & (s % 16 == 0)))
    return {}, psms, True, {}


def _byte_edge(rng):
    """L = 255, 256, 257: the last modifiable residue at 1-based position L - 1 or L, and in the truth"""
    psms = []
    for L, last in ((255, 254), (256, 254), (257, 256)):          # 0-based: L - 1, L - 2, L - 1 -- positions 255, 255, 257
        # (the L = 257 PSM has its fourth modifiable residue at position 256, so that 255, 256 and 257 are all written)
        sites = [int(rng.integers(10, 100)), int(rng.integers(120, 200)), int(rng.integers(205, 245)), 255 if L == 257 else L - 6, last]
        psms.append(planted_psm(rng, BASE_SETTINGS, L, sites, 2, 1, (int(rng.integers(0, 3)), 4), keep_p=0.8,
                                force=lambda s, c, t, l: (s >= 254) | (s <= 3)))
    return {}, psms, True, {}


def _row_psm(rng, L):
    sites = [int(rng.integers(10, 60)), int(rng.integers(80, 140)), int(rng.integers(150, 200)), int(rng.integers(210, L - 2))]
    return planted_psm(rng, BASE_SETTINGS, L, sites, 2, 8, (1, 3), keep_p=0.5)


def _last_row(rng):
    """L = 257, charge 8, by, no losses: 256 x 8 x 2 = 4 096 theoretical fragments per site assignment"""
    return {}, [_row_psm(rng, 257), _row_psm(rng, 257)], True, {}


def _past_last_row(rng):
    """the PSMs of last_row's kind around one of 258 residues: 257 x 8 x 2 = 4 112"""
    return {}, [_row_psm(rng, 257), _row_psm(rng, 258), _row_psm(rng, 257)], True, dict(refused_length=258)


def _long_list(rng):
    """L = 511, charge 8, b ions alone: 510 x 8 = 4 080 fragments in the one per-type list"""
    st = dict(BASE_SETTINGS, fragment_types="b")
    psms = []
    for truth in ((1, 3), (2, 4)):
        sites = [int(rng.integers(30, 120)), int(rng.integers(150, 250)), int(rng.integers(260, 330)), int(rng.integers(380, 440)),
                 int(rng.integers(470, 510))]
        psms.append(planted_psm(rng, st, 511, sites, 2, 8, truth, keep_p=0.5, force=lambda s, c, t, l: (c == 8) & (s > 255) & (s % 8 == 0)))
    return dict(fragment_types="b"), psms, False, {}


def _charge(L, z):
    def build(rng):
        psms = []
        for truth in ((0, 2), (1, 3), (2, 4)):
            sites = np.sort(rng.choice(np.arange(1, L - 1), size=5, replace=False)).tolist()
            psms.append(planted_psm(rng, BASE_SETTINGS, L, sites, 2, z, truth, keep_p=0.5, force=lambda s, c, t, l: (c == z) | (c == 129)))
        return {}, psms, False, {}
    build.__doc__ = "L = %d, by, fragment charge %d: %d x %d x 2 = %d fragments per site assignment" % (L, z, L - 1, z, (L - 1) * z * 2)
    return build


def _ntop16(over, z):
    def build(rng):
        st = dict(BASE_SETTINGS, n_top=16, **over)
        psms = []
        for truth in ((0, 2), (1, 3), (2, 4), (0, 4)):
            sites = np.sort(rng.choice(np.arange(3, 19), size=5, replace=False)).tolist()
            psms.append(_ntop16_psm(rng, st, 20, sites, 2, z, truth))
        return dict(n_top=16, **over), psms, False, {}
    build.__doc__ = "n_top = 16, L = 20, charge %d, %s: the intensity classes of _ntop16_psm" % (z, over.get("fragment_types", "by"))
    return build


def _eight_losses_ntop16(rng):
    """L = 20, charge 2, by, eight loss masses, n_top = 16"""
    over = dict(n_top=16, neutral_losses=EIGHT_LOSSES, mz_error=0.02)
    st = dict(BASE_SETTINGS, **over)
    psms = []
    for truth in ((0, 2), (1, 3), (2, 4)):
        sites = np.sort(rng.choice(np.arange(2, 19), size=5, replace=False)).tolist()
        psms.append(planted_psm(rng, st, 20, sites, 2, 2, truth, keep_p=0.6))
    return over, psms, False, {}


def _big_retained(rng):
    """L = 511, n_top = 16, twenty peaks laid into every 100-m/z window of the fragment range: about 12 000 peaks"""
    over = dict(n_top=16)
    psms = []
    for truth in ((2, 3), (1, 4)):
        sites = [int(rng.integers(20, 120)), int(rng.integers(150, 250)), int(rng.integers(260, 330)), int(rng.integers(380, 440)),
                 int(rng.integers(470, 510))]
        p = planted_psm(rng, dict(BASE_SETTINGS, **over), 511, sites, 2, 1, truth, keep_p=0.7, n_noise=0)
        first, last = 1, int(np.floor(p["mz"].max() / 100.0))
        laid = (100.0 * np.arange(first, last + 1)[:, None] + rng.uniform(0.0, 100.0, size=(last + 1 - first, 20))).ravel()
        psms.append(_psm(np.concatenate([p["mz"], laid]), np.concatenate([p["intensity"], rng.lognormal(4.5, 1.0, laid.size)]),
                         p["peptide"], 2, 1, truth))
    return over, psms, False, {}


def _most_peaks(rng):
    """an ordinary cfg2 PSM with noise up to 65 535 peaks"""
    base = psm_dicts(synth.make_batch("cfg2", n_psm=2, seed=8801)[0], range(2))
    return {}, [_with_peaks(rng, base[0], 65535), _with_peaks(rng, base[1], 8193)], True, {}


def _many_assignments(rng):
    """C(20,5) = 15 504 and C(17,8) = 24 310 site assignments"""
    a = psm_dicts(synth.make_batch("cfg2", n_psm=1, seed=8802, L=40, n_sites=20, n_mod=5)[0], [0])
    b = psm_dicts(synth.make_batch("cfg2", n_psm=1, seed=8803, L=30, n_sites=17, n_mod=8)[0], [0])
    return {}, a + b, True, dict(n_sig=(15504, 24310), sig_caps=(15503, 24309))


def _forms(rng):
    """for the one-call, chunked and resident forms: two far_positions PSMs and two n_top = 16 ones among cfg2 PSMs, on one
    scorer with n_top = 16"""
    far = _far_positions(rng)[1][:2]
    top = _ntop16({}, 1)(rng)[1][:2]
    return dict(n_top=16), far + top, True, {}


CASES = {
    "far_positions": _far_positions,
    "byte_edge": _byte_edge,
    "last_row": _last_row,
    "past_last_row": _past_last_row,
    "long_list": _long_list,
    "charge_40": _charge(30, 40),
    "charge_255": _charge(9, 255),
    "ntop16": _ntop16({}, 1),
    "ntop16_cfg4": _ntop16(_CFG4, 4),
    "eight_losses_ntop16": _eight_losses_ntop16,
    "big_retained": _big_retained,
    "most_peaks": _most_peaks,
    "many_assignments": _many_assignments,
    "forms": _forms,
}
NAMES = tuple(CASES)


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


def _seed(name):
    return 8700 + NAMES.index(name)


_cache = {}


def case(name):
    """(settings, batch, info); made once per process and shared -- do not modify.  info: limit (indices of the limit PSMs, in
    the builder's order), refused (indices the library refuses), truth (per limit PSM), and what the builder adds"""
    if name not in _cache:
        rng = np.random.default_rng([_seed(name), 0x11B17])
        over, limit, mixed, extra = CASES[name](rng)
        psms = list(limit) + (_ordinary(_seed(name)) if mixed else [])
        order = rng.permutation(len(psms)) if mixed else np.arange(len(psms))
        where = np.argsort(order)                                # where[j]: the place of PSM j in the batch
        info = dict(extra, limit=[int(where[j]) for j in range(len(limit))], truth=[np.asarray(p.get("truth", ()), np.int64) for p in limit],
                    mixed=mixed)
        info["refused"] = [int(where[j]) for j, p in enumerate(limit) if len(p["peptide"]) == extra.get("refused_length")]
        psms = [{k: v for k, v in psms[j].items() if k != "truth"} for j in order]
        _cache[name] = (dict(BASE_SETTINGS, **over), synth.pack_batch(psms), info)
    return _cache[name]


def sites_of(settings, peptide):
    """0-based modifiable residues, N-terminus first"""
    g, L = settings["mod_group"], len(peptide)
    return [i for i, c in enumerate(peptide) if c in g or (i == 0 and "n" in g) or (i == L - 1 and "c" in g)]


_checkers = {}


def checker(settings, kind="ref"):
    """one checker per (settings, kind) and process"""
    key = (repr(sorted(settings.items())), kind)
    if key not in _checkers:
        _checkers[key] = harness.make_scorer(orc.OracleAscore, settings, kind=kind)
    return _checkers[key]


def bits_of(raw):
    sig = raw["signature"].astype(np.uint64)
    return (sig << np.arange(sig.shape[1], dtype=np.uint64)).sum(axis=1).astype(np.uint64)


def score_psm_by_psm(chk, settings, batch):
    """(res, ps) of a checker through score(), PSM by PSM: the five result arrays in the LIBRARY's layout (alt_mask: residue bits
    up to 64 residues, modifiable-residue bits above -- the checker's own batch form cannot hold the latter) and the
    per-assignment records in the CSR layout of PyAscore.batch_pep_scores(), in the checker's sorted order"""
    n = int(batch["n_psm"])
    max_k = max(1, int(batch["n_of_mod"].max()))
    n_top = int(settings["n_top"])
    res = dict(n_sig=np.zeros(n, np.int32), best_sig=np.zeros(n, np.uint64), best_score=np.zeros(n, np.float32),
               alt_mask=np.zeros((n, max_k), np.uint64), ascores=np.zeros((n, max_k), np.float32))
    parts, off, seqs, alts = dict(sig_bits=[], counts=[], scores=[], weighted_score=[], total_fragments=[]), [0], [], []
    for i in range(n):
        kw = synth.unpack_psm(batch, i)
        chk.score(**kw)
        raw = chk.raw_pep_scores()
        bits = bits_of(raw)
        assert raw["counts"].shape[1] == n_top
        res["n_sig"][i], res["best_sig"][i], res["best_score"][i] = bits.size, bits[0], np.float32(chk.best_score)
        a = np.asarray(chk.ascores, np.float32)
        res["ascores"][i, :a.size] = a
        sites = sites_of(settings, kw["peptide"])
        alt = [np.asarray(s, np.int64) for s in chk.alt_sites]
        for j, pos in enumerate(alt):
            m = 0
            for p in pos.tolist():
                m |= 1 << ((p - 1) if len(kw["peptide"]) <= 64 else sites.index(p - 1))
            res["alt_mask"][i, j] = m
        parts["sig_bits"].append(bits)
        for key in ("counts", "scores", "weighted_score", "total_fragments"):
            parts[key].append(raw[key].copy())
        off.append(off[-1] + bits.size)
        seqs.append(chk.best_sequence)
        alts.append(alt)
    ps = {k: np.concatenate(v) for k, v in parts.items()}
    ps["rec_off"] = np.asarray(off, np.int64)
    res["best_sequence"], res["alt_sites"] = seqs, alts
    return res, ps


_answers = {}


def answer(name, kind="ref"):
    """score_psm_by_psm of a case's checker; computed once per process and shared -- do not modify"""
    if (name, kind) not in _answers:
        settings, batch, _ = case(name)
        _answers[name, kind] = score_psm_by_psm(checker(settings, kind), settings, batch)
    return _answers[name, kind]


def as_golden(res, ps):
    """a checker's answers in the layout of a golden file (harness.collect), for the checks of tests/test_*_ref.py"""
    return dict(n_sig=res["n_sig"], best_score=res["best_score"], best_sig=res["best_sig"], ascores=res["ascores"], alt_mask=res["alt_mask"],
                n_ascores=np.asarray([len(a) for a in res["alt_sites"]], np.int32), best_sequence=np.asarray(res["best_sequence"], dtype=np.str_),
                ps_off=ps["rec_off"], ps_bits=ps["sig_bits"], ps_counts=ps["counts"], ps_scores=ps["scores"], ps_ws=ps["weighted_score"],
                ps_nfrag=ps["total_fragments"])


def queries(name, res, ps):
    """the named-localisation queries of a case, one list per PSM: the runner-up of the checker's sorted list, and for the limit
    PSMs of far_positions the winner with its highest modification moved to the highest free modifiable residue"""
    settings, batch, info = case(name)
    out = []
    for i in range(int(batch["n_psm"])):
        lo, hi = int(ps["rec_off"][i]), int(ps["rec_off"][i + 1])
        q = [int(ps["sig_bits"][lo + 1])] if hi - lo > 1 else [int(res["best_sig"][i])]
        if name == "far_positions" and i in info["limit"]:
            best = int(res["best_sig"][i])
            ns = len(sites_of(settings, synth.unpack_psm(batch, i)["peptide"]))
            top_mod = max(j for j in range(ns) if best >> j & 1)
            top_free = max(j for j in range(ns) if not best >> j & 1)
            q.append((best & ~(1 << top_mod)) | (1 << top_free))
        out.append(q)
    return out


OVER_LIMIT = 17                                                   # include/pyascore_hip.h: PYA_ST_OVER_LIMIT
RANKED_K = 5
_yards = {}


def status_of(name):
    """per-PSM status of a skip_invalid run of the case: OVER_LIMIT for the PSMs the library refuses"""
    _, batch, info = case(name)
    st = np.zeros(int(batch["n_psm"]), np.int32)
    st[info["refused"]] = OVER_LIMIT
    return st


def yardsticks(name, res, ps, sig_cap=0, key=None):
    """every stage's CPU yardstick over the answers (res, ps) of a case, as one dict: evidence; ion_off / ions (canonical order
    per PSM); queries / named_off / named / named_counts / named_scores; site_off / sites; site_probs / psm_probs; ranked
    (RANKED_K rows); cov_off / cov_ions / coverage; mz_profile.  `key`: cache the result per process under (name, key, sig_cap).
    The PSMs of info["refused"] count as set aside."""
    import coverage_ref
    import evidence_ref
    import ions_ref
    import named_ref
    import probs_ref
    import ranked_ref
    import sites_ref
    from pyascore_amd import rollup as ru
    if key is not None and (name, key, sig_cap) in _yards:
        return _yards[name, key, sig_cap]
    settings, batch, info = case(name)
    status = status_of(name) if info["refused"] else None
    r = {k: np.array(res[k]) for k in KEYS}
    if status is not None:
        r["status"] = status
        bad = status != 0
        r["n_sig"][bad], r["best_sig"][bad], r["best_score"][bad], r["ascores"][bad], r["alt_mask"][bad] = -1, 0, -1.0, 0, 0
    out = dict(res=r)
    out["evidence"], _ = evidence_ref.batch_rows(settings, batch, r, ps, synth.unpack_psm)
    out["ion_off"], out["ions"] = ions_ref.batch_records(settings, batch, r, out["evidence"], synth.unpack_psm)
    q = queries(name, res, ps)
    out["queries"] = q
    out["named_off"] = np.concatenate([[0], np.cumsum([len(x) for x in q])]).astype(np.int64)
    q_bits = np.concatenate([np.asarray(x, np.uint64) for x in q])
    out["named"], out["named_counts"], out["named_scores"] = named_ref.batch_records(settings, batch, r, ps, out["named_off"], q_bits, synth.unpack_psm)
    out["site_off"], out["sites"] = sites_ref.batch_records(settings, batch, r, ps, synth.unpack_psm, sig_cap, status)
    off, out["site_probs"], out["psm_probs"] = probs_ref.batch_records(settings, batch, r, ps, synth.unpack_psm, sig_cap, status)
    assert np.array_equal(off, out["site_off"])
    out["ranked"] = ranked_ref.batch_rows(RANKED_K, r, ps, sig_cap, status)
    out["cov_off"], out["cov_ions"], out["coverage"], _ = coverage_ref.batch_records(settings, batch, r, synth.unpack_psm)
    params = ru.mz_profile_params(float(np.float32(settings["mz_error"])), max_rank=settings["n_top"] - 1)
    out["mz_profile"] = ru.mz_profile(out["ion_off"], out["ions"], r["n_sig"], None, 1, params)
    if key is not None:
        _yards[name, key, sig_cap] = out
    return out
