"""CPU yardstick for the evidence records (include/pyascore_hip.h: pya_evidence): the rows of one PSM from parts that
are pinned to the reference already -- PyBinnedSpectra, PyModifiedPeptide (consume_peak / has_match / get_match /
get_site_determining_ions) and PyBinomialDist of pyascore_amd.aux (tests/test_aux_api.py holds them to the reference's
own unit tests), and the depth scores of ``pep_scores``.  It follows cpp/Ascore.cpp:157-254 line by line; nothing of
the library's kernels is involved.  A helper module, not a test file.

What is handed in per PSM: the winner (``best_sig``), the alternative positions of every modified site (``alt_mask``),
and the PSM's score containers (signature bits -> n_top depth scores, PepScore) -- from a golden file's ``exp_ps_*``
arrays or from ``PyAscore.batch_pep_scores()``.
"""
import numpy as np

from pyascore_amd import aux
from pyascore_amd._lib import EVIDENCE_DTYPE as _FIELDS

DTYPE = np.dtype(_FIELDS)
NONE, COUNTED, TIED = 0, 1, 2


def modifiable_positions(peptide, mod_group):
    """0-based residues that can carry the modification, N-terminus first (ModifiedPeptide.cpp:24-79)."""
    L = len(peptide)
    return [i for i, c in enumerate(peptide)
            if c in mod_group or (i == 0 and "n" in mod_group) or (i == L - 1 and "c" in mod_group)]


def alt_positions(mask, peptide, sites):
    """1-based peptide positions of one alt_mask word: residue bits up to 64 residues, modifiable-residue bits above."""
    m = int(mask)
    if len(peptide) <= 64:
        return [p + 1 for p in range(64) if (m >> p) & 1]
    return [sites[j] + 1 for j in range(min(len(sites), 64)) if (m >> j) & 1]


def score(settings, depth, trials, count):
    """|-10 log10 P(X >= count)|, X ~ Binomial(trials, 2 mz_error (depth + 1) / 100), in the reference's float chain
    (Ascore.cpp:28-33, :199-207)."""
    t = np.float32(np.float32(2) * np.float32(settings["mz_error"])) * np.float32(depth + 1)
    prob = np.float32(float(t) / 100.)
    l10 = np.float32(aux.PyBinomialDist(float(prob)).log10_pvalue(int(count), int(trials)))
    return np.float32(abs(np.float32(-10) * l10))


def matcher(settings, kw):
    """A PyModifiedPeptide that has consumed the peptide and every retained peak of the spectrum (Ascore.pyx:103-152)."""
    spec = aux.PyBinnedSpectra(settings["bin_size"], settings["n_top"])
    spec.consume_spectra(np.ascontiguousarray(kw["mz_arr"], np.float64), np.ascontiguousarray(kw["int_arr"], np.float64))
    mp = aux.PyModifiedPeptide(settings["mod_group"], settings["mod_mass"], settings["mz_error"], settings["fragment_types"])
    for group, mass in settings.get("neutral_losses", []):
        mp.add_neutral_loss(group, mass)
    mp.consume_peptide(kw["peptide"], kw["n_of_mod"], kw["max_fragment_charge"], kw.get("aux_mod_pos"), kw.get("aux_mod_mass"))
    spec.reset_bin()
    while spec.bin < spec.n_bins:
        spec.reset_rank()
        while spec.rank < spec.n_peaks:
            mp.consume_peak(spec.mz, spec.rank)
            spec.next_rank()
        spec.next_bin()
    return mp


def ambiguity(settings, mp, kw, ref, other, n_sites):
    """Ascore::calculateAmbiguity (Ascore.cpp:157-210) with everything it holds: returns (value, kind, depth, ref_matched,
    ref_possible, comp_matched, comp_possible).  ref / other: (signature bits, depth scores, PepScore)."""
    if abs(np.float32(ref[2]) - np.float32(other[2])) < 1e-6:
        return np.float32(0.), TIED, 0, 0, 0, 0, 0
    best, depth = np.float32(0.), 0
    for d in range(len(ref[1])):
        diff = np.float32(ref[1][d]) - np.float32(other[1][d])
        if diff > best:
            best, depth = diff, d
    sig = [np.array([(b >> j) & 1 for j in range(n_sites)], np.uint32) for b in (int(ref[0]), int(other[0]))]
    counts, trials = [0, 0], [0, 0]
    for ftype in settings["fragment_types"]:
        ions = mp.get_site_determining_ions(sig[0], sig[1], ftype, kw["max_fragment_charge"])
        for side in (0, 1):
            trials[side] += len(ions[side])
            for mz in ions[side]:
                m = mp.get_match(mz)
                if m is not None and m[1] <= depth:
                    counts[side] += 1
    value = np.float32(score(settings, depth, trials[0], counts[0]) - score(settings, depth, trials[1], counts[1]))
    return value, COUNTED, depth, counts[0], trials[0], counts[1], trials[1]


def rows(settings, kw, best_sig, alt_mask, ascores, containers, max_k=None):
    """The evidence rows of one PSM (structured array [max_k]) and the Ascore each counted row stands for.

    kw: the PSM as ``synth.unpack_psm`` gives it; best_sig / alt_mask / ascores: its results; containers: dict
    signature bits -> (depth scores, PepScore) of its localisations (empty / None for a PSM that was not scored)."""
    k = int(kw["n_of_mod"])
    max_k = max(k, 1) if max_k is None else max_k
    out = np.zeros(max_k, DTYPE)
    values = [None] * max_k
    if not containers:
        return out, values
    peptide = kw["peptide"]
    sites = modifiable_positions(peptide, settings["mod_group"])
    best = int(best_sig)
    mod_idx = [j for j in range(len(sites)) if (best >> j) & 1]
    if len(mod_idx) != k or k >= len(sites):
        return out, values
    mp = None
    ref = (best,) + tuple(containers[best])
    for a in range(k):
        if np.isinf(ascores[a]):
            continue
        positions = alt_positions(alt_mask[a], peptide, sites)
        if not positions:
            continue
        if mp is None:
            mp = matcher(settings, kw)
        chosen = None
        for pos in positions:                                   # ascending: the smallest position wins among equals
            j = sites.index(pos - 1)
            comp = (best & ~(1 << mod_idx[a])) | (1 << j)
            other = (comp,) + tuple(containers[comp])
            res = ambiguity(settings, mp, kw, ref, other, len(sites))
            if res[1] == TIED:
                chosen = (pos, other[2]) + res
                break
            if chosen is None or res[0] < chosen[2]:
                chosen = (pos, other[2]) + res
        pos, comp_ws, value, kind, depth, c0, t0, c1, t1 = chosen
        out[a] = (np.float32(comp_ws), pos, depth, kind, c0, t0, c1, t1)
        values[a] = value
    return out, values


def containers_of(ps, lo, hi):
    """signature bits -> (depth scores, PepScore) from CSR pep_scores arrays (``sig_bits``/``bits``, ``scores``, ``ws``)."""
    bits = ps["sig_bits"] if "sig_bits" in ps else ps["ps_bits"]
    scores = ps["scores"] if "scores" in ps else ps["ps_scores"]
    ws = ps["weighted_score"] if "weighted_score" in ps else ps["ps_ws"]
    return {int(bits[r]): (np.asarray(scores[r], np.float32), np.float32(ws[r])) for r in range(lo, hi)}


def batch_rows(settings, batch, res, ps, unpack, rec_off=None):
    """rows() for every PSM of a batch: res = the batch results (best_sig, alt_mask, ascores, n_sig; optional status),
    ps = its pep_scores in CSR form with offsets ``rec_off`` (default ps["rec_off"] / ps["ps_off"])."""
    if rec_off is None:
        rec_off = ps["rec_off"] if "rec_off" in ps else ps["ps_off"]
    n, max_k = int(batch["n_psm"]), res["ascores"].shape[1]
    out = np.zeros((n, max_k), DTYPE)
    values = []
    for i in range(n):
        bad = ("status" in res and res["status"][i]) or res["n_sig"][i] <= 0
        cont = {} if bad else containers_of(ps, int(rec_off[i]), int(rec_off[i + 1]))
        out[i], v = rows(settings, unpack(batch, i), res["best_sig"][i], res["alt_mask"][i], res["ascores"][i], cont, max_k)
        values.append(v)
    return out, values
