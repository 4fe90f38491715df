"""CPU yardstick for the named-localisation records (include/pyascore_hip.h: pya_named): the record of one (PSM,
signature) from parts that are pinned to the reference already -- the PSM's score containers (``pep_scores``), and
``evidence_ref.ambiguity``: PyModifiedPeptide's site-determining ions and matches and PyBinomialDist of pyascore_amd.aux,
following cpp/Ascore.cpp:157-210 line by line for ANY two signatures, not only single moves.  Nothing of the library's
kernels is involved.  A helper module, not a test file.
"""
import numpy as np

import evidence_ref
from pyascore_amd._lib import NAMED_DTYPE as _FIELDS

DTYPE = np.dtype(_FIELDS)
NONE, INVALID, WINNER, TIED, COUNTED = 0, 1, 2, 3, 4


def containers_of(ps, lo, hi):
    """signature bits -> (counts, depth scores, PepScore, total fragments) from CSR pep_scores arrays (a golden file's
    ``exp_ps_*`` arrays without their prefix, or ``PyAscore.batch_pep_scores()``)."""
    pick = lambda *names: next(ps[n] for n in names if n in ps)  # noqa: E731
    bits, counts, scores = pick("sig_bits", "ps_bits"), pick("counts", "ps_counts"), pick("scores", "ps_scores")
    ws, nfrag = pick("weighted_score", "ps_ws"), pick("total_fragments", "ps_nfrag")
    return {int(bits[r]): (np.asarray(counts[r], np.int32), np.asarray(scores[r], np.float32), np.float32(ws[r]), int(nfrag[r]))
            for r in range(lo, hi)}


def record(settings, kw, best_sig, containers, query, mp=None):
    """One record (a DTYPE scalar as a 0-d array) and the counts / scores rows of its container.

    kw: the PSM as ``synth.unpack_psm`` gives it; best_sig: the winner the run reported; containers: ``containers_of`` for
    the PSM (empty / None: the PSM was not scored); query: signature bits; mp: ``evidence_ref.matcher(settings, kw)`` to
    reuse over the queries of a PSM."""
    n_top = int(settings["n_top"])
    out = np.zeros((), DTYPE)
    out["sig_bits"] = np.uint64(query)
    zero_rows = (np.zeros(n_top, np.int32), np.zeros(n_top, np.float32))
    if not containers:
        return out, zero_rows                                    # NONE
    k = int(kw["n_of_mod"])
    n_sites = len(evidence_ref.modifiable_positions(kw["peptide"], settings["mod_group"]))
    best, query = int(best_sig), int(query)
    if query != best and (bin(query).count("1") != k or query >> n_sites):
        out["kind"] = INVALID
        return out, zero_rows
    counts, scores, ws, nfrag = containers[query]
    out["pep_score"], out["total_fragments"] = ws, nfrag
    out["n_moved"] = k - bin(query & best).count("1")
    if query == best:
        out["kind"] = WINNER
        return out, (counts, scores)
    ref = (best,) + tuple(containers[best][1:3])
    value, kind, depth, c0, t0, c1, t1 = evidence_ref.ambiguity(settings, mp or evidence_ref.matcher(settings, kw), kw, ref,
                                                                (query, scores, ws), n_sites)
    if kind == evidence_ref.TIED:
        out["kind"] = TIED
        return out, (counts, scores)
    out["kind"], out["ambiguity"], out["depth"] = COUNTED, value, depth
    out["ref_matched"], out["ref_possible"], out["comp_matched"], out["comp_possible"] = c0, t0, c1, t1
    return out, (counts, scores)


def batch_records(settings, batch, res, ps, q_off, q_bits, unpack, rec_off=None):
    """record() for every query of a batch: res = the batch results (best_sig, n_sig; optional status), ps = its pep_scores
    in CSR form.  Returns (records [n_q], counts [n_q, n_top], scores [n_q, n_top])."""
    if rec_off is None:
        rec_off = ps["rec_off"] if "rec_off" in ps else ps["ps_off"]
    n_q, n_top = int(q_off[-1]), int(settings["n_top"])
    out, counts, scores = np.zeros(n_q, DTYPE), np.zeros((n_q, n_top), np.int32), np.zeros((n_q, n_top), np.float32)
    for i in range(int(batch["n_psm"])):
        if q_off[i] == q_off[i + 1]:
            continue
        bad = ("status" in res and res["status"][i]) or res["n_sig"][i] <= 0
        cont = {} if bad else containers_of(ps, int(rec_off[i]), int(rec_off[i + 1]))
        kw = unpack(batch, i)
        mp = None if bad else evidence_ref.matcher(settings, kw)
        for q in range(int(q_off[i]), int(q_off[i + 1])):
            out[q], (counts[q], scores[q]) = record(settings, kw, res["best_sig"][i], cont, q_bits[q], mp)
    return out, counts, scores


def single_moves(best_sig, n_sites):
    """every signature that moves ONE modification of ``best_sig`` to an unmodified site, by (site index j of the moved
    modification among the modified ones, target site)"""
    best = int(best_sig)
    mods = [j for j in range(n_sites) if best >> j & 1]
    return [(a, t, (best & ~(1 << m)) | (1 << t)) for a, m in enumerate(mods) for t in range(n_sites) if not best >> t & 1]
