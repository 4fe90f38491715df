"""CPU yardstick for the ranked localisations (include/pyascore_hip.h: pya_ranked): the K rows of one PSM from its
``pep_scores`` CSR arrays and its winner by plain numpy -- the winner first, every other record by (PepScore descending as
float32, sig bits ascending), the flags from a compare with the row above and with best_score.  pep_scores is pinned to the
reference already; nothing of the library's kernels is involved.  A helper module, not a test file.
"""
import numpy as np

from pyascore_amd._lib import RANKED_DTYPE as _FIELDS

DTYPE = np.dtype(_FIELDS)
NONE, SCORED, OVER = 0, 1, 2
TIED_PREV, IN_BEST_TIE = 1, 2
MAX_K = 64


def psm_rows(top_k, best_sig, best_score, sig_bits, weighted_score, scored=True, sig_cap=0):
    """The ``top_k`` rows of one PSM.  sig_bits / weighted_score: its pep_scores records, in any order; scored False: status
    != 0 or n_sig <= 0; sig_cap: 0 = none."""
    assert 1 <= top_k <= MAX_K
    out = np.zeros(top_k, DTYPE)
    bits = np.asarray(sig_bits, np.uint64)
    if not scored or bits.size == 0:
        return out
    best_sig, best_score = np.uint64(best_sig), np.float32(best_score)
    if sig_cap and bits.size > sig_cap:
        out[0] = (best_sig, best_score, 0, OVER, 0)
        return out
    ws = np.asarray(weighted_score, np.float32)
    others = np.flatnonzero(bits != best_sig)
    assert others.size == bits.size - 1, "best_sig is one of the PSM's site assignments, once"
    order = others[np.lexsort((bits[others], -ws[others].astype(np.float64)))]       # last key first: score desc, then bits asc
    rows = [(best_sig, best_score)] + [(bits[j], ws[j]) for j in order[:top_k - 1]]
    for r, (b, s) in enumerate(rows):
        flags = (TIED_PREV if r and s == rows[r - 1][1] else 0) | (IN_BEST_TIE if s == best_score else 0)
        out[r] = (b, s, r, SCORED, flags)
    return out


def brute_force(best_sig, sig_bits, weighted_score):
    """An independent statement: python tuples, sorted() with a key.  [(bits, score)] of the complete list."""
    recs = [(int(b), float(np.float32(s))) for b, s in zip(sig_bits, weighted_score)]
    first = [r for r in recs if r[0] == int(best_sig)]
    rest = sorted((r for r in recs if r[0] != int(best_sig)), key=lambda r: (-r[1], r[0]))
    return first + rest


def batch_rows(top_k, res, ps, sig_cap=0, status=None):
    """[n_psm, top_k] rows of a batch.  res: best_sig / best_score / n_sig of the run; ps: CSR pep_scores arrays (a golden
    file's ``exp_ps_*`` without the prefix, or ``PyAscore.batch_pep_scores()``); status: per-PSM codes of a skip_invalid run."""
    pick = lambda *names: next(ps[n] for n in names if n in ps)  # noqa: E731
    off, bits, ws = pick("rec_off", "ps_off"), pick("sig_bits", "ps_bits"), pick("weighted_score", "ps_ws")
    n = len(res["n_sig"])
    out = np.zeros((n, top_k), DTYPE)
    for i in range(n):
        lo, hi = int(off[i]), int(off[i + 1])
        scored = res["n_sig"][i] > 0 and (status is None or status[i] == 0)
        out[i] = psm_rows(top_k, res["best_sig"][i], res["best_score"][i], bits[lo:hi], ws[lo:hi], scored, sig_cap)
    return out
