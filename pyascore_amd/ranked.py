"""Ranked localisations: what ``PyAscore.score_batch(ranked=K)`` returns, turned into the columns a report of positional
isomers wants.

Pure Python / numpy: nothing here needs a scorer.  ``ranked`` (``RANKED_DTYPE``, the 16-byte ``pya_ranked`` of
include/pyascore_hip.h) has shape ``[n_psm, K]``: row 0 of a PSM is the reported localisation (``best_sig``, ``best_score``),
the rows behind it are its other site assignments by PepScore descending, equal scores by ascending ``sig_bits``.  Rows at and
beyond the PSM's number of site assignments, and every row of a PSM that was not scored, are zero (``kind == NONE``); a PSM
with more site assignments than the cap of the call has row 0 alone, of kind ``OVER``.
"""
import numpy as np

from . import _lib

RANKED_DTYPE = np.dtype(_lib.RANKED_DTYPE)          # pya_ranked, 16 bytes
assert RANKED_DTYPE.itemsize == 16
NONE, SCORED, OVER = _lib.PYA_RANK_NONE, _lib.PYA_RANK_SCORED, _lib.PYA_RANK_OVER
TIED_PREV, IN_BEST_TIE = _lib.PYA_RANK_TIED_PREV, _lib.PYA_RANK_IN_BEST_TIE
MAX_RANKED = _lib.PYA_MAX_RANKED


def check_k(top_k):
    """``top_k`` as an int in 1 .. 64 (``PYA_MAX_RANKED``); ValueError otherwise."""
    if isinstance(top_k, bool) or int(top_k) != top_k or not 1 <= int(top_k) <= MAX_RANKED:
        raise ValueError("the ranked list length must be an integer in 1 .. %d, not %r" % (MAX_RANKED, top_k))
    return int(top_k)


def _rows(ranked):
    ranked = np.asarray(ranked, RANKED_DTYPE)
    if ranked.ndim == 1:
        ranked = ranked[None, :]
    if ranked.ndim != 2:
        raise ValueError("expected ranked records of shape (n_psm, K)")
    return ranked


def lengths(ranked):
    """Rows that hold a site assignment, per PSM (int64): ``min(n_sig, K)`` for a scored PSM, 1 for a PSM over the cap, 0 for
    one that was not scored."""
    return (_rows(ranked)["kind"] != NONE).sum(axis=1).astype(np.int64)


def within(ranked, gap):
    """Boolean ``[n_psm, K]``: the rows whose PepScore lies no more than ``gap`` below the reported localisation's (row 0
    among them) -- "all assignments within 3 PepScore units of the winner".  Only rows of kind ``SCORED`` count."""
    ranked = _rows(ranked)
    score = ranked["pep_score"].astype(np.float64)
    return (ranked["kind"] == SCORED) & (score[:, :1] - score <= float(gap))


def best_tie_size(ranked):
    """How many of a PSM's listed site assignments have the best PepScore, the reported localisation among them (int64): 1
    when the winner stands alone, 0 for a PSM that was not scored or is over the cap.  A count equal to K may be cut short by
    the list length: ask for a longer list."""
    ranked = _rows(ranked)
    return ((ranked["kind"] == SCORED) & (ranked["flags"] & IN_BEST_TIE != 0)).sum(axis=1).astype(np.int64)
