"""Site tables: what ``PyAscore.score_batch(sites=True)`` returns, turned into the numbers a site-level report wants.

Pure Python / numpy: nothing here needs a scorer.  A record (``SITE_DTYPE``, the 32-byte ``pya_site`` of
include/pyascore_hip.h) belongs to one modifiable residue of one PSM and holds the best PepScore among the site assignments
that modify the residue (``with_score``, attained by ``with_sig``) and the best among those that leave it unmodified
(``without_score`` / ``without_sig``); the records of PSM i are ``sites[site_off[i]:site_off[i + 1]]``, N- to C-terminus.
"""
import numpy as np

from . import _lib

SITE_DTYPE = np.dtype(_lib.SITE_DTYPE)              # pya_site, 32 bytes
assert SITE_DTYPE.itemsize == 32
SITE_KINDS = ("none", "scored", "over")
NONE, SCORED, OVER = _lib.PYA_SITE_NONE, _lib.PYA_SITE_SCORED, _lib.PYA_SITE_OVER
IN_BEST, WITH_TIED, WITHOUT_TIED, NO_WITHOUT = (_lib.PYA_SITE_IN_BEST, _lib.PYA_SITE_WITH_TIED, _lib.PYA_SITE_WITHOUT_TIED,
                                                _lib.PYA_SITE_NO_WITHOUT)


def deltas(sites):
    """``with_score - without_score`` per record (float32): how much the best localisation with the residue modified leads
    the best one without it (negative for a residue the winner leaves alone).  NaN where the record has no such pair: not
    scored, over the cap, no assignment on one side (``PYA_SITE_NO_WITHOUT``, n_of_mod 0)."""
    sites = np.asarray(sites, SITE_DTYPE)
    d = (sites["with_score"] - sites["without_score"]).astype(np.float32)
    no_pair = (sites["kind"] != SCORED) | (sites["with_score"] < 0) | (sites["without_score"] < 0)
    d[no_pair] = np.nan
    return d


def runner_up(sites, site_off, best_sig):
    """Per PSM the best site assignment that differs from the winner: dict(sig u64[n], score f32[n], delta f32[n], found
    bool[n]).  An assignment differs from ``best_sig`` exactly when it leaves one of the winner's residues unmodified, so
    it is the ``without_sig`` / ``without_score`` of the winner's residue whose ``without_score`` is largest (the first
    such residue among equals).  ``delta`` = the winner's PepScore - ``score``.  ``found`` is False -- sig 0, score -1,
    delta NaN -- for a PSM that was not scored, is over the cap, or has a single site assignment."""
    sites = np.asarray(sites, SITE_DTYPE)
    site_off = np.asarray(site_off, np.int64)
    n = site_off.size - 1
    out = dict(sig=np.zeros(n, np.uint64), score=np.full(n, -1, np.float32), delta=np.full(n, np.nan, np.float32),
               found=np.zeros(n, bool))
    best_sig = np.asarray(best_sig, np.uint64)
    for i in range(n):
        rec = sites[site_off[i]:site_off[i + 1]]
        ok = (rec["kind"] == SCORED) & (rec["flags"] & IN_BEST != 0) & (rec["flags"] & NO_WITHOUT == 0)
        if not ok.any():
            continue
        cand = rec[ok]
        j = int(np.argmax(cand["without_score"]))
        out["sig"][i], out["score"][i] = cand["without_sig"][j], cand["without_score"][j]
        out["delta"][i] = np.float32(cand["with_score"][j]) - np.float32(cand["without_score"][j])
        out["found"][i] = True
        assert cand["with_sig"][j] == best_sig[i], "records and best_sig belong to different runs"
    return out


def table(sites, site_off, peptides):
    """Rows for a site-level report, one per record: dicts with ``psm``, ``position`` (1-based), ``residue`` (the letter),
    ``in_best``, ``kind`` (a ``SITE_KINDS`` name), ``with_score``, ``without_score``, ``delta`` (None where there is no
    pair), ``with_sig``, ``without_sig``.  ``peptides``: one str / bytes per PSM."""
    sites = np.asarray(sites, SITE_DTYPE)
    d = deltas(sites)
    rows = []
    for i in range(len(site_off) - 1):
        pep = peptides[i]
        pep = pep.decode("ascii", "replace") if isinstance(pep, (bytes, bytearray)) else str(pep)
        for r in range(int(site_off[i]), int(site_off[i + 1])):
            s = sites[r]
            pos = int(s["pos"])
            scored = int(s["kind"]) == SCORED
            rows.append(dict(psm=i, position=pos, residue=pep[pos - 1] if 1 <= pos <= len(pep) else "?",
                             in_best=bool(s["flags"] & IN_BEST), kind=SITE_KINDS[int(s["kind"])],
                             with_score=float(s["with_score"]) if scored and s["with_score"] >= 0 else None,
                             without_score=float(s["without_score"]) if scored and s["without_score"] >= 0 else None,
                             delta=None if np.isnan(d[r]) else float(d[r]),
                             with_sig=int(s["with_sig"]), without_sig=int(s["without_sig"])))
    return rows
