"""Site probabilities: what ``PyAscore.score_batch(probs=True)`` returns, turned into the columns a site-level report wants.

Pure Python / numpy: nothing here needs a scorer.  ``site_probs`` (``SITE_PROB_DTYPE``, the 16-byte ``pya_site_prob`` of
include/pyascore_hip.h) has one record per modifiable residue of a PSM, N- to C-terminus, at
``site_probs[site_off[i]:site_off[i + 1]]``: the posterior probability that the residue is modified (``with_prob``) and that
it is not (``without_prob``), under the posterior over the PSM's site assignments that their PepScores imply (weight
10^(PepScore / 10)).  ``psm_probs`` (``PSM_PROB_DTYPE``) has one record per PSM; ``1 / z`` is the posterior of the reported
localisation.  This is a PepScore-based posterior -- MaxQuant's construction -- and not part of the Ascore publication.
"""
import numpy as np

from . import _lib

SITE_PROB_DTYPE = np.dtype(_lib.SITE_PROB_DTYPE)    # pya_site_prob, 16 bytes
PSM_PROB_DTYPE = np.dtype(_lib.PSM_PROB_DTYPE)      # pya_psm_prob, 16 bytes
assert SITE_PROB_DTYPE.itemsize == 16 and PSM_PROB_DTYPE.itemsize == 16
NONE, SCORED, OVER = _lib.PYA_SITE_NONE, _lib.PYA_SITE_SCORED, _lib.PYA_SITE_OVER


def best_prob(psm_probs):
    """The posterior of the reported localisation per PSM (float64): ``1 / z``; NaN for a PSM that was not scored or has more
    site assignments than the stage was asked to sum."""
    psm_probs = np.asarray(psm_probs, PSM_PROB_DTYPE)
    out = np.full(psm_probs.shape, np.nan)
    ok = (psm_probs["kind"] == SCORED) & (psm_probs["z"] > 0)
    out[ok] = 1.0 / psm_probs["z"][ok]
    return out


def positions_of(peptide, residues):
    """The 1-based positions of the modifiable residues of ``peptide`` for a scorer whose modification group is the letters
    ``residues`` -- the residues the records of a PSM belong to, in their order.  (A group with a terminus in it makes the
    first or the last residue modifiable whatever its letter: pass the positions of ``sites["pos"]`` instead.)"""
    peptide = peptide.decode("ascii", "replace") if isinstance(peptide, (bytes, bytearray)) else str(peptide)
    return [i + 1 for i, c in enumerate(peptide) if c in residues]


def table(site_probs, psm_probs, site_off, peptides, residues=None, positions=None):
    """Rows for a site-level report, one per record: dicts with ``psm``, ``position`` (1-based), ``residue`` (the letter)
    and ``probability`` (``with_prob``; None for a PSM that was not scored or is over the cap).  ``peptides``: one str /
    bytes per PSM.  The positions come from ``positions`` (one per record, e.g. ``sites["pos"]`` of the same batch) or are
    found from ``residues``, the letters of the scorer's modification group."""
    site_probs = np.asarray(site_probs, SITE_PROB_DTYPE)
    psm_probs = np.asarray(psm_probs, PSM_PROB_DTYPE)
    if positions is None and residues is None:
        raise ValueError("table() needs the residues of the modification group, or the position of every record")
    rows = []
    for i in range(len(site_off) - 1):
        pep = peptides[i]
        pep = pep.decode("ascii", "replace") if isinstance(pep, (bytes, bytearray)) else str(pep)
        lo, hi = int(site_off[i]), int(site_off[i + 1])
        pos = [int(p) for p in positions[lo:hi]] if positions is not None else positions_of(pep, residues)
        if len(pos) != hi - lo:
            raise ValueError("PSM %d has %d records and %d modifiable residues" % (i, hi - lo, len(pos)))
        scored = int(psm_probs["kind"][i]) == SCORED
        for r, p in zip(range(lo, hi), pos):
            rows.append(dict(psm=i, position=p, residue=pep[p - 1] if 1 <= p <= len(pep) else "?",
                             probability=float(site_probs["with_prob"][r]) if scored else None))
    return rows


def annotate(peptide, positions, probs, digits=2):
    """``AS(0.98)PT(0.02)K``: the peptide with the probability of every candidate residue behind it, MaxQuant's notation.
    ``positions``: 1-based, one per entry of ``probs``."""
    peptide = peptide.decode("ascii", "replace") if isinstance(peptide, (bytes, bytearray)) else str(peptide)
    at = {int(p): float(v) for p, v in zip(positions, probs)}
    return "".join(c + ("(%.*f)" % (digits, at[i + 1]) if i + 1 in at else "") for i, c in enumerate(peptide))
