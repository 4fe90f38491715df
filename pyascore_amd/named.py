"""Named localisations: the signatures a caller asks ``PyAscore.score_batch(named=...)`` about.

Pure Python / numpy: nothing here needs a scorer (a scorer needs a device, and the command line turns reported positions
into signature bits before it scores).  A signature is a bit set over the modifiable residues of a peptide, bit j = the
j-th modifiable residue counted from the N-terminus (include/pyascore_hip.h, "sig bits"); the modifiable residues are
those of ``ModifiedPeptide::initializeResidues`` (cpp/ModifiedPeptide.cpp:24-79): a letter of the mod group, the first
residue where the group has ``n``, the last where it has ``c``.
"""
import numpy as np

from . import _lib

NAMED_DTYPE = np.dtype(_lib.NAMED_DTYPE)            # pya_named, 32 bytes
assert NAMED_DTYPE.itemsize == 32
NAMED_KINDS = ("none", "invalid", "winner", "tied", "counted")


def site_residues(peptide, mod_group):
    """0-based residue indices of the modifiable residues of ``peptide`` (str or bytes), N-terminus first."""
    pep = peptide.decode("ascii", "replace") if isinstance(peptide, (bytes, bytearray)) else str(peptide)
    last = len(pep) - 1
    allow_n, allow_c = "n" in mod_group, "c" in mod_group
    return [i for i, aa in enumerate(pep) if aa in mod_group or (allow_n and i == 0) or (allow_c and i == last)]


def sig_bits_of(peptide, positions, mod_group):
    """Signature bits of the localisation that puts a modification on each of ``positions``: 1-based peptide positions,
    0 = the n-terminus (the first residue) where ``mod_group`` has ``n``.  Returns 0 -- which the library answers with a
    ``PYA_NAMED_INVALID`` record for any PSM with a modification to place -- when a position is not a modifiable residue,
    lies outside the peptide, or names a residue twice."""
    sites = {res: j for j, res in enumerate(site_residues(peptide, mod_group))}
    bits = 0
    for pos in positions:
        pos = int(pos)
        if pos == 0 and "n" not in mod_group:
            return 0
        j = sites.get(max(pos, 1) - 1) if pos >= 0 else None
        if j is None or j >= 64 or bits >> j & 1:
            return 0
        bits |= 1 << j
    return bits


def sig_bits_batch(peptides, positions, mod_group):
    """``sig_bits_of`` for many PSMs: one peptide and one sequence of positions each -> uint64 array."""
    if len(peptides) != len(positions):
        raise ValueError("one sequence of positions per peptide expected")
    return np.array([sig_bits_of(p, q, mod_group) for p, q in zip(peptides, positions)], dtype=np.uint64)


def query_csr(named, n_psm):
    """The ``named`` argument of ``score_batch`` as the library's CSR pair ``(q_off int64[n_psm + 1], q_bits uint64)``:
    either that pair already (a tuple), or a list with one sequence of signatures (or one signature) per PSM."""
    if isinstance(named, tuple):
        if len(named) != 2:
            raise ValueError("named: a tuple is the pair (q_off, sig_bits)")
        q_off = np.ascontiguousarray(named[0], np.int64)
        q_bits = np.ascontiguousarray(named[1], np.uint64).reshape(-1)
    else:
        per_psm = [np.atleast_1d(np.asarray(q, dtype=np.uint64)).reshape(-1) if np.size(q) else np.zeros(0, np.uint64)
                   for q in named]
        if len(per_psm) != n_psm:
            raise ValueError("named: one sequence of signatures per PSM expected (%d PSMs, %d sequences)" % (n_psm, len(per_psm)))
        q_off = np.concatenate([[0], np.cumsum([q.size for q in per_psm])]).astype(np.int64)
        q_bits = np.concatenate(per_psm) if per_psm else np.zeros(0, np.uint64)
        q_bits = np.ascontiguousarray(q_bits, np.uint64)
    if q_off.size != n_psm + 1:
        raise ValueError("named: q_off must have n_psm + 1 entries")
    if n_psm and q_off[-1] > q_bits.size:
        raise ValueError("named: q_off runs past the end of the signatures")
    return q_off, q_bits


def take_queries(q_off, q_bits, perm):
    """The queries of the PSMs ``perm`` (a batch reordered by ``synth.take_psms``), and for every query of the new order
    its index in the old one."""
    n_q = np.diff(q_off)[perm]
    new_off = np.concatenate([[0], np.cumsum(n_q)]).astype(np.int64)
    src = np.repeat(q_off[:-1][perm] - new_off[:-1], n_q) + np.arange(int(n_q.sum()))
    return new_off, np.ascontiguousarray(q_bits[src]), src
