"""CPU yardstick for the site records (include/pyascore_hip.h: pya_site): the records of one PSM from its ``pep_scores``
CSR arrays by plain numpy -- masks over ``sig_bits``, ``max`` of ``weighted_score``, the tie rule, the flags.  pep_scores is
pinned to the reference already; nothing of the library's kernels is involved.  A helper module, not a test file.
"""
import numpy as np

from pyascore_amd._lib import SITE_DTYPE as _FIELDS

DTYPE = np.dtype(_FIELDS)
NONE, SCORED, OVER = 0, 1, 2
IN_BEST, WITH_TIED, WITHOUT_TIED, NO_WITHOUT = 1, 2, 4, 8


def modifiable_positions(peptide, mod_group):
    """0-based residues that can carry the modification, N-terminus first (cpp/ModifiedPeptide.cpp:24-79)"""
    pep = peptide.decode("ascii") if isinstance(peptide, (bytes, bytearray)) else str(peptide)
    last = len(pep) - 1
    return [i for i, aa in enumerate(pep) if aa in mod_group or ("n" in mod_group and i == 0) or ("c" in mod_group and i == last)]


def _best_of(bits, ws, pick, best_sig):
    """(score, sig, tied) over the records ``pick``: the maximum, best_sig if it attains it else the smallest bits"""
    if not pick.any():
        return np.float32(-1), 0, False
    top = ws[pick].max()
    at = bits[pick & (ws == top)]
    sig = int(best_sig) if (at == np.uint64(best_sig)).any() else int(at.min())
    return np.float32(top), sig, at.size > 1


def psm_records(positions, best_sig, sig_bits, weighted_score, scored=True, sig_cap=0):
    """The records of one PSM.  positions: 0-based residues of its modifiable ones; sig_bits / weighted_score: its
    pep_scores records, in any order; scored False: status != 0 or n_sig <= 0; sig_cap: 0 = none."""
    out = np.zeros(len(positions), DTYPE)
    out["pos"] = np.asarray(positions, np.int64) + 1
    if not scored:
        return out
    bits = np.asarray(sig_bits, np.uint64)
    ws = np.asarray(weighted_score, np.float32)
    best = int(best_sig)
    for s in range(len(positions)):
        out["flags"][s] = IN_BEST if best >> s & 1 else 0
    if sig_cap and bits.size > sig_cap:
        out["kind"] = OVER
        return out
    out["kind"] = SCORED
    for s in range(len(positions)):
        has = (bits >> np.uint64(s)) & np.uint64(1) == np.uint64(1)
        w_score, w_sig, w_tied = _best_of(bits, ws, has, best)
        o_score, o_sig, o_tied = _best_of(bits, ws, ~has, best)
        out["with_score"][s], out["with_sig"][s] = w_score, w_sig
        out["without_score"][s], out["without_sig"][s] = o_score, o_sig
        out["flags"][s] |= (WITH_TIED if w_tied else 0) | (WITHOUT_TIED if o_tied else 0) | (0 if (~has).any() else NO_WITHOUT)
    return out


def batch_records(settings, batch, res, ps, unpack, sig_cap=0, status=None):
    """(site_off, records) of a batch.  res: best_sig / n_sig of the run; ps: CSR pep_scores arrays (a golden file's
    ``exp_ps_*`` without the prefix, or ``PyAscore.batch_pep_scores()``); status: per-PSM codes of a skip_invalid run --
    a PSM the host pre-pass set aside (code >= 16) has no records."""
    pick = lambda *names: next(ps[n] for n in names if n in ps)  # noqa: E731
    off, bits, ws = pick("rec_off", "ps_off"), pick("sig_bits", "ps_bits"), pick("weighted_score", "ps_ws")
    recs, site_off = [], [0]
    for i in range(int(batch["n_psm"])):
        if status is not None and status[i] >= 16:
            site_off.append(site_off[-1])
            continue
        kw = unpack(batch, i)
        positions = modifiable_positions(kw["peptide"], settings["mod_group"])
        lo, hi = int(off[i]), int(off[i + 1])
        scored = res["n_sig"][i] > 0 and (status is None or status[i] == 0)
        recs.append(psm_records(positions, res["best_sig"][i], bits[lo:hi], ws[lo:hi], scored, sig_cap))
        site_off.append(site_off[-1] + len(positions))
    return np.asarray(site_off, np.int64), (np.concatenate(recs) if recs else np.zeros(0, DTYPE))
