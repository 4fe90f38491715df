"""CPU yardstick for the site probabilities (include/pyascore_hip.h: pya_site_prob, pya_psm_prob): the records of one PSM
from its ``pep_scores`` CSR arrays by plain numpy -- the weights 10^((s - s*) / 10) as exp2 of a double, sequential sums.
``psm_records`` sums the records in ascending order of their sig bits: the device sums in the order of the shape's signature
list, which pep_scores does not show, and reordering a sum of N positive doubles moves it by up to about N / 2^53 relative
(1.7e-12 for the 15 000 assignments a fast PSM can have, typically its square root), which is why records made this way are
compared at RTOL.  ``psm_records(..., order=...)`` replays the device's own order (pya_debug_signature_list): then exp2 --
an ulp or two per weight -- is all that separates the two, and they are compared at RTOL_ORDERED.  A helper module, not a
test file.
"""
import math

import numpy as np

from pyascore_amd._lib import PSM_PROB_DTYPE as _PSM_FIELDS, SITE_PROB_DTYPE as _SITE_FIELDS
from sites_ref import modifiable_positions

SITE_DTYPE, PSM_DTYPE = np.dtype(_SITE_FIELDS), np.dtype(_PSM_FIELDS)
NONE, SCORED, OVER = 0, 1, 2
C = 0.33219280948873623          # log2(10) / 10
RTOL = 1e-12
RTOL_ORDERED = 16 * 2.0 ** -53   # a few ulps: exp2 on either side, the division


def weights(weighted_score, best_score):
    """w_i of the definition: exp2(((double)s_i - (double)s*) * C)"""
    d = np.asarray(weighted_score, np.float32).astype(np.float64) - float(np.float32(best_score))
    return np.exp2(d * C)


def psm_records(n_sites, best_score, sig_bits, weighted_score, scored=True, sig_cap=0, order=None):
    """(site records [n_sites], the PSM's record) of one PSM.  sig_bits / weighted_score: its pep_scores records, in any
    order; scored False: status != 0 or n_sig <= 0; sig_cap: 0 = none; order: the sig bits in the order they are to be
    summed in (every record's bits, once), default ascending."""
    sites, psm = np.zeros(n_sites, SITE_DTYPE), np.zeros(1, PSM_DTYPE)[0]
    if not scored:
        return sites, psm
    bits = np.asarray(sig_bits, np.uint64)
    if sig_cap and bits.size > sig_cap:
        sites["with_prob"] = sites["without_prob"] = -1.0
        psm["kind"] = OVER
        return sites, psm
    if order is None:
        order = np.argsort(bits, kind="stable")
    else:
        at = {int(b): i for i, b in enumerate(bits)}
        assert len(at) == bits.size == len(order)
        order = np.asarray([at[int(b)] for b in order], np.int64)
    bits, w = bits[order], weights(weighted_score, best_score)[order]
    z = 0.0
    for x in w:
        z += float(x)
    for r in range(n_sites):
        has = (bits >> np.uint64(r)) & np.uint64(1) == np.uint64(1)
        a = b = 0.0
        for x, h in zip(w, has):
            if h:
                a += float(x)
            else:
                b += float(x)
        sites["with_prob"][r], sites["without_prob"][r] = a / z, b / z
    psm["z"], psm["n_summed"], psm["kind"] = z, bits.size, SCORED
    return sites, psm


def brute_force(n_sites, sig_bits, weighted_score):
    """An independent statement: a dict of assignments -> 10^(s / 10) ratios, math.fsum.  (with [n_sites], z) as floats."""
    top = max(float(np.float32(s)) for s in weighted_score)
    ratio = {int(b): 10.0 ** ((float(np.float32(s)) - top) / 10.0) for b, s in zip(sig_bits, weighted_score)}
    z = math.fsum(ratio.values())
    return [math.fsum(v for b, v in ratio.items() if b >> r & 1) / z for r in range(n_sites)], z


def batch_records(settings, batch, res, ps, unpack, sig_cap=0, status=None):
    """(site_off, site records, PSM records) of a batch; arguments as sites_ref.batch_records (res: best_score / n_sig)."""
    pick = lambda *names: next(ps[n] for n in names if n in ps)  # noqa: E731
    off, bits, ws = pick("rec_off", "ps_off"), pick("sig_bits", "ps_bits"), pick("weighted_score", "ps_ws")
    n = int(batch["n_psm"])
    recs, site_off, psms = [], [0], np.zeros(n, PSM_DTYPE)
    for i in range(n):
        if status is not None and status[i] >= 16:
            site_off.append(site_off[-1])
            continue
        positions = modifiable_positions(unpack(batch, i)["peptide"], settings["mod_group"])
        lo, hi = int(off[i]), int(off[i + 1])
        scored = res["n_sig"][i] > 0 and (status is None or status[i] == 0)
        s, psms[i] = psm_records(len(positions), res["best_score"][i], bits[lo:hi], ws[lo:hi], scored, sig_cap)
        recs.append(s)
        site_off.append(site_off[-1] + len(positions))
    return np.asarray(site_off, np.int64), (np.concatenate(recs) if recs else np.zeros(0, SITE_DTYPE)), psms
