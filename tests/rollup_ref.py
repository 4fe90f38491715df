"""CPU yardstick for the site roll-up (include/pyascore_hip.h: pya_site_rollup): the table from the arrays
``score_batch(probs=True)`` returns, written for clarity rather than speed -- one Python loop over the residue records, one
slot at a time, no atomics and no order to depend on.  Pure numpy; nothing here needs a device.

A record contributes when its PSM's ``psm_probs["kind"]`` is SCORED and its slot lies in [0, n_slots).  Per slot:
best_prob = the largest with_prob by its uint64 bit pattern; best_psm = the smallest psm_id among the records with exactly
those bits; n_psm, n_confident (with_prob >= threshold), n_in_best (bit r of best_sig, r the record's place in its PSM) are
counts; best_ascore = the largest Ascore of the in-best records -- column popcount(best_sig & ((1 << r) - 1)) of the PSM's
ascores row -- under the total order of float32 bit patterns (-NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN).
"""
import numpy as np

from pyascore_amd._lib import PYA_ROLLUP_NO_PSM, PYA_SITE_SCORED, ROLLUP_DTYPE as _FIELDS

DTYPE = np.dtype(_FIELDS)
assert DTYPE.itemsize == 32


def ascore_key(bits):
    """the order-preserving image of a float32 bit pattern"""
    bits = int(bits)
    return 0xFFFFFFFF - bits if bits >> 31 else bits + 0x80000000


def empty(n_slots):
    t = np.zeros(int(n_slots), DTYPE)
    t["best_psm"] = PYA_ROLLUP_NO_PSM
    return t


def contributions(site_probs, psm_probs, site_off, best_sig, ascores, slot, n_slots, psm_id=None, psm_base=0):
    """The multiset the table is a function of: (slot, with_prob bits, psm_id, in_best, ascore bits) per contributing record."""
    site_off = np.asarray(site_off, np.int64)
    ascores = np.asarray(ascores, np.float32)
    slot = np.asarray(slot)
    assert slot.size == int(site_off[-1]), "one slot per residue record"
    prob_bits = np.ascontiguousarray(site_probs["with_prob"], np.float64).view(np.uint64)
    out = []
    for i in range(site_off.size - 1):
        if int(psm_probs["kind"][i]) != PYA_SITE_SCORED:
            continue
        sig = int(best_sig[i])
        ident = int(psm_id[i]) if psm_id is not None else psm_base + i
        for r, rec in enumerate(range(int(site_off[i]), int(site_off[i + 1]))):
            s = int(slot[rec])
            if s < 0 or s >= n_slots:
                continue
            in_best = bool(sig >> r & 1)
            a_bits = 0
            if in_best:
                col = bin(sig & ((1 << r) - 1)).count("1")
                a_bits = int(ascores[i, col:col + 1].view(np.uint32)[0])
            out.append((s, int(prob_bits[rec]), ident, in_best, a_bits))
    return out


def accumulate(table, contribs, threshold):
    """Adds contributions to a table IN PLACE, slot by slot, reading the table's own fields as the earlier contributions."""
    threshold = float(threshold)
    for s, p_bits, ident, in_best, a_bits in contribs:
        row = table[s]
        have = int(np.array(row["best_prob"]).view(np.uint64))
        if p_bits > have:
            row["best_prob"] = np.array(p_bits, np.uint64).view(np.float64)
            row["best_psm"] = ident
        elif p_bits == have:                    # (an empty slot holds NO_PSM, the largest id there is)
            row["best_psm"] = min(int(row["best_psm"]), ident)
        row["n_psm"] += 1
        if float(np.array(p_bits, np.uint64).view(np.float64)) >= threshold:
            row["n_confident"] += 1
        if in_best:
            old = int(np.array(row["best_ascore"]).view(np.uint32))
            if int(row["n_in_best"]) == 0 or ascore_key(a_bits) > ascore_key(old):
                row["best_ascore"] = np.array(a_bits, np.uint32).view(np.float32)
            row["n_in_best"] += 1
    return table


def table(site_probs, psm_probs, site_off, best_sig, ascores, slot, n_slots, threshold, psm_id=None, psm_base=0, into=None):
    """The roll-up of a batch: a new table of n_slots records, or ``into`` (a copy of it) with the batch added."""
    t = empty(n_slots) if into is None else np.array(into, DTYPE)
    return accumulate(t, contributions(site_probs, psm_probs, site_off, best_sig, ascores, slot, n_slots, psm_id, psm_base), threshold)
