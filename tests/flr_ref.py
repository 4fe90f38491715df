"""The yardstick of the site FLR stage (pya_site_flr, include/pyascore_hip.h): a deliberately naive restatement of the
definition -- a Python sort of (-bits, slot) tuples, Python-int sums, float(a) / float(b).  It shares no code with
pyascore_amd.rollup.flr (the product's host form) or with the kernels; tests/test_flr_ref.py pins it to hand-computed answers."""
import numpy as np

DTYPE = np.dtype([("rank", "<u4"), ("n_decoy", "<u4"), ("err_sum", "<u8"), ("flr", "<f8"), ("decoy_q", "<f8")])
TARGET, DECOY, LEFT_OUT = 0, 1, 2


def err(p):
    """the expected error of a site with localisation probability p, scaled by 2^32 and truncated"""
    return int(max(0.0, 1.0 - p) * 4294967296.0)


def flr(table, cls=None, reported_only=False):
    """(records, order, n_ranked) of a roll-up table (any structured array with best_prob, n_psm, n_in_best)"""
    n = len(table)
    probs = [float(p) for p in table["best_prob"]]
    bits = [int(b) for b in np.ascontiguousarray(table["best_prob"]).view(np.uint64)]
    n_psm = [int(x) for x in table["n_psm"]]
    n_in_best = [int(x) for x in table["n_in_best"]]
    kind = [TARGET] * n if cls is None else [int(c) for c in cls]
    if any(k not in (TARGET, DECOY, LEFT_OUT) for k in kind):
        raise ValueError("a class byte that is none of 0, 1, 2")
    ranked = [n_psm[s] != 0 and kind[s] != LEFT_OUT and not (reported_only and n_in_best[s] == 0) for s in range(n)]
    keyed = sorted((-bits[s], s) for s in range(n) if ranked[s])
    order = [s for _, s in keyed] + [s for s in range(n) if not ranked[s]]
    groups = []                      # (first position, one past the last, rank, n_decoy, err_sum) of every tie group
    rank = n_decoy = err_sum = 0
    i = 0
    while i < len(keyed):
        j = i
        while j < len(keyed) and keyed[j][0] == keyed[i][0]:
            s = keyed[j][1]
            rank += 1
            n_decoy += kind[s] == DECOY
            err_sum += err(probs[s])
            j += 1
        groups.append((i, j, rank, n_decoy, err_sum))
        i = j
    records = np.zeros(n, DTYPE)
    q = float("inf")
    for i, j, rank, n_decoy, err_sum in reversed(groups):
        q = min(q, float(n_decoy) / float(max(rank - n_decoy, 1)))
        for at in range(i, j):
            records[keyed[at][1]] = (rank, n_decoy, err_sum, float(err_sum) / float(rank << 32), q)
    return records, np.array(order, np.uint32), len(keyed)
