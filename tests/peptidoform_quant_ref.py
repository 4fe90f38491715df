"""CPU yardstick for the peptidoform quantification (include/pyascore_hip.h): the pair -- the peptidoform list and the table
row-aligned with it -- from the arrays ``score_batch(probs=True)`` returns, a channel matrix and the rows of the PSMs.  Written
for clarity rather than speed: one Python loop over the PSMs, a dict keyed by (group, sig_bits), Python integers for every
sum, no atomics and no order to depend on.  The list is peptidoforms_ref's (the yardstick of that stage), the quantum is
site_quant_ref's; nothing is shared with ``pyascore_amd.rollup.peptidoform_quant`` or with the kernels.

A PSM contributes to the table when it contributes to the list (kind SCORED, group not negative), its min_prob -- the smallest
``with_prob`` bit pattern over the residues of ``best_sig``, 1.0 for ``best_sig == 0`` -- is at or above the quant threshold
as a double, and its row lies in [0, n_rows).  A negative row is left out; a row at or above n_rows raises Outside.
"""
import struct

import numpy as np

import peptidoforms_ref
from site_quant_ref import CELL, HEAD, Outside, quantum

DTYPE = peptidoforms_ref.DTYPE
M32, M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF


def _f64(bits):
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def contributions(best_sig, ascores, site_off, site_probs, psm_probs, group, n_rows, row, threshold):
    """The multiset the table is a function of: (group, sig, row) per contributing PSM."""
    out = []
    entries = peptidoforms_ref.psm_entries(best_sig, ascores, site_off, site_probs, psm_probs, group, 0.0, psm_id=list(range(len(best_sig))))
    for g, sig, _, _, i, min_prob, _, _ in entries:
        rw = i if row is None else int(row[i])
        if rw < 0 or not _f64(min_prob) >= float(threshold):
            continue
        if rw >= n_rows:
            raise Outside("PSM %d: row %d of %d" % (i, rw, n_rows))
        out.append((g, sig, rw))
    return out


def _rows_of(pair, n_ch):
    """(key, head fields, cell fields) of the records of a pair with n_psm != 0; head / cell None: zeros"""
    records, head, cell = pair
    records = np.ascontiguousarray(records, DTYPE).reshape(-1)
    for j in range(records.size):
        if int(records["n_psm"][j]) == 0:
            continue
        key = (int(records["group"][j]), int(records["sig_bits"][j]))
        if head is None:
            yield key, [0, 0], [[0, 0, 0] for _ in range(n_ch)]
        else:
            yield key, [int(head["n_records"][j]), int(head["n_complete"][j])], \
                [[int(cell["sum"][j, c]), int(cell["n"][j, c]), int(cell["n_saturated"][j, c])] for c in range(n_ch)]


def _emit(records, rows, n_ch, cap):
    """the table row-aligned with `records` from the dict `rows`; rows at or above cap are dropped with their records"""
    m = len(records) if cap is None else min(len(records), int(cap))
    records = records[:m].copy()
    h, c = np.zeros(m, HEAD), np.zeros((m, n_ch), CELL)
    for j in range(m):
        got = rows.get((int(records["group"][j]), int(records["sig_bits"][j])))
        if got is None:
            continue
        h["n_records"][j], h["n_complete"][j] = got[0][0] & M32, got[0][1] & M32
        for k in range(n_ch):
            c["sum"][j, k], c["n"][j, k], c["n_saturated"][j, k] = got[1][k][0] & M64, got[1][k][1] & M32, got[1][k][2] & M32
    return records, h, c


def _add(rows, key, head, cell, n_ch):
    have = rows.setdefault(key, ([0, 0], [[0, 0, 0] for _ in range(n_ch)]))
    have[0][0] += head[0]
    have[0][1] += head[1]
    for k in range(n_ch):
        for f in range(3):
            have[1][k][f] += cell[k][f]


def pair(best_sig, ascores, site_off, site_probs, psm_probs, group, values, row, list_threshold, threshold, scale_log2,
         complete_only=False, psm_id=None, psm_base=0, prev=None, cap=None):
    """``(list, head, cell)`` of a batch, with the earlier pair ``prev`` (``(list, head, cell)``; head and cell None: an all-zero
    table) merged in"""
    values = np.asarray(values, np.float64)
    n_rows, n_ch = values.shape
    records = peptidoforms_ref.from_psms(best_sig, ascores, site_off, site_probs, psm_probs, group, list_threshold, psm_id, psm_base,
                                         None if prev is None else prev[0])
    rows = {}
    for g, sig, rw in contributions(best_sig, ascores, site_off, site_probs, psm_probs, group, n_rows, row, threshold):
        vals = [float(v) for v in values[rw]]
        usable = [v == v and v > 0.0 for v in vals]
        complete = all(usable)
        cell = [[0, 0, 0] for _ in range(n_ch)]
        if complete or not complete_only:
            for c in range(n_ch):
                if usable[c]:
                    q, sat = quantum(vals[c], scale_log2)
                    cell[c] = [q, 1, 1 if sat else 0]
        _add(rows, (g, sig), [1, 1 if complete else 0], cell, n_ch)
    if prev is not None:
        for key, head, cell in _rows_of(prev, n_ch):
            _add(rows, key, head, cell, n_ch)
    return _emit(records, rows, n_ch, cap)


def reduce(a, b, n_ch, cap=None):
    """the merge of two pairs: the keys' union, rows of equal keys added field by field"""
    records = peptidoforms_ref.reduce(a[0], b[0])
    rows = {}
    for side in (a, b):
        for key, head, cell in _rows_of(side, n_ch):
            _add(rows, key, head, cell, n_ch)
    return _emit(records, rows, n_ch, cap)
