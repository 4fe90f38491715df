"""The yardstick of the peptidoform stage (pya_peptidoform, include/pyascore_hip.h) in plain Python: the definitions of the
header, literally, one entry at a time into a dict keyed by (group, sig_bits).  Bit patterns are Python ints; nothing here
is shared with pyascore_amd.rollup.merge_peptidoforms or with the kernels."""
import struct

import numpy as np

from pyascore_amd import _lib

DTYPE = np.dtype(_lib.PEPTIDOFORM_DTYPE)
SCORED = 1
ONE_BITS = struct.unpack("<Q", struct.pack("<d", 1.0))[0]
INF_BITS = struct.unpack("<I", struct.pack("<f", float("inf")))[0]


def akey(bits):
    """float32 bits -> their place in -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN"""
    return 0xFFFFFFFF - bits if bits >> 31 else bits + 0x80000000


def _f64(bits):
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def _merge_into(table, e):
    """e = (group, sig, n_psm, n_confident, best_psm, prob bits, z bits, ascore bits)"""
    key = (e[0], e[1])
    have = table.get(key)
    if have is None:
        table[key] = list(e[2:])
        return
    have[0] = (have[0] + e[2]) & 0xFFFFFFFF
    have[1] = (have[1] + e[3]) & 0xFFFFFFFF
    if e[5] > have[3]:
        have[3], have[2] = e[5], e[4]
    elif e[5] == have[3]:
        have[2] = min(have[2], e[4])
    have[4] = min(have[4], e[6])
    if akey(e[7]) > akey(have[5]):
        have[5] = e[7]


def _records(table):
    out = np.zeros(len(table), DTYPE)
    per_group = {}
    for g, _ in table:
        per_group[g] = per_group.get(g, 0) + 1
    for j, (g, sig) in enumerate(sorted(table)):
        n, nc, psm, prob, z, asc = table[(g, sig)]
        out[j] = (sig, g, n, nc, psm, 0.0, 0.0, 0.0, per_group[g])
        out["best_min_prob"][j:j + 1].view(np.uint64)[0] = prob
        out["best_z"][j:j + 1].view(np.uint64)[0] = z
        out["best_min_ascore"][j:j + 1].view(np.uint32)[0] = asc
    return out


def _entries_of_records(records):
    r = np.ascontiguousarray(records, DTYPE).reshape(-1)
    cols = [r["group"].tolist(), r["sig_bits"].tolist(), r["n_psm"].tolist(), r["n_confident"].tolist(), r["best_psm"].tolist(),
            np.ascontiguousarray(r["best_min_prob"]).view(np.uint64).tolist(), np.ascontiguousarray(r["best_z"]).view(np.uint64).tolist(),
            np.ascontiguousarray(r["best_min_ascore"]).view(np.uint32).tolist()]
    return [e for e in zip(*cols) if e[2] != 0]


def reduce(a, b=None):
    """the list over one or two arrays of records: records with n_psm == 0 are skipped, n_isomers is recomputed"""
    table = {}
    for src in (a, b):
        if src is not None:
            for e in _entries_of_records(src):
                _merge_into(table, e)
    return _records(table)


def psm_entries(best_sig, ascores, site_off, site_probs, psm_probs, group, threshold, psm_id=None, psm_base=0):
    """the contributing PSMs as entries"""
    ascores = np.ascontiguousarray(ascores, np.float32)
    max_k = ascores.shape[1]
    abits = ascores.view(np.uint32)
    pbits = np.ascontiguousarray(site_probs["with_prob"]).view(np.uint64)
    zbits = np.ascontiguousarray(psm_probs["z"]).view(np.uint64)
    out = []
    for i in range(len(best_sig)):
        if int(psm_probs["kind"][i]) != SCORED or int(group[i]) < 0:
            continue
        sig = int(best_sig[i])
        lo = int(site_off[i])
        rs = [r for r in range(64) if sig >> r & 1]
        assert not rs or lo + rs[-1] < int(site_off[i + 1]), "best_sig names a residue the PSM has no record of"
        min_prob = ONE_BITS if sig == 0 else min(int(pbits[lo + r]) for r in rs)
        k = len(rs)
        assert k <= max_k
        min_asc = INF_BITS if k == 0 else min((int(abits[i, c]) for c in range(k)), key=akey)
        conf = 1 if _f64(min_prob) >= threshold else 0
        ident = int(psm_id[i]) if psm_id is not None else psm_base + i
        out.append((int(group[i]), sig, 1, conf, ident, min_prob, int(zbits[i]), min_asc))
    return out


def from_psms(best_sig, ascores, site_off, site_probs, psm_probs, group, threshold=0.75, psm_id=None, psm_base=0, prev=None):
    """the list over the contributing PSMs and the records of an earlier list"""
    table = {}
    for e in psm_entries(best_sig, ascores, site_off, site_probs, psm_probs, group, threshold, psm_id, psm_base):
        _merge_into(table, e)
    if prev is not None:
        for e in _entries_of_records(prev):
            _merge_into(table, e)
    return _records(table)
