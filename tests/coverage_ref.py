"""CPU yardstick for the coverage records (include/pyascore_hip.h: pya_coverage): section 1 of one PSM from
``ions_ref.winner_section`` -- PyBinnedSpectra, PyModifiedPeptide and PyFragmentGraph of pyascore_amd.aux, which are pinned to
the reference -- plus the raw arrays, with the four sums in the stated order in plain Python floats.  Nothing of the library's
kernels and nothing of ``pyascore_amd.rollup.coverage`` is involved.  A helper module, not a test file."""
import numpy as np

import evidence_ref
import ions_ref
from pyascore_amd import aux
from pyascore_amd._lib import COVERAGE_DTYPE as _FIELDS

DTYPE = np.dtype(_FIELDS)
NONE, SCORED = 0, 1
FORWARD = "bc"


def retained_count(settings, kw):
    """The peaks the reference's binning keeps of one spectrum (the sum over its windows)."""
    spec = aux.PyBinnedSpectra(settings["bin_size"], settings["n_top"])
    spec.consume_spectra(np.ascontiguousarray(kw["mz_arr"], np.float64), np.ascontiguousarray(kw["int_arr"], np.float64))
    total = 0
    spec.reset_bin()
    while spec.bin < spec.n_bins:
        total += int(spec.n_peaks)
        spec.next_bin()
    return total


def section_one(settings, kw, best_sig):
    """The section-1 ion records of one scored PSM (``ions_ref.DTYPE``)."""
    sites = evidence_ref.modifiable_positions(kw["peptide"], settings["mod_group"])
    mp = evidence_ref.matcher(settings, kw)
    out = ions_ref.winner_section(settings, kw, mp, best_sig, len(sites))
    return np.array(out, ions_ref.DTYPE) if out else np.zeros(0, ions_ref.DTYPE)


def lane_sum(values):
    """p[l] = ((0.0 + x[l]) + x[l + 64]) + ..., then s = (((0.0 + p[0]) + p[1]) + ...) + p[63]"""
    part = []
    for lane in range(64):
        p = 0.0
        k = lane
        while k < len(values):
            p = p + values[k]
            k += 64
        part.append(p)
    s = 0.0
    for p in part:
        s = s + p
    return s


def longest_run(sizes):
    best = 0
    for s in sizes:
        n = 0
        while s + n in sizes:
            n += 1
        best = max(best, n)
    return best


def record(settings, kw, ions, scored=True):
    """The coverage record of one PSM: kw as ``synth.unpack_psm`` gives it (the arrays in the element types that were
    scored), ions its section-1 records."""
    out = np.zeros(1, DTYPE)
    if not scored:
        return out[0]
    x = [np.float32(v) for v in np.asarray(kw["mz_arr"])]
    y = [float(v) for v in np.asarray(kw["int_arr"])]
    fwd_peaks = [np.float32(r["peak_mz"]) for r in ions if chr(int(r["type"])) in FORWARD]
    bwd_peaks = [np.float32(r["peak_mz"]) for r in ions if chr(int(r["type"])) not in FORWARD]
    in_fwd = [any(v == p for p in fwd_peaks) for v in x]         # (float32 equality: a NaN equals nothing)
    in_bwd = [any(v == p for p in bwd_peaks) for v in x]
    L = len(kw["peptide"])
    f_sizes = set(int(r["size"]) for r in ions if chr(int(r["type"])) in FORWARD)
    b_sizes = set(int(r["size"]) for r in ions if chr(int(r["type"])) not in FORWARD)
    out[0] = (lane_sum(y), lane_sum([v if f or b else 0.0 for v, f, b in zip(y, in_fwd, in_bwd)]),
              lane_sum([v if f else 0.0 for v, f in zip(y, in_fwd)]), lane_sum([v if b else 0.0 for v, b in zip(y, in_bwd)]),
              len(x), retained_count(settings, kw), sum(1 for f, b in zip(in_fwd, in_bwd) if f or b), len(ions),
              len(f_sizes), len(b_sizes), longest_run(f_sizes), longest_run(b_sizes),
              len(set(range(1, L)) & (f_sizes | set(L - s for s in b_sizes))), SCORED, [0] * 5)
    return out[0]


def batch_records(settings, batch, res, unpack):
    """For every PSM of a private batch (a shared one: expand it first): (ion_off int64 [n + 1], the section-1 ion records,
    the coverage records, n_retained per PSM -- 0 where the PSM was not scored).  res: best_sig, n_sig and, where PSMs were set
    aside, status."""
    n = int(batch["n_psm"])
    parts, off, recs, kept = [], [0], np.zeros(n, DTYPE), np.zeros(n, np.int64)
    for i in range(n):
        scored = not ("status" in res and res["status"][i]) and res["n_sig"][i] > 0
        kw = unpack(batch, i)
        ions = section_one(settings, kw, res["best_sig"][i]) if scored else np.zeros(0, ions_ref.DTYPE)
        recs[i] = record(settings, kw, ions, scored)
        kept[i] = recs[i]["n_retained"]
        parts.append(ions)
        off.append(off[-1] + ions.size)
    return np.asarray(off, np.int64), (np.concatenate(parts) if parts else np.zeros(0, ions_ref.DTYPE)), recs, kept
