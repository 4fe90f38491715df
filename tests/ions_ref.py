"""CPU yardstick for the ion records (include/pyascore_hip.h: pya_ion): both sections of one PSM from parts that are
pinned to the reference already -- PyBinnedSpectra, PyModifiedPeptide (consume_peak / get_match /
get_site_determining_ions) and PyFragmentGraph (set_signature / get_fragment_mz / get_fragment_size / is_loss) of
pyascore_amd.aux (tests/test_aux_api.py holds them to the reference's own unit tests) -- and the evidence rows of the PSM
(tests/evidence_ref.py: competitor and depth of every counted column).  Nothing of the library's kernels is involved.
A helper module, not a test file.

The order inside a section is the implementation's (see the header): comparisons sort both sides by record bytes
(``canonical``).
"""
import numpy as np

import evidence_ref
from pyascore_amd import aux
from pyascore_amd._lib import ION_DTYPE as _FIELDS

DTYPE = np.dtype(_FIELDS)
WINNER, NO_MATCH = 255, 255
LOSS, COMP, COUNTED = 1, 2, 4


def fragments(mp, sig, ftype, zmax):
    """Every fragment of one localisation and ion type as the reference iterates them (cpp/Ascore.cpp:53-121: charge,
    then size, then loss variant): (float32 m/z, size, charge, loss, number of the variant inside its size)."""
    out = []
    for z in range(1, zmax + 1):
        g = aux.PyFragmentGraph(mp, ftype, z)
        g.set_signature(sig)
        size, nth = -1, 0
        while not g.is_fragment_end():
            nth = nth + 1 if g.get_fragment_size() == size else 0
            size = g.get_fragment_size()
            out.append((np.float32(g.get_fragment_mz()), size, z, bool(g.is_loss()), nth))
            g.incr_fragment()
    return out


def _record(mp, mz, size, ftype, z, loss, site, flags, depth=None):
    m = mp.get_match(float(mz))
    rank = NO_MATCH if m is None else int(m[1])
    flags |= LOSS if loss else 0
    if depth is not None and rank <= depth:
        flags |= COUNTED
    return (np.float32(mz), np.float32(0. if m is None else m[0]), size, ord(ftype), z, rank, site, flags, 0)


def signature(bits, n_sites):
    return np.array([(int(bits) >> j) & 1 for j in range(n_sites)], np.uint32)


def winner_section(settings, kw, mp, best_sig, n_sites):
    """Section 1: every fragment of the best localisation that has a match among the retained peaks."""
    out = []
    sig = signature(best_sig, n_sites)
    for ftype in settings["fragment_types"]:
        for mz, size, z, loss, _ in fragments(mp, sig, ftype, kw["max_fragment_charge"]):
            if mp.has_match(float(mz)):
                out.append(_record(mp, mz, size, ftype, z, loss, WINNER, 0))
    return out


def site_section(settings, kw, mp, best_sig, n_sites, sites, mod_idx, column, row):
    """Section 2 of one counted column: the survivors of the greedy walk on both sides, with their identity.  The
    reference hands out m/z values only (get_site_determining_ions); a survivor is the fragment of that m/z, and where
    several fragments of a list share a float32 m/z the walk drops the first of them first (order: size, loss variant,
    charge), so the survivors are the last ones."""
    out = []
    best = int(best_sig)
    comp = (best & ~(1 << mod_idx[column])) | (1 << sites.index(int(row["comp_pos"]) - 1))
    sigs = [signature(best, n_sites), signature(comp, n_sites)]
    zmax, depth = kw["max_fragment_charge"], int(row["depth"])
    by_side = [[], []]
    for ftype in settings["fragment_types"]:
        lists = mp.get_site_determining_ions(sigs[0], sigs[1], ftype, zmax)
        for side in (0, 1):
            full = sorted(fragments(mp, sigs[side], ftype, zmax), key=lambda f: (f[0], f[1], f[4], f[2]))
            values, counts = np.unique(np.asarray(lists[side], np.float32), return_counts=True)
            for v, c in zip(values, counts):
                same = [f for f in full if f[0] == v]
                assert len(same) >= c, "a site-determining ion that is no fragment of its localisation"
                for mz, size, z, loss, _ in same[len(same) - int(c):]:
                    by_side[side].append(_record(mp, mz, size, ftype, z, loss, column, COMP if side else 0, depth))
    return by_side[0] + by_side[1]


def records(settings, kw, best_sig, ev_rows, scored=True):
    """The ion records of one PSM (structured array): kw as ``synth.unpack_psm`` gives it, best_sig its winner, ev_rows
    its evidence rows (tests/evidence_ref.py or the library's), scored: it has a result (status 0, n_sig > 0)."""
    if not scored:
        return np.zeros(0, DTYPE)
    sites = evidence_ref.modifiable_positions(kw["peptide"], settings["mod_group"])
    mp = evidence_ref.matcher(settings, kw)
    out = winner_section(settings, kw, mp, best_sig, len(sites))
    mod_idx = [j for j in range(len(sites)) if (int(best_sig) >> j) & 1]
    for a in range(min(len(ev_rows), int(kw["n_of_mod"]))):
        if int(ev_rows[a]["kind"]) == evidence_ref.COUNTED:
            out += site_section(settings, kw, mp, best_sig, len(sites), sites, mod_idx, a, ev_rows[a])
    return np.array(out, DTYPE) if out else np.zeros(0, DTYPE)


def canonical(rec):
    """The records of one PSM in byte order (both sides of a comparison go through this)."""
    rec = np.ascontiguousarray(rec, DTYPE)
    if rec.size == 0:
        return rec
    return rec[np.lexsort(rec.view(np.uint8).reshape(-1, 16).T[::-1])]


def batch_records(settings, batch, res, evidence, unpack):
    """records() for every PSM of a batch: (ion_off int64 [n + 1], records in canonical order per PSM)."""
    n = int(batch["n_psm"])
    parts, off = [], [0]
    for i in range(n):
        scored = not ("status" in res and res["status"][i]) and res["n_sig"][i] > 0
        parts.append(canonical(records(settings, unpack(batch, i), res["best_sig"][i], evidence[i], scored)))
        off.append(off[-1] + parts[-1].size)
    return np.asarray(off, np.int64), (np.concatenate(parts) if parts else np.zeros(0, DTYPE))


def canonical_batch(ion_off, rec):
    """a CSR batch of records with every PSM's range in canonical order"""
    rec = np.ascontiguousarray(rec, DTYPE).copy()
    for i in range(len(ion_off) - 1):
        rec[ion_off[i]:ion_off[i + 1]] = canonical(rec[ion_off[i]:ion_off[i + 1]])
    return rec
