"""Site roll-up: the slots ``PyAscore.score_batch(rollup=...)`` rolls the residue records of a batch into, and the table it
returns turned into the rows of a site-level report.

Pure Python / numpy: nothing here needs a scorer.  A batch has one residue record per modifiable residue of every PSM that
was not set aside, N- to C-terminus, at ``site_off[i]:site_off[i + 1]`` (``score_batch(probs=True)`` returns ``site_off``;
``site_offsets`` below finds it from the peptides).  A *slot* is one site in the key the caller chooses; ``slot`` names the
slot of every record (negative: the record is left out), and the table (``ROLLUP_DTYPE``, the 32-byte ``pya_site_rollup`` of
include/pyascore_hip.h) has one record per slot: the best localisation probability any PSM gives the site and which PSM
gives it, how many PSMs cover it, how many put it at or above the threshold, how many report it as the localisation, and the
best Ascore of those.

``flr`` turns such a table into false-localisation rates (``FLR_DTYPE``, the 32-byte ``pya_site_flr``): the slots sorted by
``best_prob``, the expected errors ``1 - p`` accumulated down the list, and -- with decoy residues in the modification group,
``decoy_classes`` -- the decoys above every cut as a q-value.  ``PyAscore.rollup_flr`` and ``DevicePlan.rollup_flr`` do the
same on the device; the function here is the host form, with the same bytes.  ``cut`` names the slots reportable at a rate.

Peptidoforms: ``peptide_groups`` numbers the peptides of a batch for ``score_batch(peptidoforms=dict(group=...))``, which
returns one record per (peptide, reported site assignment) (``PEPTIDOFORM_DTYPE``, the 48-byte ``pya_peptidoform``);
``merge_peptidoforms`` is the host form of ``PyAscore.peptidoform_reduce`` with the same bytes, and ``peptidoform_table``
turns a list into the rows of a report.

Fragment mass-error profile: ``score_batch(mz_profile=dict(run=..., n_slots=...))`` returns one ``MZ_PROFILE_DTYPE`` record
(the 4 128-byte ``pya_mz_profile``) per run slot; ``mz_profile_params`` is the only place the three inverse widths are
computed, ``mz_profile`` restates the stage over ion records with the same IEEE operations (equal counts, not close ones),
``merge_mz_profiles`` adds tables and ``mz_profile_summary`` reads a tolerance off one.

Fragment m/z recalibration: ``fit_mz_calibration`` reads one systematic error per band of m/z off a profile
(``MZ_CALIBRATION_DTYPE``, the 128-byte ``pya_mz_calibration``) and ``recalibrate`` corrects m/z arrays with it -- the host
forms of ``PyAscore.fit_mz_calibration`` / ``DevicePlan.fit_mz_calibration`` and of ``DevicePlan.recalibrate`` /
``score_batch(recalibrate=...)``, with the same bytes; ``mz_calibration_rows`` / ``read_mz_calibration`` are the file of
``--mz_calibration_out`` / ``--mz_calibration``, ``suggest_mz_error`` a convenience for the narrow re-run.

Deisotoping: ``deisotope_params`` checks and fills the parameters of ``pya_deisotope_params`` (the only place ``step / z`` is
computed) and ``deisotope`` restates the rule over numpy arrays with the same IEEE operations -- the host form of
``PyAscore.deisotope_spectra`` / ``pyascore_amd.device.deisotope`` / ``score_batch(deisotope=...)``, with the same bytes.

Charge deconvolution: ``decharge_params`` is ``deisotope_params`` with ``carrier`` and ``witness`` beside it
(``pya_decharge_params``) and ``decharge`` restates that rule -- deisotoping, and every kept peak whose satellites show a charge
of 2 or more moved to its m/z at 1+, the output sorted -- the host form of ``PyAscore.decharge_spectra`` /
``pyascore_amd.device.decharge`` / ``score_batch(decharge=...)``, with the same bytes.

Precursor stripping: ``strip_params`` checks and fills the parameters of ``pya_strip_params``, ``strip_windows`` gives the
windows of a precursor and ``strip`` restates the rule -- the peaks inside a window of the precursor, of its neutral-loss forms
and of its charge-reduced forms, and the peaks outside an m/z range, removed -- the host form of ``PyAscore.strip_spectra`` /
``pyascore_amd.device.strip`` / ``score_batch(strip=...)``, with the same bytes; ``STRIP_REPORT_DTYPE`` is the 16-byte
``pya_strip_report`` and ``strip_hits`` reads its ``hit`` word.

Explained ion current: ``score_batch(coverage=True)`` returns one ``COVERAGE_DTYPE`` record (the 64-byte ``pya_coverage``) per
PSM; ``coverage`` restates the stage over section-1 ion records and the raw arrays with the sums in the definition's order
(equal bytes, not close ones) and ``coverage_ratios`` turns records into the four ratios a report shows.

Marker ions: ``marker_params`` checks and fills the parameters of ``pya_marker_params`` (fixed targets -- reporter and
immonium m/z -- first, precursor losses behind them), ``marker_windows`` gives the windows of a precursor and ``markers`` restates
the read-only rule -- per (spectrum, target) the most intense peak inside the window, per spectrum the ion current and the base
peak -- the host form of ``PyAscore.marker_spectra`` / ``pyascore_amd.device.markers`` / ``score_batch(markers=...)``, with the
same bytes; ``MARKER_DTYPE`` / ``MARKER_SPECTRUM_DTYPE`` are the 24-byte ``pya_marker`` and the 32-byte ``pya_marker_spectrum``
and ``marker_matrix`` is what a quantification step takes.

Site quantification: ``score_batch(rollup=..., quant=...)`` returns per roll-up slot and channel the summed intensity of the PSMs
that place the modification on the site confidently (``SITE_QUANT_HEAD_DTYPE`` / ``SITE_QUANT_DTYPE``, the 8-byte
``pya_site_quant_head`` and the 16-byte ``pya_site_quant``); ``site_quant_params`` checks and fills the parameters,
``site_quant`` restates the stage over the probability records with integer sums (equal bytes), ``merge_site_quant`` adds tables
and ``site_quant_sums`` turns one into intensities.

Peptidoform quantification: ``score_batch(peptidoforms=..., peptidoform_quant=...)`` returns the peptidoform list and, row-aligned
with it, the same head / cell records per peptidoform and channel; ``peptidoform_quant`` restates the pair over the probability
records (the list through ``merge_peptidoforms``, integer sums, equal bytes), ``merge_peptidoform_quant`` merges pairs and
``site_quant_sums`` turns the table into intensities.
"""
import numpy as np

from . import _lib
from .named import site_residues

ROLLUP_DTYPE = np.dtype(_lib.ROLLUP_DTYPE)          # pya_site_rollup, 32 bytes
assert ROLLUP_DTYPE.itemsize == 32
NO_PSM = _lib.PYA_ROLLUP_NO_PSM
FLR_DTYPE = np.dtype(_lib.FLR_DTYPE)                # pya_site_flr, 32 bytes
assert FLR_DTYPE.itemsize == 32
PEPTIDOFORM_DTYPE = np.dtype(_lib.PEPTIDOFORM_DTYPE)    # pya_peptidoform, 48 bytes
assert PEPTIDOFORM_DTYPE.itemsize == 48
MZ_PROFILE_DTYPE = np.dtype(_lib.MZ_PROFILE_DTYPE)  # pya_mz_profile, 4 128 bytes
assert MZ_PROFILE_DTYPE.itemsize == 4128
MZ_CALIBRATION_DTYPE = np.dtype(_lib.MZ_CALIBRATION_DTYPE)  # pya_mz_calibration, 128 bytes
assert MZ_CALIBRATION_DTYPE.itemsize == 128
COVERAGE_DTYPE = np.dtype(_lib.COVERAGE_DTYPE)      # pya_coverage, 64 bytes
assert COVERAGE_DTYPE.itemsize == 64
MZC_MAX_PPM = _lib.PYA_MZC_MAX_PPM
MZP_BANDS, MZP_BINS = _lib.PYA_MZP_BANDS, _lib.PYA_MZP_BINS
DEISO_MAX_CHARGE = _lib.PYA_DEISO_MAX_CHARGE
DECHARGE_CARRIER = _lib.PYA_DECHARGE_CARRIER
STRIP_REPORT_DTYPE = np.dtype(_lib.STRIP_REPORT_DTYPE)  # pya_strip_report, 16 bytes
assert STRIP_REPORT_DTYPE.itemsize == 16
STRIP_MAX_CHARGE, STRIP_MAX_LOSS, STRIP_MAX_ISOTOPES = _lib.PYA_STRIP_MAX_CHARGE, _lib.PYA_STRIP_MAX_LOSS, _lib.PYA_STRIP_MAX_ISOTOPES
STRIP_STEP = _lib.PYA_STRIP_STEP
STRIP_WINDOWS = STRIP_MAX_CHARGE * (STRIP_MAX_LOSS + 1)     # 64: one bit of ``hit`` each
CENTROID_MAX_HALF_WIDTH = _lib.PYA_CENTROID_MAX_HALF_WIDTH
MARKER_DTYPE = np.dtype(_lib.MARKER_DTYPE)          # pya_marker, 24 bytes
MARKER_SPECTRUM_DTYPE = np.dtype(_lib.MARKER_SPECTRUM_DTYPE)    # pya_marker_spectrum, 32 bytes
assert MARKER_DTYPE.itemsize == 24 and MARKER_SPECTRUM_DTYPE.itemsize == 32
MARKER_MAX_TARGETS = _lib.PYA_MARKER_MAX_TARGETS
MARKER_ACTIVE, MARKER_PICKED = _lib.PYA_MARKER_ACTIVE, _lib.PYA_MARKER_PICKED
PURITY_DTYPE = np.dtype(_lib.PURITY_DTYPE)          # pya_purity, 48 bytes
assert PURITY_DTYPE.itemsize == 48
PURITY_MAX_CENTRES, PURITY_MAX_BELOW = _lib.PYA_PURITY_MAX_CENTRES, _lib.PYA_PURITY_MAX_BELOW
PURITY_ACTIVE, PURITY_SEEN = _lib.PYA_PURITY_ACTIVE, _lib.PYA_PURITY_SEEN
XIC_DTYPE = np.dtype(_lib.XIC_DTYPE)                # pya_xic, 64 bytes
assert XIC_DTYPE.itemsize == 64
XIC_MAX_SCANS, XIC_MAX_ISOTOPES, XIC_MAX_GAP = _lib.PYA_XIC_MAX_SCANS, _lib.PYA_XIC_MAX_ISOTOPES, _lib.PYA_XIC_MAX_GAP
XIC_ACTIVE, XIC_SEEN, XIC_SEED_PRESENT = _lib.PYA_XIC_ACTIVE, _lib.PYA_XIC_SEEN, _lib.PYA_XIC_SEED_PRESENT
XIC_LEFT_VALLEY, XIC_RIGHT_VALLEY, XIC_UNSORTED = _lib.PYA_XIC_LEFT_VALLEY, _lib.PYA_XIC_RIGHT_VALLEY, _lib.PYA_XIC_UNSORTED
XIC_LEFT_OPEN, XIC_RIGHT_OPEN = _lib.PYA_XIC_LEFT_OPEN, _lib.PYA_XIC_RIGHT_OPEN
XIC_COLUMNS = ("area", "apex_intensity", "seed_intensity", "sum_intensity")     # ``which`` 0 .. 3 of ``xic_values``
SITE_QUANT_HEAD_DTYPE = np.dtype(_lib.SITE_QUANT_HEAD_DTYPE)   # pya_site_quant_head, 8 bytes
SITE_QUANT_DTYPE = np.dtype(_lib.SITE_QUANT_DTYPE)             # pya_site_quant, 16 bytes
assert SITE_QUANT_HEAD_DTYPE.itemsize == 8 and SITE_QUANT_DTYPE.itemsize == 16
QUANT_MAX_CHANNELS = _lib.PYA_QUANT_MAX_CHANNELS
TARGET, DECOY, LEFT_OUT =_lib.PYA_FLR_TARGET, _lib.PYA_FLR_DECOY, _lib.PYA_FLR_LEFT_OUT


def _text(peptide):
    return peptide.decode("ascii", "replace") if isinstance(peptide, (bytes, bytearray)) else str(peptide)


def empty(n_slots):
    """A table of ``n_slots`` empty slots (``best_psm`` is ``NO_PSM``, everything else 0)."""
    t = np.zeros(int(n_slots), ROLLUP_DTYPE)
    t["best_psm"] = NO_PSM
    return t


def site_offsets(peptides, residues):
    """``(site_off, positions)`` of a batch whose PSMs are all scored: the record offsets (int64 ``[n + 1]``) and the 1-based
    position of every record (int64), for a scorer whose modification group is ``residues`` (``n`` / ``c`` in it: the first /
    last residue whatever its letter).  A PSM that the library sets aside has no records: take ``site_off`` from the batch
    then."""
    pos = [[j + 1 for j in site_residues(_text(p), residues)] for p in peptides]
    off = np.concatenate([[0], np.cumsum([len(p) for p in pos])]).astype(np.int64)
    return off, np.array([j for p in pos for j in p], np.int64)


def _positions(peptides, site_off, positions, residues):
    site_off = np.asarray(site_off, np.int64)
    if site_off.size != len(peptides) + 1:
        raise ValueError("site_off must have one entry per PSM and one more")
    if positions is None:
        if residues is None:
            raise ValueError("the slots need the residues of the modification group, or the position of every record")
        off, positions = site_offsets(peptides, residues)
        # (a PSM without records was set aside: its positions are dropped)
        keep = np.repeat(np.diff(site_off) != 0, np.diff(off))
        positions = positions[keep]
    positions = np.asarray(positions, np.int64)
    if positions.size != int(site_off[-1]):
        raise ValueError("%d positions for %d residue records" % (positions.size, int(site_off[-1])))
    return site_off, positions


def _number(keys_of_records):
    """slots in order of first appearance"""
    index, keys = {}, []
    slot = np.empty(len(keys_of_records), np.int32)
    for r, k in enumerate(keys_of_records):
        s = index.get(k)
        if s is None:
            s = index[k] = len(keys)
            keys.append(k)
        slot[r] = s
    return slot, len(keys), keys


def peptide_slots(peptides, site_off, positions=None, residues=None):
    """``(slot, n_slots, keys)`` keyed by (unmodified peptide sequence, 1-based position): every PSM of a peptide lands on the
    same slots.  Slots are numbered in order of first appearance; ``keys[s]`` is the key of slot ``s``.  ``peptides``: one
    str / bytes per PSM; ``positions``: one per record (e.g. ``sites["pos"]`` of the same batch), or found from ``residues``,
    the scorer's modification group."""
    site_off, positions = _positions(peptides, site_off, positions, residues)
    owner = np.repeat(np.arange(len(peptides)), np.diff(site_off))
    text = [_text(p) for p in peptides]
    return _number([(text[i], int(p)) for i, p in zip(owner, positions)])


def protein_slots(protein_of, start_of, site_off, positions):
    """``(slot, n_slots, keys)`` keyed by (protein id, absolute 1-based position): ``protein_of[i]`` is the protein of PSM
    ``i``'s peptide and ``start_of[i]`` the 1-based position of its first residue there, so two overlapping peptides land on
    one slot.  A PSM whose ``protein_of`` is None is left out (slot -1)."""
    site_off = np.asarray(site_off, np.int64)
    positions = np.asarray(positions, np.int64)
    if site_off.size != len(protein_of) + 1 or len(start_of) != len(protein_of) or positions.size != int(site_off[-1]):
        raise ValueError("protein_of and start_of have one entry per PSM, positions one per residue record")
    owner = np.repeat(np.arange(len(protein_of)), np.diff(site_off))
    known = np.array([protein_of[i] is not None for i in owner], bool)
    slot = np.full(positions.size, -1, np.int32)
    got, n_slots, keys = _number([(protein_of[i], int(start_of[i]) + int(p) - 1) for i, p in zip(owner[known], positions[known])])
    slot[known] = got
    return slot, n_slots, keys


def merge(a, b):
    """The table of the PSMs behind ``a`` and the PSMs behind ``b`` together (same slots, same threshold): every field is a
    max, a min or a count, so tables of several ranks, files or runs add up on the host to the bytes of one call over all of
    their PSMs."""
    a, b = np.asarray(a, ROLLUP_DTYPE), np.asarray(b, ROLLUP_DTYPE)
    if a.shape != b.shape:
        raise ValueError("tables over different slots")
    out = a.copy()
    pa, pb = a["best_prob"].view(np.uint64), b["best_prob"].view(np.uint64)
    out["best_prob"] = np.where(pb > pa, b["best_prob"], a["best_prob"])
    out["best_psm"] = np.where(pb > pa, b["best_psm"], np.where(pb == pa, np.minimum(a["best_psm"], b["best_psm"]), a["best_psm"]))
    for f in ("n_psm", "n_confident", "n_in_best"):
        out[f] = a[f] + b[f]
    ka, kb = _ascore_key(a["best_ascore"]), _ascore_key(b["best_ascore"])
    ka[a["n_in_best"] == 0] = -1
    kb[b["n_in_best"] == 0] = -1
    out["best_ascore"] = np.where(kb > ka, b["best_ascore"], a["best_ascore"])
    return out


def _ascore_key(x):
    """the order-preserving image of float32 bit patterns (int64): -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN"""
    bits = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.int64)
    return np.where(bits >> 31 != 0, 0xFFFFFFFF - bits, bits + 0x80000000)


def flr(table, cls=None, reported_only=False):
    """``(records, order, n_ranked)`` of a roll-up table, on the host: ``records`` (``FLR_DTYPE``) one per slot, ``order``
    (uint32) the ranked slots by ``best_prob`` descending (as bit patterns; equal bits by slot), then the others by index.
    ``cls``: one byte per slot, ``TARGET`` / ``DECOY`` / ``LEFT_OUT``, or None: all targets; ``reported_only``: a slot no PSM
    reports is not ranked.  A slot's ``rank``, ``n_decoy``, ``err_sum`` count the ranked slots at least as good as it, TIES
    INCLUDED (every member of a tie group has the values at the group's end); ``flr`` is their mean expected error, ``decoy_q``
    the smallest decoy / target ratio of this cut and every wider one.  The bytes are those of ``PyAscore.rollup_flr``."""
    table = np.ascontiguousarray(table, ROLLUP_DTYPE)
    n = table.size
    if n > 0x7FFFFFFF:
        raise ValueError("more than 2^31 - 1 slots")
    ranked = table["n_psm"] != 0
    if cls is not None:
        cls = np.ascontiguousarray(cls, np.uint8)
        if cls.shape != (n,):
            raise ValueError("cls has one byte per slot")
        if (cls > LEFT_OUT).any():
            raise ValueError("class byte %d of slot %d is none of 0, 1, 2" % (cls[cls > LEFT_OUT][0], np.flatnonzero(cls > LEFT_OUT)[0]))
        ranked &= cls < LEFT_OUT
    if reported_only:
        ranked &= table["n_in_best"] != 0
    bits = table["best_prob"].view(np.uint64)
    idx = np.flatnonzero(ranked)
    idx = idx[np.argsort(~bits[idx], kind="stable")]                 # bits descending, slots ascending within equal bits
    order = np.concatenate([idx, np.flatnonzero(~ranked)]).astype(np.uint32)
    records = np.zeros(n, FLR_DTYPE)
    m = idx.size
    if m == 0:
        return records, order, 0
    sb = bits[idx]
    with np.errstate(invalid="ignore"):
        d = 1.0 - table["best_prob"][idx]
        err = (np.where(d > 0.0, d, 0.0) * 4294967296.0).astype(np.uint64)
    decoy = (cls[idx] == DECOY) if cls is not None else np.zeros(m, bool)
    end = np.flatnonzero(np.concatenate([sb[1:] != sb[:-1], [True]]))      # last position of every tie group
    group = np.searchsorted(end, np.arange(m))                             # the group of every position
    rank = (end + 1).astype(np.uint64)
    n_decoy = np.cumsum(decoy, dtype=np.uint64)[end]
    err_sum = np.cumsum(err, dtype=np.uint64)[end]
    ratio = n_decoy.astype(np.float64) / np.maximum(rank - n_decoy, 1).astype(np.float64)
    q = np.minimum.accumulate(ratio[::-1])[::-1]
    r = records[idx]
    r["rank"], r["n_decoy"], r["err_sum"] = rank[group], n_decoy[group], err_sum[group]
    r["flr"] = (err_sum.astype(np.float64) / (rank << np.uint64(32)).astype(np.float64))[group]
    r["decoy_q"] = q[group]
    records[idx] = r
    return records, order, int(m)


def decoy_classes(keys, peptides_or_letters=None, decoys="A"):
    """``cls`` for ``flr``: ``DECOY`` for the slots on a decoy residue, ``TARGET`` for the others.  ``keys``: the
    (peptide, 1-based position) keys of ``peptide_slots``; the residue is the letter of the key's peptide at its position --
    or ``peptides_or_letters`` says it: one letter per slot (a str of ``len(keys)`` letters or a sequence of them), or a
    mapping from a key's first element (a protein id, ...) to the sequence the position counts in.  ``decoys``: the decoy
    letters of the modification group (Ala, Pro, Gly, ... beside STY)."""
    cls = np.zeros(len(keys), np.uint8)
    letters = peptides_or_letters
    if letters is not None and not hasattr(letters, "get") and len(letters) != len(keys):
        raise ValueError("%d letters for %d slots" % (len(letters), len(keys)))
    for s, key in enumerate(keys):
        if letters is None or hasattr(letters, "get"):
            seq = _text(key[0] if letters is None else letters.get(key[0], ""))
            pos = int(key[1])
            letter = seq[pos - 1] if 1 <= pos <= len(seq) else ""
        else:
            letter = _text(letters[s])
        if letter and letter in decoys:
            cls[s] = DECOY
    return cls


def cut(records, order, n_ranked, flr=0.01):
    """The slots reportable at model FLR ``flr``, best first: the longest prefix of the ranked slots whose cut has
    ``records["flr"] <= flr`` (the rate does not decrease down the list, and a tie group is taken or left as a whole)."""
    records = np.asarray(records, FLR_DTYPE)
    ranked = np.asarray(order)[:int(n_ranked)].astype(np.int64)
    return ranked[:int(np.searchsorted(records["flr"][ranked], float(flr), side="right"))].astype(np.uint32)


def table(rollup, keys, flr=None):
    """Rows for a site-level report, one per slot that any PSM covers: dicts with ``key`` (``keys[s]``), ``best_prob``,
    ``best_psm``, ``n_psm``, ``n_confident``, ``n_in_best`` and ``best_ascore`` (None when no PSM reports the site).
    ``flr``: the ``(records, order, n_ranked)`` of ``flr`` / ``rollup_flr`` over the same table; the rows then come in
    ``order`` and gain ``rank``, ``flr`` and ``decoy_q`` (None for a slot that is not ranked)."""
    rollup = np.asarray(rollup, ROLLUP_DTYPE)
    if len(keys) != rollup.size:
        raise ValueError("%d keys for %d slots" % (len(keys), rollup.size))
    slots = np.flatnonzero(rollup["n_psm"])
    if flr is not None:
        records, order = np.asarray(flr[0], FLR_DTYPE), np.asarray(flr[1]).astype(np.int64)
        if records.size != rollup.size or order.size != rollup.size:
            raise ValueError("FLR records over another table")
        slots = order[rollup["n_psm"][order] != 0]
    rows = []
    for s in slots:
        r = rollup[s]
        rows.append(dict(key=keys[s], best_prob=float(r["best_prob"]), best_psm=int(r["best_psm"]), n_psm=int(r["n_psm"]),
                         n_confident=int(r["n_confident"]), n_in_best=int(r["n_in_best"]),
                         best_ascore=float(r["best_ascore"]) if r["n_in_best"] else None))
        if flr is not None:
            f = records[s]
            on = int(f["rank"]) != 0
            rows[-1].update(rank=int(f["rank"]) if on else None, flr=float(f["flr"]) if on else None,
                            decoy_q=float(f["decoy_q"]) if on else None)
    return rows


def peptide_groups(peptides):
    """``(group, n_groups, keys)`` keyed by the unmodified peptide sequence: ``group`` (int32, one per PSM) is what
    ``score_batch(peptidoforms=dict(group=...))`` takes, numbered in order of first appearance; ``keys[g]`` is the sequence
    of group ``g``.  ``peptides``: one str / bytes per PSM."""
    return _number([_text(p) for p in peptides])


def merge_peptidoforms(a, b=None):
    """The peptidoform list over the records of ``a`` and ``b`` (``PEPTIDOFORM_DTYPE``; any order, keys may repeat, records
    with ``n_psm == 0`` are skipped, ``n_isomers`` is recomputed): one record per (group, sig_bits), ordered by group then
    sig_bits.  Counts add, ``best_min_prob`` is the max over bit patterns with the smallest ``best_psm`` that has them,
    ``best_z`` the min over bit patterns, ``best_min_ascore`` the max under the total order of float32 bit patterns: the host
    form of ``PyAscore.peptidoform_reduce`` / ``pya_peptidoform_reduce``, with the same bytes."""
    r = np.ascontiguousarray(a, PEPTIDOFORM_DTYPE).reshape(-1)
    if b is not None:
        r = np.concatenate([r, np.ascontiguousarray(b, PEPTIDOFORM_DTYPE).reshape(-1)])
    r = r[r["n_psm"] != 0]
    if r.size == 0:
        return np.zeros(0, PEPTIDOFORM_DTYPE)
    r = r[np.lexsort((r["sig_bits"], r["group"]))]
    head = np.ones(r.size, bool)
    head[1:] = (r["group"][1:] != r["group"][:-1]) | (r["sig_bits"][1:] != r["sig_bits"][:-1])
    first = np.flatnonzero(head)
    seg = np.cumsum(head) - 1
    out = np.zeros(first.size, PEPTIDOFORM_DTYPE)
    out["sig_bits"], out["group"] = r["sig_bits"][first], r["group"][first]
    for f in ("n_psm", "n_confident"):
        out[f] = np.add.reduceat(r[f].astype(np.uint64), first).astype(np.uint32)       # (32-bit counts wrap, as on the device)
    bits = np.ascontiguousarray(r["best_min_prob"]).view(np.uint64)
    top = np.maximum.reduceat(bits, first)
    out["best_min_prob"] = top.view(np.float64)
    out["best_psm"] = np.minimum.reduceat(np.where(bits == top[seg], r["best_psm"], np.uint32(0xFFFFFFFF)), first)
    out["best_z"] = np.minimum.reduceat(np.ascontiguousarray(r["best_z"]).view(np.uint64), first).view(np.float64)
    key = np.maximum.reduceat(_ascore_key(r["best_min_ascore"]), first)
    out["best_min_ascore"] = np.where(key >> 31 != 0, key - 0x80000000, 0xFFFFFFFF - key).astype(np.uint32).view(np.float32)
    ghead = np.ones(first.size, bool)
    ghead[1:] = out["group"][1:] != out["group"][:-1]
    gfirst = np.flatnonzero(ghead)
    out["n_isomers"] = np.repeat(np.diff(np.append(gfirst, first.size)), np.diff(np.append(gfirst, first.size))).astype(np.uint32)
    return out


def peptidoform_table(records, keys, residues=None):
    """The list as the rows of a report, in the list's order: one dict per peptidoform with ``peptide`` (``keys[group]``),
    ``sites`` -- the modified residues: their 1-based positions when ``residues``, the scorer's modification group, is given,
    otherwise the ordinals of the modifiable residues (bit numbers of ``sig_bits``) --, ``n_psm``, ``n_confident``,
    ``best_psm``, ``best_min_prob``, ``best_posterior`` (``1 / best_z``), ``best_min_ascore`` and ``n_isomers``."""
    records = np.asarray(records, PEPTIDOFORM_DTYPE)
    rows = []
    for rec in records:
        g = int(rec["group"])
        if g >= len(keys):
            raise ValueError("group %d has no key (%d keys)" % (g, len(keys)))
        sig = int(rec["sig_bits"])
        ordinals = [r for r in range(64) if sig >> r & 1]
        text = _text(keys[g])
        if residues is not None:
            where = site_residues(text, residues)
            if ordinals and ordinals[-1] >= len(where):
                raise ValueError("peptide %s has %d modifiable residues, sig_bits names residue %d" % (text, len(where), ordinals[-1]))
            ordinals = [where[r] + 1 for r in ordinals]
        z = float(rec["best_z"])
        rows.append(dict(peptide=text, sites=ordinals, n_psm=int(rec["n_psm"]), n_confident=int(rec["n_confident"]),
                         best_psm=int(rec["best_psm"]), best_min_prob=float(rec["best_min_prob"]),
                         best_posterior=1.0 / z if z > 0.0 else 0.0, best_min_ascore=float(rec["best_min_ascore"]),
                         n_isomers=int(rec["n_isomers"])))
    return rows


def mz_profile_params(da_half_width, ppm_half_width=50.0, band_width=250.0, max_rank=9):
    """``dict(inv_da, inv_ppm, inv_band, max_rank)`` of a profile whose Da axis spans ``+-da_half_width``, whose ppm axis spans
    ``+-ppm_half_width`` (``MZP_BINS`` half-open bins each, 0 at the lower edge of bin ``MZP_BINS / 2``) and whose m/z bands
    are ``band_width`` wide (the last of the ``MZP_BANDS`` is open-ended): bins per Da, bins per ppm, bands per m/z unit, as
    the doubles the device and ``mz_profile`` multiply by.  Refuses what the C ABI refuses: a width whose inverse is not a
    finite positive number, ``max_rank`` outside 0 .. 15."""
    half = MZP_BINS // 2
    out = dict(inv_da=half / float(da_half_width) if da_half_width else float("inf"),
               inv_ppm=half / float(ppm_half_width) if ppm_half_width else float("inf"),
               inv_band=1.0 / float(band_width) if band_width else float("inf"))
    for k, v in out.items():
        if not (np.isfinite(v) and v > 0.0):
            raise ValueError("mz_profile: %s = %r is not a finite positive number" % (k, v))
    if int(max_rank) != max_rank or not 0 <= int(max_rank) <= 15:
        raise ValueError("mz_profile: max_rank must be in 0 .. 15")
    out["max_rank"] = int(max_rank)
    return out


def _mzp_cell(x):
    """floor(x) + MZP_BINS / 2 per element, -1 below the axis, MZP_BINS at or above it (csrc/mz_profile.hip: mzp_bin)"""
    half = MZP_BINS // 2
    fl = np.floor(x)
    below = ~(fl >= -float(half))
    above = ~below & ~(fl < float(half))
    q = np.where(below | above, 0.0, fl).astype(np.int64) + half
    return np.where(below, -1, np.where(above, MZP_BINS, q))


def mz_profile(ion_off, ions, n_sig, run, n_slots, params):
    """The table ``score_batch(mz_profile=...)`` returns, from the ion records of the same batch (``score_batch(ions=True)``:
    ``ion_off``, ``ions``) and its ``n_sig``: the definition of ``pya_mz_profile`` operation for operation, in float64.
    ``run``: one slot per PSM (negative: left out) or None (slot 0); a contributing PSM whose slot is at or above ``n_slots``
    is a ValueError (the library answers PYA_ERR_LIMIT).  ``params``: ``mz_profile_params(...)``."""
    ion_off = np.asarray(ion_off, np.int64)
    ions = np.asarray(ions, np.dtype(_lib.ION_DTYPE))
    n_sig = np.asarray(n_sig)
    n = n_sig.size
    run = np.zeros(n, np.int64) if run is None else np.asarray(run).astype(np.int64)
    if ion_off.size != n + 1 or run.shape != (n,):
        raise ValueError("mz_profile: ion_off has n_psm + 1 entries, run one per PSM")
    n_slots = int(n_slots)
    table = np.zeros(n_slots, MZ_PROFILE_DTYPE)
    contributes = (n_sig > 0) & (run >= 0)
    if (run[contributes] >= n_slots).any():
        raise ValueError("mz_profile: PSM %d names run slot %d of %d" % (int(np.flatnonzero(contributes & (run >= n_slots))[0]),
                                                                       int(run[contributes].max()), n_slots))
    np.add.at(table["n_psm"], run[contributes], 1)
    psm_of = np.repeat(np.arange(n), np.diff(ion_off))
    take = (ions["site"] == _lib.PYA_ION_WINNER) & contributes[psm_of]
    rec, slot = ions[take], run[psm_of[take]]
    deep = rec["rank"] > params["max_rank"]
    np.add.at(table["n_rank_skipped"], slot[deep], 1)
    rec, slot = rec[~deep], slot[~deep]
    np.add.at(table["n_ions"], slot, 1)
    theo, peak = rec["theo_mz"].astype(np.float64), rec["peak_mz"].astype(np.float64)
    d = peak - theo
    scaled = d * 1e6
    p = scaled / theo
    fb = np.floor(theo * params["inv_band"])
    band = np.where(~(fb >= 0.0), 0.0, np.where(~(fb < float(MZP_BANDS - 1)), float(MZP_BANDS - 1), fb)).astype(np.int64)
    for unit, value, inv in (("da", d, params["inv_da"]), ("ppm", p, params["inv_ppm"])):
        q = _mzp_cell(value * inv)
        inside = (q >= 0) & (q < MZP_BINS)
        np.add.at(table[unit], (slot[inside], band[inside], q[inside]), 1)
        np.add.at(table["out_" + unit], (slot[q < 0], 0), 1)
        np.add.at(table["out_" + unit], (slot[q >= MZP_BINS], 1), 1)
    return table


def _lane_sum(values):
    """The sum of ``pya_coverage``: 64 partials, element k into partial k mod 64 from 0.0 in index order, the partials then
    added in order from 0.0 -- plain Python floats (IEEE double), two explicit loops."""
    part = [0.0] * 64
    for k, v in enumerate(values):
        part[k & 63] = part[k & 63] + v
    s = 0.0
    for lane in range(64):
        s = s + part[lane]
    return s


def _longest_run(sizes):
    best = run = 0
    prev = None
    for s in sorted(sizes):
        run = run + 1 if prev is not None and s == prev + 1 else 1
        best = max(best, run)
        prev = s
    return best


def coverage(ion_off, ions, mz, intensity, peak_off, pep_len, forward_types, scored, spec_of=None, n_retained=None):
    """The records ``score_batch(coverage=True)`` returns, from the ion records of the same batch (``score_batch(ions=True)``:
    ``ion_off``, ``ions``; only section 1, ``site`` 255, is read) and the raw arrays that were scored: the definition of
    ``pya_coverage`` restated, the four sums in its order with explicit loops.  ``pep_len``: the peptide length of every PSM;
    ``forward_types``: the forward ion types of the scorer, e.g. ``"b"`` or ``"bc"``; ``scored``: one boolean per PSM (status 0
    and ``n_sig > 0``), the others get the all-zero record; ``spec_of``: the spectrum of every PSM of a shared batch;
    ``n_retained``: the peaks the binning kept per PSM, which neither the ion records nor the raw arrays tell (None: the field
    stays 0)."""
    ion_off = np.asarray(ion_off, np.int64)
    ions = np.asarray(ions, np.dtype(_lib.ION_DTYPE))
    peak_off = np.asarray(peak_off, np.int64)
    scored = np.asarray(scored, bool)
    n = scored.size
    pep_len = np.asarray(pep_len, np.int64)
    if ion_off.size != n + 1 or pep_len.shape != (n,):
        raise ValueError("coverage: ion_off has n_psm + 1 entries, pep_len and scored one per PSM")
    mz, intensity = np.asarray(mz), np.asarray(intensity)
    fwd_codes = [ord(c) for c in forward_types]
    out = np.zeros(n, COVERAGE_DTYPE)
    for i in range(n):
        if not scored[i]:
            continue
        s = i if spec_of is None else int(spec_of[i])
        a, b = int(peak_off[s]), int(peak_off[s + 1])
        x = mz[a:b].astype(np.float32)                      # (a float32 m/z is taken as it is)
        y = intensity[a:b].astype(np.float64).tolist()      # (float32 widens exactly)
        rec = ions[ion_off[i]:ion_off[i + 1]]
        rec = rec[rec["site"] == _lib.PYA_ION_WINNER]
        is_fwd = np.isin(rec["type"], fwd_codes)
        in_fwd = np.isin(x, rec["peak_mz"][is_fwd]).tolist()        # (float32 equality: a NaN equals nothing)
        in_bwd = np.isin(x, rec["peak_mz"][~is_fwd]).tolist()
        r = out[i]
        r["total_current"] = _lane_sum(y)
        r["explained_current"] = _lane_sum([v if f or k else 0.0 for v, f, k in zip(y, in_fwd, in_bwd)])
        r["nterm_current"] = _lane_sum([v if f else 0.0 for v, f in zip(y, in_fwd)])
        r["cterm_current"] = _lane_sum([v if k else 0.0 for v, k in zip(y, in_bwd)])
        r["n_peaks"] = b - a
        r["n_retained"] = 0 if n_retained is None else int(n_retained[i])
        r["n_explained"] = sum(1 for f, k in zip(in_fwd, in_bwd) if f or k)
        r["n_fragments"] = rec.size
        L = int(pep_len[i])
        f_sizes = set(rec["size"][is_fwd].tolist())
        b_sizes = set(rec["size"][~is_fwd].tolist())
        r["nterm_sizes"], r["cterm_sizes"] = len(f_sizes), len(b_sizes)
        r["nterm_run"], r["cterm_run"] = _longest_run(f_sizes), _longest_run(b_sizes)
        r["bonds"] = len(f_sizes | set(L - t for t in b_sizes))
        r["kind"] = _lib.PYA_COV_SCORED
    return out


def coverage_ratios(rec):
    """``dict(explained, nterm, cterm, peaks)`` of coverage records, one float64 per record: explained / total, N-terminal /
    total and C-terminal / total ion current, explained peaks / retained peaks -- 0 where the denominator is 0."""
    rec = np.asarray(rec, COVERAGE_DTYPE)
    total, kept = rec["total_current"], rec["n_retained"].astype(np.float64)

    def over(num, den):
        out = np.zeros(rec.shape, np.float64)
        ok = den != 0
        with np.errstate(invalid="ignore", over="ignore"):
            out[ok] = num[ok] / den[ok]
        return out
    return dict(explained=over(rec["explained_current"], total), nterm=over(rec["nterm_current"], total),
                cterm=over(rec["cterm_current"], total), peaks=over(rec["n_explained"].astype(np.float64), kept))


def merge_mz_profiles(*tables):
    """The sum of tables of one shape, word by word (32-bit counts wrap, as on the device): the profile of the PSMs behind
    all of them."""
    if not tables:
        raise ValueError("merge_mz_profiles: no table")
    parts = [np.ascontiguousarray(t, MZ_PROFILE_DTYPE).reshape(-1) for t in tables]
    if any(p.size != parts[0].size for p in parts):
        raise ValueError("merge_mz_profiles: the tables have different numbers of slots")
    words = np.zeros(parts[0].size * (MZ_PROFILE_DTYPE.itemsize // 4), np.uint32)
    for p in parts:
        words += p.view(np.uint32)
    return words.view(MZ_PROFILE_DTYPE)


def _mzp_quantile(hist, q):
    """where the fraction q of the counts of a 1-D histogram lies, in bins from the lower edge of bin 0, interpolated inside
    the bin; nan for an empty histogram"""
    total = float(hist.sum())
    if total == 0.0:
        return float("nan")
    cum = np.cumsum(hist.astype(np.float64))
    target = q * total
    j = int(np.searchsorted(cum, target, side="left"))
    j = min(j, hist.size - 1)
    while hist[j] == 0:                                  # (target == 0: the first bin that has counts)
        j += 1
    before = cum[j] - float(hist[j])
    return j + (target - before) / float(hist[j])


def mz_profile_summary(table, params=None):
    """One dict per slot: ``n_psm``, ``n_ions``, ``n_rank_skipped`` and per unit (``"da"``, ``"ppm"``) a dict with ``total``
    (the ions inside the axis), ``below`` / ``above`` (outside it), ``median``, ``q05``, ``q95`` (interpolated inside the bins),
    ``background`` (the mean count per bin of the two outermost bins on each side: the flat floor random matches leave) and
    ``band_medians`` (``MZP_BANDS`` values, nan for a band without ions).  With ``params`` (``mz_profile_params``) the
    positions are in Da and ppm; without, in bins from 0 (bin ``MZP_BINS / 2`` starts at 0.0)."""
    table = np.asarray(table, MZ_PROFILE_DTYPE).reshape(-1)
    half = MZP_BINS // 2
    out = []
    for rec in table:
        row = dict(n_psm=int(rec["n_psm"]), n_ions=int(rec["n_ions"]), n_rank_skipped=int(rec["n_rank_skipped"]))
        for unit in ("da", "ppm"):
            width = 1.0 if params is None else 1.0 / params["inv_" + unit]
            bands = rec[unit].astype(np.int64)
            hist = bands.sum(axis=0)
            where = lambda h, q: float((_mzp_quantile(h, q) - half) * width)
            row[unit] = dict(total=int(hist.sum()), below=int(rec["out_" + unit][0]), above=int(rec["out_" + unit][1]),
                             median=where(hist, 0.5), q05=where(hist, 0.05), q95=where(hist, 0.95),
                             background=float(hist[[0, 1, MZP_BINS - 2, MZP_BINS - 1]].mean()),
                             band_medians=[where(b, 0.5) for b in bands])
        out.append(row)
    return out


def fit_mz_calibration(table, params, min_ions=20):
    """One ``MZ_CALIBRATION_DTYPE`` record per slot of a profile ``table`` (``MZ_PROFILE_DTYPE``): the definition of
    ``pya_mz_calibration`` in include/pyascore_hip.h, integer sums and the same IEEE divisions, so the bytes are those of
    ``pya_mz_profile_fit``.  Per band of m/z the four outermost bins of the ppm axis give the flat floor of random matches;
    what stands above it is the signal, its median the systematic error ``ppm`` at the band's centre, half of its 16 % .. 84 %
    width ``spread_ppm``; a band with fewer than ``min_ions`` signal ions copies the nearest fitted band (the lower on a tie).
    ``params``: ``mz_profile_params(...)`` the table was binned with (``inv_ppm`` is what is used)."""
    table = np.ascontiguousarray(table, MZ_PROFILE_DTYPE).reshape(-1)
    inv_ppm = float(params["inv_ppm"])
    if not (np.isfinite(inv_ppm) and inv_ppm > 0.0):
        raise ValueError("fit_mz_calibration: inv_ppm = %r is not a finite positive number" % inv_ppm)
    if int(min_ions) != min_ions or not 1 <= int(min_ions) <= 0xFFFFFFFF:
        raise ValueError("fit_mz_calibration: min_ions must be in 1 .. 2^32 - 1")
    min_ions = int(min_ions)
    out = np.zeros(table.size, MZ_CALIBRATION_DTYPE)
    half = MZP_BINS // 2
    for s, rec in enumerate(table):
        fitted = []
        for b in range(MZP_BANDS):
            h = [int(v) for v in rec["ppm"][b]]
            floor4 = h[0] + h[1] + h[MZP_BINS - 2] + h[MZP_BINS - 1]
            ex = [max(0, 4 * v - floor4) for v in h]
            cum, run = [], 0
            for v in ex:
                run += v
                cum.append(run)
            E = run
            out["n_signal"][s, b] = min(E // 4, 0xFFFFFFFF)
            if E < 4 * min_ions:
                continue
            pos = {}
            for num in (16, 50, 84):
                j = next(i for i in range(MZP_BINS) if 100 * cum[i] >= num * E)
                pos[num] = float(j) + float(num * E - 100 * (cum[j] - ex[j])) / float(100 * ex[j])
            out["ppm"][s, b] = (pos[50] - float(half)) / inv_ppm
            out["spread_ppm"][s, b] = np.float32((0.5 * (pos[84] - pos[16])) / inv_ppm)
            fitted.append(b)
        for b in range(MZP_BANDS):
            if fitted and b not in fitted:
                out["ppm"][s, b] = out["ppm"][s, min(fitted, key=lambda f: (abs(f - b), f))]
    return out


def _check_calibration(cal):
    cal = np.ascontiguousarray(cal, MZ_CALIBRATION_DTYPE).reshape(-1)
    bad = ~(np.abs(cal["ppm"]) <= float(MZC_MAX_PPM))                   # (nan fails the comparison)
    if bad.any():
        raise ValueError("calibration slot %d has a knot that is not finite or beyond %d ppm" % (int(np.flatnonzero(bad.any(axis=1))[0]), MZC_MAX_PPM))
    return cal


def recalibrate(mz, peak_off, run, cal, band_width=250.0):
    """The m/z array of spectra corrected with a calibration: the APPLY of ``pya_mz_calibration``, operation for operation in
    float64, so the bytes are those of ``pya_recalibrate_spectra``.  ``mz``: float64 or float32 (the result keeps the dtype:
    float32 is widened, corrected and rounded back once), ``peak_off[n_spectra + 1]``, ``run``: one slot per spectrum
    (negative: left as it is) or None (slot 0), ``cal``: ``MZ_CALIBRATION_DTYPE`` records.  The knots sit at the centres of the
    bands and the error is linear between them, constant outside; a value that is not finite or not positive is copied.  A
    slot outside ``cal`` or a knot that is not finite or beyond ``MZC_MAX_PPM`` is a ValueError.  Returns a new array."""
    mz = np.asarray(mz)
    if mz.dtype not in (np.dtype(np.float64), np.dtype(np.float32)):
        raise ValueError("recalibrate: mz is float64 or float32, not %s" % mz.dtype)
    peak_off = np.asarray(peak_off, np.int64)
    n_spec = peak_off.size - 1
    cal = _check_calibration(cal)
    inv_band = 1.0 / float(band_width) if band_width else float("inf")
    if not (np.isfinite(inv_band) and inv_band > 0.0):
        raise ValueError("recalibrate: band_width = %r has no finite positive inverse" % band_width)
    run = np.zeros(n_spec, np.int64) if run is None else np.asarray(run).astype(np.int64)
    if run.shape != (n_spec,):
        raise ValueError("recalibrate: run is one slot per spectrum")
    if (run >= cal.size).any():
        raise ValueError("recalibrate: spectrum %d names slot %d of %d" % (int(np.flatnonzero(run >= cal.size)[0]), int(run.max()), cal.size))
    out = mz.copy()
    lo, hi = int(peak_off[0]), int(peak_off[-1])
    slot = np.repeat(run, np.diff(peak_off))
    x = mz[lo:hi].astype(np.float64)
    take = (slot >= 0) & (x > 0.0) & (x < np.inf)
    x, slot = x[take], slot[take]
    u = x * inv_band - 0.5
    fl = np.floor(u)
    top = float(MZP_BANDS - 2)
    j = np.where(~(fl >= 0.0), 0.0, np.where(~(fl < top), top, fl))
    rel = u - j
    t = np.where(~(rel >= 0.0), 0.0, np.where(~(rel < 1.0), 1.0, rel))
    j = j.astype(np.int64)
    a, b = cal["ppm"][slot, j], cal["ppm"][slot, j + 1]
    step = (b - a) * t
    e = a + step
    c = e * 1e-6
    shift = x * c
    view = out[lo:hi]
    view[take] = (x - shift).astype(mz.dtype)
    return out


def mz_calibration_rows(cal, band_width=250.0):
    """The ``--mz_calibration_out`` table: one row ``[slot, band, band centre, ppm, spread, signal ions, band width]`` per slot
    and band; floats as ``repr``, so ``read_mz_calibration`` gives the same bytes back."""
    cal = np.ascontiguousarray(cal, MZ_CALIBRATION_DTYPE).reshape(-1)
    width = float(band_width)
    return [[s, b, repr((b + 0.5) * width), repr(float(rec["ppm"][b])), repr(float(rec["spread_ppm"][b])), int(rec["n_signal"][b]), repr(width)]
            for s, rec in enumerate(cal) for b in range(MZP_BANDS)]


def read_mz_calibration(path):
    """``(cal, band_width)`` of a file of ``mz_calibration_rows`` under a header line (``--mz_calibration_out`` writes it):
    ``MZ_CALIBRATION_DTYPE`` records, one per slot, and the width of the bands they were fitted over."""
    rows = []
    with open(path) as f:
        next(f, None)
        for line in f:
            if line.strip():
                rows.append(line.rstrip("\n").split("\t"))
    if not rows:
        return np.zeros(0, MZ_CALIBRATION_DTYPE), 250.0
    if any(len(r) != 7 for r in rows):
        raise ValueError("%s: a calibration line has seven columns" % path)
    widths = {float(r[6]) for r in rows}
    if len(widths) != 1:
        raise ValueError("%s: more than one band width" % path)
    cal = np.zeros(max(int(r[0]) for r in rows) + 1, MZ_CALIBRATION_DTYPE)
    seen = set()
    for r in rows:
        s, b = int(r[0]), int(r[1])
        if not 0 <= b < MZP_BANDS or s < 0 or (s, b) in seen:
            raise ValueError("%s: slot %d band %d is out of range or given twice" % (path, s, b))
        seen.add((s, b))
        cal["ppm"][s, b], cal["spread_ppm"][s, b], cal["n_signal"][s, b] = float(r[3]), np.float32(float(r[4])), int(r[5])
    if len(seen) != cal.size * MZP_BANDS:
        raise ValueError("%s: every slot needs its %d bands" % (path, MZP_BANDS))
    return cal, widths.pop()


def suggest_mz_error(cal, mz_max, k=3.0):
    """A convenience, not a rule: ``k`` times the largest fitted ``spread_ppm`` at ``mz_max``, in Da -- a tolerance for the
    narrow re-run on recalibrated spectra that covers ``k`` spreads of the worst band at the highest fragment m/z.  0.0 when
    nothing was fitted."""
    cal = np.ascontiguousarray(cal, MZ_CALIBRATION_DTYPE).reshape(-1)
    worst = float(cal["spread_ppm"].max()) if cal.size else 0.0
    return float(k) * worst * 1e-6 * float(mz_max)


def _transform_entry(who, mz, intensity, peak_off):
    """What ``deisotope``, ``decharge``, ``strip`` and ``centroid`` (``who``) refuse about their spectra alike.  Returns
    ``(raw_mz, raw_it, rel)``: the elements ``peak_off[0]:peak_off[-1]`` of the arrays (views, the dtypes stay) and the offsets
    into them."""
    mz, intensity = np.asarray(mz), np.asarray(intensity)
    for name, a in (("mz", mz), ("intensity", intensity)):
        if a.dtype not in (np.dtype(np.float64), np.dtype(np.float32)) or a.ndim != 1:
            raise ValueError("%s: %s is a one-dimensional float64 or float32 array" % (who, name))
    peak_off = np.asarray(peak_off, np.int64)
    if peak_off.ndim != 1 or peak_off.size < 1 or peak_off[0] < 0 or (np.diff(peak_off) < 0).any():
        raise ValueError("%s: peak_off has n_spectra + 1 offsets that do not descend" % who)
    first, last = int(peak_off[0]), int(peak_off[-1])
    if mz.size < last or intensity.size < last:
        raise ValueError("%s: peak_off runs past the end of the spectrum arrays" % who)
    return mz[first:last], intensity[first:last], peak_off - first


def _transform_exit(keep, rel):
    """``(before, kept, new_off)`` of a mask over the peaks: the kept peaks in front of every peak, the kept peaks of every
    spectrum and their offsets (from 0)"""
    before = np.concatenate([[0], np.cumsum(keep, dtype=np.int64)])
    kept = before[rel[1:]] - before[rel[:-1]]
    return before, kept, np.concatenate([[0], np.cumsum(kept)]).astype(np.int64)


def deisotope_params(tol=0.01, max_charge=3, step=1.0033548378, ratio=1.0, ratio_per_mz=0.0):
    """The parameters of the deisotoping rule (``pya_deisotope_params``) as a dict: ``tol`` the half width of the match on the
    isotope spacing in m/z units, ``max_charge`` the largest charge tried (1 .. 8), ``spacing`` the tuple ``step / z`` for
    z = 1 .. max_charge -- computed here, once, so the device and ``deisotope`` read the same bits --, ``ratio0`` and
    ``ratio_per_mz``: a satellite is at most ``ratio0 + ratio_per_mz * (m/z of the parent) * z`` times as intense as its
    parent.  ValueError where the library would refuse: a ``tol`` that is not finite or negative, a charge outside 1 .. 8, a
    ``step`` that is not finite and positive, ``step / max_charge <= 2 tol``, a ratio that is not finite."""
    tol, step, ratio, ratio_per_mz = float(tol), float(step), float(ratio), float(ratio_per_mz)
    if int(max_charge) != max_charge or not 1 <= int(max_charge) <= DEISO_MAX_CHARGE:
        raise ValueError("deisotope: max_charge = %r is not an integer in 1 .. %d" % (max_charge, DEISO_MAX_CHARGE))
    max_charge = int(max_charge)
    if not (np.isfinite(tol) and tol >= 0.0):
        raise ValueError("deisotope: tol = %r is not a finite number >= 0" % tol)
    if not (np.isfinite(step) and step > 0.0):
        raise ValueError("deisotope: step = %r is not finite and positive" % step)
    if not (np.isfinite(ratio) and np.isfinite(ratio_per_mz)):
        raise ValueError("deisotope: ratio and ratio_per_mz must be finite")
    return check_deisotope_params(dict(tol=tol, ratio0=ratio, ratio_per_mz=ratio_per_mz, max_charge=max_charge,
                                       spacing=tuple(step / float(z) for z in range(1, max_charge + 1))))


def check_deisotope_params(params):
    """``params`` (a dict as ``deisotope_params`` makes it, possibly with spacings of the caller's own) checked against the
    conditions of ``pya_deisotope_params``; returns it with plain Python numbers."""
    try:
        out = dict(tol=float(params["tol"]), ratio0=float(params["ratio0"]), ratio_per_mz=float(params["ratio_per_mz"]),
                   max_charge=int(params["max_charge"]), spacing=tuple(float(v) for v in params["spacing"]))
    except (KeyError, TypeError):
        raise ValueError("deisotope: params is the dict of pyascore_amd.rollup.deisotope_params "
                         "(tol, ratio0, ratio_per_mz, max_charge, spacing)") from None
    sp, n = out["spacing"], out["max_charge"]
    if not 1 <= n <= DEISO_MAX_CHARGE or len(sp) < n:
        raise ValueError("deisotope: max_charge = %d is not in 1 .. %d or has no spacing" % (n, DEISO_MAX_CHARGE))
    out["spacing"] = sp = sp[:n]
    if not (np.isfinite(out["tol"]) and out["tol"] >= 0.0):
        raise ValueError("deisotope: tol = %r is not a finite number >= 0" % out["tol"])
    if not (np.isfinite(out["ratio0"]) and np.isfinite(out["ratio_per_mz"])):
        raise ValueError("deisotope: ratio0 and ratio_per_mz must be finite")
    if not all(np.isfinite(v) and v > 0.0 for v in sp) or any(not sp[z] < sp[z - 1] for z in range(1, n)):
        raise ValueError("deisotope: spacing must be finite, positive and strictly decreasing")
    if not sp[n - 1] > 2.0 * out["tol"]:
        raise ValueError("deisotope: the smallest spacing %r is not above 2 tol = %r" % (sp[n - 1], 2.0 * out["tol"]))
    return out


def deisotope_c_params(params):
    """``params`` as the ``pya_deisotope_params`` structure the library reads."""
    p = check_deisotope_params(params)
    sp = list(p["spacing"]) + [0.0] * (DEISO_MAX_CHARGE - len(p["spacing"]))
    return _lib.DeisotopeParams(p["tol"], p["ratio0"], p["ratio_per_mz"], (_lib.C.c_double * DEISO_MAX_CHARGE)(*sp), p["max_charge"], 0)


def _deisotope_keep(x, y, p):
    """keep[] of one ascending spectrum (float64 views): the rule, candidates by searchsorted, the exact predicate decides"""
    n = x.size
    keep = np.ones(n, bool)
    if n < 2:
        return keep
    tol, idx = p["tol"], np.arange(n)
    with np.errstate(invalid="ignore", over="ignore"):
        for z0, sp in enumerate(p["spacing"]):
            z = float(z0 + 1)
            t = x - sp
            slack = 1e-14 * (np.abs(x) + sp + tol)          # (far above the rounding of t and of the predicate: a superset)
            lo = np.searchsorted(x, t - tol - slack, "left")
            hi = np.minimum(np.searchsorted(x, t + tol + slack, "right"), idx)
            cnt = np.maximum(hi - lo, 0)
            total = int(cnt.sum())
            if total == 0:
                continue
            jj = np.repeat(idx, cnt)
            ii = np.repeat(lo, cnt) + (np.arange(total) - np.repeat(np.cumsum(cnt) - cnt, cnt))
            d = x[jj] - x[ii]
            e = d - sp
            m = x[ii] * z
            b = p["ratio0"] + p["ratio_per_mz"] * m
            ok = (np.fabs(e) <= tol) & (y[jj] <= y[ii] * b)
            keep[jj[ok]] = False
    return keep


def deisotope(mz, intensity, peak_off, params):
    """Deisotoped spectra: the rule of ``pya_deisotope_params``, operation for operation in float64, so the bytes are those of
    ``pya_deisotope_spectra``.  ``mz`` / ``intensity``: float64 or float32 (widened for the decision, the kept elements are
    copied bit for bit and the dtype stays), ``peak_off[n_spectra + 1]``, ``params`` of ``deisotope_params``.  Peak j of a
    spectrum goes iff a peak i of it and a charge z have ``|mz[j] - mz[i] - spacing[z - 1]| <= tol`` and ``intensity[j] <=
    intensity[i] * (ratio0 + ratio_per_mz * mz[i] * z)``; the parent may itself go, the lowest peak always stays.  A spectrum
    that is not ascending (a descending pair or a NaN m/z) comes back unchanged.  Returns ``(mz, intensity, peak_off, keep)``:
    new arrays of the kept peaks, their offsets (from 0) and the boolean mask over ``peak_off[0]:peak_off[-1]``."""
    p = check_deisotope_params(params)
    raw_mz, raw_it, rel = _transform_entry("deisotope", mz, intensity, peak_off)
    x, y = raw_mz.astype(np.float64), raw_it.astype(np.float64)
    keep = np.ones(x.size, bool)
    for s in range(rel.size - 1):
        a, b = int(rel[s]), int(rel[s + 1])
        if b - a < 2 or not (x[a:b - 1] <= x[a + 1:b]).all():
            continue
        keep[a:b] = _deisotope_keep(x[a:b], y[a:b], p)
    return raw_mz[keep].copy(), raw_it[keep].copy(), _transform_exit(keep, rel)[2], keep


def decharge_params(tol=0.01, max_charge=3, step=1.0033548378, ratio=1.0, ratio_per_mz=0.0, carrier=DECHARGE_CARRIER, witness=0.3):
    """The parameters of charge deconvolution (``pya_decharge_params``) as a dict: those of ``deisotope_params`` (same
    arguments, same checks) and beside them ``carrier``, the mass one charge adds -- by default the 1.007825 the scoring
    kernels add per charge, so that a reduced peak lands where a run computes the fragment at 1+ --, and ``witness``: a removed
    satellite testifies to a charge of its parent only when it has at least ``witness`` times the parent's intensity.  The
    default 0.3 rests on a synthetic measurement (satellites at 0.5 and 0.2 times the parent), not on real
    isotope envelopes.  ValueError where the library would refuse: what ``deisotope_params`` refuses, a ``carrier`` that is not
    finite and positive, a ``witness`` that is not finite or negative."""
    iso = deisotope_params(tol=tol, max_charge=max_charge, step=step, ratio=ratio, ratio_per_mz=ratio_per_mz)
    return check_decharge_params(dict(iso, carrier=carrier, witness=witness))


def check_decharge_params(params):
    """``params`` (a dict as ``decharge_params`` makes it) checked against the conditions of ``pya_decharge_params``; returns it
    with plain Python numbers."""
    try:
        out = check_deisotope_params(params)
        out.update(carrier=float(params["carrier"]), witness=float(params["witness"]))
    except (KeyError, TypeError):
        raise ValueError("decharge: params is the dict of pyascore_amd.rollup.decharge_params "
                         "(tol, ratio0, ratio_per_mz, max_charge, spacing, carrier, witness)") from None
    if not (np.isfinite(out["carrier"]) and out["carrier"] > 0.0):
        raise ValueError("decharge: carrier = %r is not finite and positive" % out["carrier"])
    if not (np.isfinite(out["witness"]) and out["witness"] >= 0.0):
        raise ValueError("decharge: witness = %r is not a finite number >= 0" % out["witness"])
    return out


def decharge_c_params(params):
    """``params`` as the ``pya_decharge_params`` structure the library reads."""
    p = check_decharge_params(params)
    return _lib.DechargeParams(deisotope_c_params(p), p["carrier"], p["witness"])


def _decharge_charge(x, y, p):
    """c[] of one ascending spectrum (float64 views) as if every peak were kept: the largest witnessed z of 2 .. max_charge,
    else 1; candidates by searchsorted, the exact predicate decides"""
    n = x.size
    c = np.ones(n, np.int64)
    if n < 2:
        return c
    tol, idx = p["tol"], np.arange(n)
    with np.errstate(invalid="ignore", over="ignore"):
        least = y * p["witness"]
        for z0, sp in enumerate(p["spacing"]):
            if z0 == 0:
                continue
            z = float(z0 + 1)
            t = x + sp
            slack = 1e-14 * (np.abs(x) + sp + tol)          # (far above the rounding of t and of the predicate: a superset)
            lo = np.maximum(np.searchsorted(x, t - tol - slack, "left"), idx + 1)
            hi = np.searchsorted(x, t + tol + slack, "right")
            cnt = np.maximum(hi - lo, 0)
            total = int(cnt.sum())
            if total == 0:
                continue
            ii = np.repeat(idx, cnt)
            jj = np.repeat(lo, cnt) + (np.arange(total) - np.repeat(np.cumsum(cnt) - cnt, cnt))
            d = x[jj] - x[ii]
            e = d - sp
            m = x[ii] * z
            b = p["ratio0"] + p["ratio_per_mz"] * m
            ok = (np.fabs(e) <= tol) & (y[jj] <= y[ii] * b) & (y[jj] >= least[ii])
            c[ii[ok]] = z0 + 1                              # (z rises: the largest stays)
    return c


def decharge(mz, intensity, peak_off, params):
    """Charge-deconvolved spectra: the rule of ``pya_decharge_params``, operation for operation in float64, so the bytes are
    those of ``pya_decharge_spectra``.  Arguments as ``deisotope`` takes them, ``params`` of ``decharge_params``.  The kept peaks
    are those ``deisotope`` keeps; a kept peak with a witnessed satellite at spacing / z, z >= 2, moves to ``mz * c -
    (c - 1) * carrier`` (c the largest such z; rounded once to the dtype of ``mz``) if that is finite and above where it was;
    every spectrum comes out sorted by m/z, equal values in raw order.  A spectrum that is not ascending comes back unchanged.
    Returns ``(mz, intensity, peak_off, charge, keep)``: new arrays of the output peaks, their offsets (from 0), one ``uint8``
    per output peak with its charge (1: not moved, bits of m/z copied), and the boolean mask of the kept peaks over
    ``peak_off[0]:peak_off[-1]`` of the input."""
    p = check_decharge_params(params)
    raw_mz, raw_it, rel = _transform_entry("decharge", mz, intensity, peak_off)
    x, y = raw_mz.astype(np.float64), raw_it.astype(np.float64)
    keep = np.ones(x.size, bool)
    order = np.arange(x.size)                                # raw indices, to become the output order of the kept peaks
    stored, charge = raw_mz.copy(), np.ones(x.size, np.uint8)
    for s in range(rel.size - 1):
        a, b = int(rel[s]), int(rel[s + 1])
        if b - a < 2 or not (x[a:b - 1] <= x[a + 1:b]).all():
            continue
        keep[a:b] = _deisotope_keep(x[a:b], y[a:b], p)
        if p["max_charge"] < 2:
            continue
        c = np.where(keep[a:b], _decharge_charge(x[a:b], y[a:b], p), 1)
        with np.errstate(invalid="ignore", over="ignore"):
            t = x[a:b] * c.astype(np.float64)
            u = (c - 1).astype(np.float64) * p["carrier"]
            v = t - u
            new = v.astype(raw_mz.dtype)
            wide = new.astype(np.float64)
            moves = (c >= 2) & np.isfinite(wide) & (wide > x[a:b])
        if not moves.any():
            continue
        stored[a:b][moves] = new[moves]
        charge[a:b][moves] = c[moves]
        kept = np.flatnonzero(keep[a:b])
        value = np.where(moves, wide, x[a:b])[kept]
        order[a:b][kept] = kept[np.argsort(value, kind="stable")] + a
    pick = order[keep]
    return stored[pick].copy(), raw_it[pick].copy(), _transform_exit(keep, rel)[2], charge[pick].copy(), keep


def strip_params(tol, losses=(), reduced=False, isotopes=0, step=STRIP_STEP, mz_lo=float("-inf"), mz_hi=float("inf")):
    """The parameters of precursor stripping (``pya_strip_params``) as a dict: ``tol`` the half width of a window in m/z units,
    ``loss`` the tuple ``(0.0,) + losses`` -- entry 0 is the precursor itself, the others the neutral masses taken off it (up to
    7: 97.976896 for H3PO4, 18.010565 for water, ...) --, ``reduced``: windows at every charge from the precursor's down to 1
    (the charge-reduced precursors of ETD) instead of at the precursor's alone, ``isotopes`` the isotope peaks above its centre
    a window covers (0 .. 4) at ``step / charge`` each, ``mz_lo`` / ``mz_hi`` the range outside which every peak goes (a TMT
    reporter region: ``mz_lo=140``).  ValueError where the library would refuse: a ``tol`` that is not finite or negative, a
    ``step`` that is not finite and positive, a NaN bound or ``mz_lo > mz_hi``, more than 7 losses or one that is not finite or
    negative, ``isotopes`` outside 0 .. 4."""
    try:
        losses = tuple(float(v) for v in losses)
    except TypeError:
        raise ValueError("strip: losses is a sequence of neutral masses") from None
    if isinstance(reduced, (bool, np.bool_)):
        reduced = int(reduced)
    return check_strip_params(dict(tol=tol, step=step, mz_lo=mz_lo, mz_hi=mz_hi, loss=(0.0,) + losses, reduced=reduced, isotopes=isotopes))


def check_strip_params(params):
    """``params`` (a dict as ``strip_params`` makes it) checked against the conditions of ``pya_strip_params``; returns it with
    plain Python numbers."""
    try:
        out = dict(tol=float(params["tol"]), step=float(params["step"]), mz_lo=float(params["mz_lo"]), mz_hi=float(params["mz_hi"]),
                   loss=tuple(float(v) for v in params["loss"]), reduced=params["reduced"], isotopes=params["isotopes"])
    except (KeyError, TypeError, ValueError):
        raise ValueError("strip: params is the dict of pyascore_amd.rollup.strip_params "
                         "(tol, step, mz_lo, mz_hi, loss, reduced, isotopes)") from None
    if not (np.isfinite(out["tol"]) and out["tol"] >= 0.0):
        raise ValueError("strip: tol = %r is not a finite number >= 0" % out["tol"])
    if not (np.isfinite(out["step"]) and out["step"] > 0.0):
        raise ValueError("strip: step = %r is not finite and positive" % out["step"])
    if np.isnan(out["mz_lo"]) or np.isnan(out["mz_hi"]) or not out["mz_lo"] <= out["mz_hi"]:
        raise ValueError("strip: mz_lo = %r and mz_hi = %r are not numbers with mz_lo <= mz_hi" % (out["mz_lo"], out["mz_hi"]))
    loss = out["loss"]
    if not 1 <= len(loss) <= STRIP_MAX_LOSS + 1 or loss[0] != 0.0:
        raise ValueError("strip: loss is (0.0, ...) with at most %d losses behind it" % STRIP_MAX_LOSS)
    if not all(np.isfinite(v) and v >= 0.0 for v in loss):
        raise ValueError("strip: every loss is a finite number >= 0")
    for name, top in (("reduced", 1), ("isotopes", STRIP_MAX_ISOTOPES)):
        v = out[name]
        try:
            ok = int(v) == v and 0 <= int(v) <= top
        except (TypeError, ValueError, OverflowError):
            ok = False
        if not ok:
            raise ValueError("strip: %s = %r is not an integer in 0 .. %d" % (name, v, top))
        out[name] = int(v)
    return out


def strip_c_params(params):
    """``params`` as the ``pya_strip_params`` structure the library reads."""
    p = check_strip_params(params)
    loss = list(p["loss"]) + [0.0] * (STRIP_MAX_LOSS + 1 - len(p["loss"]))
    return _lib.StripParams(p["tol"], p["step"], p["mz_lo"], p["mz_hi"], (_lib.C.c_double * (STRIP_MAX_LOSS + 1))(*loss), len(p["loss"]) - 1,
                            p["reduced"], p["isotopes"], 0)


def _strip_precursors(prec_mz, prec_z, what="strip"):
    pm, pz = np.asarray(prec_mz), np.asarray(prec_z)
    if pm.dtype.kind not in "fiu" or pz.dtype.kind not in "iu" or pm.shape != pz.shape or pm.ndim > 1:
        raise ValueError("%s: prec_mz is one number per spectrum and prec_z one integer per spectrum" % what)
    if pz.size and (pz.min() < -2 ** 31 or pz.max() > 2 ** 31 - 1):
        raise ValueError("%s: prec_z does not fit an int32" % what)
    return np.ascontiguousarray(pm, np.float64), np.ascontiguousarray(pz, np.int32)


def strip_windows(prec_mz, prec_z, params):
    """The windows of ``pya_strip_params`` for precursors ``prec_mz`` (float64) / ``prec_z`` (int32), one per spectrum (or one
    pair of numbers): ``(lo, hi, active)``, float64, float64 and bool of shape ``[n_spectra, 64]`` (``[64]`` for one pair),
    column ``w = c * (n_loss + 1) + l`` being the window of charge ``prec_z - c`` and ``loss[l]`` -- the header's operations in
    float64, one rounding each.  ``lo`` / ``hi`` are NaN where ``active`` is False."""
    p = check_strip_params(params)
    one = np.ndim(prec_mz) == 0
    pm, pz = _strip_precursors(prec_mz, prec_z, "strip_windows")
    pm, pz = pm.reshape(-1), pz.reshape(-1)
    per = len(p["loss"])
    w = np.arange(STRIP_WINDOWS)
    c, l = w // per, w % per
    loss = np.asarray(p["loss"], np.float64)[l]
    has = (pz >= 1) & (pz <= STRIP_MAX_CHARGE) & np.isfinite(pm) & (pm > 0.0)
    n_charge = np.where(has, pz if p["reduced"] else 1, 0)
    valid = c[None, :] < n_charge[:, None]
    zr = np.where(valid, pz[:, None] - c[None, :], 1).astype(np.float64)
    with np.errstate(all="ignore"):
        m = pm * pz.astype(np.float64)
        cen = (m[:, None] - loss[None, :]) / zr
        span = np.float64(p["isotopes"]) * (np.float64(p["step"]) / zr)
        lo = cen - np.float64(p["tol"])
        hi = (cen + span) + np.float64(p["tol"])
        active = valid & np.isfinite(cen) & (cen > 0.0)
    lo, hi = np.where(active, lo, np.nan), np.where(active, hi, np.nan)
    return (lo[0], hi[0], active[0]) if one else (lo, hi, active)


def strip_hits(report, params):
    """The ``hit`` word of ``STRIP_REPORT_DTYPE`` records read as a bool array ``[n_spectra, n_charges, n_loss + 1]``:
    ``[s, c, l]`` says that spectrum s had a peak in the window of charge ``prec_z - c`` and ``loss[l]`` (``l = 0``: the
    precursor itself).  ``n_charges`` is 8 with ``reduced``, else 1."""
    p = check_strip_params(params)
    per = len(p["loss"])
    n_c = STRIP_MAX_CHARGE if p["reduced"] else 1
    hit = np.asarray(report, STRIP_REPORT_DTYPE).reshape(-1)["hit"]
    bits = (hit[:, None] >> np.arange(n_c * per, dtype=np.uint64)[None, :]) & np.uint64(1)
    return bits.astype(bool).reshape(hit.size, n_c, per)


def strip(mz, intensity, peak_off, prec_mz, prec_z, params):
    """Spectra without their precursor-derived peaks: the rule of ``pya_strip_params``, operation for operation in float64, so
    the bytes are those of ``pya_strip_spectra``.  ``mz`` / ``intensity``: float64 or float32 (widened for the decision, the
    kept elements are copied bit for bit and the dtype stays), ``peak_off[n_spectra + 1]``, ``prec_mz`` / ``prec_z`` one
    precursor m/z and charge per spectrum (a charge outside 1 .. 8 or an m/z that is not finite and positive: no windows),
    ``params`` of ``strip_params``.  A peak goes iff its m/z lies below ``mz_lo``, above ``mz_hi`` or inside an active window of
    its spectrum (``strip_windows``), bounds included; a NaN m/z stays; the order of the peaks plays no part.  Returns ``(mz,
    intensity, peak_off, report)``: new arrays of the kept peaks in input order, their offsets (from 0) and one
    ``STRIP_REPORT_DTYPE`` record per spectrum (``hit``: bit w set iff a peak lay in active window w; ``n_removed``;
    ``n_windows``).  ValueError where ``pya_strip_spectra_host`` returns ``PYA_ERR_ARG``."""
    p = check_strip_params(params)
    raw_mz, raw_it, rel = _transform_entry("strip", mz, intensity, peak_off)
    n_spec = rel.size - 1
    pm, pz = _strip_precursors(prec_mz, prec_z)
    if pm.shape != (n_spec,):
        raise ValueError("strip: prec_mz and prec_z have one entry per spectrum")
    x = raw_mz.astype(np.float64)
    lo, hi, active = strip_windows(pm, pz, p)
    in_window = np.zeros(x.size, bool)
    report = np.zeros(n_spec, STRIP_REPORT_DTYPE)
    report["n_windows"] = active.sum(axis=1)
    for s in np.flatnonzero(active.any(axis=1) & (np.diff(rel) > 0)):
        a, b = int(rel[s]), int(rel[s + 1])
        ws = np.flatnonzero(active[s])
        xs = x[a:b, None]
        inside = (lo[s, ws][None, :] <= xs) & (xs <= hi[s, ws][None, :])          # [peaks, active windows]
        in_window[a:b] = inside.any(axis=1)
        report["hit"][s] = sum(1 << int(w) for w in ws[inside.any(axis=0)])
    keep = ~((x < p["mz_lo"]) | (x > p["mz_hi"]) | in_window)
    _, kept, new_off = _transform_exit(keep, rel)
    report["n_removed"] = np.diff(rel) - kept
    return raw_mz[keep].copy(), raw_it[keep].copy(), new_off, report


def marker_params(mz=(), losses=(), tol=0.0, tol_ppm=0.0):
    """The parameters of the marker-ion stage (``pya_marker_params``) as a dict: ``value`` the tuple of the fixed targets ``mz``
    (reporter ions, immonium ions: their m/z) FIRST and the ``losses`` (neutral masses taken off the precursor: 97.976896 for
    H3PO4, 79.966331 for HPO3) behind them, ``loss_mask`` with bit t set for every loss target, ``tol`` the half width of a window
    in m/z units and ``tol_ppm`` in ppm of its centre, added to it.  At most 64 targets together and at least one.  ValueError
    where the library would refuse: a ``tol`` or ``tol_ppm`` that is not finite or negative, a fixed m/z that is not finite and
    positive, a loss that is not finite or negative, no target or more than 64."""
    try:
        mz, losses = tuple(float(v) for v in mz), tuple(float(v) for v in losses)
    except TypeError:
        raise ValueError("markers: mz and losses are sequences of numbers") from None
    n = len(mz) + len(losses)
    return check_marker_params(dict(tol=tol, tol_ppm=tol_ppm, value=mz + losses, loss_mask=((1 << n) - 1) ^ ((1 << len(mz)) - 1)))


def check_marker_params(params):
    """``params`` (a dict as ``marker_params`` makes it) checked against the conditions of ``pya_marker_params``; returns it
    with plain Python numbers."""
    try:
        out = dict(tol=float(params["tol"]), tol_ppm=float(params["tol_ppm"]), value=tuple(float(v) for v in params["value"]),
                   loss_mask=params["loss_mask"])
    except (KeyError, TypeError, ValueError):
        raise ValueError("markers: params is the dict of pyascore_amd.rollup.marker_params (tol, tol_ppm, value, loss_mask)") from None
    for name in ("tol", "tol_ppm"):
        if not (np.isfinite(out[name]) and out[name] >= 0.0):
            raise ValueError("markers: %s = %r is not a finite number >= 0" % (name, out[name]))
    n = len(out["value"])
    if not 1 <= n <= MARKER_MAX_TARGETS:
        raise ValueError("markers: %d targets are not 1 .. %d" % (n, MARKER_MAX_TARGETS))
    mask = out["loss_mask"]
    try:
        ok = int(mask) == mask and 0 <= int(mask) < (1 << n)
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError("markers: loss_mask = %r is not an integer with a bit per loss target and none at or above %d" % (mask, n))
    out["loss_mask"] = mask = int(mask)
    for t, v in enumerate(out["value"]):
        if (mask >> t) & 1:
            if not (np.isfinite(v) and v >= 0.0):
                raise ValueError("markers: the loss %r of target %d is not a finite number >= 0" % (v, t))
        elif not (np.isfinite(v) and v > 0.0):
            raise ValueError("markers: the m/z %r of target %d is not finite and positive" % (v, t))
    return out


def marker_c_params(params):
    """``params`` as the ``pya_marker_params`` structure the library reads."""
    p = check_marker_params(params)
    value = list(p["value"]) + [0.0] * (MARKER_MAX_TARGETS - len(p["value"]))
    return _lib.MarkerParams(p["tol"], p["tol_ppm"], (_lib.C.c_double * MARKER_MAX_TARGETS)(*value), p["loss_mask"], len(p["value"]), 0)


def marker_windows(prec_mz, prec_z, params):
    """The windows of ``pya_marker_params`` for precursors ``prec_mz`` (float64) / ``prec_z`` (int32), one per spectrum (or one
    pair of numbers): ``(centre, lo, hi, active)``, three float64 arrays and a bool array of shape ``[n_spectra, n_targets]``
    (``[n_targets]`` for one pair) -- the header's operations in float64, one rounding each.  A fixed target is active
    everywhere; a loss target where the precursor is usable (a charge in 1 .. 8, an m/z that is finite and positive) and its
    centre finite and positive.  ``centre`` / ``lo`` / ``hi`` are NaN where ``active`` is False."""
    p = check_marker_params(params)
    one = np.ndim(prec_mz) == 0
    pm, pz = _strip_precursors(prec_mz, prec_z, "marker_windows")
    pm, pz = pm.reshape(-1), pz.reshape(-1)
    value = np.asarray(p["value"], np.float64)
    is_loss = ((p["loss_mask"] >> np.arange(value.size, dtype=object)) & 1).astype(bool)
    has = (pz >= 1) & (pz <= STRIP_MAX_CHARGE) & np.isfinite(pm) & (pm > 0.0)
    zd = np.where(has, pz, 1).astype(np.float64)
    with np.errstate(all="ignore"):
        rel = ((pm * zd)[:, None] - value[None, :]) / zd[:, None]
        cen = np.where(is_loss[None, :], rel, value[None, :])
        active = np.where(is_loss[None, :], has[:, None] & np.isfinite(rel) & (rel > 0.0), True)
        w = np.float64(p["tol"]) + np.float64(p["tol_ppm"] * 1e-6) * cen
        lo, hi = cen - w, cen + w
    cen, lo, hi = np.where(active, cen, np.nan), np.where(active, lo, np.nan), np.where(active, hi, np.nan)
    return (cen[0], lo[0], hi[0], active[0]) if one else (cen, lo, hi, active)


def markers(mz, intensity, peak_off, params, prec_mz=None, prec_z=None):
    """The marker ions of spectra: the rule of ``pya_marker_params``, operation for operation in float64 and plain Python
    floats, so the bytes are those of ``pya_marker_spectra``.  ``mz`` / ``intensity``: float64 or float32 (widened),
    ``peak_off[n_spectra + 1]``, ``params`` of ``marker_params``, ``prec_mz`` / ``prec_z`` one precursor m/z and charge per
    spectrum -- needed iff ``params`` has loss targets.  Per (spectrum, target) the record of the peak the target picks: among
    the peaks with ``lo <= x <= hi`` whose intensity is a number the most intense, then the one nearest the centre, then the one
    at the smaller m/z -- an order-free definition --, with the count of ALL peaks inside; per spectrum the ion current (NaN
    intensities left out; summed in the order of ``pya_coverage``'s sums), the base peak, the peak count, the active targets
    and the ``hit`` word.  Returns ``(markers, spectra)``: ``MARKER_DTYPE[n_spectra, n_targets]`` and
    ``MARKER_SPECTRUM_DTYPE[n_spectra]``.  The spectra are only read.  ValueError where ``pya_marker_spectra_host`` returns
    ``PYA_ERR_ARG``."""
    p = check_marker_params(params)
    raw_mz, raw_it, rel = _transform_entry("markers", mz, intensity, peak_off)
    n_spec, n_t = rel.size - 1, len(p["value"])
    if prec_mz is None or prec_z is None:
        if p["loss_mask"]:
            raise ValueError("markers: loss targets need prec_mz and prec_z, one entry per spectrum")
        pm, pz = np.full(n_spec, np.nan), np.zeros(n_spec, np.int32)
    else:
        pm, pz = _strip_precursors(prec_mz, prec_z, "markers")
        if pm.shape != (n_spec,):
            raise ValueError("markers: prec_mz and prec_z have one entry per spectrum")
    cen, lo, hi, active = marker_windows(pm, pz, p)
    x, y = raw_mz.astype(np.float64), raw_it.astype(np.float64)
    rec = np.zeros((n_spec, n_t), MARKER_DTYPE)
    spec = np.zeros(n_spec, MARKER_SPECTRUM_DTYPE)
    rec["flags"] = np.where(active, MARKER_ACTIVE, 0)
    spec["n_peaks"] = np.diff(rel)
    spec["n_active"] = active.sum(axis=1)
    for s in np.flatnonzero(np.diff(rel) > 0):
        xs, ys = x[rel[s]:rel[s + 1]], y[rel[s]:rel[s + 1]]
        num = ys == ys
        spec["tic"][s] = _lane_sum(np.where(num, ys, 0.0).tolist())
        if num.any():
            spec["base_peak"][s] = ys[num].max() + 0.0
        ts = np.flatnonzero(active[s])
        inside = (lo[s, ts][None, :] <= xs[:, None]) & (xs[:, None] <= hi[s, ts][None, :])        # [peaks, active targets]
        hit = 0
        for k in np.flatnonzero(inside.any(axis=0)):
            t = int(ts[k])
            rec["n_peaks"][s, t] = inside[:, k].sum()
            at = np.flatnonzero(inside[:, k] & num)
            if not at.size:
                continue
            top = ys[at].max()
            at = at[ys[at] == top]
            d = np.abs(xs[at] - cen[s, t])
            at = at[d == d.min()]
            rec["mz"][s, t] = xs[at].min() + 0.0
            rec["intensity"][s, t] = top + 0.0
            rec["flags"][s, t] |= MARKER_PICKED
            hit |= 1 << t
        spec["hit"][s] = np.uint64(hit)
    return rec, spec


def marker_matrix(records, field="intensity"):
    """``MARKER_DTYPE`` records ``[n_spectra, n_targets]`` as a float64 array of the same shape: ``field`` (``"intensity"``,
    ``"mz"`` or ``"n_peaks"``) of every target that picked a peak, NaN where none was picked -- what a quantification step
    takes (the rows of the PSMs behind a roll-up slot are summed or averaged by the caller, in an order of the caller's)."""
    if field not in ("intensity", "mz", "n_peaks"):
        raise ValueError("marker_matrix: field is 'intensity', 'mz' or 'n_peaks'")
    records = np.asarray(records, MARKER_DTYPE)
    picked = (records["flags"] & MARKER_PICKED) != 0
    return np.where(picked, records[field].astype(np.float64), np.nan)


def purity_params(tol=0.0, tol_ppm=10.0, isotopes=3, below=0, step=STRIP_STEP):
    """The parameters of the precursor-purity stage (``pya_purity_params``) as a dict: ``tol`` the half width of a centre's window
    in m/z units and ``tol_ppm`` in ppm of the centre, added to it; ``isotopes`` the isotope positions above the selected m/z
    that still count as the precursor, ``below`` those under it (0 .. 4: an instrument that picked the second isotope);
    ``step`` the isotope spacing at charge 1.  The defaults are choices, not measurements.  ValueError where the library would
    refuse."""
    return check_purity_params(dict(tol=tol, tol_ppm=tol_ppm, step=step, below=below, isotopes=isotopes))


def check_purity_params(params):
    """``params`` (a dict as ``purity_params`` makes it) checked against the conditions of ``pya_purity_params``; returns it
    with plain Python numbers."""
    try:
        out = dict(tol=float(params["tol"]), tol_ppm=float(params["tol_ppm"]), step=float(params["step"]), below=params["below"],
                   isotopes=params["isotopes"])
    except (KeyError, TypeError, ValueError):
        raise ValueError("purity: params is the dict of pyascore_amd.rollup.purity_params (tol, tol_ppm, step, below, isotopes)") from None
    for name in ("tol", "tol_ppm"):
        if not (np.isfinite(out[name]) and out[name] >= 0.0):
            raise ValueError("purity: %s = %r is not a finite number >= 0" % (name, out[name]))
    if not (np.isfinite(out["step"]) and out["step"] > 0.0):
        raise ValueError("purity: step = %r is not finite and positive" % (out["step"],))
    for name in ("below", "isotopes"):
        v = out[name]
        try:
            ok = not isinstance(v, (bool, np.bool_)) and int(v) == v and int(v) >= 0
        except (TypeError, ValueError, OverflowError):
            ok = False
        if not ok:
            raise ValueError("purity: %s = %r is not an integer >= 0" % (name, v))
        out[name] = int(v)
    if out["below"] > PURITY_MAX_BELOW:
        raise ValueError("purity: below = %d is not in 0 .. %d" % (out["below"], PURITY_MAX_BELOW))
    if out["below"] + 1 + out["isotopes"] > PURITY_MAX_CENTRES:
        raise ValueError("purity: below + 1 + isotopes = %d centres are more than %d" % (out["below"] + 1 + out["isotopes"], PURITY_MAX_CENTRES))
    return out


def purity_c_params(params):
    """``params`` as the ``pya_purity_params`` structure the library reads."""
    p = check_purity_params(params)
    return _lib.PurityParams(p["tol"], p["tol_ppm"], p["step"], p["below"], p["isotopes"], (_lib.C.c_uint32 * 2)(0, 0))


def purity_queries(survey, prec_mz, prec_z, win_lo, win_hi, what="purity"):
    """The five per-query arrays of the purity stage as the library takes them: ``(survey int64, prec_mz float64, prec_z int32,
    win_lo float64, win_hi float64)``, contiguous and of one length.  ValueError otherwise."""
    sv, pz = np.asarray(survey), np.asarray(prec_z)
    try:
        pm, wl, wh = (np.ascontiguousarray(a, np.float64) for a in (prec_mz, win_lo, win_hi))
    except (TypeError, ValueError):
        raise ValueError("%s: prec_mz, win_lo and win_hi are numbers, one per query" % what) from None
    if (sv.size and sv.dtype.kind not in "iu") or (pz.size and pz.dtype.kind not in "iu"):
        raise ValueError("%s: survey and prec_z are integers, one per query" % what)
    if sv.ndim != 1 or any(a.shape != sv.shape for a in (pm, pz, wl, wh)):
        raise ValueError("%s: survey, prec_mz, prec_z, win_lo and win_hi have one entry per query" % what)
    if sv.size and (int(sv.max()) > 2 ** 63 - 1):
        raise ValueError("%s: survey does not fit an int64" % what)
    return (np.ascontiguousarray(sv, np.int64), pm, np.ascontiguousarray(np.clip(pz, -1, 0x7FFFFFFF), np.int32), wl, wh)


def purity(ms1_mz, ms1_intensity, ms1_peak_off, survey, prec_mz, prec_z, win_lo, win_hi, params):
    """The precursor purity of isolation windows: the rule of ``pya_purity_params``, operation for operation in float64 and
    plain Python floats, so the bytes are those of ``pya_purity_spectra``.  ``ms1_mz`` / ``ms1_intensity``: the survey (MS1)
    spectra, float64 or float32 (widened), ``ms1_peak_off[n_survey + 1]``; per query (one per MS2 spectrum) ``survey`` the index
    of its survey spectrum (negative: none), ``prec_mz`` / ``prec_z`` the selected m/z and charge, ``win_lo`` / ``win_hi`` the
    absolute m/z bounds of the isolation window; ``params`` of ``purity_params``.  Returns ``(records, over)``:
    ``PURITY_DTYPE[n_query]`` -- ``window`` the summed intensity of the peaks with ``win_lo <= x <= win_hi`` and ``y > 0``,
    ``precursor`` that of those inside a centre window (the selected m/z and its isotope positions), both summed in the order of
    the survey spectrum, the most intense other peak, the counts, ``iso_hit`` and the flags -- and ``over = (count, first)`` for
    the queries whose ``survey`` is ``>= n_survey`` (their records are zero), ``(0, None)`` when there is none.  The spectra are
    only read.  ValueError where ``pya_purity_spectra_host`` returns ``PYA_ERR_ARG``."""
    p = check_purity_params(params)
    raw_mz, raw_it, rel = _transform_entry("purity", ms1_mz, ms1_intensity, ms1_peak_off)
    n_survey = rel.size - 1
    sv, pm, pz, wl, wh = purity_queries(survey, prec_mz, prec_z, win_lo, win_hi)
    rec = np.zeros(sv.size, PURITY_DTYPE)
    tol, ppm, step, below = p["tol"], p["tol_ppm"] * 1e-6, p["step"], p["below"]
    usable = (pz >= 1) & (pz <= STRIP_MAX_CHARGE) & np.isfinite(pm) & (pm > 0.0)
    with np.errstate(invalid="ignore"):
        active = (sv >= 0) & usable & (wl <= wh) & np.isfinite(wl) & np.isfinite(wh)
    beyond = active & (sv >= n_survey)
    for q in np.flatnonzero(active & ~beyond):
        a, b = int(rel[sv[q]]), int(rel[sv[q] + 1])
        xs = raw_mz[a:b].astype(np.float64)
        with np.errstate(invalid="ignore"):
            at = np.flatnonzero((wl[q] <= xs) & (xs <= wh[q]))
        ys = raw_it[a:b][at].astype(np.float64)
        d = step / float(int(pz[q]))
        bounds = []
        for i in range(-below, p["isotopes"] + 1):
            c = float(pm[q]) + float(i) * d
            w = tol + ppm * c
            bounds.append((c - w, c + w))
        window = precursor = ox = oy = 0.0
        n_window = n_precursor = iso_hit = 0
        have_other = False
        for x, y in zip(xs[at].tolist(), ys.tolist()):                 # (index order: the order of the two sums)
            if not y > 0.0:
                continue
            hit = sum(1 << k for k, (lo, hi) in enumerate(bounds) if lo <= x <= hi)
            window = window + y
            n_window += 1
            if hit:
                precursor = precursor + y
                n_precursor += 1
                iso_hit |= hit
            elif not have_other or y > oy or (y == oy and x < ox):
                ox, oy, have_other = x, y, True
        rec[q] = (window, precursor, ox + 0.0 if have_other else 0.0, oy + 0.0 if have_other else 0.0, n_window, n_precursor, iso_hit,
                  PURITY_ACTIVE | (PURITY_SEEN if n_precursor else 0))
    first = np.flatnonzero(beyond)
    return rec, (int(first.size), int(first[0]) if first.size else None)


def purity_ratio(records):
    """``precursor / window`` of ``PURITY_DTYPE`` records as float64, NaN where ``window`` is not > 0 (an inactive query, an
    empty window): the number the record itself does not store."""
    rec = np.asarray(records, PURITY_DTYPE)
    out = np.full(rec.shape, np.nan)
    known = rec["window"] > 0.0
    with np.errstate(invalid="ignore"):
        out[known] = rec["precursor"][known] / rec["window"][known]
    return out


def check_purity_gate(threshold, keep_unknown=True, what="purity_gate"):
    """``(threshold, keep_unknown)`` of THE GATE checked: a number in [0, 1] and a boolean."""
    try:
        t = float(threshold)
    except (TypeError, ValueError):
        raise ValueError("%s: threshold is a number in 0 .. 1" % what) from None
    if isinstance(threshold, (bool, np.bool_)) or not 0.0 <= t <= 1.0:
        raise ValueError("%s: threshold = %r is not a number in 0 .. 1" % (what, threshold))
    if not isinstance(keep_unknown, (bool, np.bool_)):
        raise ValueError("%s: keep_unknown = %r is not a boolean" % (what, keep_unknown))
    return t, bool(keep_unknown)


def purity_gate(records, threshold, keep_unknown=True, values=None):
    """THE GATE of ``pya_purity_params`` over ``PURITY_DTYPE`` records, the bytes of ``pya_purity_gate``: a row whose record is
    active with ``window > 0`` passes iff ``precursor >= threshold * window`` (one multiplication, no division); any other row
    passes iff ``keep_unknown``.  Returns ``(select, values)``: uint8 ``[n_rows]`` and, when ``values`` (float64 ``[n_rows,
    n_channels]``) is given, a new matrix with the readings of the passing rows copied bit for bit and those of the failing rows
    NaN (``marker_matrix``'s "no reading"), else None."""
    t, keep = check_purity_gate(threshold, keep_unknown)
    rec = np.asarray(records, PURITY_DTYPE)
    if rec.ndim != 1:
        raise ValueError("purity_gate: records is one PURITY_DTYPE record per row")
    known = ((rec["flags"] & PURITY_ACTIVE) != 0) & (rec["window"] > 0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        ok = rec["precursor"] >= np.float64(t) * rec["window"]
    select = np.where(known, ok, keep).astype(np.uint8)
    if values is None:
        return select, None
    v = np.ascontiguousarray(values, np.float64)
    if v.ndim != 2 or v.shape[0] != rec.size:
        raise ValueError("purity_gate: values is a float64 matrix with one row per record")
    out = v.copy()
    out.view(np.uint64)[select == 0, :] = np.uint64(0x7FF8000000000000)
    return select, out


def survey_index(survey_scans, scans, parent_scans=None):
    """The survey spectrum of every MS2 scan as an index into ``survey_scans`` (the scan numbers of the MS1 spectra in file
    order, ascending): the one ``parent_scans`` names where the file names one that is among ``survey_scans`` (None or a
    negative number: it names none), else the last survey scan in front of the MS2 scan, -1 when there is none.  int64
    ``[len(scans)]``: the ``survey`` of ``purity``."""
    sv = np.asarray(survey_scans, np.int64).reshape(-1)
    sc = np.asarray(scans, np.int64).reshape(-1)
    if sv.size > 1 and (np.diff(sv) <= 0).any():
        raise ValueError("survey_index: survey_scans ascend")
    out = np.searchsorted(sv, sc, side="left").astype(np.int64) - 1           # the last survey scan BEFORE the scan
    if parent_scans is not None:
        if len(parent_scans) != sc.size:
            raise ValueError("survey_index: parent_scans has one entry per scan")
        par = np.asarray([-1 if p is None else int(p) for p in parent_scans], np.int64)
        at = np.searchsorted(sv, par, side="left")
        named = (par >= 0) & (at < sv.size)
        named[named] = sv[at[named]] == par[named]
        out[named] = at[named]
    return out


def xic_params(tol=0.0, tol_ppm=10.0, isotopes=2, step=STRIP_STEP, rise=2.0, max_gap=1):
    """The parameters of the precursor-XIC stage (``pya_xic_params``) as a dict: ``tol`` the half width of an isotope's window in
    m/z units and ``tol_ppm`` in ppm of its centre, added to it; ``isotopes`` the isotope positions above the selected m/z whose
    intensity is added to the trace (0 .. 3); ``step`` the isotope spacing at charge 1; ``rise``: a scan is a valley when
    ``rise`` times its intensity lies below the maxima on both sides (>= 1); ``max_gap`` the absent scans a trace may bridge
    (0 .. 8).  The defaults are choices, not measurements.  ValueError where the library would refuse."""
    return check_xic_params(dict(tol=tol, tol_ppm=tol_ppm, step=step, rise=rise, isotopes=isotopes, max_gap=max_gap))


def check_xic_params(params):
    """``params`` (a dict as ``xic_params`` makes it) checked against the conditions of ``pya_xic_params``; returns it with
    plain Python numbers."""
    try:
        out = dict(tol=float(params["tol"]), tol_ppm=float(params["tol_ppm"]), step=float(params["step"]), rise=float(params["rise"]),
                   isotopes=params["isotopes"], max_gap=params["max_gap"])
    except (KeyError, TypeError, ValueError):
        raise ValueError("xic: params is the dict of pyascore_amd.rollup.xic_params (tol, tol_ppm, step, rise, isotopes, max_gap)") from None
    for name in ("tol", "tol_ppm"):
        if not (np.isfinite(out[name]) and out[name] >= 0.0):
            raise ValueError("xic: %s = %r is not a finite number >= 0" % (name, out[name]))
    if not (np.isfinite(out["step"]) and out["step"] > 0.0):
        raise ValueError("xic: step = %r is not finite and positive" % (out["step"],))
    if not (np.isfinite(out["rise"]) and out["rise"] >= 1.0):
        raise ValueError("xic: rise = %r is not a finite number >= 1" % (out["rise"],))
    for name, most in (("isotopes", XIC_MAX_ISOTOPES), ("max_gap", XIC_MAX_GAP)):
        v = out[name]
        try:
            ok = not isinstance(v, (bool, np.bool_)) and int(v) == v and int(v) >= 0
        except (TypeError, ValueError, OverflowError):
            ok = False
        if not ok:
            raise ValueError("xic: %s = %r is not an integer >= 0" % (name, v))
        out[name] = int(v)
        if out[name] > most:
            raise ValueError("xic: %s = %d is not in 0 .. %d" % (name, out[name], most))
    return out


def xic_c_params(params):
    """``params`` as the ``pya_xic_params`` structure the library reads."""
    p = check_xic_params(params)
    return _lib.XicParams(p["tol"], p["tol_ppm"], p["step"], p["rise"], p["isotopes"], p["max_gap"])


def xic_queries(seed, scan_lo, scan_hi, prec_mz, prec_z, what="xic"):
    """The five per-query arrays of the XIC stage as the library takes them: ``(seed int64, scan_lo int64, scan_hi int64, prec_mz
    float64, prec_z int32)``, contiguous and of one length.  ValueError otherwise."""
    ints = [np.asarray(a) for a in (seed, scan_lo, scan_hi, prec_z)]
    try:
        pm = np.ascontiguousarray(prec_mz, np.float64)
    except (TypeError, ValueError):
        raise ValueError("%s: prec_mz is a number per query" % what) from None
    if any(a.size and a.dtype.kind not in "iu" for a in ints):
        raise ValueError("%s: seed, scan_lo, scan_hi and prec_z are integers, one per query" % what)
    if ints[0].ndim != 1 or any(a.shape != ints[0].shape for a in ints[1:] + [pm]):
        raise ValueError("%s: seed, scan_lo, scan_hi, prec_mz and prec_z have one entry per query" % what)
    if any(a.size and int(a.max()) > 2 ** 63 - 1 for a in ints[:3]):
        raise ValueError("%s: seed, scan_lo and scan_hi do not fit an int64" % what)
    sd, lo, hi = (np.ascontiguousarray(a, np.int64) for a in ints[:3])
    return sd, lo, hi, pm, np.ascontiguousarray(np.clip(ints[3], -1, 0x7FFFFFFF), np.int32)


def survey_ascending(mz, peak_off):
    """``scan_ok`` of the XIC stage, the bytes of ``pya_xic_survey_check``: uint8 ``[n_survey]``, 1 iff ``x[j] <= x[j + 1]`` for
    every adjacent pair of the scan's m/z -- a NaN among two or more peaks fails, scans of 0 or 1 peaks pass."""
    mz = np.asarray(mz)
    raw_mz, _, rel = _transform_entry("survey_ascending", mz, mz, peak_off)
    ok = np.ones(rel.size - 1, np.uint8)
    with np.errstate(invalid="ignore"):
        for s in range(rel.size - 1):
            xs = raw_mz[int(rel[s]):int(rel[s + 1])]
            ok[s] = 1 if bool(np.all(xs[:-1] <= xs[1:])) else 0
    return ok


def xic(ms1_mz, ms1_intensity, ms1_peak_off, rt, seed, scan_lo, scan_hi, prec_mz, prec_z, params, scan_ok=None):
    """The precursor XIC: the rule of ``pya_xic_params``, operation for operation in float64 and plain Python floats, so the
    bytes are those of ``pya_xic_spectra``.  ``ms1_mz`` / ``ms1_intensity``: the survey (MS1) spectra, float64 or float32
    (widened), ``ms1_peak_off[n_survey + 1]``, ``rt[n_survey]`` their retention times in seconds; per query (one per MS2
    spectrum) ``seed`` the survey scan of the identification (negative: none), ``scan_lo`` / ``scan_hi`` the window
    ``[scan_lo, scan_hi)`` of at most 64 survey scans around it (``xic_windows`` makes them), ``prec_mz`` / ``prec_z``;
    ``params`` of ``xic_params``; ``scan_ok``: the bytes of ``survey_ascending``, computed when None.  Returns ``(records,
    over)``: ``XIC_DTYPE[n_query]`` and ``over = (count, first)`` for the queries with ``seed >= 0`` whose window is out of
    range (their records are zero), ``(0, None)`` when there is none.  The spectra are only read.  ValueError where
    ``pya_xic_spectra_host`` returns ``PYA_ERR_ARG``."""
    p = check_xic_params(params)
    raw_mz, raw_it, rel = _transform_entry("xic", ms1_mz, ms1_intensity, ms1_peak_off)
    n_survey = rel.size - 1
    try:
        rt = np.ascontiguousarray(rt, np.float64)
    except (TypeError, ValueError):
        raise ValueError("xic: rt is a number per survey spectrum") from None
    if rt.shape != (n_survey,):
        raise ValueError("xic: rt has one entry per survey spectrum")
    ok = survey_ascending(raw_mz, rel) if scan_ok is None else np.asarray(scan_ok)
    if ok.shape != (n_survey,):
        raise ValueError("xic: scan_ok has one byte per survey spectrum")
    sd, s_lo, s_hi, pm, pz = xic_queries(seed, scan_lo, scan_hi, prec_mz, prec_z)
    rec = np.zeros(sd.size, XIC_DTYPE)
    tol, ppm, step, rise = p["tol"], p["tol_ppm"] * 1e-6, p["step"], p["rise"]
    n_iso, reach = p["isotopes"], p["max_gap"] + 1
    wide = {}                                                               # survey scan -> its (x, y) widened

    def scan(s):
        if s not in wide:
            a, b = int(rel[s]), int(rel[s + 1])
            wide[s] = (raw_mz[a:b].astype(np.float64), raw_it[a:b].astype(np.float64))
        return wide[s]

    outside = []
    for q in range(sd.size):
        s0, lo, hi = int(sd[q]), int(s_lo[q]), int(s_hi[q])
        if s0 < 0:
            continue
        if not (0 <= lo <= s0 < hi <= n_survey and hi - lo <= XIC_MAX_SCANS):
            outside.append(q)
            continue
        z, m = int(pz[q]), float(pm[q])
        if not (1 <= z <= STRIP_MAX_CHARGE and np.isfinite(m) and m > 0.0):
            continue
        W, sj = hi - lo, s0 - lo
        # THE TRACE
        d = step / float(z)
        bounds = []
        for i in range(n_iso + 1):
            c = m + float(i) * d
            w = tol + ppm * c
            bounds.append((c - w, c + w))
        pk = [[0.0] * W for _ in bounds]
        flags = XIC_ACTIVE
        for j in range(W):
            if not ok[lo + j]:
                flags |= XIC_UNSORTED
                continue
            xs, ys = scan(lo + j)
            for i, (b_lo, b_hi) in enumerate(bounds):
                with np.errstate(invalid="ignore"):
                    at = (b_lo <= xs) & (xs <= b_hi) & (ys > 0.0)
                if at.any():
                    pk[i][j] = float(ys[at].max())
        present = [pk[0][j] > 0.0 for j in range(W)]
        t = [0.0] * W
        for j in range(W):
            if present[j]:
                v = pk[0][j]
                for i in range(1, n_iso + 1):
                    v = v + pk[i][j]
                t[j] = v
        n_present = sum(present)
        # START
        a0 = sj if present[sj] else -1
        for dd in range(1, reach + 1):
            if a0 >= 0:
                break
            if sj - dd >= 0 and present[sj - dd]:
                a0 = sj - dd
            elif sj + dd < W and present[sj + dd]:
                a0 = sj + dd
        if a0 < 0:
            rec[q] = (0.0, 0.0, 0.0, 0.0, 0, 0, 0, 0, 0, n_present, 0, flags)
            continue
        # REGION
        r_lo = r_hi = a0
        gap = 0
        for j in range(a0 + 1, W):
            gap = 0 if present[j] else gap + 1
            if gap > p["max_gap"]:
                break
            if present[j]:
                r_hi = j
        gap = 0
        for j in range(a0 - 1, -1, -1):
            gap = 0 if present[j] else gap + 1
            if gap > p["max_gap"]:
                break
            if present[j]:
                r_lo = j
        pts = [j for j in range(r_lo, r_hi + 1) if present[j]]
        # VALLEYS: the first one on either side of a0
        bound, valley = [r_lo, r_hi], [False, False]
        for side, away in ((1, [j for j in pts if j > a0]), (0, [j for j in reversed(pts) if j < a0])):
            for k, v in enumerate(away[:-1]):
                nearer, farther = [a0] + away[:k + 1], away[k + 1:]
                low = rise * t[v]
                if t[v] <= t[away[k + 1]] and low < max(t[u] for u in nearer) and low < max(t[u] for u in farther):
                    bound[side], valley[side] = v, True
                    break
        e_l, e_r = bound
        # THE PEAK
        peak = [j for j in pts if e_l <= j <= e_r]
        apex = peak[0]
        for j in peak:
            if t[j] > t[apex]:
                apex = j
        total = area = 0.0
        for k, j in enumerate(peak):
            total = total + t[j]
            if k:
                u = peak[k - 1]
                with np.errstate(all="ignore"):
                    area = area + (0.5 * (t[u] + t[j])) * (np.float64(rt[lo + j]) - np.float64(rt[lo + u]))
        flags |= XIC_SEEN | (XIC_SEED_PRESENT if a0 == sj else 0) | (XIC_LEFT_VALLEY if valley[0] else 0) | (XIC_RIGHT_VALLEY if valley[1] else 0)
        flags |= (XIC_LEFT_OPEN if not valley[0] and e_l == 0 else 0) | (XIC_RIGHT_OPEN if not valley[1] and e_r == W - 1 else 0)
        iso_hit = sum(1 << i for i in range(n_iso + 1) if pk[i][apex] > 0.0)
        rec[q] = (float(area), t[apex], t[sj], total, lo + apex, lo + e_l, lo + e_r, lo + a0, len(peak), n_present, iso_hit, flags)
    return rec, (len(outside), outside[0] if outside else None)


def xic_values(records, which="area"):
    """One column of ``XIC_DTYPE`` records as the one-channel matrix ``site_quant`` and ``peptidoform_quant`` take, the bytes of
    ``pya_xic_values``: float64 ``[n]``, ``which`` 0 .. 3 or 'area', 'apex', 'seed', 'sum'; NaN (``marker_matrix``'s "no
    reading") where the record is not SEEN or the value is not > 0."""
    names = {"area": 0, "apex": 1, "seed": 2, "sum": 3}
    if isinstance(which, str):
        if which not in names:
            raise ValueError("xic_values: which is 0 .. 3 or one of 'area', 'apex', 'seed', 'sum'")
        which = names[which]
    if isinstance(which, (bool, np.bool_)) or not isinstance(which, (int, np.integer)) or not 0 <= int(which) <= 3:
        raise ValueError("xic_values: which is 0 .. 3 or one of 'area', 'apex', 'seed', 'sum'")
    rec = np.asarray(records, XIC_DTYPE)
    v = rec[XIC_COLUMNS[int(which)]]
    with np.errstate(invalid="ignore"):
        take = ((rec["flags"] & XIC_SEEN) != 0) & (v > 0.0)
    out = np.full(rec.shape, np.nan)
    out[take] = v[take]
    return out


def xic_windows(survey_rt, seed, half_width_s, run_bounds=None):
    """The windows of ``xic`` from retention times: for every ``seed`` (an index into ``survey_rt``, seconds in file order) the
    survey scans around it whose time lies within ``half_width_s`` of the seed's, as ``(scan_lo, scan_hi)`` int64 arrays --
    contiguous from the seed outwards, never across a run (file) boundary (``run_bounds``: the ascending survey indices
    ``[n_runs + 1]`` at which the runs begin and the last one ends; None: one run), and cut to the 64 scans nearest the seed:
    ``scan_lo >= seed - 31``, ``scan_hi <= seed + 33``.  A negative seed (no survey scan) gets ``(0, 0)``."""
    rt = np.ascontiguousarray(survey_rt, np.float64).reshape(-1)
    sd = np.asarray(seed)
    if sd.size and sd.dtype.kind not in "iu":
        raise ValueError("xic_windows: seed is an integer per query")
    sd = np.ascontiguousarray(sd, np.int64).reshape(-1)
    hw = float(half_width_s)
    if not hw >= 0.0:
        raise ValueError("xic_windows: half_width_s = %r is not a number >= 0" % (half_width_s,))
    bounds = np.asarray([0, rt.size] if run_bounds is None else run_bounds, np.int64).reshape(-1)
    if bounds.size < 2 or bounds[0] != 0 or bounds[-1] != rt.size or (np.diff(bounds) < 0).any():
        raise ValueError("xic_windows: run_bounds ascend from 0 to the number of survey spectra")
    if sd.size and int(sd.max()) >= rt.size:
        raise ValueError("xic_windows: a seed lies beyond the survey spectra")
    lo, hi = np.zeros(sd.size, np.int64), np.zeros(sd.size, np.int64)
    for q in range(sd.size):
        s = int(sd[q])
        if s < 0:
            continue
        run = int(np.searchsorted(bounds, s, side="right")) - 1
        first, last = max(int(bounds[run]), s - 31), min(int(bounds[run + 1]), s + 33)
        a, b = s, s + 1
        while a > first and abs(rt[a - 1] - rt[s]) <= hw:
            a -= 1
        while b < last and abs(rt[b] - rt[s]) <= hw:
            b += 1
        lo[q], hi[q] = a, b
    return lo, hi


def centroid_params(gap, gap_ppm=0.0, half_width=4, min_height=0.0, area=False):
    """The parameters of centroiding (``pya_centroid_params``) as a dict: two adjacent points belong to one peak iff they are
    at most ``gap0 + gap_per_mz * mz`` apart -- ``gap0 = gap`` in m/z units (2 to 3 times the sampling step) and ``gap_per_mz =
    gap_ppm * 1e-6``, computed here, once, so the device and ``centroid`` read the same bits --, ``half_width`` the points on
    either side of an apex its centroid may take in (1 .. 8), ``min_height`` the least intensity of an apex, ``area``: the
    output intensity is the sum over the footprint instead of the apex's own.  ValueError where the library would refuse."""
    if isinstance(area, (bool, np.bool_)):
        area = int(area)
    try:
        gap_per_mz = float(gap_ppm) * 1e-6
    except (TypeError, ValueError):
        raise ValueError("centroid: gap_ppm = %r is not a number" % (gap_ppm,)) from None
    return check_centroid_params(dict(gap0=gap, gap_per_mz=gap_per_mz, min_height=min_height, half_width=half_width, area=area))


def check_centroid_params(params):
    """``params`` (a dict as ``centroid_params`` makes it) checked against the conditions of ``pya_centroid_params``; returns
    it with plain Python numbers."""
    try:
        out = dict(gap0=float(params["gap0"]), gap_per_mz=float(params["gap_per_mz"]), min_height=float(params["min_height"]),
                   half_width=params["half_width"], area=params["area"])
    except (KeyError, TypeError, ValueError):
        raise ValueError("centroid: params is the dict of pyascore_amd.rollup.centroid_params "
                         "(gap0, gap_per_mz, min_height, half_width, area)") from None
    for name in ("gap0", "gap_per_mz", "min_height"):
        if not (np.isfinite(out[name]) and out[name] >= 0.0):
            raise ValueError("centroid: %s = %r is not a finite number >= 0" % (name, out[name]))
    if out["gap0"] == 0.0 and out["gap_per_mz"] == 0.0:
        raise ValueError("centroid: gap0 and gap_per_mz are both 0")
    for name, low, top in (("half_width", 1, CENTROID_MAX_HALF_WIDTH), ("area", 0, 1)):
        v = out[name]
        try:
            ok = int(v) == v and low <= int(v) <= top
        except (TypeError, ValueError, OverflowError):
            ok = False
        if not ok:
            raise ValueError("centroid: %s = %r is not an integer in %d .. %d" % (name, v, low, top))
        out[name] = int(v)
    return out


def centroid_c_params(params):
    """``params`` as the ``pya_centroid_params`` structure the library reads."""
    p = check_centroid_params(params)
    return _lib.CentroidParams(p["gap0"], p["gap_per_mz"], p["min_height"], p["half_width"], p["area"], 0)


def centroid_select(select, n_spec, what="centroid"):
    """``select`` as the uint8 array ``pya_centroid_spectra`` reads (one byte per spectrum, 0: copied unchanged), or None."""
    if select is None:
        return None
    sel = np.asarray(select)
    if sel.dtype.kind not in "biu" or sel.shape != (n_spec,):
        raise ValueError("%s: select has one boolean or integer per spectrum" % what)
    return np.ascontiguousarray(sel != 0, np.uint8)


def centroid(mz, intensity, peak_off, params, select=None):
    """Centroided spectra: the rule of ``pya_centroid_params``, operation for operation in float64, so the bytes are those of
    ``pya_centroid_spectra``.  ``mz`` / ``intensity``: float64 or float32 (widened for the arithmetic; the dtype stays),
    ``peak_off[n_spectra + 1]``, ``params`` of ``centroid_params``, ``select`` one boolean per spectrum (False: copied
    unchanged) or None for all.  Every local maximum of a run of connected points (the first point of a plateau) becomes one
    peak at the intensity-weighted mean m/z of its monotone flanks, at most ``half_width`` points on either side, summed from
    the left in the rule's order; an isolated point is copied bit for bit, so centroided spectra pass through.  A spectrum that
    is not ascending (a descending pair or a NaN m/z) comes back unchanged.  Returns ``(mz, intensity, peak_off, unordered)``:
    new arrays, their offsets (from 0) and a boolean per spectrum that is True where the spectrum was selected and not
    ascending (what ``d_over`` counts)."""
    p = check_centroid_params(params)
    raw_mz, raw_it, rel = _transform_entry("centroid", mz, intensity, peak_off)
    n_spec, n = rel.size - 1, raw_mz.size
    sel = centroid_select(select, n_spec)
    chosen = np.ones(n_spec, bool) if sel is None else sel != 0
    x, y = raw_mz.astype(np.float64), raw_it.astype(np.float64)
    spec = np.repeat(np.arange(n_spec), np.diff(rel))
    hw = p["half_width"]
    with np.errstate(all="ignore"):
        # step[k]: the step k - 1 -> k lies inside one spectrum; conn[k]: ... and is CONNECTED
        step = np.zeros(n + 1, bool)
        step[1:n] = spec[1:] == spec[:-1]
        conn = np.zeros(n + 1, bool)
        conn[1:n] = step[1:n] & ((x[1:] - x[:-1]) <= (p["gap0"] + p["gap_per_mz"] * x[:-1]))
        unordered = np.zeros(n_spec, bool)
        if n > 1:
            unordered[spec[1:][step[1:n] & ~(x[:-1] <= x[1:])]] = True
        unordered &= chosen
        active = (chosen & ~unordered)[spec]
        y_left, y_right = np.concatenate([[0.0], y[:-1]]), np.concatenate([y[1:], [0.0]])
        apex = (y > 0.0) & (y >= p["min_height"]) & (~conn[:n] | (y_left < y)) & (~conn[1:] | (y_right <= y))
        keep = apex | ~active
        idx = np.flatnonzero(apex & active)
        # FOOTPRINT
        l, go = idx.copy(), np.ones(idx.size, bool)
        for _ in range(hw):
            go = go & conn[l] & (y[np.maximum(l - 1, 0)] < y[l])
            l = np.where(go, l - 1, l)
        r, go = idx.copy(), np.ones(idx.size, bool)
        for _ in range(hw):
            go = go & conn[r + 1] & (y[np.minimum(r + 1, n - 1)] <= y[r])
            r = np.where(go, r + 1, r)
        # CENTROID: the at most 2 half_width + 1 terms in order, masked
        sw, s = np.zeros(idx.size), np.zeros(idx.size)
        for t in range(2 * hw + 1):
            k = l + t
            m = k <= r
            k = np.where(m, k, idx)
            sw = np.where(m, sw + y[k], sw)
            d = x[k] - x[idx]
            s = np.where(m, s + d * y[k], s)
        q = s / sw
        c = x[idx] + q
        c = np.where(c >= x[l], c, x[l])
        c = np.where(c <= x[r], c, x[r])
    out_mz, out_it = raw_mz[keep].copy(), raw_it[keep].copy()
    before, _, new_off = _transform_exit(keep, rel)
    pos = before[idx]
    wide = l != r
    out_mz[pos[wide]] = c[wide].astype(raw_mz.dtype)
    if p["area"]:
        with np.errstate(over="ignore"):
            out_it[pos] = sw.astype(raw_it.dtype)
    return out_mz, out_it, new_off, unordered


def site_quant_params(threshold=0.75, scale_log2=10, n_channels=None, complete_only=False):
    """The parameters of the site quantification (``pya_site_quant_params``) as a dict: ``threshold`` the localisation
    probability a record needs to contribute, ``scale_log2`` the power of two a reading is multiplied by before it is
    truncated to an integer -- the default 10 is a choice, not a measurement: about 1e-3 intensity units of resolution and
    2^38 per reading before it saturates --, ``n_channels`` the columns of the matrix (1 .. 64), ``complete_only`` whether only
    records with a usable value in every channel are summed.  ValueError where the library would refuse."""
    if n_channels is None:
        raise ValueError("site_quant: n_channels is missing (the columns of the channel matrix, 1 .. %d)" % QUANT_MAX_CHANNELS)
    return check_site_quant_params(dict(threshold=threshold, scale_log2=scale_log2, n_channels=n_channels, complete_only=complete_only))


def check_site_quant_params(params):
    """``params`` (a dict as ``site_quant_params`` makes it) checked against the conditions of ``pya_site_quant_params``;
    returns it with plain Python numbers."""
    try:
        out = dict(threshold=float(params["threshold"]), scale_log2=params["scale_log2"], n_channels=params["n_channels"],
                   complete_only=params["complete_only"])
    except (KeyError, TypeError, ValueError):
        raise ValueError("site_quant: params is the dict of pyascore_amd.rollup.site_quant_params (threshold, scale_log2, n_channels, "
                         "complete_only)") from None
    if out["threshold"] != out["threshold"]:
        raise ValueError("site_quant: threshold is not a number")
    for name, lo, hi in (("scale_log2", -64, 64), ("n_channels", 1, QUANT_MAX_CHANNELS)):
        v = out[name]
        try:
            ok = not isinstance(v, bool) and int(v) == v and lo <= int(v) <= hi
        except (TypeError, ValueError, OverflowError):
            ok = False
        if not ok:
            raise ValueError("site_quant: %s = %r is not an integer in %d .. %d" % (name, v, lo, hi))
        out[name] = int(v)
    if not isinstance(out["complete_only"], (bool, np.bool_)):
        raise ValueError("site_quant: complete_only = %r is not a boolean" % (out["complete_only"],))
    out["complete_only"] = bool(out["complete_only"])
    return out


def site_quant_c_params(params):
    """``params`` as the ``pya_site_quant_params`` structure the library reads."""
    p = check_site_quant_params(params)
    return _lib.SiteQuantParams(p["threshold"], p["scale_log2"], p["n_channels"], _lib.PYA_QUANT_COMPLETE_ONLY if p["complete_only"] else 0, 0)


def empty_site_quant(n_slots, n_channels):
    """``(head, cell)`` of an empty table: ``SITE_QUANT_HEAD_DTYPE[n_slots]`` and ``SITE_QUANT_DTYPE[n_slots, n_channels]``,
    all zero."""
    return np.zeros(int(n_slots), SITE_QUANT_HEAD_DTYPE), np.zeros((int(n_slots), int(n_channels)), SITE_QUANT_DTYPE)


def _site_quant_table(table, what):
    head = np.ascontiguousarray(table[0], SITE_QUANT_HEAD_DTYPE)
    cell = np.ascontiguousarray(table[1], SITE_QUANT_DTYPE)
    if head.ndim != 1 or cell.ndim != 2 or cell.shape[0] != head.size:
        raise ValueError("%s: a table is (head[n_slots], cell[n_slots, n_channels])" % what)
    return head, cell


def site_quant(site_probs, psm_probs, site_off, best_sig, slot, n_slots, values, row, params, into=None):
    """The table ``score_batch(quant=...)`` returns, from the probability records of the same batch (``score_batch(probs=True)``:
    ``site_probs``, ``psm_probs``, ``site_off``) and its ``best_sig``: the definition of ``pya_site_quant`` restated in numpy,
    with the same bytes.  ``slot``: one per residue record as for ``rollup=``; ``values``: float64 ``[n_rows, n_channels]``;
    ``row``: the row of every PSM (negative: left out) or None (PSM i has row i); ``params``: ``site_quant_params(...)``;
    ``into``: a ``(head, cell)`` to accumulate into (it is copied), None: the empty table.  A record that would contribute but
    names a slot at or above ``n_slots`` or a row at or above ``n_rows`` is a ValueError (the library answers PYA_ERR_LIMIT).
    Returns ``(head, cell)``: ``SITE_QUANT_HEAD_DTYPE[n_slots]``, ``SITE_QUANT_DTYPE[n_slots, n_channels]``."""
    p = check_site_quant_params(params)
    n_ch, n_slots = p["n_channels"], int(n_slots)
    site_off = np.asarray(site_off, np.int64)
    n = site_off.size - 1
    site_probs = np.asarray(site_probs, np.dtype(_lib.SITE_PROB_DTYPE))
    psm_probs = np.asarray(psm_probs, np.dtype(_lib.PSM_PROB_DTYPE))
    best_sig = np.asarray(best_sig).astype(np.uint64)
    slot = np.asarray(slot).astype(np.int64)
    values = np.ascontiguousarray(values, np.float64)
    if values.ndim != 2 or values.shape[1] != n_ch:
        raise ValueError("site_quant: values is a float64 matrix with %d columns" % n_ch)
    n_rec = int(site_off[-1]) if n >= 0 else 0
    if n < 0 or site_probs.shape != (n_rec,) or psm_probs.shape != (n,) or best_sig.shape != (n,) or slot.shape != (n_rec,):
        raise ValueError("site_quant: site_off has n_psm + 1 entries, psm_probs and best_sig one per PSM, site_probs and slot one per residue record")
    row = np.arange(n, dtype=np.int64) if row is None else np.asarray(row).astype(np.int64)
    if row.shape != (n,):
        raise ValueError("site_quant: row has one entry per PSM")
    head, cell = empty_site_quant(n_slots, n_ch) if into is None else tuple(a.copy() for a in _site_quant_table(into, "site_quant"))
    if head.shape != (n_slots,) or cell.shape != (n_slots, n_ch):
        raise ValueError("site_quant: into is a table of other slots or channels")
    owner = np.repeat(np.arange(n), np.diff(site_off))
    r = np.arange(n_rec, dtype=np.int64) - site_off[owner]
    in_best = (r < 64) & (((best_sig[owner] >> np.minimum(r, 63).astype(np.uint64)) & np.uint64(1)) != 0)
    rw = row[owner]
    with np.errstate(invalid="ignore"):
        cand = (slot >= 0) & (psm_probs["kind"][owner] == _lib.PYA_SITE_SCORED) & in_best & (site_probs["with_prob"] >= p["threshold"]) & (rw >= 0)
    outside = cand & ((slot >= n_slots) | (rw >= values.shape[0]))
    if outside.any():
        first = int(np.flatnonzero(outside)[0])
        raise ValueError("site_quant: residue record %d (PSM %d) names slot %d of %d, row %d of %d"
                         % (first, int(owner[first]), int(slot[first]), n_slots, int(rw[first]), values.shape[0]))
    s, v = slot[cand], values[rw[cand]]
    usable = (v == v) & (v > 0.0)
    complete = usable.all(axis=1)
    with np.errstate(over="ignore", invalid="ignore"):
        t = v * 2.0 ** p["scale_log2"]
    saturated = usable & (t >= 281474976710656.0)
    q = np.where(usable & ~saturated, t, 0.0).astype(np.uint64)
    q[saturated] = np.uint64(1 << 48)
    summed = usable & complete[:, None] if p["complete_only"] else usable
    np.add.at(head["n_records"], s, 1)
    np.add.at(head["n_complete"], s[complete], 1)
    at = np.nonzero(summed)
    np.add.at(cell["sum"], (s[at[0]], at[1]), q[at])
    np.add.at(cell["n"], (s[at[0]], at[1]), 1)
    at = np.nonzero(summed & saturated)
    np.add.at(cell["n_saturated"], (s[at[0]], at[1]), 1)
    return head, cell


def merge_site_quant(*tables):
    """The sum of ``(head, cell)`` tables over the same slots and channels, field by field (counts and sums wrap as on the
    device): the table of the records behind all of them."""
    if not tables:
        raise ValueError("merge_site_quant: no table")
    parts = [_site_quant_table(t, "merge_site_quant") for t in tables]
    if any(h.shape != parts[0][0].shape or c.shape != parts[0][1].shape for h, c in parts):
        raise ValueError("merge_site_quant: the tables have different slots or channels")
    head, cell = parts[0][0].copy(), parts[0][1].copy()
    for h, c in parts[1:]:
        for f in ("n_records", "n_complete"):
            head[f] += h[f]
        for f in ("sum", "n", "n_saturated"):
            cell[f] += c[f]
    return head, cell


def site_quant_sums(head, cell, params):
    """The channel sums of a table in intensity units: float64 ``[n_slots, n_channels]``, ``sum / 2^scale_log2``, NaN where no
    reading was summed (``n == 0``).  The head / cell arrays of a peptidoform quantification (``peptidoform_quant``,
    ``score_batch(peptidoform_quant=...)``) are tables of the same records: they go through unchanged, one row per peptidoform."""
    p = check_site_quant_params(params)
    head, cell = _site_quant_table((head, cell), "site_quant_sums")
    return np.where(cell["n"] != 0, cell["sum"].astype(np.float64) * 2.0 ** -p["scale_log2"], np.nan)


def _pfq_place(records):
    """(group, sig_bits) -> row of a peptidoform list"""
    return {(int(g), int(b)): j for j, (g, b) in enumerate(zip(records["group"].tolist(), records["sig_bits"].tolist()))}


def _pfq_pair(pair, what):
    """a pair as (list, head, cell); head and cell None: an all-zero table"""
    if len(pair) != 3:
        raise ValueError("%s: a pair is (list, head, cell)" % what)
    records = np.ascontiguousarray(pair[0], PEPTIDOFORM_DTYPE).reshape(-1)
    if (pair[1] is None) != (pair[2] is None):
        raise ValueError("%s: head and cell of a pair are both given or both None" % what)
    if pair[1] is None:
        return records, None, None
    head, cell = _site_quant_table((pair[1], pair[2]), what)
    if head.size != records.size:
        raise ValueError("%s: the table of a pair is not row-aligned with its list" % what)
    return records, head, cell


def _pfq_add_rows(place, head, cell, pair):
    """the rows of ``pair`` (records with n_psm != 0) added to the rows of their keys; a key without a place (behind cap) is left out"""
    records, h, c = pair
    if h is None:
        return
    keep = np.flatnonzero(records["n_psm"] != 0)
    at = np.array([place.get((int(records["group"][j]), int(records["sig_bits"][j])), -1) for j in keep], np.int64)
    keep, at = keep[at >= 0], at[at >= 0]
    for f in ("n_records", "n_complete"):
        np.add.at(head[f], at, h[f][keep])
    for f in ("sum", "n", "n_saturated"):
        np.add.at(cell[f], at, c[f][keep])


def _pfq_min_prob(site_probs, psm_probs, site_off, sig, group):
    """(in_list, min_prob, k) per PSM: whether the PSM contributes to the peptidoform list, the smallest with_prob over the
    residues of its best_sig as bit patterns (1.0 for best_sig == 0; of no meaning where not in_list) and their number"""
    n = site_off.size - 1
    in_list = (psm_probs["kind"] == _lib.PYA_SITE_SCORED) & (group >= 0)
    sig = np.where(in_list, sig, np.uint64(0))
    n_res = np.diff(site_off)
    pbits = np.ascontiguousarray(site_probs["with_prob"]).view(np.uint64)
    prob = np.where(sig != 0, np.uint64(0xFFFFFFFFFFFFFFFF), np.float64(1.0).view(np.uint64))
    k = np.zeros(n, np.int64)
    for r in range(64):
        has = ((sig >> np.uint64(r)) & np.uint64(1)) != 0
        if not has.any():
            continue
        if (n_res[has] <= r).any():
            raise ValueError("peptidoform_quant: PSM %d has a best_sig that does not fit its residue records" % int(np.flatnonzero(has & (n_res <= r))[0]))
        prob[has] = np.minimum(prob[has], pbits[site_off[:-1][has] + r])
        k += has
    return in_list, prob.view(np.float64), k


def peptidoform_min_prob(site_probs, psm_probs, site_off, best_sig, group):
    """``min_prob`` of every PSM as the peptidoform stages compute it (float64 ``[n_psm]``; NaN for a PSM that does not
    contribute to the list): what ``peptidoform_quant``'s threshold is compared with -- its median makes about half of the
    listed PSMs contribute."""
    site_off = np.asarray(site_off, np.int64)
    in_list, min_prob, _ = _pfq_min_prob(np.asarray(site_probs, np.dtype(_lib.SITE_PROB_DTYPE)), np.asarray(psm_probs, np.dtype(_lib.PSM_PROB_DTYPE)),
                                         site_off, np.asarray(best_sig).astype(np.uint64), np.asarray(group).astype(np.int64))
    return np.where(in_list, min_prob, np.nan)


def peptidoform_quant(site_probs, psm_probs, site_off, best_sig, ascores, group, values, row, params, threshold=0.75, psm_id=None,
                      psm_base=0, prev=None, cap=None):
    """The pair ``score_batch(peptidoforms=dict(group=, threshold=, psm_id=), peptidoform_quant=...)`` returns, from the
    probability records of the same batch (``score_batch(probs=True)``: ``site_probs``, ``psm_probs``, ``site_off``), its
    ``best_sig`` and ``ascores``: the peptidoform quantification of ``include/pyascore_hip.h`` restated in numpy, with the same
    bytes.  The list goes through ``merge_peptidoforms`` (every contributing PSM a record with ``n_psm == 1``), the table is
    row-aligned with it.  ``values`` / ``row`` / ``params`` as for ``site_quant``; ``threshold`` is the list's ("confident"),
    ``params["threshold"]`` the table's; ``prev``: an earlier pair ``(list, head, cell)`` (head and cell None: an all-zero table) --
    the result is then the pair over the PSMs behind both; ``cap``: only the first ``cap`` rows are kept, a key behind them adds
    nothing.  A PSM that would contribute but names a row at or above ``n_rows`` is a ValueError (the library answers
    PYA_ERR_LIMIT), as is a ``best_sig`` that does not fit the residue records.  Returns ``(list, head, cell)``:
    ``PEPTIDOFORM_DTYPE[n]``, ``SITE_QUANT_HEAD_DTYPE[n]``, ``SITE_QUANT_DTYPE[n, n_channels]``."""
    p = check_site_quant_params(params)
    n_ch = p["n_channels"]
    site_off = np.asarray(site_off, np.int64)
    n = site_off.size - 1
    site_probs = np.asarray(site_probs, np.dtype(_lib.SITE_PROB_DTYPE))
    psm_probs = np.asarray(psm_probs, np.dtype(_lib.PSM_PROB_DTYPE))
    sig = np.asarray(best_sig).astype(np.uint64)
    group = np.asarray(group).astype(np.int64)
    ascores = np.ascontiguousarray(ascores, np.float32)
    values = np.ascontiguousarray(values, np.float64)
    if values.ndim != 2 or values.shape[1] != n_ch:
        raise ValueError("peptidoform_quant: values is a float64 matrix with %d columns" % n_ch)
    n_rec = int(site_off[-1]) if n >= 0 else 0
    if n < 0 or site_probs.shape != (n_rec,) or psm_probs.shape != (n,) or sig.shape != (n,) or group.shape != (n,) or ascores.ndim != 2 \
            or ascores.shape[0] != n:
        raise ValueError("peptidoform_quant: site_off has n_psm + 1 entries, psm_probs, best_sig, group and the rows of ascores one per "
                         "PSM, site_probs one per residue record")
    row = np.arange(n, dtype=np.int64) if row is None else np.asarray(row).astype(np.int64)
    if row.shape != (n,):
        raise ValueError("peptidoform_quant: row has one entry per PSM")
    ident = (np.arange(n, dtype=np.int64) + int(psm_base)) if psm_id is None else np.asarray(psm_id).astype(np.int64)
    in_list, min_prob, k = _pfq_min_prob(site_probs, psm_probs, site_off, sig, group)
    sig = np.where(in_list, sig, np.uint64(0))
    max_k = ascores.shape[1]
    if (k > max_k).any():
        raise ValueError("peptidoform_quant: PSM %d has more modified residues than ascores has columns" % int(np.flatnonzero(k > max_k)[0]))
    akey = np.where(np.arange(max_k)[None, :] < k[:, None], _ascore_key(ascores).reshape(n, max_k), 0xFFFFFFFF).min(axis=1, initial=0xFFFFFFFF)
    akey = np.where(k == 0, int(_ascore_key(np.float32([np.inf]))[0]), akey)
    psms = np.zeros(n, PEPTIDOFORM_DTYPE)
    psms["sig_bits"], psms["group"], psms["n_psm"] = sig, np.where(in_list, group, 0).astype(np.uint32), 1
    with np.errstate(invalid="ignore"):
        psms["n_confident"] = min_prob >= float(threshold)
        quantified = in_list & (min_prob >= p["threshold"]) & (row >= 0)
    psms["best_psm"] = ident.astype(np.uint32)
    psms["best_min_prob"], psms["best_z"] = min_prob, psm_probs["z"]
    psms["best_min_ascore"] = np.where(akey >> 31 != 0, akey - 0x80000000, 0xFFFFFFFF - akey).astype(np.uint32).view(np.float32)
    psms["n_psm"][~in_list] = 0
    before = None if prev is None else _pfq_pair(prev, "peptidoform_quant")
    if before is not None and before[2] is not None and before[2].shape[1] != n_ch:
        raise ValueError("peptidoform_quant: prev is a table of other channels")
    records = merge_peptidoforms(psms, None if before is None else before[0])
    if cap is not None:
        records = records[:int(cap)]
    outside = quantified & (row >= values.shape[0])
    if outside.any():
        first = int(np.flatnonzero(outside)[0])
        raise ValueError("peptidoform_quant: PSM %d names row %d of %d" % (first, int(row[first]), values.shape[0]))
    head, cell = empty_site_quant(records.size, n_ch)
    place = _pfq_place(records)
    who = np.flatnonzero(quantified)
    at = np.array([place.get((int(psms["group"][i]), int(sig[i])), -1) for i in who], np.int64)
    who, at = who[at >= 0], at[at >= 0]
    v = values[row[who]].reshape(who.size, n_ch)
    usable = (v == v) & (v > 0.0)
    complete = usable.all(axis=1)
    with np.errstate(over="ignore", invalid="ignore"):
        t = v * 2.0 ** p["scale_log2"]
    saturated = usable & (t >= 281474976710656.0)
    q = np.where(usable & ~saturated, t, 0.0).astype(np.uint64)
    q[saturated] = np.uint64(1 << 48)
    summed = usable & complete[:, None] if p["complete_only"] else usable
    np.add.at(head["n_records"], at, 1)
    np.add.at(head["n_complete"], at[complete], 1)
    hit = np.nonzero(summed)
    np.add.at(cell["sum"], (at[hit[0]], hit[1]), q[hit])
    np.add.at(cell["n"], (at[hit[0]], hit[1]), 1)
    hit = np.nonzero(summed & saturated)
    np.add.at(cell["n_saturated"], (at[hit[0]], hit[1]), 1)
    if before is not None:
        _pfq_add_rows(place, head, cell, before)
    return records, head, cell


def merge_peptidoform_quant(*pairs, cap=None):
    """The merge of peptidoform quantification pairs ``(list, head, cell)`` over the same channels: the keys' union through
    ``merge_peptidoforms``, the rows of equal keys added field by field (counts and sums wrap as on the device); records with
    ``n_psm == 0`` are skipped and their rows with them; a pair whose head and cell are None has an all-zero table.  The host
    form of ``PyAscore.peptidoform_quant_reduce`` / ``pya_peptidoform_quant_reduce``, with the same bytes."""
    if not pairs:
        raise ValueError("merge_peptidoform_quant: no pair")
    parts = [_pfq_pair(t, "merge_peptidoform_quant") for t in pairs]
    widths = {c.shape[1] for _, _, c in parts if c is not None}
    if len(widths) != 1:
        raise ValueError("merge_peptidoform_quant: the tables have different channel counts, or no pair has a table")
    records = merge_peptidoforms(np.concatenate([r for r, _, _ in parts]))
    if cap is not None:
        records = records[:int(cap)]
    head, cell = empty_site_quant(records.size, widths.pop())
    place = _pfq_place(records)
    for part in parts:
        _pfq_add_rows(place, head, cell, part)
    return records, head, cell


CHANNEL_TILE = _lib.PYA_CHANNEL_TILE                # rows per workgroup of csrc/channel_correct.hip


def channel_spill(n_channels, entries):
    """The spill matrix ``S`` of a reagent lot, float64 ``[n_channels, n_channels]`` with ``observed = S @ true``, from
    ``(from, to, fraction)`` triples: ``fraction`` of channel ``from``'s reporter shows up in channel ``to`` (``S[to, from]``);
    ``to = -1``: it leaves to no channel (an isotope peak outside the plex).  The diagonal is 1 minus what leaves.  The numbers
    are the caller's, from the lot's sheet: no presets are shipped.  ValueError for a channel outside the plex, ``from == to``, a
    fraction that is not finite or negative, a triple named twice, or a channel that loses everything."""
    try:
        n = int(n_channels)
        ok = n == n_channels and not isinstance(n_channels, bool) and 1 <= n <= QUANT_MAX_CHANNELS
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError("channel_spill: n_channels = %r is not an integer in 1 .. %d" % (n_channels, QUANT_MAX_CHANNELS))
    s = np.zeros((n, n), np.float64)
    leaves = [0.0] * n
    seen = set()
    for entry in entries:
        try:
            a, b, frac = entry
            a, b, frac = int(a), int(b), float(frac)
        except (TypeError, ValueError):
            raise ValueError("channel_spill: an entry is (from, to, fraction), not %r" % (entry,)) from None
        if not 0 <= a < n or not -1 <= b < n or a == b:
            raise ValueError("channel_spill: entry %r names a channel outside 0 .. %d (to may be -1), or from == to" % (entry, n - 1))
        if not np.isfinite(frac) or frac < 0.0:
            raise ValueError("channel_spill: the fraction of entry %r is not a finite number >= 0" % (entry,))
        if b >= 0 and (a, b) in seen:
            raise ValueError("channel_spill: (%d, %d) is named twice" % (a, b))
        seen.add((a, b))
        leaves[a] += frac
        if b >= 0:
            s[b, a] = frac
    for c in range(n):
        if not leaves[c] < 1.0:
            raise ValueError("channel_spill: channel %d loses %g of itself" % (c, leaves[c]))
        s[c, c] = 1.0 - leaves[c]
    return s


def channel_matrix(spill):
    """The correction matrix of ``correct_channels``: the inverse of the spill matrix ``S`` (``channel_spill``), by
    ``numpy.linalg.inv`` in float64.  ValueError for a matrix that is not square, not finite, larger than the channel limit, or
    whose condition number (2-norm) is above 1e6: such a lot sheet does not determine the true intensities."""
    try:
        s = np.array(spill, np.float64)
    except (TypeError, ValueError):
        raise ValueError("channel_matrix: spill is a square matrix of numbers") from None
    if s.ndim != 2 or s.shape[0] != s.shape[1] or not 1 <= s.shape[0] <= QUANT_MAX_CHANNELS:
        raise ValueError("channel_matrix: spill is a square matrix of 1 .. %d channels" % QUANT_MAX_CHANNELS)
    if not np.isfinite(s).all():
        raise ValueError("channel_matrix: spill has entries that are not finite")
    try:
        cond = float(np.linalg.cond(s))
        inv = np.linalg.inv(s)
    except np.linalg.LinAlgError:
        raise ValueError("channel_matrix: spill is singular") from None
    if not cond <= 1e6 or not np.isfinite(inv).all():
        raise ValueError("channel_matrix: the condition number of spill, %g, is above 1e6" % cond)
    return np.ascontiguousarray(inv)


def _channel_values(values, what):
    v = np.ascontiguousarray(values, np.float64)
    if v.ndim != 2 or not 1 <= v.shape[1] <= QUANT_MAX_CHANNELS:
        raise ValueError("%s: values is a float64 matrix, one row per spectrum and 1 .. %d channels" % (what, QUANT_MAX_CHANNELS))
    return v


def check_channel_matrix(matrix, n_channels, what="correct_channels"):
    """``matrix`` as the contiguous float64 ``[n_channels, n_channels]`` array the library reads; ValueError for another shape"""
    try:
        m = np.ascontiguousarray(matrix, np.float64)
    except (TypeError, ValueError):
        raise ValueError("%s: matrix is a square matrix of numbers" % what) from None
    if m.shape != (n_channels, n_channels):
        raise ValueError("%s: matrix has shape %r, not (%d, %d)" % (what, m.shape, n_channels, n_channels))
    return m


def correct_channels(values, matrix=None, factor=None):
    """APPLY of the channel correction (``pya_channel_correct`` in include/pyascore_hip.h) restated in numpy, with the same
    bytes: ``values`` float64 ``[n_rows, n_channels]``, ``matrix`` ``[n_channels, n_channels]`` (``channel_matrix``) or None,
    ``factor`` ``[n_channels]`` (``channel_factors``) or None, not both None.  Vectorised over the rows only: the chain over the
    channels runs in the rule's order, one multiplication and one addition per term.  Returns a new matrix."""
    v = _channel_values(values, "correct_channels")
    n_ch = v.shape[1]
    if matrix is None and factor is None:
        raise ValueError("correct_channels: neither a matrix nor a factor")
    usable = (v == v) & (v > 0.0)
    with np.errstate(all="ignore"):
        if matrix is not None:
            m = check_channel_matrix(matrix, n_ch)
            u = np.where(usable, v, 0.0)
            x = np.empty_like(v)
            for c in range(n_ch):
                acc = np.zeros(v.shape[0], np.float64)
                for j in range(n_ch):
                    t = m[c, j] * u[:, j]
                    acc = acc + t
                x[:, c] = acc
        else:
            x = v.copy()
        if factor is not None:
            f = np.ascontiguousarray(factor, np.float64)
            if f.shape != (n_ch,):
                raise ValueError("correct_channels: factor has one entry per channel")
            x = x * f[None, :]
        x = np.where((x == x) & (x > 0.0), x, 0.0)
    out = v.copy()
    out[usable] = x[usable]
    return out


def channel_sums(values, select=None, scale_log2=10, into=None):
    """SUMS of the channel correction (``pya_channel_sums``) restated in numpy: the table row ``SITE_QUANT_DTYPE[n_channels]``
    of the column sums of ``values`` over the rows ``select`` names (one byte or bool per row; None: all), added to ``into``
    (it is copied; None: the empty row)."""
    v = _channel_values(values, "channel_sums")
    p = check_site_quant_params(dict(threshold=0.0, scale_log2=scale_log2, n_channels=v.shape[1], complete_only=False))
    cell = np.zeros(v.shape[1], SITE_QUANT_DTYPE) if into is None else np.array(into, SITE_QUANT_DTYPE)
    if cell.shape != (v.shape[1],):
        raise ValueError("channel_sums: into is a row of one cell per channel")
    if select is not None:
        select = np.asarray(select)
        if select.shape != (v.shape[0],):
            raise ValueError("channel_sums: select has one entry per row")
        v = v[select != 0]
    usable = (v == v) & (v > 0.0)
    with np.errstate(over="ignore", invalid="ignore"):
        t = v * 2.0 ** p["scale_log2"]
    saturated = usable & (t >= 281474976710656.0)
    q = np.where(usable & ~saturated, t, 0.0).astype(np.uint64)
    q[saturated] = np.uint64(1 << 48)
    cell["sum"] += q.sum(axis=0, dtype=np.uint64)
    cell["n"] += usable.sum(axis=0).astype(np.uint32)
    cell["n_saturated"] += saturated.sum(axis=0).astype(np.uint32)
    return cell


def channel_factors(cell):
    """FACTORS of the channel correction (``pya_channel_factors``) restated in numpy: float64 ``[n_channels]``, the largest
    ``sum`` of the row over each ``sum`` (1.0 for an empty column), both converted to the nearest double and divided once."""
    cell = np.ascontiguousarray(cell, SITE_QUANT_DTYPE)
    if cell.ndim != 1 or not 1 <= cell.size <= QUANT_MAX_CHANNELS:
        raise ValueError("channel_factors: cell is a row of 1 .. %d cells" % QUANT_MAX_CHANNELS)
    s = cell["sum"]
    top = np.full(s.shape, s.max(), np.uint64).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(s == 0, 1.0, top / s.astype(np.float64))


def _is_number(text):
    try:
        float(text)
    except ValueError:
        return False
    return True


def read_channel_spill(path, n_channels):
    """The spill matrix (``channel_spill``) of a tab-separated file of ``from``, ``to``, ``fraction`` lines, the channels
    numbered from 0 in the order the caller's channels have; blank lines, lines that start with ``#`` and one header line whose
    first field is no number are skipped.  ValueError (with the line) for anything else."""
    entries, header = [], False
    with open(path) as f:
        for n, line in enumerate(f, 1):
            text = line.strip()
            if not text or text.startswith("#"):
                continue
            fields = text.split("\t")
            try:
                if len(fields) != 3:
                    raise ValueError
                entries.append((int(fields[0]), int(fields[1]), float(fields[2])))
            except ValueError:
                if not entries and not header and len(fields) == 3 and not _is_number(fields[0]):
                    header = True
                    continue
                raise ValueError("%s line %d: expected from<TAB>to<TAB>fraction, got %r" % (path, n, text)) from None
    try:
        return channel_spill(n_channels, entries)
    except ValueError as e:
        raise ValueError("%s: %s" % (path, e)) from None
