"""Batched counterpart of pyAscore's CLI scoring loop.

The reference's `pyascore/__main__.py:127-172` walks the identifications one PSM at a time:
split each PSM's modifications into the unlocalised (variable) ones and the fixed ones
(`process_mods`, :83-103), pick the fragment-charge limit from the PSM charge (:138-145), call
``PyAscore.score`` and read four properties, then write a TSV.  With scoring on the GPU that
Python loop is the end-to-end bottleneck, so here the same decisions are taken per PSM on the
host, all PSMs are packed into ONE batch, scored with one ``PyAscore.score_batch`` call, and the
rows are produced from the batch results.  Inputs are the already-parsed records the reference's
parsers produce (dicts); file parsing itself (pyteomics) stays out of scope.

Output rows/columns follow docs/source/cli.rst:135-180: Scan, LocalizedSequence, PepScore,
Ascores (';' separated), AltSites (',' within ';').
"""
from itertools import groupby

import numpy as np

from .ascore import PyAscore
from .named import sig_bits_of
from . import sites as site_tables
from . import probs as site_probs
from . import ranked as ranked_lists
from . import rollup as site_rollup
from .synth import pack_batch, pack_shared_batch

COLUMNS = ("Scan", "LocalizedSequence", "PepScore", "Ascores", "AltSites")
# ``--evidence``: what stands behind every Ascore (pya_evidence), one entry per modified site like Ascores
EVIDENCE_COLUMNS = ("Depth", "SiteIons", "CompScore")
# ``--reported``: the search engine's own site assignment, scored (pya_named)
REPORTED_COLUMNS = ("ReportedSequence", "ReportedPepScore", "ReportedAscore")
# ``--ions FILE``: one line per ion record (pya_ion), long format
# ``--sites FILE``: one line per (scan, candidate residue) (pya_site), and two more columns of the main table
SITE_COLUMNS = ("Scan", "Peptide", "Position", "Residue", "InBest", "WithScore", "WithoutScore", "Delta", "BestWith", "BestWithout")
RUNNER_UP_COLUMNS = ("RunnerUpSequence", "DeltaPepScore")
# ``--probs``: the localisation probabilities of a PSM (pya_site_prob, pya_psm_prob)
PROB_COLUMNS = ("SiteProbs", "BestProb")
# ``--ranked FILE``: one line per (scan, hit, rank) (pya_ranked)
RANKED_COLUMNS = ("Scan", "Hit", "Rank", "LocalizedSequence", "PepScore", "DeltaToBest", "Tied")
# ``--site_table FILE``: one line per (peptide, position) over all PSMs (pya_site_rollup)
SITE_TABLE_COLUMNS = ("Peptide", "Position", "Residue", "BestProb", "BestScan", "PSMs", "Confident", "InBest", "BestAscore")
# ``--site_table_flr``: three more columns of the ``--site_table`` table (pya_site_flr), its rows best site first
SITE_TABLE_FLR_COLUMNS = ("Rank", "FLR", "DecoyQ")
# ``--peptidoform_table FILE``: one line per (peptide, reported site assignment) over all PSMs (pya_peptidoform)
PEPTIDOFORM_TABLE_COLUMNS = ("Peptide", "Positions", "PSMs", "Confident", "BestScan", "BestMinProb", "BestPosterior", "BestMinAscore",
                             "Isomers")
# ``--mz_profile FILE``: one line per slot, band, unit and bin of the fragment mass-error profile (pya_mz_profile)
MZ_PROFILE_COLUMNS = ("Slot", "Band", "Unit", "Bin", "Low", "High", "Count")
# ``--mz_calibration_out FILE``: one line per slot and band of the m/z calibration fitted to the profile (pya_mz_calibration)
MZ_CALIBRATION_COLUMNS = ("Slot", "Band", "BandCentre", "Ppm", "SpreadPpm", "SignalIons", "BandWidth")
ION_COLUMNS = ("Scan", "Hit", "Section", "Site", "Side", "Ion", "TheoMz", "PeakMz", "Rank", "Counted")
# ``--coverage FILE``: one line per PSM, the coverage record (pya_coverage) and its four ratios
COVERAGE_COLUMNS = ("Scan", "Hit", "Scored", "TotalCurrent", "ExplainedCurrent", "NTermCurrent", "CTermCurrent", "Peaks", "RetainedPeaks",
                    "ExplainedPeaks", "Fragments", "NTermSizes", "CTermSizes", "NTermRun", "CTermRun", "Bonds", "ExplainedRatio",
                    "NTermRatio", "CTermRatio", "PeakRatio")


def process_mods(residues, mod_mass, sequence, positions, masses, mod_correction_tol=1.0,
                 zero_based=False):
    """Variable/fixed split of one PSM's modifications (`__main__.py:83-103`).

    A modification counts as one of the unlocalised ones when its mass matches ``mod_mass``
    (numpy.isclose, rtol 1e-6, atol ``mod_correction_tol``) AND it sits on a residue of
    ``residues`` ('n' for position 0).  Everything else is returned as a fixed modification at its
    1-based position (0 = n-terminus).  Returns (uint32 positions, float32 masses, n_variable)."""
    shift = 1 if zero_based else 0
    n_variable = 0
    const_pos, const_masses = [], []
    for pos, mass in zip(positions, masses):
        pos = int(pos)
        aa = "n" if pos + shift == 0 else sequence[pos - 1 + shift]
        if np.isclose(mod_mass, mass, rtol=1e-6, atol=mod_correction_tol) and aa in residues:
            n_variable += 1
        else:
            const_pos.append(pos + shift)
            const_masses.append(mass)
    return np.array(const_pos, dtype=np.uint32), np.array(const_masses, dtype=np.float32), n_variable


def reported_positions(residues, mod_mass, sequence, positions, masses, mod_correction_tol=1.0, zero_based=False):
    """Where the search engine put the modifications ``process_mods`` counts as variable: their 1-based peptide
    positions (0 = n-terminus), in input order -- the site assignment `__main__.py:83-103` reads and drops."""
    shift = 1 if zero_based else 0
    out = []
    for pos, mass in zip(positions, masses):
        pos = int(pos)
        aa = "n" if pos + shift == 0 else sequence[pos - 1 + shift]
        if np.isclose(mod_mass, mass, rtol=1e-6, atol=mod_correction_tol) and aa in residues:
            out.append(pos + shift)
    return out


def psm_charge(match, spectrum):
    """Charge used to bound the fragment charge (`__main__.py:138-145`): the identification's
    charge, else the spectrum's precursor charge, else 2; never below 2."""
    if match.get("charge_state") is not None and match["charge_state"] != 0:
        z = match["charge_state"]
    elif spectrum.get("precursor_charge") is not None and spectrum["precursor_charge"] != 0:
        z = spectrum["precursor_charge"]
    else:
        z = 2
    return max(int(z), 2)


def save_match(spectra, match):
    """``--match_save`` (`__main__.py:106-111`): the spectrum and the identification of a PSM as the two
    pickle files the reference writes, in the working directory."""
    import pickle
    with open("dump_spectra.pkl", "wb") as dst:
        pickle.dump([spectra], dst)
    with open("dump_match.pkl", "wb") as dst:
        pickle.dump([match], dst)


def select_psms(psms, spectra_map, residues, mod_mass, hit_depth=1, max_fragment_charge=5,
                mod_correction_tol=1.0, zero_based=False, match_save=False, reported=None):
    """The reference's loop header (`__main__.py:129-147`): group by scan (input sorted by scan),
    take the first ``hit_depth`` hits of a scan (negative = all), drop PSMs without an
    unlocalised modification.  Returns (list of PSM dicts for pack_batch, list of scans).
    ``match_save``: the reference dumps every PSM it is about to score over the previous one
    (`__main__.py:148-149`), so what it leaves behind is the last one: that is what is written here.
    ``reported``: a list that receives the ``reported_positions`` of every picked PSM."""
    picked, scans = [], []
    last = None
    for _, group in groupby(psms, lambda m: m["scan"]):
        for ind, match in enumerate(group):
            if ind == hit_depth:
                break
            spectrum = spectra_map[match["scan"]]
            const_pos, const_masses, n_variable = process_mods(
                residues, mod_mass, match["peptide"], match["mod_positions"], match["mod_masses"],
                mod_correction_tol, zero_based)
            if n_variable <= 0:
                continue
            picked.append(dict(mz=spectrum["mz_values"], intensity=spectrum["intensity_values"],
                               peptide=match["peptide"], n_of_mod=n_variable,
                               max_charge=min(max_fragment_charge, psm_charge(match, spectrum) - 1),
                               aux_pos=const_pos, aux_mass=const_masses, precursor_mz=spectrum.get("precursor_mz"),
                               precursor_charge=spectrum.get("precursor_charge"), profile=spectrum.get("profile")))
            scans.append(match["scan"])
            if reported is not None:
                reported.append(reported_positions(residues, mod_mass, match["peptide"], match["mod_positions"], match["mod_masses"],
                                                   mod_correction_tol, zero_based))
            last = (spectrum, match)
    if match_save and last is not None:
        save_match(*last)
    return picked, scans


def pack_hits(picked, scans):
    """``select_psms``' output as one batch in which the hits of a scan share the scan's spectrum: consecutive PSMs of
    one scan (the reference scores every one of them against ``spectra_map[scan]``, `__main__.py:129-164`) refer to ONE
    copy of its peaks.  With one hit per scan this is ``pack_batch(picked)``, array for array.  Spectra read with
    ``ingest.SpectraParser(native_precision=True)`` keep their float32 arrays through the pack (typed batch)."""
    spectra, spec_of = [], []
    for i, psm in enumerate(picked):
        if not (i and scans[i] == scans[i - 1] and psm["mz"] is picked[i - 1]["mz"] and psm["intensity"] is picked[i - 1]["intensity"]):
            spectra.append(dict(mz=psm["mz"], intensity=psm["intensity"]))
        spec_of.append(len(spectra) - 1)
    if len(spectra) == len(picked):
        return pack_batch(picked)
    return pack_shared_batch(spectra, [dict(p, spectrum=s) for p, s in zip(picked, spec_of)])


def hit_precursors(picked, scans):
    """The precursor m/z (float64) and charge (int32) of every spectrum of ``pack_hits(picked, scans)``, in its order: what
    ``select_psms`` took from the spectra's ``precursor_mz`` / ``precursor_charge``.  A value that is missing or no number
    becomes m/z 0 and charge 0: a spectrum without windows (``pya_strip_params``)."""
    def number(v, kind):
        try:
            return kind(v) if v is not None else kind(0)
        except (TypeError, ValueError, OverflowError):
            return kind(0)

    prec_mz, prec_z = [], []
    for i, psm in enumerate(picked):
        if i and scans[i] == scans[i - 1] and psm["mz"] is picked[i - 1]["mz"] and psm["intensity"] is picked[i - 1]["intensity"]:
            continue
        prec_mz.append(number(psm.get("precursor_mz"), float))
        prec_z.append(min(max(number(psm.get("precursor_charge"), int), -1), 0x7FFFFFFF))
    return np.asarray(prec_mz, np.float64), np.asarray(prec_z, np.int32)


def hit_profiles(picked, scans):
    """One boolean per spectrum of ``pack_hits(picked, scans)``, in its order: True unless the file declared the spectrum
    centroided (``profile`` False, as ``ingest.SpectraParser`` keeps it) -- the ``select`` of ``--centroid``: a spectrum that
    says nothing is centroided too, which leaves it as it is when it holds centroids already."""
    select = []
    for i, psm in enumerate(picked):
        if i and scans[i] == scans[i - 1] and psm["mz"] is picked[i - 1]["mz"] and psm["intensity"] is picked[i - 1]["intensity"]:
            continue
        select.append(psm.get("profile") is not False)
    return np.asarray(select, bool)


def localize(ascore, psms, spectra_map, residues, mod_mass, hit_depth=1, max_fragment_charge=5,
             mod_correction_tol=1.0, zero_based=False, match_save=False, log=None, evidence=False, ions=None, reported=False,
             sites=None, probs=False, ranked=None, ranked_depth=5, site_table=None, site_table_threshold=0.75,
             site_table_flr=False, site_table_decoys="", peptidoform_table=None, peptidoform_threshold=0.75, mz_profile=None,
             recalibrate=None, deisotope=None, decharge=None, strip=None, centroid=None, coverage=None, markers=None,
             marker_rows=None, site_quant=None, site_quant_rows=None, peptidoform_quant=None, peptidoform_quant_rows=None, channels=None,
             purity=None, purity_rows=None, xic=None, xic_rows=None):
    """Scores every selected PSM in one batched call and returns the TSV rows
    ``[scan, localized_sequence, pep_score, "a;b", "1,2;3"]`` in input order.  PSMs the library sets
    aside (invalid, or beyond one of its documented limits) keep their row -- empty localisation, PepScore
    nan -- and are reported through ``log`` (a callable taking one string) with their count, scans and codes.
    ``evidence=True`` appends three fields per row, ';'-joined per site (``evidence_fields``): Depth, SiteIons, CompScore.
    ``ions``: a list that receives the ion table of the scored PSMs, one ``ion_fields`` row per record behind the PSM's
    scan and its hit number inside the scan (``write_ions_tsv``).
    ``reported=True`` appends three fields per row (``reported_fields``): the search engine's own site assignment as a
    sequence, its PepScore, and the ambiguity of the winner against it -- did Ascore move the site, and by how much.
    ``sites``: a list that receives the site table of the scored PSMs, one ``site_fields`` row per candidate residue
    (``write_sites_tsv``); every row of the main table then ends with two more fields (``RUNNER_UP_COLUMNS``): the best
    localisation that differs from the winner, and how far its PepScore lies behind.
    ``probs=True`` appends two fields per row, last (``prob_fields``): the peptide with the localisation probability of every
    candidate residue, and the posterior of the reported localisation.
    ``ranked``: a list that receives the ranked localisations of the scored PSMs, the ``ranked_depth`` best site assignments
    of each in order, one ``[scan, hit] + ranked_fields`` row per assignment (``write_ranked_tsv``); the main table does not
    change.
    ``site_table``: a list that receives the site-level table over ALL scored PSMs, one ``site_table_fields`` row per
    (unmodified peptide, position) (``write_site_table_tsv``): the residue records of the batch are rolled up on the device,
    ``site_table_threshold`` being the "confident" cut; the main table does not change.  ``site_table_flr=True``: the rows
    come best site first and end with three more fields (``SITE_TABLE_FLR_COLUMNS``) -- the number of sites at least as good,
    the model-based false-localisation rate of that cut, and the decoy q-value --, computed on the device over the table;
    ``site_table_decoys``: the letters of the modification group that are decoy residues (sites on them count as decoys).
    ``peptidoform_table``: a list that receives one ``peptidoform_table_fields`` row per (unmodified peptide, reported site
    assignment) over ALL scored PSMs (``write_peptidoform_table_tsv``), reduced on the device; ``peptidoform_threshold`` is
    the "confident" cut on a PSM's smallest site probability; the main table does not change.
    ``mz_profile``: a list that receives the fragment mass-error profile of ALL scored PSMs as slot 0: the one-record table
    (``pyascore_amd.rollup.MZ_PROFILE_DTYPE``) and the parameters it was binned with (``mz_profile_rows``,
    ``write_mz_profile_tsv``, ``mz_profile_report``); the main table does not change.
    ``coverage``: a list that receives one ``[scan, hit] + coverage_fields`` row per picked PSM (``write_coverage_tsv``): the
    coverage record of the PSM on the spectra that were scored, and its four ratios; the main table does not change.
    ``recalibrate``: ``dict(calibration=, band_width=)`` as ``PyAscore.score_batch(recalibrate=...)`` takes it: the m/z of every
    spectrum is corrected with slot 0 of the calibration on the device before it is scored (``read_mz_calibration`` gives both
    from the file ``write_mz_calibration_tsv`` wrote); every table is then that of the corrected spectra.
    ``deisotope``: ``dict(tol=, max_charge=, ratio=)`` as ``PyAscore.score_batch(deisotope=...)`` takes it: isotope satellites are
    removed from every spectrum on the device before it is scored (and before ``recalibrate`` corrects it); every table is then
    that of the filtered spectra.
    ``decharge``: ``dict(tol=, max_charge=, ratio=, witness=)`` as ``PyAscore.score_batch(decharge=...)`` takes it: every spectrum is
    deisotoped and its multiply charged fragments are reduced to 1+ on the device before it is scored; not together with
    ``deisotope`` or ``recalibrate``.
    ``strip``: ``dict(tol=, losses=, reduced=, isotopes=, mz_lo=, mz_hi=)`` as ``PyAscore.score_batch(strip=...)`` takes it, without
    the precursors: they are the spectra's own ``precursor_mz`` / ``precursor_charge`` (``hit_precursors``; a spectrum that lacks
    one keeps its peaks but for the range cut).  The precursor-derived peaks are removed from every spectrum on the device
    before anything else is done to it; goes with each of ``deisotope``, ``decharge`` and ``recalibrate``.
    ``centroid``: ``dict(gap=, gap_ppm=, half_width=, min_height=, area=)`` as ``PyAscore.score_batch(centroid=...)`` takes it, without
    ``select``: that is ``hit_profiles`` -- every spectrum the file did not declare centroided (``profile`` of
    ``ingest.SpectraParser``) is centroided on the device, in front of ``strip`` and everything else.
    ``markers``: ``dict(mz=, losses=, tol=, tol_ppm=)`` as ``PyAscore.score_batch(markers=...)`` takes it, without the precursors:
    they are the spectra's own (``hit_precursors``), as for ``strip``.  ``marker_rows``: the list that then receives one
    ``[scan] + marker_fields`` row per picked PSM (``write_markers_tsv``): the ion current and the base peak of its spectrum and
    the peak every target picked in it, read-only and on the spectra ``strip`` is about to cut; the main table does not change.
    ``site_quant``: ``dict(threshold=, scale_log2=, complete_only=)`` as ``PyAscore.score_batch(quant=...)`` takes it, without a
    matrix: the channels are the fixed targets of ``markers``, the rows the spectra, the slots those of ``site_table`` -- it
    needs both.  ``site_quant_rows``: the list that then receives one ``site_quant_fields`` row per site with a contributing
    record (``write_site_quant_tsv``); no other table changes.
    ``peptidoform_quant``: ``dict(threshold=, scale_log2=, complete_only=)`` as ``PyAscore.score_batch(peptidoform_quant=...)``
    takes it, without a matrix: the channels are the fixed targets ``mz`` of ``markers``, which it needs (``losses`` are no
    channels).  ``peptidoform_quant_rows``: the list that then receives one ``peptidoform_quant_fields`` row per peptidoform
    (``write_peptidoform_quant_tsv``); the list is the one ``peptidoform_table`` gets, with ``peptidoform_threshold``.
    ``channels``: ``dict(matrix=, normalize=)`` as the ``channels=`` entry of ``PyAscore.score_batch(quant=...)`` takes it, without
    ``select``: the reporter matrix is corrected for the lot's isotope impurities (``matrix``, of as many channels as ``markers``
    has fixed targets) and / or brought to equal column totals before ``site_quant`` and ``peptidoform_quant`` sum it; it needs
    one of the two.
    ``purity``: ``dict(survey=, tol=, tol_ppm=, isotopes=, below=, window=None, threshold=None, keep_unknown=True)``: ``survey`` the
    MS1 records of the spectrum file (``ingest.SpectraParser(..., ms_level=1).to_list()``), the rule as
    ``pyascore_amd.rollup.purity_params`` takes it, ``window`` the ``(lower, upper)`` offsets around the precursor m/z used where
    a spectrum's record declares no ``isolation``; the survey scan of a spectrum is its ``parent_scan`` where the file names one,
    else the last survey scan in front of it (``pyascore_amd.rollup.survey_index``).  ``purity_rows``: the list that then
    receives one ``[scan] + purity_fields`` row per picked PSM (``write_purity_tsv``).  With ``threshold`` the gate of
    ``PyAscore.score_batch(purity=dict(gate=...))`` is applied to what ``site_quant`` / ``peptidoform_quant`` sum; it needs one of
    them.
    ``xic``: ``dict(survey=, rt_window=, tol=, tol_ppm=, isotopes=, step=, rise=, max_gap=, channel=None)``: ``survey`` the MS1 records
    of the spectrum file WITH their retention times (``ingest.SpectraParser(..., ms_level=1, times=True).to_list()``), the rule as
    ``pyascore_amd.rollup.xic_params`` takes it, ``rt_window`` the seconds on either side of the seed scan a window reaches
    (``pyascore_amd.rollup.xic_windows``: at most 64 scans); the seed scan of a spectrum is its survey scan as for ``purity``.
    ``xic_rows``: the list that then receives one ``[scan] + xic_fields`` row per picked PSM (``write_xic_tsv``).  ``channel``:
    'area' or 'apex' -- where ``markers`` has no fixed targets, ``site_quant`` / ``peptidoform_quant`` then sum that column as
    their one channel: label-free tables."""
    label_free = None
    if xic is not None:                                    # (a bad request is refused before anything is read or scored)
        xic_rule, xic_rt_window, xic_channel = xic_request(xic, xic_rows)
        if xic_channel is not None and not (isinstance(markers, dict) and tuple(markers.get("mz", ()))):
            label_free = "xic_" + xic_channel
            if channels is not None:
                raise ValueError("channels corrects reporter channels: it does not go with a label-free xic channel")
    if purity is not None:                                 # (a bad request is refused before anything is read or scored)
        purity_rule, purity_window, purity_gate = purity_request(purity, purity_rows, site_quant is not None or peptidoform_quant is not None)
    if channels is not None:                               # (a bad request is refused before anything is read or scored)
        from .ascore import _channels_request
        if site_quant is None and peptidoform_quant is None:
            raise ValueError("channels corrects the matrix site_quant and peptidoform_quant sum: it needs one of them")
        if not isinstance(channels, dict) or "select" in channels or not isinstance(markers, dict):
            raise ValueError("channels takes a dict of matrix and normalize beside markers")
        n_ch = len(tuple(markers.get("mz", ())))
        _channels_request("channels", dict(values=np.zeros((0, n_ch)), channels=channels))
    if peptidoform_quant is not None:                      # (a bad request is refused before anything is read or scored)
        if not isinstance(peptidoform_quant, dict) or set(peptidoform_quant) - {"threshold", "scale_log2", "complete_only"} \
                or peptidoform_quant_rows is None:
            raise ValueError("peptidoform_quant takes a dict of threshold, scale_log2 and complete_only beside a list peptidoform_quant_rows")
        if label_free is None and (not isinstance(markers, dict) or not tuple(markers.get("mz", ()))):
            raise ValueError("peptidoform_quant needs markers with fixed targets mz (its channels), or xic with a channel")
        site_rollup.site_quant_params(n_channels=1 if label_free else len(tuple(markers["mz"])), **peptidoform_quant)
    if site_quant is not None:                             # (a bad request is refused before anything is read or scored)
        if not isinstance(site_quant, dict) or set(site_quant) - {"threshold", "scale_log2", "complete_only"} or site_quant_rows is None:
            raise ValueError("site_quant takes a dict of threshold, scale_log2 and complete_only beside a list site_quant_rows")
        if site_table is None or (label_free is None and (not isinstance(markers, dict) or not tuple(markers.get("mz", ())))):
            raise ValueError("site_quant needs site_table (its slots) and markers with fixed targets mz (its channels), or xic with a channel")
        site_rollup.site_quant_params(n_channels=1 if label_free else len(tuple(markers["mz"])), **site_quant)
    if markers is not None:                                # (a bad request is refused before anything is read or scored)
        from .ascore import _markers_request
        if not isinstance(markers, dict) or "precursor_mz" in markers or "precursor_charge" in markers or marker_rows is None:
            raise ValueError("markers takes a dict of mz, losses, tol and tol_ppm beside a list marker_rows: the precursors are the spectra's")
        _markers_request(dict(markers, precursor_mz=np.zeros(0), precursor_charge=np.zeros(0, np.int32)), getattr(ascore, "_mz_error", 0.0))
    if centroid is not None:                             # (a bad request is refused before anything is read or scored)
        from .ascore import _centroid_request
        if not isinstance(centroid, dict) or "select" in centroid:
            raise ValueError("centroid takes a dict of gap, gap_ppm, half_width, min_height and area: select is what the spectra declare")
        _centroid_request(centroid)
    if strip is not None:                                  # (a bad request is refused before anything is read or scored)
        from .ascore import _strip_request
        if not isinstance(strip, dict) or "precursor_mz" in strip or "precursor_charge" in strip:
            raise ValueError("strip takes a dict of tol, losses, reduced, isotopes, step, mz_lo and mz_hi: the precursors are the spectra's")
        _strip_request(dict(strip, precursor_mz=np.zeros(0), precursor_charge=np.zeros(0, np.int32)), getattr(ascore, "_mz_error", 0.0))
    if not isinstance(ascore, PyAscore):
        raise TypeError("ascore must be a pyascore_amd.PyAscore")
    where = [] if reported else None
    picked, scans = select_psms(psms, spectra_map, residues, mod_mass, hit_depth, max_fragment_charge,
                                mod_correction_tol, zero_based, match_save, reported=where)
    if not picked:
        if mz_profile is not None:           # (no PSM: the empty table, with the parameters a scored batch would have had)
            none = ascore.score_batch(pack_hits([], []), skip_invalid=True, mz_profile=dict(n_slots=1))
            mz_profile.extend([none["mz_profile"], none["mz_profile_params"]])
        return []
    batch = pack_hits(picked, scans)
    named = [[sig_bits_of(p["peptide"], q, residues)] for p, q in zip(picked, where)] if reported else None
    # One PSM the kernels cannot take (longer than 64 residues, more than 15 000 site assignments,
    # an unknown residue, ...) must not cost the whole run its output: such PSMs are set aside by the
    # library, reported here, and written as rows without a localisation.
    stages = dict(skip_invalid=True, evidence=evidence, ions=ions is not None, named=named, sites=sites is not None, probs=probs,
                  ranked=ranked_depth if ranked is not None else None)
    keys = None
    form_keys = None
    if peptidoform_table is not None or peptidoform_quant is not None:
        group, _, form_keys = site_rollup.peptide_groups([p["peptide"] for p in picked])
        stages["peptidoforms"] = dict(group=group, threshold=float(peptidoform_threshold))
    if mz_profile is not None:
        stages["mz_profile"] = dict(n_slots=1)
    if coverage is not None:
        stages["coverage"] = True
    if recalibrate is not None:
        stages["recalibrate"] = dict(recalibrate)
    if deisotope is not None:
        from .ascore import _deisotope_request
        _deisotope_request(deisotope)                      # (a bad request is refused before anything is read or scored)
        stages["deisotope"] = dict(deisotope)
    if decharge is not None:
        from .ascore import _decharge_request
        if deisotope is not None or recalibrate is not None:
            raise ValueError("decharge cannot be combined with deisotope (it contains it) or with recalibrate (correct the spectra first)")
        _decharge_request(decharge)
        stages["decharge"] = dict(decharge)
    if strip is not None:
        prec_mz, prec_z = hit_precursors(picked, scans)
        stages["strip"] = dict(strip, precursor_mz=prec_mz, precursor_charge=prec_z)
    if centroid is not None:
        stages["centroid"] = dict(centroid, select=hit_profiles(picked, scans))
    if markers is not None:
        prec_mz, prec_z = hit_precursors(picked, scans)
        stages["markers"] = dict(markers, precursor_mz=prec_mz, precursor_charge=prec_z)
    if purity is not None:
        stages["purity"] = purity_stage(picked, scans, spectra_map, purity["survey"], purity_rule, purity_window, purity_gate)
    if xic is not None:
        stages["xic"] = xic_stage(picked, scans, spectra_map, xic["survey"], xic_rule, xic_rt_window)
    corrected = {} if channels is None else dict(channels=dict(channels))
    if site_quant is not None:
        stages["quant"] = dict(site_quant, values=label_free, **corrected)
    if peptidoform_quant is not None:
        stages["peptidoform_quant"] = dict(peptidoform_quant, values=label_free, **corrected)
    if site_table is not None:
        peptides = [p["peptide"] for p in picked]
        # (the PSMs the library will set aside have no residue records: the offsets come from its own pre-pass, before anything
        # is scored)
        slot, n_slots, keys = site_rollup.peptide_slots(peptides, ascore.site_offsets(batch, skip_invalid=True), residues=residues)
        res = ascore.score_batch(batch, rollup=dict(slot=slot, n_slots=n_slots, threshold=float(site_table_threshold)), **stages)
    else:
        res = ascore.score_batch(batch, **stages)
    bad = np.flatnonzero(res["status"])
    if bad.size:
        import warnings
        warnings.warn("%d of %d PSMs were not scored (first: %s); their rows carry no localisation"
                      % (bad.size, len(picked), res["status_message"]), RuntimeWarning)
        if log is not None:
            shown = ", ".join("%s (code %d)" % (scans[i], int(res["status"][i])) for i in bad[:50])
            log("%d of %d PSMs set aside (rows written with an empty LocalizedSequence and PepScore nan); first: %s"
                % (bad.size, len(picked), res["status_message"]))
            log("set-aside scans: %s%s" % (shown, " ..." if bad.size > 50 else ""))
    ok = (res["status"] == 0) & (res["n_sig"] > 0)
    seqs = ascore.format_batch(batch, res["best_sig"], valid=ok.astype(np.int32))   # every string in one call
    if reported:                                 # (one query per PSM: record i belongs to PSM i)
        rep_seqs = ascore.format_batch(batch, res["named"]["sig_bits"], valid=(res["named"]["kind"] >= 2).astype(np.int32))
    if sites is not None:                        # every sequence of the site table and the runner-up column in one call each
        rec, off = res["sites"], res["site_off"]
        rec_psm = np.repeat(np.arange(len(picked), dtype=np.int64), np.diff(off))
        scored = rec["kind"] == site_tables.SCORED
        with_seqs = ascore.format_batch(batch, rec["with_sig"], valid=(scored & (rec["with_score"] >= 0)).astype(np.int32), rec_psm=rec_psm)
        without_seqs = ascore.format_batch(batch, rec["without_sig"], valid=(scored & (rec["without_score"] >= 0)).astype(np.int32),
                                           rec_psm=rec_psm)
        runner = site_tables.runner_up(rec, off, res["best_sig"])
        runner_seqs = ascore.format_batch(batch, runner["sig"], valid=runner["found"].astype(np.int32))
    if ranked is not None:                       # every sequence of the ranked table in one call
        rk = res["ranked"]
        rk_psm = np.repeat(np.arange(len(picked), dtype=np.int64), rk.shape[1])
        rk_seqs = ascore.format_batch(batch, rk["sig_bits"].ravel(), valid=(rk["kind"].ravel() != ranked_lists.NONE).astype(np.int32),
                                      rec_psm=rk_psm)
    if site_table is not None:
        flr = None
        if site_table_flr:
            flr = ascore.rollup_flr(res["rollup"], site_rollup.decoy_classes(keys, decoys=site_table_decoys) if site_table_decoys else None)
        site_table.extend(site_table_fields(row, scans) for row in site_rollup.table(res["rollup"], keys, flr=flr))
    if site_quant is not None:
        sums = site_rollup.site_quant_sums(res["quant_head"], res["quant"], res["quant_params"])
        site_quant_rows.extend(site_quant_fields(keys[s], res["quant_head"][s], sums[s]) for s in np.flatnonzero(res["quant_head"]["n_records"]))
    if mz_profile is not None:
        mz_profile.extend([res["mz_profile"], res["mz_profile_params"]])
    if peptidoform_table is not None:
        peptidoform_table.extend(peptidoform_table_fields(row, scans)
                                 for row in site_rollup.peptidoform_table(res["peptidoforms"], form_keys, residues=residues))
    if peptidoform_quant is not None:
        sums = site_rollup.site_quant_sums(res["peptidoform_quant_head"], res["peptidoform_quant"], res["peptidoform_quant_params"])
        forms = site_rollup.peptidoform_table(res["peptidoforms"], form_keys, residues=residues)
        peptidoform_quant_rows.extend(peptidoform_quant_fields(row, scans, res["peptidoform_quant_head"][j], sums[j])
                                      for j, row in enumerate(forms))
    if coverage is not None:
        cov_ratios = site_rollup.coverage_ratios(res["coverage"])
    rows = []
    hit = 0
    for i, psm in enumerate(picked):
        hit = hit + 1 if i and scans[i] == scans[i - 1] else 1
        if coverage is not None:
            coverage.append([scans[i], hit] + coverage_fields(res["coverage"][i], {k: v[i] for k, v in cov_ratios.items()}))
        if markers is not None:                  # (the records are per spectrum: the hits of a scan share its row)
            spec = i if batch.get("spec_of") is None else int(batch["spec_of"][i])
            marker_rows.append([scans[i]] + marker_fields(res["markers"][spec], res["marker_spectra"][spec]))
        if purity is not None:                   # (per spectrum, as the marker records)
            spec = i if batch.get("spec_of") is None else int(batch["spec_of"][i])
            q = stages["purity"]
            survey_scan = int(purity["survey"][int(q["survey"][spec])]["scan"]) if q["survey"][spec] >= 0 else ""
            purity_rows.append([scans[i], survey_scan, float(q["window_lo"][spec]), float(q["window_hi"][spec])] +
                               purity_fields(res["purity"][spec]))
        if xic is not None:                      # (per spectrum, as the marker records)
            spec = i if batch.get("spec_of") is None else int(batch["spec_of"][i])
            q = stages["xic"]
            xic_rows.append([scans[i]] + xic_fields(res["xic"][spec], xic["survey"], int(q["seed"][spec]), int(q["scan_lo"][spec]),
                                                    int(q["scan_hi"][spec])))
        if ranked is not None:
            ranked.extend([scans[i], hit] + ranked_fields(rk[i, r], rk[i, 0], rk_seqs[i * rk.shape[1] + r])
                          for r in range(int(ranked_lists.lengths(rk[i])[0])))
        if sites is not None:
            sites.extend([scans[i]] + site_fields(rec[r], psm["peptide"], with_seqs[r], without_seqs[r])
                         for r in range(int(off[i]), int(off[i + 1])))
        if ions is not None:
            ions.extend([scans[i], hit] + ion_fields(rec) for rec in res["ions"][res["ion_off"][i]:res["ion_off"][i + 1]])
        if res["status"][i]:
            rows.append([scans[i], "", float("nan"), "", ""] + (["", "", ""] if evidence else []) + (["", "", ""] if reported else []) +
                        (["", ""] if sites is not None else []) + (["", ""] if probs else []))
            continue
        k = psm["n_of_mod"]
        ascores = ";".join(str(s) for s in res["ascores"][i, :k])
        alts = ";".join(",".join(str(q) for q in ascore.alt_positions(m, psm["peptide"].encode("utf8")))
                        for m in res["alt_mask"][i, :k])
        rows.append([scans[i], seqs[i], float(res["best_score"][i]), ascores, alts] +
                    (evidence_fields(res["evidence"][i, :k]) if evidence else []) +
                    (reported_fields(res["named"][i], rep_seqs[i]) if reported else []) +
                    ([runner_seqs[i], str(runner["delta"][i])] if sites is not None and runner["found"][i] else
                     (["", ""] if sites is not None else [])) +
                    (prob_fields(res["site_probs"][res["site_off"][i]:res["site_off"][i + 1]], res["psm_probs"][i], psm["peptide"],
                                 residues) if probs else []))
    return rows


def prob_fields(site_recs, psm_rec, peptide, residues):
    """The two ``--probs`` fields of one PSM: SiteProbs -- the peptide with the probability that it is modified behind every
    candidate residue, ``AS(0.98)PT(0.02)K`` --, and BestProb -- the posterior of the reported localisation, ``1 / z``.  Both
    are empty for a PSM that was not scored or has more site assignments than the stage sums; SiteProbs alone when the
    candidate residues cannot be told from the letters of ``residues`` (a modification group with a terminus)."""
    if int(psm_rec["kind"]) != site_probs.SCORED:
        return ["", ""]
    pos = site_probs.positions_of(peptide, residues)
    text = site_probs.annotate(peptide, pos, site_recs["with_prob"]) if len(pos) == len(site_recs) else ""
    return [text, repr(float(site_probs.best_prob(np.asarray([psm_rec], site_probs.PSM_PROB_DTYPE))[0]))]


def site_table_fields(row, scans):
    """One row of ``pyascore_amd.rollup.table`` keyed by (peptide, position) as the fields of the ``--site_table`` table:
    Peptide, Position (1-based), Residue, BestProb -- the best localisation probability any PSM gives the site --, BestScan --
    the scan that attains it (the first PSM of the input among equals) --, PSMs -- scored PSMs that cover the site --, Confident
    -- those that put it at or above the threshold --, InBest -- those that report it as the localisation --, BestAscore -- the
    best Ascore of those, empty when no PSM reports the site.  A row of ``table(..., flr=...)`` has three more
    (``SITE_TABLE_FLR_COLUMNS``): Rank -- the sites at least as good as this one, ties included --, FLR and DecoyQ of that cut;
    empty for a site that is not ranked."""
    peptide, pos = row["key"]
    more = []
    if "rank" in row:
        more = ["", "", ""] if row["rank"] is None else [str(row["rank"]), repr(row["flr"]), repr(row["decoy_q"])]
    return _site_table_fields(row, scans, peptide, pos) + more


def _site_table_fields(row, scans, peptide, pos):
    return [peptide, str(pos), peptide[pos - 1] if 1 <= pos <= len(peptide) else "?", repr(row["best_prob"]),
            scans[row["best_psm"]] if row["best_psm"] < len(scans) else "", str(row["n_psm"]), str(row["n_confident"]), str(row["n_in_best"]),
            "" if row["best_ascore"] is None else str(np.float32(row["best_ascore"]))]


def write_site_table_tsv(site_table_rows, path, flr=False):
    """The ``--site_table`` table: the rows ``localize(..., site_table=[])`` collected, under ``SITE_TABLE_COLUMNS`` (and,
    ``flr=True``, ``SITE_TABLE_FLR_COLUMNS``: the rows of ``localize(..., site_table_flr=True)``)."""
    wide = bool(flr)
    with open(path, "w") as out:
        out.write("\t".join(SITE_TABLE_COLUMNS + (SITE_TABLE_FLR_COLUMNS if wide else ())) + "\n")
        for row in site_table_rows:
            out.write("\t".join("%s" % f for f in row) + "\n")


def site_quant_columns(mz=(), named=()):
    """The header of the ``--site_quant`` table: Peptide, Position, Residue, Records, Complete, then the sum of every channel under
    the name of its target, ``mz<value>``, in the order of ``--marker_mz``; ``named``: channels that are no targets, under their
    own names (the label-free ``xic_area`` / ``xic_apex``)."""
    return ("Peptide", "Position", "Residue", "Records", "Complete") + tuple("mz%r" % float(v) for v in mz) + tuple(named)


def site_quant_fields(key, head, sums):
    """One slot of the site quantification (``pya_site_quant``) keyed by (peptide, position) as the fields of the ``--site_quant``
    table: Peptide, Position (1-based), Residue, Records -- the records that place the modification on the site at or above the
    threshold --, Complete -- those of them with a reading in every channel --, then per channel the summed intensity (``repr``),
    empty where no reading was summed."""
    peptide, pos = key
    return [peptide, str(pos), peptide[pos - 1] if 1 <= pos <= len(peptide) else "?", str(int(head["n_records"])), str(int(head["n_complete"]))] + \
        ["" if v != v else repr(float(v)) for v in sums]


def write_site_quant_tsv(site_quant_rows, path, mz=(), named=()):
    """The ``--site_quant`` table: the rows ``localize(..., site_quant=dict(...), site_quant_rows=[])`` collected, under
    ``site_quant_columns(mz, named)``."""
    with open(path, "w") as out:
        out.write("\t".join(site_quant_columns(mz, named)) + "\n")
        for row in site_quant_rows:
            out.write("\t".join("%s" % f for f in row) + "\n")


def peptidoform_table_fields(row, scans):
    """One row of ``pyascore_amd.rollup.peptidoform_table`` as the fields of the ``--peptidoform_table`` table: Peptide,
    Positions -- the modified positions, 1-based, joined by ``;`` --, PSMs -- scored PSMs that report this assignment --,
    Confident -- those whose smallest site probability is at or above the threshold --, BestScan -- the scan with the best
    such probability (the first PSM of the input among equals) --, BestMinProb, BestPosterior (``1 / best_z``), BestMinAscore
    and Isomers -- the assignments the peptide was seen with."""
    return [row["peptide"], ";".join(str(p) for p in row["sites"]), str(row["n_psm"]), str(row["n_confident"]),
            scans[row["best_psm"]] if row["best_psm"] < len(scans) else "", repr(row["best_min_prob"]), repr(row["best_posterior"]),
            str(np.float32(row["best_min_ascore"])), str(row["n_isomers"])]


def peptidoform_quant_columns(mz=(), named=()):
    """The header of the ``--peptidoform_quant`` table: the columns of ``--peptidoform_table``, Records, Complete, then the sum of
    every channel under the name of its target, ``mz<value>``, in the order of ``--marker_mz``; ``named`` as for
    ``site_quant_columns``."""
    return tuple(PEPTIDOFORM_TABLE_COLUMNS) + ("Records", "Complete") + tuple("mz%r" % float(v) for v in mz) + tuple(named)


def peptidoform_quant_fields(row, scans, head, sums):
    """One peptidoform with its row of the peptidoform quantification as the fields of the ``--peptidoform_quant`` table: those
    of ``peptidoform_table_fields``, Records -- the PSMs whose smallest site probability is at or above the quant threshold --,
    Complete -- those of them with a reading in every channel --, then per channel the summed intensity (``repr``), empty where no
    reading was summed."""
    return peptidoform_table_fields(row, scans) + [str(int(head["n_records"])), str(int(head["n_complete"]))] + \
        ["" if v != v else repr(float(v)) for v in sums]


def write_peptidoform_quant_tsv(peptidoform_quant_rows, path, mz=(), named=()):
    """The ``--peptidoform_quant`` table: the rows ``localize(..., peptidoform_quant=dict(...), peptidoform_quant_rows=[])``
    collected, under ``peptidoform_quant_columns(mz, named)``."""
    with open(path, "w") as out:
        out.write("\t".join(peptidoform_quant_columns(mz, named)) + "\n")
        for row in peptidoform_quant_rows:
            out.write("\t".join("%s" % f for f in row) + "\n")


def mz_profile_rows(table, params):
    """The ``--mz_profile`` table: one ``MZ_PROFILE_COLUMNS`` row per slot, band, unit and bin of a profile, with the bin's
    lower and upper edge in the unit (the counts outside an axis are the rows of bin -1 and bin ``MZP_BINS``, band -1)."""
    rows = []
    half = site_rollup.MZP_BINS // 2
    for s, rec in enumerate(np.asarray(table, site_rollup.MZ_PROFILE_DTYPE).reshape(-1)):
        for unit in ("da", "ppm"):
            w = 1.0 / params["inv_" + unit]
            rows.append([s, -1, unit, -1, "-inf", repr(-half * w), int(rec["out_" + unit][0])])
            for band in range(site_rollup.MZP_BANDS):
                rows.extend([s, band, unit, q, repr((q - half) * w), repr((q + 1 - half) * w), int(rec[unit][band, q])]
                            for q in range(site_rollup.MZP_BINS))
            rows.append([s, -1, unit, site_rollup.MZP_BINS, repr(half * w), "inf", int(rec["out_" + unit][1])])
    return rows


def write_mz_profile_tsv(table, params, path):
    """The ``--mz_profile`` file: ``mz_profile_rows`` under ``MZ_PROFILE_COLUMNS``."""
    with open(path, "w") as out:
        out.write("\t".join(MZ_PROFILE_COLUMNS) + "\n")
        for row in mz_profile_rows(table, params):
            out.write("\t".join(str(f) for f in row) + "\n")


def write_mz_calibration_tsv(cal, band_width, path):
    """The ``--mz_calibration_out`` file: ``pyascore_amd.rollup.mz_calibration_rows`` under ``MZ_CALIBRATION_COLUMNS``;
    ``pyascore_amd.rollup.read_mz_calibration`` reads it back to the same bytes."""
    with open(path, "w") as out:
        out.write("\t".join(MZ_CALIBRATION_COLUMNS) + "\n")
        for row in site_rollup.mz_calibration_rows(cal, band_width):
            out.write("\t".join(str(f) for f in row) + "\n")


def mz_profile_report(table, params):
    """The lines ``--mz_profile`` prints: per slot and unit the ions, the median and the 5 % / 95 % quantiles of the error,
    the flat floor, and the per-band medians."""
    lines = []
    for s, row in enumerate(site_rollup.mz_profile_summary(table, params)):
        lines.append("mass-error profile, slot %d: %d PSMs, %d ions (%d beyond max_rank)" % (s, row["n_psm"], row["n_ions"], row["n_rank_skipped"]))
        for unit in ("da", "ppm"):
            u = row[unit]
            lines.append("  %-3s median %.6g, 5 %% %.6g, 95 %% %.6g, %d inside (%d below, %d above), floor %.3g per bin; band medians %s"
                         % (unit, u["median"], u["q05"], u["q95"], u["total"], u["below"], u["above"], u["background"],
                            " ".join("%.4g" % m for m in u["band_medians"])))
    return lines


def write_peptidoform_table_tsv(peptidoform_rows, path):
    """The ``--peptidoform_table`` table: the rows ``localize(..., peptidoform_table=[])`` collected, under
    ``PEPTIDOFORM_TABLE_COLUMNS``."""
    with open(path, "w") as out:
        out.write("\t".join(PEPTIDOFORM_TABLE_COLUMNS) + "\n")
        for row in peptidoform_rows:
            out.write("\t".join("%s" % f for f in row) + "\n")


def ranked_fields(rec, first, sequence):
    """One ranked record as the fields behind Scan and Hit of the ``--ranked`` table: Rank (1: the reported localisation),
    LocalizedSequence -- the site assignment in the notation of the main table --, PepScore, DeltaToBest -- how far the
    PepScore lies behind the reported localisation's (``first``, row 0 of the PSM) --, Tied (1: the PepScore equals the row
    above's).  A PSM with more site assignments than the stage enumerates has its first row alone."""
    return [str(int(rec["rank"]) + 1), sequence, repr(float(rec["pep_score"])),
            str(np.float32(first["pep_score"]) - np.float32(rec["pep_score"])), "1" if int(rec["flags"]) & ranked_lists.TIED_PREV else "0"]


def write_ranked_tsv(ranked_rows, path):
    """The ``--ranked`` table: the rows ``localize(..., ranked=[])`` collected, under ``RANKED_COLUMNS``."""
    with open(path, "w") as out:
        out.write("\t".join(RANKED_COLUMNS) + "\n")
        for row in ranked_rows:
            out.write("\t".join("%s" % f for f in row) + "\n")


def site_fields(rec, peptide, with_sequence, without_sequence):
    """One site record as the fields behind Scan of the ``--sites`` table: Peptide, Position (1-based), Residue, InBest (1:
    the reported localisation modifies the residue), WithScore / WithoutScore -- the best PepScore among the site
    assignments that modify the residue / leave it unmodified, Delta = WithScore - WithoutScore, BestWith / BestWithout --
    site assignments that attain the two scores, in the notation of LocalizedSequence.  A PSM that was not scored, or has
    more site assignments than the stage enumerates, has the first four fields only; a side without any assignment is empty."""
    pos = int(rec["pos"])
    scored = int(rec["kind"]) == site_tables.SCORED
    has_with, has_without = scored and rec["with_score"] >= 0, scored and rec["without_score"] >= 0
    return [peptide, str(pos), peptide[pos - 1] if 1 <= pos <= len(peptide) else "", "1" if int(rec["flags"]) & site_tables.IN_BEST else "0",
            str(rec["with_score"]) if has_with else "", str(rec["without_score"]) if has_without else "",
            str(np.float32(rec["with_score"]) - np.float32(rec["without_score"])) if has_with and has_without else "",
            with_sequence if has_with else "", without_sequence if has_without else ""]


def write_sites_tsv(site_rows, path):
    """The ``--sites`` table: the rows ``localize(..., sites=[])`` collected, under ``SITE_COLUMNS``."""
    with open(path, "w") as out:
        out.write("\t".join(SITE_COLUMNS) + "\n")
        for row in site_rows:
            out.write("\t".join("%s" % f for f in row) + "\n")


def reported_fields(rec, sequence):
    """The three ``--reported`` fields of one PSM from the named record of the search engine's site assignment:
    ReportedSequence -- that assignment in the notation of LocalizedSequence; ReportedPepScore -- its PepScore;
    ReportedAscore -- the ambiguity of the winner against it (``0``: it IS the winner; ``tie``: its PepScore ties the
    winner's).  All empty where the reported positions are no site assignment of the PSM, or the PSM was not scored."""
    kind = int(rec["kind"])
    if kind < 2:
        return ["", "", ""]
    return [sequence, repr(float(rec["pep_score"])), "0" if kind == 2 else ("tie" if kind == 3 else str(rec["ambiguity"]))]


def evidence_fields(ev):
    """The three ``--evidence`` fields of one PSM from its evidence records (one per modified site): Depth -- the peak
    depth the Ascore was taken at, 1-based as a user counts the peaks of a window; SiteIons -- ``matched/possible`` of
    the winner, ``|``, the same of the competitor, or ``tie`` where the competitor's PepScore ties the winner's;
    CompScore -- the competitor's PepScore.  A site with nothing to compare (kind 0) has empty entries."""
    depth, ions, comp = [], [], []
    for e in ev:
        kind = int(e["kind"])
        depth.append(str(int(e["depth"]) + 1) if kind == 1 else "")
        ions.append("%d/%d|%d/%d" % (e["ref_matched"], e["ref_possible"], e["comp_matched"], e["comp_possible"]) if kind == 1
                    else ("tie" if kind == 2 else ""))
        comp.append(str(e["comp_score"]) if kind else "")
    return [";".join(depth), ";".join(ions), ";".join(comp)]


def ion_fields(rec):
    """One ion record as the fields behind Scan and Hit of the ``--ions`` table: Section (``winner``: a matched fragment of
    the reported localisation; ``site``: a site-determining ion), Site (which Ascore of the PSM, 1-based; empty for
    ``winner``), Side (``winner`` or ``competitor``), Ion (type, size, ``+`` per charge, ``*`` for a neutral-loss variant:
    ``y7++*``), TheoMz, PeakMz and Rank (1-based like Depth; empty without a match), Counted (1: matched at the site's depth)."""
    flags, matched = int(rec["flags"]), int(rec["rank"]) != 255
    winner_section = int(rec["site"]) == 255
    ion = "%s%d%s%s" % (chr(int(rec["type"])), int(rec["size"]), "+" * int(rec["charge"]), "*" if flags & 1 else "")
    return ["winner" if winner_section else "site", "" if winner_section else str(int(rec["site"]) + 1),
            "competitor" if flags & 2 else "winner", ion, str(rec["theo_mz"]), str(rec["peak_mz"]) if matched else "",
            str(int(rec["rank"]) + 1) if matched else "", "1" if flags & 4 else "0"]


def coverage_fields(rec, ratios):
    """One coverage record and its ratios (``pyascore_amd.rollup.coverage_ratios``, one entry each) as the fields behind Scan and
    Hit of the ``--coverage`` table; a PSM that was not scored has Scored 0 and zeros."""
    return [str(int(rec["kind"]))] + [repr(float(rec[f])) for f in ("total_current", "explained_current", "nterm_current", "cterm_current")] + \
        [str(int(rec[f])) for f in ("n_peaks", "n_retained", "n_explained", "n_fragments", "nterm_sizes", "cterm_sizes", "nterm_run",
                                    "cterm_run", "bonds")] + [repr(float(ratios[k])) for k in ("explained", "nterm", "cterm", "peaks")]


def write_coverage_tsv(coverage_rows, path):
    """The ``--coverage`` table: the rows ``localize(..., coverage=[])`` collected, under ``COVERAGE_COLUMNS``."""
    with open(path, "w") as out:
        out.write("\t".join(COVERAGE_COLUMNS) + "\n")
        for row in coverage_rows:
            out.write("\t".join("%s" % f for f in row) + "\n")


def purity_request(purity, purity_rows, have_quant):
    """``localize(purity=...)`` checked: ``(rule, window, gate)`` -- the dict of ``pyascore_amd.rollup.purity_params``, the
    ``(lower, upper)`` offsets or None, and ``dict(threshold=, keep_unknown=)`` or None"""
    names = ("survey", "tol", "tol_ppm", "isotopes", "below", "step", "window", "threshold", "keep_unknown")
    if not isinstance(purity, dict) or set(purity) - set(names) or purity.get("survey") is None or purity_rows is None:
        raise ValueError("purity takes a dict of " + ", ".join(names) + " beside a list purity_rows; survey is the MS1 records")
    try:
        rule = site_rollup.purity_params(**{k: purity[k] for k in ("tol", "tol_ppm", "isotopes", "below", "step") if purity.get(k) is not None})
    except TypeError:
        raise ValueError("purity: tol, tol_ppm and step are numbers, isotopes and below integers") from None
    window = purity.get("window")
    if window is not None:
        try:
            window = tuple(float(v) for v in window)
        except (TypeError, ValueError):
            window = ()
        if len(window) != 2 or not all(np.isfinite(v) and v >= 0.0 for v in window):
            raise ValueError("purity: window is a pair of offsets (lower, upper), finite and >= 0")
    gate = None
    if purity.get("threshold") is not None:
        t, keep = site_rollup.check_purity_gate(purity["threshold"], purity.get("keep_unknown", True), "purity")
        if not have_quant:
            raise ValueError("purity: threshold gates what site_quant and peptidoform_quant sum: it needs one of them")
        gate = dict(threshold=t, keep_unknown=keep)
    elif purity.get("keep_unknown", True) is not True:
        raise ValueError("purity: keep_unknown goes with threshold")
    return rule, window, gate


def purity_stage(picked, scans, spectra_map, survey, rule, window, gate):
    """The ``purity=`` request of ``PyAscore.score_batch`` for the spectra of ``pack_hits(picked, scans)``, in its order: the
    survey records ``survey`` packed as one CSR set, the survey spectrum of every MS2 spectrum
    (``pyascore_amd.rollup.survey_index``: its ``parent_scan``, else the last survey scan in front of it) and its isolation
    window -- the record's ``isolation`` as ``target - lower .. target + upper``, else the precursor m/z with the offsets
    ``window``, else NaN bounds: an inactive query."""
    survey = list(survey)
    lens = [np.size(r["mz_values"]) for r in survey]
    ms1_mz = np.concatenate([np.asarray(r["mz_values"]) for r in survey]) if survey else np.zeros(0)
    ms1_it = np.concatenate([np.asarray(r["intensity_values"]) for r in survey]) if survey else np.zeros(0)
    spec_scans, parents, lo, hi = [], [], [], []
    for i, psm in enumerate(picked):
        if i and scans[i] == scans[i - 1] and psm["mz"] is picked[i - 1]["mz"] and psm["intensity"] is picked[i - 1]["intensity"]:
            continue
        rec = spectra_map[scans[i]]
        spec_scans.append(scans[i])
        parents.append(rec.get("parent_scan"))
        iso, pm = rec.get("isolation"), rec.get("precursor_mz")
        if iso is not None:
            lo.append(float(iso[0]) - float(iso[1]))
            hi.append(float(iso[0]) + float(iso[2]))
        elif window is not None and pm is not None:
            lo.append(float(pm) - window[0])
            hi.append(float(pm) + window[1])
        else:
            lo.append(float("nan"))
            hi.append(float("nan"))
    prec_mz, prec_z = hit_precursors(picked, scans)
    stage = dict(rule, ms1_mz=ms1_mz, ms1_intensity=ms1_it, ms1_peak_off=np.concatenate([[0], np.cumsum(lens)]).astype(np.int64),
                 survey=site_rollup.survey_index([r["scan"] for r in survey], spec_scans, parents), precursor_mz=prec_mz,
                 precursor_charge=prec_z, window_lo=np.asarray(lo, np.float64), window_hi=np.asarray(hi, np.float64))
    if gate is not None:
        stage["gate"] = dict(gate)
    return stage


def xic_request(xic, xic_rows):
    """``localize(xic=...)`` checked: ``(rule, rt_window, channel)`` -- the dict of ``pyascore_amd.rollup.xic_params``, the
    seconds on either side of the seed scan, and 'area', 'apex' or None"""
    rule_names = ("tol", "tol_ppm", "isotopes", "step", "rise", "max_gap")
    names = ("survey", "rt_window") + rule_names + ("channel",)
    if not isinstance(xic, dict) or set(xic) - set(names) or xic.get("survey") is None or xic.get("rt_window") is None or xic_rows is None:
        raise ValueError("xic takes a dict of " + ", ".join(names) + " beside a list xic_rows; survey is the MS1 records with their rt")
    try:
        rule = site_rollup.xic_params(**{k: xic[k] for k in rule_names if xic.get(k) is not None})
        rt_window = float(xic["rt_window"])
    except TypeError:
        raise ValueError("xic: rt_window, tol, tol_ppm, step and rise are numbers, isotopes and max_gap integers") from None
    if not rt_window >= 0.0:
        raise ValueError("xic: rt_window = %r is not a number of seconds >= 0" % (xic["rt_window"],))
    if xic.get("channel") not in (None, "area", "apex"):
        raise ValueError("xic: channel is 'area' or 'apex'")
    return rule, rt_window, xic.get("channel")


def survey_arrays(survey):
    """the MS1 records ``survey`` packed as one CSR set: ``(ms1_mz, ms1_intensity, ms1_peak_off)``"""
    lens = [np.size(r["mz_values"]) for r in survey]
    ms1_mz = np.concatenate([np.asarray(r["mz_values"]) for r in survey]) if survey else np.zeros(0)
    ms1_it = np.concatenate([np.asarray(r["intensity_values"]) for r in survey]) if survey else np.zeros(0)
    return ms1_mz, ms1_it, np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def xic_stage(picked, scans, spectra_map, survey, rule, rt_window):
    """The ``xic=`` request of ``PyAscore.score_batch`` for the spectra of ``pack_hits(picked, scans)``, in its order: the survey
    records packed as one CSR set with their ``rt`` (NaN where the file gave none: such a scan is in no window but its own), the
    seed scan of every MS2 spectrum (``pyascore_amd.rollup.survey_index``, as for ``purity``) and the window of ``rt_window``
    seconds around it (``pyascore_amd.rollup.xic_windows``)."""
    survey = list(survey)
    ms1_mz, ms1_it, ms1_off = survey_arrays(survey)
    rt = np.asarray([float("nan") if r.get("rt") is None else float(r["rt"]) for r in survey], np.float64)
    spec_scans, parents = [], []
    for i, psm in enumerate(picked):
        if i and scans[i] == scans[i - 1] and psm["mz"] is picked[i - 1]["mz"] and psm["intensity"] is picked[i - 1]["intensity"]:
            continue
        spec_scans.append(scans[i])
        parents.append(spectra_map[scans[i]].get("parent_scan"))
    prec_mz, prec_z = hit_precursors(picked, scans)
    seed = site_rollup.survey_index([r["scan"] for r in survey], spec_scans, parents)
    lo, hi = site_rollup.xic_windows(rt, seed, rt_window)
    return dict(rule, ms1_mz=ms1_mz, ms1_intensity=ms1_it, ms1_peak_off=ms1_off, rt=rt, seed=seed, scan_lo=lo, scan_hi=hi, precursor_mz=prec_mz,
                precursor_charge=prec_z)


XIC_TABLE_COLUMNS = ["Scan", "SeedScan", "WindowFirst", "WindowLast", "Area", "Apex", "ApexScan", "ApexRT", "SeedIntensity", "Sum", "LeftScan",
                     "RightScan", "Points", "Present", "IsoHit", "Flags"]


def xic_fields(rec, survey, seed, scan_lo, scan_hi):
    """One ``XIC_DTYPE`` record as the fields behind the scan of the ``--xic`` table: the scan numbers of the seed and of the
    window's first and last survey scan (empty without a seed), Area, Apex, the apex's scan number and retention time, the seed
    scan's intensity, Sum, the scan numbers of the peak's bounds, Points, Present, IsoHit (one 0 / 1 per isotope, lowest first) and
    the flags as names joined by ``|``; the peak's fields are empty where none was found."""
    number = lambda s: int(survey[s]["scan"])                              # noqa: E731
    window = [number(seed), number(scan_lo), number(scan_hi - 1)] if seed >= 0 and scan_hi > scan_lo else ["", "", ""]
    flags = int(rec["flags"])
    names = "|".join(n for n, bit in (("active", 1), ("seen", 2), ("seed_present", 4), ("left_valley", 8), ("right_valley", 16), ("unsorted", 32),
                                      ("left_open", 64), ("right_open", 128)) if flags & bit)
    if not flags & site_rollup.XIC_SEEN:
        return window + [""] * 9 + [int(rec["n_present"]) if flags else "", "", names]
    apex = int(rec["apex_scan"])
    rt = survey[apex].get("rt")
    return window + [float(rec["area"]), float(rec["apex_intensity"]), number(apex), "" if rt is None else float(rt), float(rec["seed_intensity"]),
                     float(rec["sum_intensity"]), number(int(rec["left_scan"])), number(int(rec["right_scan"])), int(rec["n_points"]),
                     int(rec["n_present"]), format(int(rec["iso_hit"]), "b")[::-1], names]


def write_xic_tsv(xic_rows, path):
    """The ``--xic`` table: the rows ``localize(..., xic=dict(...), xic_rows=[])`` collected, under ``XIC_TABLE_COLUMNS``."""
    with open(path, "w") as out:
        out.write("\t".join(XIC_TABLE_COLUMNS) + "\n")
        for row in xic_rows:
            out.write("\t".join(str(v) for v in row) + "\n")


PURITY_COLUMNS = ["Scan", "SurveyScan", "WindowLo", "WindowHi", "Window", "Precursor", "Ratio", "Peaks", "PrecursorPeaks", "IsoHit",
                  "OtherMz", "OtherIntensity"]


def purity_fields(rec):
    """One ``PURITY_DTYPE`` record as the fields behind the window bounds of the ``--purity`` table: Window, Precursor, Ratio
    (empty where the window held nothing), Peaks, PrecursorPeaks, IsoHit (one 0 / 1 per centre, lowest first) and the m/z and
    intensity of the most intense other peak (empty where there is none)."""
    ratio = float(site_rollup.purity_ratio(np.asarray([rec], site_rollup.PURITY_DTYPE))[0])
    other = float(rec["other_intensity"]) > 0.0
    return [float(rec["window"]), float(rec["precursor"]), "" if ratio != ratio else ratio, int(rec["n_window"]), int(rec["n_precursor"]),
            format(int(rec["iso_hit"]), "b")[::-1], float(rec["other_mz"]) if other else "", float(rec["other_intensity"]) if other else ""]


def write_purity_tsv(purity_rows, path):
    """The ``--purity`` table: the rows ``localize(..., purity=dict(...), purity_rows=[])`` collected, under ``PURITY_COLUMNS``."""
    with open(path, "w") as out:
        out.write("\t".join(PURITY_COLUMNS) + "\n")
        for row in purity_rows:
            out.write("\t".join(str(v) for v in row) + "\n")


def marker_columns(mz=(), losses=()):
    """The header of the ``--markers`` table: Scan, TIC, BasePeak, then Mz, Intensity and Peaks of every target under its name
    -- ``mz<value>`` for a fixed target, ``loss<value>`` for a precursor loss, in the order of ``pyascore_amd.rollup.marker_params``."""
    names = ["mz%r" % float(v) for v in mz] + ["loss%r" % float(v) for v in losses]
    return ("Scan", "TIC", "BasePeak") + tuple("%s_%s" % (n, f) for n in names for f in ("Mz", "Intensity", "Peaks"))


def marker_fields(records, spectrum):
    """The marker records of one spectrum (``MARKER_DTYPE[n_targets]``) and its ``MARKER_SPECTRUM_DTYPE`` record as the fields
    behind Scan of the ``--markers`` table: TIC, BasePeak, then per target the m/z and the intensity of the peak it picked
    (empty when it picked none) and the peaks inside its window."""
    out = [repr(float(spectrum["tic"])), repr(float(spectrum["base_peak"]))]
    for rec in records:
        picked = int(rec["flags"]) & site_rollup.MARKER_PICKED
        out += [repr(float(rec["mz"])) if picked else "", repr(float(rec["intensity"])) if picked else "", str(int(rec["n_peaks"]))]
    return out


def write_markers_tsv(marker_rows, path, mz=(), losses=()):
    """The ``--markers`` table: the rows ``localize(..., markers=dict(mz=, losses=, ...), marker_rows=[])`` collected, under
    ``marker_columns(mz, losses)``."""
    with open(path, "w") as out:
        out.write("\t".join(marker_columns(mz, losses)) + "\n")
        for row in marker_rows:
            out.write("\t".join("%s" % f for f in row) + "\n")


def write_ions_tsv(ion_rows, path):
    """The ``--ions`` table: the rows ``localize(..., ions=[])`` collected, under ``ION_COLUMNS``."""
    with open(path, "w") as out:
        out.write("\t".join(ION_COLUMNS) + "\n")
        for row in ion_rows:
            out.write("\t".join("%s" % f for f in row) + "\n")


def write_tsv(rows, path, evidence=False, reported=False, sites=False, probs=False):
    """Same file pandas' ``DataFrame(rows, columns=COLUMNS).to_csv(path, sep="\\t", index=False)``
    writes in the reference (`__main__.py:166-172`); ``evidence=True``: the rows of ``localize(..., evidence=True)``,
    with their three columns behind the reference's; ``reported=True``: those of ``localize(..., reported=True)`` behind them;
    ``sites=True``: the two of ``localize(..., sites=[])`` behind those; ``probs=True``: the two of ``localize(..., probs=True)`` last."""
    with open(path, "w") as out:
        out.write("\t".join(COLUMNS + (EVIDENCE_COLUMNS if evidence else ()) + (REPORTED_COLUMNS if reported else ()) +
                            (RUNNER_UP_COLUMNS if sites else ()) + (PROB_COLUMNS if probs else ())) + "\n")
        for scan, seq, pep_score, ascores, alts, *more in rows:
            out.write("\t".join(["%s" % scan, "%s" % seq, repr(float(pep_score)), ascores, alts] + list(more)) + "\n")
