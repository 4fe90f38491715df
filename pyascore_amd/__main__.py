"""``python -m pyascore_amd [options] spec_file ident_file out_file`` -- the reference's command line
(`pyascore/__main__.py`, options of `pyascore/config.py:19-93`, same names and defaults) on the
MI355X scorer: the files are read by :mod:`pyascore_amd.ingest`, every selected PSM is scored in ONE
batched call (:func:`pyascore_amd.batch_cli.localize`) and the TSV of docs/source/cli.rst:135-180 is
written.  ``--parameter_file`` takes ``name = value`` lines ('#' starts a comment); options on the
command line override it.  ``--device`` (HIP ordinal), ``--evidence`` (three more columns: what stands behind every
Ascore), ``--ions FILE`` (a second table: which ions, one line each), ``--coverage FILE`` (a table with a line per PSM: the ion
current of its spectrum and the part the reported localisation explains) and ``--reported`` (three more columns: the search
engine's own site assignment, scored against the winner) and ``--sites FILE`` (a table with a line per candidate residue, and
the runner-up localisation in the main one) and ``--probs`` (two more columns: the localisation probability of every
candidate residue and the posterior of the reported localisation) and ``--ranked FILE`` with ``--ranked_depth K`` (a table
with a line per ranked site assignment: the K best localisations of every PSM, in order) and ``--site_table FILE`` with
``--site_table_threshold P`` (a site-level table over all PSMs, a line per peptide and position; ``--site_table_flr`` ranks
its sites and adds false-localisation rates, ``--site_table_decoys LETTERS`` names decoy residues) and
``--peptidoform_table FILE`` with ``--peptidoform_threshold P`` (a line per peptide and reported site assignment) and
``--mz_profile FILE`` (the fragment mass-error profile of the whole file, a line per m/z band, unit and bin, and its summary
in the log) and ``--mz_calibration_out FILE`` / ``--mz_calibration FILE`` (fit an m/z calibration to that profile; score with
the spectra corrected by one) and ``--deisotope`` with ``--deisotope_tol DA``, ``--deisotope_charge Z`` and
``--deisotope_ratio R`` (remove isotope satellites from every spectrum on the device before it is scored) and ``--decharge``
with ``--decharge_tol DA``, ``--decharge_charge Z``, ``--decharge_ratio R`` and ``--decharge_witness W`` (deisotope, and reduce
multiply charged fragments to 1+) and ``--strip_precursor`` with ``--strip_tol DA``, ``--strip_losses M1,M2,...``,
``--strip_reduced``, ``--strip_isotopes N``, ``--strip_mz_min X`` and ``--strip_mz_max X`` (remove the precursor, its
neutral-loss and charge-reduced forms and the peaks outside an m/z range from every spectrum) and ``--centroid`` with
``--centroid_gap DA``, ``--centroid_gap_ppm PPM``, ``--centroid_width W``, ``--centroid_min_height H`` and ``--centroid_area``
(peak-pick every spectrum the file does not declare centroided, before anything else) and ``--markers FILE`` with
``--marker_mz M1,M2,...``, ``--marker_losses L1,...``, ``--marker_tol DA`` and ``--marker_tol_ppm PPM`` (a table with a line per PSM:
the intensities of reporter and diagnostic ions in its spectrum, read before anything is stripped) and ``--site_quant FILE`` with
``--site_quant_threshold P``, ``--site_quant_scale E`` and ``--site_quant_complete`` (a line per site of ``--site_table``: the
intensities of the ``--marker_mz`` targets summed over the PSMs that localise the modification there) and ``--peptidoform_quant FILE``
with ``--peptidoform_quant_threshold P``, ``--peptidoform_quant_scale E`` and ``--peptidoform_quant_complete`` (a line per peptidoform:
the columns of ``--peptidoform_table``, then the same intensities summed over the PSMs that report the assignment; it needs
``--marker_mz``) and ``--channel_spill FILE`` and ``--channel_normalize`` (the reporter intensities corrected for the reagent lot's
isotope impurities and brought to equal channel totals before either table sums them) and ``--purity FILE`` with ``--purity_tol``,
``--purity_tol_ppm``, ``--purity_isotopes``, ``--purity_below``, ``--purity_window LO,HI``, ``--purity_threshold P`` and
``--purity_drop_unknown`` (per PSM the share of its isolation window that was its precursor, read off the survey scans of the
spectrum file; with a threshold the impure spectra are left out of both quantification tables) and ``--xic FILE`` with
``--xic_rt_window SECONDS``, ``--xic_tol``, ``--xic_tol_ppm``, ``--xic_isotopes``, ``--xic_rise``, ``--xic_gap`` and ``--xic_channel
area|apex`` (per PSM the label-free MS1 intensity of its precursor: the chromatographic peak over the survey scans around it, read in
the pass ``--purity`` makes; with a channel and no ``--marker_mz`` both quantification tables sum that column) are the additions."""
import argparse
import re
import sys
from datetime import datetime


def args_from_file(path):
    """``name = value`` lines -> ``["--name", "value", ...]`` (config.py:5-17)."""
    out = []
    with open(path) as f:
        for line in f:
            m = re.search(r"^(\S+)\s*=\s*(\S+)$", line.split("#")[0].strip())
            if m:
                out += ["--" + m.group(1), m.group(2)]
    return out


def build_parser():
    p = argparse.ArgumentParser(prog="pyascore_amd", description="PTM site localisation (Ascore) on an MI355X: "
                                "spectra (mzML / mzXML) + identifications (pepXML / mzIdentML / percolatorTXT / "
                                "mokapotTXT) -> Scan, LocalizedSequence, PepScore, Ascores, AltSites.")
    p.add_argument("--match_save", action="store_true",
                   help="write dump_spectra.pkl / dump_match.pkl of the last scored PSM, as the reference's loop leaves them")
    p.add_argument("--residues", type=str, default="STY", help="residues that can carry the modification")
    p.add_argument("--mod_mass", type=float, default=79.966331, help="exact mass of the modification")
    p.add_argument("--mz_error", type=float, default=0.5, help="fragment match tolerance in m/z")
    p.add_argument("--mod_correction_tol", type=float, default=1.0,
                   help="how far a reported modification mass may be from --mod_mass")
    p.add_argument("--zero_based", type=bool, default=False, help="modification positions count from 0")
    p.add_argument("--neutral_loss_groups", type=str, default="", help="comma separated residue groups (lower case: modified form)")
    p.add_argument("--neutral_loss_masses", type=str, default="", help="one loss mass per group")
    p.add_argument("--static_mod_groups", type=str, default="C", help="comma separated residue groups with a constant modification")
    p.add_argument("--static_mod_masses", type=str, default="57.021464", help="one mass per static group")
    p.add_argument("--fragment_types", type=str, default="by", help="ion types to score, of bcyzZ")
    p.add_argument("--max_fragment_charge", type=int, default=5, help="upper limit of the fragment charge (also PSM charge - 1)")
    p.add_argument("--hit_depth", type=int, default=1, help="PSMs taken per scan; negative = all")
    p.add_argument("--parameter_file", type=str, default="", help="file of 'name = value' lines")
    p.add_argument("--spec_file_type", type=str, default="mzML", help="mzML or mzXML")
    p.add_argument("--ident_file_type", type=str, default="pepXML", help="pepXML, mzIdentML, percolatorTXT or mokapotTXT")
    p.add_argument("--device", type=int, default=None, help="HIP device ordinal (default: LOCAL_RANK or 0)")
    p.add_argument("--evidence", action="store_true",
                   help="append Depth, SiteIons and CompScore: per site the peak depth of the Ascore, the site-determining ions "
                        "matched/possible of the winner | of the competitor, and the competitor's PepScore")
    p.add_argument("--ions", type=str, default="", metavar="FILE",
                   help="write the ion table to FILE: one line per matched fragment of the reported localisation and per "
                        "site-determining ion of every site (Scan, Hit, Section, Site, Side, Ion, TheoMz, PeakMz, Rank, Counted)")
    p.add_argument("--coverage", type=str, default="", metavar="FILE",
                   help="write the coverage table to FILE: one line per PSM with the ion current of its spectrum, the part the matched "
                        "fragments of the reported localisation explain (in all, N-terminal, C-terminal), peak, fragment and bond "
                        "counts, and the four ratios (Scan, Hit, Scored, TotalCurrent, ExplainedCurrent, ..., ExplainedRatio, "
                        "NTermRatio, CTermRatio, PeakRatio)")
    p.add_argument("--reported", action="store_true",
                   help="append ReportedSequence, ReportedPepScore and ReportedAscore: the site assignment the identification "
                        "file reports, its PepScore, and the ambiguity of the winner against it (0: Ascore kept the site)")
    p.add_argument("--sites", type=str, default="", metavar="FILE",
                   help="write the site table to FILE: one line per candidate residue of every scored PSM (Scan, Peptide, Position, "
                        "Residue, InBest, WithScore, WithoutScore, Delta, BestWith, BestWithout), and append RunnerUpSequence and "
                        "DeltaPepScore to the main table: the best localisation that differs from the reported one, and its distance")
    p.add_argument("--probs", action="store_true",
                   help="append SiteProbs and BestProb: the peptide with the localisation probability of every candidate residue "
                        "behind it, AS(0.98)PT(0.02)K, and the posterior of the reported localisation -- a PepScore-based "
                        "posterior (MaxQuant's construction), not part of the Ascore publication")
    p.add_argument("--ranked", type=str, default=None, metavar="FILE",
                   help="write the ranked localisations to FILE: one line per (scan, hit, rank) for the --ranked_depth best site "
                        "assignments of every scored PSM in order, the reported localisation first (Scan, Hit, Rank, "
                        "LocalizedSequence, PepScore, DeltaToBest, Tied); the main table does not change")
    p.add_argument("--ranked_depth", type=int, default=5, metavar="K",
                   help="how many site assignments per PSM --ranked lists, 1 .. 64 (default 5)")
    p.add_argument("--site_table", type=str, default=None, metavar="FILE",
                   help="write the site-level table to FILE: one line per (unmodified peptide, position) over all scored PSMs "
                        "(Peptide, Position, Residue, BestProb, BestScan, PSMs, Confident, InBest, BestAscore), rolled up on the "
                        "device from the localisation probabilities; the main table does not change")
    p.add_argument("--site_table_threshold", type=float, default=0.75, metavar="P",
                   help="the localisation probability from which a PSM counts as Confident in --site_table (default 0.75)")
    p.add_argument("--site_table_flr", action="store_true",
                   help="rank the sites of --site_table on the device: its rows come best site first and gain the columns Rank "
                        "(sites at least as good), FLR (the model-based false-localisation rate of that cut) and DecoyQ (the "
                        "q-value of the decoy / target ratio); without this option the file is unchanged")
    p.add_argument("--site_table_decoys", type=str, default="", metavar="LETTERS",
                   help="with --site_table_flr: sites on these residues are decoys (meaningful when the letters are in "
                        "--residues, e.g. --residues STYA --site_table_decoys A)")
    p.add_argument("--peptidoform_table", type=str, default=None, metavar="FILE",
                   help="write the peptidoform table to FILE: one line per (unmodified peptide, reported site assignment) over all "
                        "scored PSMs (Peptide, Positions, PSMs, Confident, BestScan, BestMinProb, BestPosterior, BestMinAscore, "
                        "Isomers), reduced on the device; the main table does not change")
    p.add_argument("--peptidoform_threshold", type=float, default=0.75, metavar="P",
                   help="the smallest site probability from which a PSM counts as Confident in --peptidoform_table (default 0.75)")
    p.add_argument("--mz_profile", type=str, default=None, metavar="FILE",
                   help="write the fragment mass-error profile of the whole file to FILE (slot 0): one line per band of m/z, unit "
                        "(da, ppm) and bin with the number of matched fragments of the reported localisations whose m/z error "
                        "falls into it, binned on the device, and print its summary; errors are only seen inside +-mz_error, "
                        "so run wide, read the profile, re-run narrow; the main table does not change")
    p.add_argument("--mz_calibration_out", type=str, default=None, metavar="FILE",
                   help="profile the run as --mz_profile does, fit the systematic fragment m/z error per band of m/z on the device "
                        "and write it to FILE: one line per slot and band (band centre, ppm, spread, signal ions, band width); run "
                        "wide for this, then re-run narrow with --mz_calibration FILE")
    p.add_argument("--mz_calibration_min_ions", type=int, default=20, metavar="N",
                   help="the ions above the flat floor a band of m/z needs to be fitted by --mz_calibration_out (default 20); a band "
                        "with fewer copies its nearest fitted neighbour")
    p.add_argument("--mz_calibration", type=str, default=None, metavar="FILE",
                   help="correct the m/z of every spectrum with the calibration in FILE (written by --mz_calibration_out) on the device "
                        "before it is scored; together with --mz_profile the profile shows the residual errors")
    p.add_argument("--deisotope", action="store_true",
                   help="remove isotope satellites from every spectrum on the device before it is scored (and before "
                        "--mz_calibration corrects it): a peak goes when a peak one isotope spacing / z below it, z = 1 .. "
                        "--deisotope_charge, is at least as intense (times --deisotope_ratio); one more transfer of the spectra")
    p.add_argument("--deisotope_tol", type=float, default=0.01, metavar="DA",
                   help="with --deisotope: how far the distance of two peaks may be from the isotope spacing, in m/z (default 0.01)")
    p.add_argument("--deisotope_charge", type=int, default=3, metavar="Z",
                   help="with --deisotope: the largest charge whose spacing is tried, 1 .. 8 (default 3)")
    p.add_argument("--deisotope_ratio", type=float, default=1.0, metavar="R",
                   help="with --deisotope: a satellite is at most R times as intense as its parent (default 1.0)")
    p.add_argument("--decharge", action="store_true",
                   help="charge-deconvolve every spectrum on the device before it is scored: deisotope it, and move every kept peak "
                        "whose satellites show a charge z of 2 .. --decharge_charge to its m/z at 1+, so that b/y ions at 1+ find "
                        "multiply charged fragments; leave --max_fragment_charge at 1 with it; not together with --deisotope "
                        "(it contains it) or --mz_calibration (correct the spectra first); one more transfer of the spectra")
    p.add_argument("--decharge_tol", type=float, default=0.01, metavar="DA",
                   help="with --decharge: how far the distance of two peaks may be from the isotope spacing, in m/z (default 0.01)")
    p.add_argument("--decharge_charge", type=int, default=3, metavar="Z",
                   help="with --decharge: the largest charge whose spacing is tried, 1 .. 8 (default 3)")
    p.add_argument("--decharge_ratio", type=float, default=1.0, metavar="R",
                   help="with --decharge: a satellite is at most R times as intense as its parent (default 1.0)")
    p.add_argument("--decharge_witness", type=float, default=0.3, metavar="W",
                   help="with --decharge: a satellite testifies to a charge only if it is at least W times as intense as its parent "
                        "(default 0.3, from synthetic spectra)")
    p.add_argument("--strip_precursor", action="store_true",
                   help="remove the precursor-derived peaks from every spectrum on the device before it is scored, in front of "
                        "--deisotope / --decharge / --mz_calibration: the peaks within --strip_tol of the spectrum's precursor m/z "
                        "and of its --strip_losses forms; a spectrum without a precursor m/z or charge keeps them; one more "
                        "transfer of the spectra")
    p.add_argument("--strip_tol", type=float, default=None, metavar="DA",
                   help="with --strip_precursor: the half width of a window around a precursor form, in m/z (default: --mz_error)")
    p.add_argument("--strip_losses", type=str, default="", metavar="M1,M2,...",
                   help="with --strip_precursor: up to 7 neutral masses whose loss from the precursor is removed as well, e.g. "
                        "97.976896,18.010565 (default: none)")
    p.add_argument("--strip_reduced", action="store_true",
                   help="with --strip_precursor: also at every charge below the precursor's, down to 1 (the charge-reduced "
                        "precursors of ETD)")
    p.add_argument("--strip_isotopes", type=int, default=0, metavar="N",
                   help="with --strip_precursor: the isotope peaks above each form that its window covers, 0 .. 4 (default 0)")
    p.add_argument("--strip_mz_min", type=float, default=float("-inf"), metavar="X",
                   help="with --strip_precursor: peaks below this m/z are removed too (a TMT reporter region: 140)")
    p.add_argument("--strip_mz_max", type=float, default=float("inf"), metavar="X",
                   help="with --strip_precursor: peaks above this m/z are removed too")
    p.add_argument("--centroid", action="store_true",
                   help="centroid (peak-pick) on the device every spectrum that the file does not declare centroided (mzML cvParam "
                        "MS:1000127, mzXML centroided=\"1\"), in front of --strip_precursor / --deisotope / --decharge / "
                        "--mz_calibration; a spectrum of isolated peaks passes through unchanged; one more transfer of the spectra")
    p.add_argument("--centroid_gap", type=float, default=None, metavar="DA",
                   help="with --centroid: two adjacent samples belong to one peak when they are at most this far apart, in m/z: 2 to "
                        "3 times the sampling step (needed unless --centroid_gap_ppm is given)")
    p.add_argument("--centroid_gap_ppm", type=float, default=0.0, metavar="PPM",
                   help="with --centroid: ... plus this many ppm of the m/z (a TOF's step grows with m/z; default 0)")
    p.add_argument("--centroid_width", type=int, default=4, metavar="W",
                   help="with --centroid: the samples on either side of an apex its centroid takes in, 1 .. 8 (default 4)")
    p.add_argument("--centroid_min_height", type=float, default=0.0, metavar="H",
                   help="with --centroid: local maxima below this intensity are dropped (default 0)")
    p.add_argument("--centroid_area", action="store_true",
                   help="with --centroid: a peak's intensity is the sum over its samples instead of the apex's own")
    p.add_argument("--markers", type=str, default="", metavar="FILE",
                   help="write the marker-ion table to FILE: one line per PSM with the ion current and the base peak of its spectrum "
                        "and, per target of --marker_mz / --marker_losses, the m/z and the intensity of the most intense peak within "
                        "the tolerance and the peaks inside it; read off the spectra before --strip_precursor cuts them; one more "
                        "upload of the spectra")
    p.add_argument("--marker_mz", type=str, default="", metavar="M1,M2,...",
                   help="with --markers: the m/z of the fixed targets (reporter ions, immonium ions); up to 64 targets with "
                        "--marker_losses together (default: none)")
    p.add_argument("--marker_losses", type=str, default="", metavar="L1,L2,...",
                   help="with --markers: neutral masses whose loss from the spectrum's precursor is a target, e.g. 97.976896 "
                        "(default: none)")
    p.add_argument("--marker_tol", type=float, default=None, metavar="DA",
                   help="with --markers: the half width of a target's window in m/z (default: --mz_error)")
    p.add_argument("--marker_tol_ppm", type=float, default=0.0, metavar="PPM",
                   help="with --markers: ... plus this many ppm of the target's m/z (default 0)")
    p.add_argument("--site_quant", type=str, default="", metavar="FILE",
                   help="write the site quantification to FILE: one line per site of --site_table with a contributing PSM, the "
                        "intensities of the --marker_mz targets summed on the device over the PSMs that place the modification on "
                        "the site with at least --site_quant_threshold; needs --site_table and --marker_mz")
    p.add_argument("--site_quant_threshold", type=float, default=0.75, metavar="P",
                   help="with --site_quant: the localisation probability from which a PSM's reading is summed (default 0.75)")
    p.add_argument("--site_quant_scale", type=int, default=10, metavar="E",
                   help="with --site_quant: readings are summed as integers in units of 2^-E (default 10; -64 .. 64)")
    p.add_argument("--site_quant_complete", action="store_true",
                   help="with --site_quant: only PSMs with a reading in every channel are summed")
    p.add_argument("--peptidoform_quant", type=str, default="", metavar="FILE",
                   help="write the peptidoform quantification to FILE: one line per peptidoform, the columns of --peptidoform_table, then "
                        "the intensities of the --marker_mz targets summed on the device over the PSMs that report the assignment with "
                        "a smallest site probability of at least --peptidoform_quant_threshold; needs --marker_mz (fixed targets)")
    p.add_argument("--peptidoform_quant_threshold", type=float, default=0.75, metavar="P",
                   help="with --peptidoform_quant: the smallest site probability from which a PSM's reading is summed (default 0.75)")
    p.add_argument("--peptidoform_quant_scale", type=int, default=10, metavar="E",
                   help="with --peptidoform_quant: readings are summed as integers in units of 2^-E (default 10; -64 .. 64)")
    p.add_argument("--peptidoform_quant_complete", action="store_true",
                   help="with --peptidoform_quant: only PSMs with a reading in every channel are summed")
    p.add_argument("--channel_spill", type=str, default="", metavar="FILE",
                   help="with --site_quant / --peptidoform_quant: correct the reporter intensities for the isotope impurities of the "
                        "reagent lot before they are summed; FILE holds tab-separated lines from, to, fraction -- that fraction of "
                        "channel from's reporter shows up in channel to (-1: in no channel) --, the channels numbered from 0 in "
                        "--marker_mz order")
    p.add_argument("--channel_normalize", action="store_true",
                   help="with --site_quant / --peptidoform_quant: bring the channels to equal totals over all spectra (after "
                        "--channel_spill) before they are summed")
    p.add_argument("--purity", type=str, default="", metavar="FILE",
                   help="write the precursor-purity table to FILE: one line per PSM with the survey (MS1) scan in front of its "
                        "spectrum, the bounds of its isolation window, the intensity inside the window there, the part of it at the "
                        "precursor's m/z and isotope positions, their ratio, the peak counts, which isotope positions held a peak "
                        "and the most intense other peak (the survey scans are a second read of the spectrum file)")
    p.add_argument("--purity_tol", type=float, default=0.0, metavar="DA",
                   help="with --purity: the half width of the window around an isotope position in m/z (default 0)")
    p.add_argument("--purity_tol_ppm", type=float, default=10.0, metavar="PPM",
                   help="with --purity: ... plus this many ppm of the position's m/z (default 10)")
    p.add_argument("--purity_isotopes", type=int, default=3, metavar="N",
                   help="with --purity: isotope positions above the precursor's m/z that count as the precursor (default 3)")
    p.add_argument("--purity_below", type=int, default=0, metavar="N",
                   help="with --purity: isotope positions under the precursor's m/z that count as the precursor, 0 .. 4 (default 0)")
    p.add_argument("--purity_window", type=str, default="", metavar="LO,HI",
                   help="with --purity: the offsets of the isolation window under and above the precursor's m/z, used where the "
                        "spectrum file declares none (default: such a spectrum has no purity)")
    p.add_argument("--purity_threshold", type=float, default=None, metavar="P",
                   help="with --purity beside --site_quant / --peptidoform_quant: leave out the reporter readings of every spectrum "
                        "whose precursor made up less than P of its isolation window")
    p.add_argument("--purity_drop_unknown", action="store_true",
                   help="with --purity_threshold: also leave out the spectra whose purity is not known (no survey scan, no window, "
                        "an empty window)")
    p.add_argument("--xic", type=str, default="", metavar="FILE",
                   help="write the precursor-XIC table to FILE: one line per PSM with its survey (MS1) scan, the survey scans its "
                        "window reaches, and the area, apex, sum and bounds of the precursor's chromatographic peak there (the survey "
                        "scans are read in the pass --purity makes, once for both)")
    p.add_argument("--xic_rt_window", type=float, default=60.0, metavar="SECONDS",
                   help="with --xic: how far on either side of the survey scan a window reaches in retention time, 64 scans at the most "
                        "(default 60: a choice, not a measurement)")
    p.add_argument("--xic_tol", type=float, default=0.0, metavar="DA",
                   help="with --xic: the half width of the window around an isotope position in m/z (default 0)")
    p.add_argument("--xic_tol_ppm", type=float, default=10.0, metavar="PPM",
                   help="with --xic: ... plus this many ppm of the position's m/z (default 10)")
    p.add_argument("--xic_isotopes", type=int, default=2, metavar="N",
                   help="with --xic: isotope positions above the precursor's m/z whose intensity is added to the trace, 0 .. 3 (default 2)")
    p.add_argument("--xic_rise", type=float, default=2.0, metavar="R",
                   help="with --xic: a scan splits the trace where R times its intensity lies below the maxima on both sides (default 2)")
    p.add_argument("--xic_gap", type=int, default=1, metavar="N",
                   help="with --xic: survey scans without the precursor a trace may bridge, 0 .. 8 (default 1)")
    p.add_argument("--xic_channel", type=str, default="", choices=("", "area", "apex"),
                   help="with --xic and without --marker_mz: --site_quant / --peptidoform_quant sum this column of the XIC table as "
                        "their one channel (label-free tables); with --marker_mz the channels are the reporters")
    p.add_argument("spec_file", type=str)
    p.add_argument("ident_file", type=str)
    p.add_argument("out_file", type=str)
    return p


def strip_request(args):
    """The rule of ``--strip_precursor`` as the dict ``batch_cli.localize(strip=...)`` takes (the precursors come from the
    spectra), checked; None without the flag: the other ``--strip_*`` values are then not looked at."""
    if not getattr(args, "strip_precursor", False):
        return None
    from .rollup import strip_params
    try:
        losses = tuple(float(v) for v in args.strip_losses.split(",") if v.strip())
    except ValueError:
        raise ValueError("--strip_losses takes neutral masses separated by commas, not %r" % args.strip_losses) from None
    req = dict(tol=args.strip_tol, losses=losses, reduced=bool(args.strip_reduced), isotopes=args.strip_isotopes, mz_lo=args.strip_mz_min,
               mz_hi=args.strip_mz_max)
    strip_params(**dict(req, tol=args.mz_error if args.strip_tol is None else args.strip_tol))
    return req


def xic_request(args):
    """``--xic`` as the dict ``batch_cli.localize(xic=...)`` takes, without the survey records (``run`` reads them), checked; None
    without the option: the other ``--xic_*`` values are then not looked at -- but for ``--xic_channel``, which is refused
    without it."""
    if not getattr(args, "xic", ""):
        if getattr(args, "xic_channel", ""):
            raise ValueError("--xic_channel names a column of the table of --xic: give --xic FILE as well")
        return None
    from . import batch_cli
    req = dict(rt_window=args.xic_rt_window, tol=args.xic_tol, tol_ppm=args.xic_tol_ppm, isotopes=args.xic_isotopes, rise=args.xic_rise,
               max_gap=args.xic_gap, channel=args.xic_channel or None)
    try:
        batch_cli.xic_request(dict(req, survey=()), [])
    except ValueError as e:
        raise ValueError("--xic: %s" % e) from None
    return req


def label_free(args):
    """the column ``--site_quant`` / ``--peptidoform_quant`` sum without reporter targets ('xic_area' / 'xic_apex'), or None"""
    targets = [v for v in getattr(args, "marker_mz", "").split(",") if v.strip()]
    return "xic_" + args.xic_channel if getattr(args, "xic", "") and getattr(args, "xic_channel", "") and not targets else None


def site_quant_request(args):
    """``--site_quant`` as the dict ``batch_cli.localize(site_quant=...)`` takes, checked; None without the option: the other
    ``--site_quant_*`` values are then not looked at."""
    if not getattr(args, "site_quant", ""):
        return None
    from .rollup import site_quant_params
    if not args.site_table:
        raise ValueError("--site_quant sums over the sites of --site_table: give --site_table FILE as well")
    channels = [v for v in args.marker_mz.split(",") if v.strip()] or ([label_free(args)] if label_free(args) else [])
    if not channels:
        raise ValueError("--site_quant sums the intensities of the --marker_mz targets: give --marker_mz M1,M2,... as well "
                         "(or --xic FILE --xic_channel area|apex for a label-free table)")
    req = dict(threshold=args.site_quant_threshold, scale_log2=args.site_quant_scale, complete_only=bool(args.site_quant_complete))
    site_quant_params(n_channels=min(len(channels), 64), **req)
    return req


def peptidoform_quant_request(args):
    """``--peptidoform_quant`` as the dict ``batch_cli.localize(peptidoform_quant=...)`` takes, checked; None without the option:
    the other ``--peptidoform_quant_*`` values are then not looked at."""
    if not getattr(args, "peptidoform_quant", ""):
        return None
    from .rollup import site_quant_params
    channels = [v for v in args.marker_mz.split(",") if v.strip()] or ([label_free(args)] if label_free(args) else [])
    if not channels:
        raise ValueError("--peptidoform_quant sums the intensities of the fixed --marker_mz targets (--marker_losses are no channels): "
                         "give --marker_mz M1,M2,... as well (or --xic FILE --xic_channel area|apex for a label-free table)")
    req = dict(threshold=args.peptidoform_quant_threshold, scale_log2=args.peptidoform_quant_scale,
               complete_only=bool(args.peptidoform_quant_complete))
    try:
        site_quant_params(n_channels=min(len(channels), 64), **req)
    except ValueError as e:
        raise ValueError("--peptidoform_quant_scale / --peptidoform_quant_threshold: %s" % e) from None
    return req


def channels_request(args):
    """``--channel_spill`` / ``--channel_normalize`` as the dict ``batch_cli.localize(channels=...)`` takes, the spill file read and
    inverted, checked; None without either option."""
    spill, normalize = getattr(args, "channel_spill", ""), bool(getattr(args, "channel_normalize", False))
    if not spill and not normalize:
        return None
    if not getattr(args, "site_quant", "") and not getattr(args, "peptidoform_quant", ""):
        raise ValueError("--channel_spill / --channel_normalize correct what --site_quant and --peptidoform_quant sum: give one of them")
    from .rollup import channel_matrix, read_channel_spill
    n_ch = len([v for v in args.marker_mz.split(",") if v.strip()])
    req = dict(normalize=normalize)
    if spill:
        try:
            req["matrix"] = channel_matrix(read_channel_spill(spill, n_ch))
        except OSError as e:
            raise ValueError("--channel_spill: %s" % e) from None
        except ValueError as e:
            raise ValueError("--channel_spill %s" % e) from None
    return req


def markers_request(args):
    """The rule of ``--markers`` as the dict ``batch_cli.localize(markers=...)`` takes (the precursors come from the spectra),
    checked; None without the option (and without ``--site_quant`` / ``--peptidoform_quant``, which read the same targets): the
    other ``--marker_*`` values are then not looked at."""
    if not getattr(args, "markers", "") and not getattr(args, "site_quant", "") and not getattr(args, "peptidoform_quant", ""):
        return None
    if not getattr(args, "markers", "") and label_free(args):      # (the tables sum the XIC column: no targets are read)
        return None
    from .rollup import marker_params
    lists = {}
    for name in ("marker_mz", "marker_losses"):
        try:
            lists[name] = tuple(float(v) for v in getattr(args, name).split(",") if v.strip())
        except ValueError:
            raise ValueError("--%s takes numbers separated by commas, not %r" % (name, getattr(args, name))) from None
    req = dict(mz=lists["marker_mz"], losses=lists["marker_losses"], tol=args.marker_tol, tol_ppm=args.marker_tol_ppm)
    marker_params(**dict(req, tol=args.mz_error if args.marker_tol is None else args.marker_tol))
    return req


def purity_request(args):
    """``--purity`` as the dict ``batch_cli.localize(purity=...)`` takes, without the survey records (``run`` reads them),
    checked; None without the option: the other ``--purity_*`` values are then not looked at -- but for ``--purity_threshold``,
    which is refused without it."""
    if not getattr(args, "purity", ""):
        if getattr(args, "purity_threshold", None) is not None or getattr(args, "purity_drop_unknown", False):
            raise ValueError("--purity_threshold / --purity_drop_unknown gate on the table of --purity: give --purity FILE as well")
        return None
    from . import batch_cli
    req = dict(tol=args.purity_tol, tol_ppm=args.purity_tol_ppm, isotopes=args.purity_isotopes, below=args.purity_below)
    if args.purity_window:
        try:
            req["window"] = tuple(float(v) for v in args.purity_window.split(","))
        except ValueError:
            raise ValueError("--purity_window takes two offsets LO,HI, not %r" % args.purity_window) from None
        if len(req["window"]) != 2:
            raise ValueError("--purity_window takes two offsets LO,HI, not %r" % args.purity_window)
    if args.purity_threshold is not None:
        req["threshold"] = args.purity_threshold
        req["keep_unknown"] = not args.purity_drop_unknown
    elif args.purity_drop_unknown:
        raise ValueError("--purity_drop_unknown goes with --purity_threshold")
    try:
        batch_cli.purity_request(dict(req, survey=()), [], bool(getattr(args, "site_quant", "") or getattr(args, "peptidoform_quant", "")))
    except ValueError as e:
        raise ValueError("--purity: %s" % e) from None
    return req


def centroid_request(args):
    """The rule of ``--centroid`` as the dict ``batch_cli.localize(centroid=...)`` takes (which spectra it applies to comes
    from the spectra), checked; None without the flag: the other ``--centroid_*`` values are then not looked at."""
    if not getattr(args, "centroid", False):
        return None
    from .rollup import centroid_params
    req = dict(gap=0.0 if args.centroid_gap is None else args.centroid_gap, gap_ppm=args.centroid_gap_ppm, half_width=args.centroid_width,
               min_height=args.centroid_min_height, area=bool(args.centroid_area))
    centroid_params(**req)
    return req


def validate_args(args):
    """`__main__.py:48-65`."""
    for aa in args.residues:
        if aa not in "ncACDEFGHIKLMNOPQRSTUVWY":
            raise ValueError("The residue inputed, {}, is not allowed.".format(aa))
    for frag in args.fragment_types:
        if frag not in "cbyzZ":
            raise ValueError("The fragment type inputed, {}, is not allowed.".format(frag))
    if args.max_fragment_charge < 1:
        raise ValueError("The max fragment charge must be greater than or equal to 1")
    if getattr(args, "deisotope", False):
        from .rollup import deisotope_params
        deisotope_params(tol=args.deisotope_tol, max_charge=args.deisotope_charge, ratio=args.deisotope_ratio)
    strip_request(args)
    centroid_request(args)
    markers_request(args)
    site_quant_request(args)
    peptidoform_quant_request(args)
    channels_request(args)
    purity_request(args)
    xic_request(args)
    if getattr(args, "decharge", False):
        from .rollup import decharge_params
        if getattr(args, "deisotope", False):
            raise ValueError("--decharge contains --deisotope: give one of the two")
        if getattr(args, "mz_calibration", None):
            raise ValueError("--decharge moves peaks and --mz_calibration is a function of the measured m/z: write the corrected "
                             "spectra first, then run with --decharge")
        decharge_params(tol=args.decharge_tol, max_charge=args.decharge_charge, ratio=args.decharge_ratio, witness=args.decharge_witness)


def parse_args(argv):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.parameter_file:
        args = parser.parse_args(args_from_file(args.parameter_file) + list(argv))
    validate_args(args)
    return args


def static_mods_of(args):
    mods = {}
    for group, mass in zip(args.static_mod_groups.split(","), args.static_mod_masses.split(",")):
        mods.update({aa: float(mass) for aa in group})
    return mods


def run(args, log=print):
    from . import batch_cli, ingest
    from .ascore import PyAscore
    stamp = lambda: datetime.now().strftime("%m/%d/%y %H:%M:%S")
    log("{} -- Ascore Started".format(stamp()))
    log("{} -- Reading spectra from: {}".format(stamp(), args.spec_file))
    # (the arrays in the precision the file holds them: float32 ones go to the device as they are, results are those of
    # the widened arrays bit for bit)
    spectra = ingest.SpectraParser(args.spec_file, args.spec_file_type, native_precision=True).to_dict()
    log("{} -- Reading identifications from: {}".format(stamp(), args.ident_file))
    static = static_mods_of(args)
    known = dict(ingest.COMMON_MODS)                       # `__main__.py:30-35`
    known.update({aa: args.mod_mass for aa in args.residues})
    known.update(static)
    psms = sorted(ingest.IdentificationParser(args.ident_file, args.ident_file_type,
                                              ingest.MassCorrector(mod_mass_dict=known), static_mods=static).to_list(),
                  key=lambda p: p["scan"])
    log("{} -- Anlyzing PSMs".format(stamp()))
    kw = {} if args.device is None else {"device": args.device}
    ascore = PyAscore(bin_size=100.0, n_top=10, mod_group=args.residues, mod_mass=args.mod_mass,
                      mz_error=args.mz_error, fragment_types=args.fragment_types, **kw)
    if args.neutral_loss_groups and args.neutral_loss_masses:
        for group, mass in zip(args.neutral_loss_groups.split(","), args.neutral_loss_masses.split(",")):
            ascore.add_neutral_loss(group, float(mass))
    ion_rows = [] if args.ions else None
    coverage_rows = [] if args.coverage else None
    site_rows = [] if args.sites else None
    ranked_rows = [] if args.ranked else None
    site_table_rows = [] if args.site_table else None
    peptidoform_rows = [] if args.peptidoform_table else None
    profile = [] if args.mz_profile or args.mz_calibration_out else None
    recalibrate = None
    if args.mz_calibration:
        from .rollup import read_mz_calibration
        cal, band_width = read_mz_calibration(args.mz_calibration)
        recalibrate = dict(calibration=cal, band_width=band_width)
    deisotope = dict(tol=args.deisotope_tol, max_charge=args.deisotope_charge, ratio=args.deisotope_ratio) if args.deisotope else None
    decharge = dict(tol=args.decharge_tol, max_charge=args.decharge_charge, ratio=args.decharge_ratio,
                    witness=args.decharge_witness) if args.decharge else None
    markers = markers_request(args)
    marker_rows = [] if markers is not None else None
    site_quant = site_quant_request(args)
    site_quant_rows = [] if site_quant is not None else None
    pform_quant = peptidoform_quant_request(args)
    pform_quant_rows = [] if pform_quant is not None else None
    purity = purity_request(args)
    purity_rows = [] if purity is not None else None
    xic = xic_request(args)
    xic_rows = [] if xic is not None else None
    if purity is not None or xic is not None:              # (one pass over the file serves both)
        log("{} -- Reading survey scans from: {}".format(stamp(), args.spec_file))
        survey = ingest.SpectraParser(args.spec_file, args.spec_file_type, ms_level=1, native_precision=True, times=xic is not None).to_list()
        if purity is not None:
            purity["survey"] = survey
        if xic is not None:
            xic["survey"] = survey
    quant_channels = dict(named=(label_free(args),)) if label_free(args) else dict(mz=markers["mz"] if markers is not None else ())
    if ranked_rows is not None:
        from .ranked import check_k
        check_k(args.ranked_depth)
    rows = batch_cli.localize(ascore, psms, spectra, args.residues, args.mod_mass, args.hit_depth,
                              args.max_fragment_charge, args.mod_correction_tol, args.zero_based,
                              match_save=args.match_save, log=lambda m: log("{} -- {}".format(stamp(), m)),
                              evidence=args.evidence, ions=ion_rows, reported=args.reported, sites=site_rows,
                              probs=args.probs, ranked=ranked_rows, ranked_depth=args.ranked_depth, site_table=site_table_rows,
                              site_table_threshold=args.site_table_threshold, site_table_flr=args.site_table_flr,
                              site_table_decoys=args.site_table_decoys, peptidoform_table=peptidoform_rows,
                              peptidoform_threshold=args.peptidoform_threshold, mz_profile=profile, recalibrate=recalibrate,
                              deisotope=deisotope, decharge=decharge, strip=strip_request(args),
                              centroid=centroid_request(args), coverage=coverage_rows, markers=markers,
                              marker_rows=marker_rows, site_quant=site_quant, site_quant_rows=site_quant_rows,
                              peptidoform_quant=pform_quant, peptidoform_quant_rows=pform_quant_rows,
                              channels=channels_request(args), purity=purity, purity_rows=purity_rows, xic=xic, xic_rows=xic_rows)
    batch_cli.write_tsv(rows, args.out_file, evidence=args.evidence, reported=args.reported, sites=site_rows is not None,
                        probs=args.probs)
    if site_rows is not None:
        batch_cli.write_sites_tsv(site_rows, args.sites)
    if ranked_rows is not None:
        batch_cli.write_ranked_tsv(ranked_rows, args.ranked)
    if site_table_rows is not None:
        batch_cli.write_site_table_tsv(site_table_rows, args.site_table, flr=args.site_table_flr)
    if peptidoform_rows is not None:
        batch_cli.write_peptidoform_table_tsv(peptidoform_rows, args.peptidoform_table)
    if args.mz_profile:
        batch_cli.write_mz_profile_tsv(profile[0], profile[1], args.mz_profile)
        for line in batch_cli.mz_profile_report(profile[0], profile[1]):
            log("{} -- {}".format(stamp(), line))
    if args.mz_calibration_out:
        cal = ascore.fit_mz_calibration(profile[0], profile[1], min_ions=args.mz_calibration_min_ions)
        batch_cli.write_mz_calibration_tsv(cal, 1.0 / profile[1]["inv_band"], args.mz_calibration_out)
    if ion_rows is not None:
        batch_cli.write_ions_tsv(ion_rows, args.ions)
    if coverage_rows is not None:
        batch_cli.write_coverage_tsv(coverage_rows, args.coverage)
    if site_quant_rows is not None:
        batch_cli.write_site_quant_tsv(site_quant_rows, args.site_quant, **quant_channels)
    if pform_quant_rows is not None:
        batch_cli.write_peptidoform_quant_tsv(pform_quant_rows, args.peptidoform_quant, **quant_channels)
    if xic_rows is not None:
        batch_cli.write_xic_tsv(xic_rows, args.xic)
    if purity_rows is not None:
        batch_cli.write_purity_tsv(purity_rows, args.purity)
    if marker_rows is not None and args.markers:
        batch_cli.write_markers_tsv(marker_rows, args.markers, mz=markers["mz"], losses=markers["losses"])
    log("{} -- Ascore Completed".format(stamp()))
    return rows


def main(argv=None):
    run(parse_args(sys.argv[1:] if argv is None else argv))


if __name__ == "__main__":
    main()
