"""ctypes binding of include/pyascore_hip.h (libpyascore_hip.so, built in-tree by build.py).

There is no fallback: if the library is missing or no HIP device is usable, importing the
scorer fails loudly.
"""
import ctypes as C
import importlib.util
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PYA_LIB") or os.path.join(_HERE, "libpyascore_hip.so")   # PYA_LIB: A/B builds

PYA_OK, PYA_ERR_ARG, PYA_ERR_HIP, PYA_ERR_PSM, PYA_ERR_LIMIT, PYA_ERR_STATE = 0, -1, -2, -3, -4, -5
PYA_FLAG_KEEP, PYA_FLAG_TIMING, PYA_FLAG_SKIP_INVALID, PYA_FLAG_EVIDENCE, PYA_FLAG_IONS = 1, 2, 4, 8, 16
PYA_FLAG_NAMED = 32
PYA_FLAG_SITES = 64
PYA_FLAG_PROBS = 128
PYA_FLAG_RANKED = 256
PYA_FLAG_ROLLUP = 512
PYA_FLAG_PEPTIDOFORMS = 1024
PYA_FLAG_MZ_PROFILE = 2048
PYA_FLAG_RECALIBRATE = 4096
PYA_FLAG_COVERAGE = 8192
PYA_FLAG_QUANT = 16384
PYA_FLAG_PFORM_QUANT = 32768
PYA_QUANT_COMPLETE_ONLY = 1
PYA_QUANT_MAX_CHANNELS = 64
PYA_CHANNEL_NORMALIZE = 1
PYA_CHANNEL_TILE = 128       # rows per workgroup of csrc/channel_correct.hip
PYA_COV_NONE, PYA_COV_SCORED = 0, 1
PYA_MZC_MAX_PPM = 1000       # the largest knot of a pya_mz_calibration, in ppm
PYA_MZP_BANDS, PYA_MZP_BINS = 8, 64
PYA_MZP_CHUNK = 128          # PSMs per workgroup of csrc/mz_profile.hip
PYA_PFORM_TILE = 1024        # entries per workgroup and sort pass of csrc/peptidoforms.hip
PYA_PFORM_PHASES = 4         # (include/pyascore_debug.h: pya_debug_last_peptidoform_ms)
PYA_ROLLUP_NO_PSM = 0xFFFFFFFF
PYA_FLR_TARGET, PYA_FLR_DECOY, PYA_FLR_LEFT_OUT = 0, 1, 2
PYA_FLR_REPORTED_ONLY = 1
PYA_FLR_TILE = 1024          # slots per workgroup and sort pass of csrc/flr.hip
PYA_FLR_PHASES = 11          # (include/pyascore_debug.h: pya_debug_rollup_flr_timed)
# (include/pyascore_debug.h: the test-only calls on the device building blocks)
PYA_DEBUG_LOOKUP_MAX_N = 8192
(PYA_DBG_FASTDIV, PYA_DBG_CHARGE_MZ, PYA_DBG_NTH_SET_BIT, PYA_DBG_DEPOSIT_SITES, PYA_DBG_XCD_SLOT, PYA_DBG_NL_BUMP, PYA_DBG_LUT_ROW,
 PYA_DBG_HIST) = range(8)
(PYA_DBG_WAVE_SUM_U64, PYA_DBG_WAVE_MINMAX_F64, PYA_DBG_MARKER_LANE_F64, PYA_DBG_ION_SCAN_U64, PYA_DBG_HIST_WAVE_SUM,
 PYA_DBG_SAME_DIGIT) = range(6)
PYA_DBG_WAVE_IN, PYA_DBG_WAVE_OUT = 192, 4096
PYA_DBG_SCAN_ADD, PYA_DBG_SCAN_SEG = 0, 1
PYA_MAX_RANKED = 64
PYA_RANK_NONE, PYA_RANK_SCORED, PYA_RANK_OVER = 0, 1, 2
PYA_RANK_TIED_PREV, PYA_RANK_IN_BEST_TIE = 1, 2
PYA_SITE_NONE, PYA_SITE_SCORED, PYA_SITE_OVER = 0, 1, 2
PYA_SITE_IN_BEST, PYA_SITE_WITH_TIED, PYA_SITE_WITHOUT_TIED, PYA_SITE_NO_WITHOUT = 1, 2, 4, 8
PYA_FAST_SIGNATURES = 15000
PYA_NAMED_NONE, PYA_NAMED_INVALID, PYA_NAMED_WINNER, PYA_NAMED_TIED, PYA_NAMED_COUNTED = 0, 1, 2, 3, 4
PYA_EV_NONE, PYA_EV_COUNTED, PYA_EV_TIED = 0, 1, 2
PYA_ION_WINNER, PYA_ION_LOSS, PYA_ION_COMP, PYA_ION_COUNTED = 255, 1, 2, 4
PYA_MAX_PEPTIDE_LEN = 511

_vp = C.c_void_p


class Config(C.Structure):
    _fields_ = [("bin_size", C.c_float), ("n_top", C.c_uint32), ("mod_group", C.c_char_p),
                ("mod_mass", C.c_float), ("mz_error", C.c_float), ("fragment_types", C.c_char_p),
                ("device", C.c_int32)]


class Batch(C.Structure):
    _fields_ = [("n_psm", C.c_uint64), ("peak_off", _vp), ("pep", _vp), ("pep_off", _vp),
                ("n_of_mod", _vp), ("max_charge", _vp), ("aux_pos", _vp), ("aux_mass", _vp),
                ("aux_off", _vp)]


class Results(C.Structure):
    _fields_ = [("max_k", C.c_uint32), ("best_score", _vp), ("best_sig", _vp), ("n_sig", _vp),
                ("ascores", _vp), ("alt_mask", _vp)]


class TypedSpectra(C.Structure):
    """pya_typed_spectra: host (pya_score_batch_typed) or device (pya_plan_run_typed) arrays and their element types"""
    _fields_ = [("mz", _vp), ("intensity", _vp), ("mz_type", C.c_uint32), ("intensity_type", C.c_uint32)]


class Evidence(C.Structure):
    """pya_evidence: what stands behind one Ascore (depth, site-determining ion counts, the competitor)"""
    _fields_ = [("comp_score", C.c_float), ("comp_pos", C.c_uint16), ("depth", C.c_uint8), ("kind", C.c_uint8),
                ("ref_matched", C.c_uint16), ("ref_possible", C.c_uint16),
                ("comp_matched", C.c_uint16), ("comp_possible", C.c_uint16)]


assert C.sizeof(Evidence) == 16, "pya_evidence is a 16-byte record"
# the same record as a numpy structured dtype (a view on the C buffer, no copy)
EVIDENCE_DTYPE = [("comp_score", "<f4"), ("comp_pos", "<u2"), ("depth", "u1"), ("kind", "u1"),
                  ("ref_matched", "<u2"), ("ref_possible", "<u2"), ("comp_matched", "<u2"), ("comp_possible", "<u2")]


class Ion(C.Structure):
    """pya_ion: one matched fragment of the winner, or one site-determining ion of a counted pair"""
    _fields_ = [("theo_mz", C.c_float), ("peak_mz", C.c_float), ("size", C.c_uint16), ("type", C.c_uint8), ("charge", C.c_uint8),
                ("rank", C.c_uint8), ("site", C.c_uint8), ("flags", C.c_uint8), ("reserved", C.c_uint8)]


assert C.sizeof(Ion) == 16, "pya_ion is a 16-byte record"
ION_DTYPE = [("theo_mz", "<f4"), ("peak_mz", "<f4"), ("size", "<u2"), ("type", "u1"), ("charge", "u1"),
             ("rank", "u1"), ("site", "u1"), ("flags", "u1"), ("reserved", "u1")]


class Named(C.Structure):
    """pya_named: the score container of a localisation the caller named, and its ambiguity against the winner"""
    _fields_ = [("sig_bits", C.c_uint64), ("pep_score", C.c_float), ("ambiguity", C.c_float), ("total_fragments", C.c_uint32),
                ("kind", C.c_uint8), ("depth", C.c_uint8), ("n_moved", C.c_uint8), ("reserved", C.c_uint8),
                ("ref_matched", C.c_uint16), ("ref_possible", C.c_uint16),
                ("comp_matched", C.c_uint16), ("comp_possible", C.c_uint16)]


assert C.sizeof(Named) == 32, "pya_named is a 32-byte record"
NAMED_DTYPE = [("sig_bits", "<u8"), ("pep_score", "<f4"), ("ambiguity", "<f4"), ("total_fragments", "<u4"),
               ("kind", "u1"), ("depth", "u1"), ("n_moved", "u1"), ("reserved", "u1"),
               ("ref_matched", "<u2"), ("ref_possible", "<u2"), ("comp_matched", "<u2"), ("comp_possible", "<u2")]



class Site(C.Structure):
    """pya_site: the best PepScore with and without one modifiable residue, and the site assignments that attain them"""
    _fields_ = [("with_sig", C.c_uint64), ("without_sig", C.c_uint64), ("with_score", C.c_float), ("without_score", C.c_float),
                ("pos", C.c_uint16), ("kind", C.c_uint8), ("flags", C.c_uint8), ("reserved", C.c_uint32)]


assert C.sizeof(Site) == 32, "pya_site is a 32-byte record"
SITE_DTYPE = [("with_sig", "<u8"), ("without_sig", "<u8"), ("with_score", "<f4"), ("without_score", "<f4"),
              ("pos", "<u2"), ("kind", "u1"), ("flags", "u1"), ("reserved", "<u4")]


class SiteProb(C.Structure):
    """pya_site_prob: the posterior probability that one modifiable residue is modified, and that it is not"""
    _fields_ = [("with_prob", C.c_double), ("without_prob", C.c_double)]


class PsmProb(C.Structure):
    """pya_psm_prob: the sum of the likelihood ratios of a PSM's site assignments against the winner (1 / z: its posterior)"""
    _fields_ = [("z", C.c_double), ("n_summed", C.c_uint32), ("kind", C.c_uint8), ("pad", C.c_uint8 * 3)]


assert C.sizeof(SiteProb) == 16 and C.sizeof(PsmProb) == 16, "pya_site_prob and pya_psm_prob are 16-byte records"
SITE_PROB_DTYPE = [("with_prob", "<f8"), ("without_prob", "<f8")]
PSM_PROB_DTYPE = [("z", "<f8"), ("n_summed", "<u4"), ("kind", "u1"), ("pad", "u1", (3,))]


class Ranked(C.Structure):
    """pya_ranked: one row of a PSM's ranked localisations -- a site assignment, its PepScore, its rank"""
    _fields_ = [("sig_bits", C.c_uint64), ("pep_score", C.c_float), ("rank", C.c_uint16), ("kind", C.c_uint8), ("flags", C.c_uint8)]


assert C.sizeof(Ranked) == 16, "pya_ranked is a 16-byte record"
RANKED_DTYPE = [("sig_bits", "<u8"), ("pep_score", "<f4"), ("rank", "<u2"), ("kind", "u1"), ("flags", "u1")]


class SiteRollup(C.Structure):
    """pya_site_rollup: one slot of a site roll-up -- the best localisation probability any PSM gives a site, who gives it,
    how many PSMs cover it, how many confidently, how many report it, and the best Ascore of those"""
    _fields_ = [("best_prob", C.c_double), ("best_psm", C.c_uint32), ("n_psm", C.c_uint32), ("n_confident", C.c_uint32),
                ("n_in_best", C.c_uint32), ("best_ascore", C.c_float), ("reserved", C.c_uint32)]


assert C.sizeof(SiteRollup) == 32, "pya_site_rollup is a 32-byte record"
ROLLUP_DTYPE = [("best_prob", "<f8"), ("best_psm", "<u4"), ("n_psm", "<u4"), ("n_confident", "<u4"), ("n_in_best", "<u4"),
                ("best_ascore", "<f4"), ("reserved", "<u4")]


class SiteFlr(C.Structure):
    """pya_site_flr: one slot of a roll-up table under the cut "this site and everything at least as good" -- how many
    ranked sites, how many decoys among them, their summed expected error, the model FLR and the decoy q-value"""
    _fields_ = [("rank", C.c_uint32), ("n_decoy", C.c_uint32), ("err_sum", C.c_uint64), ("flr", C.c_double), ("decoy_q", C.c_double)]


assert C.sizeof(SiteFlr) == 32, "pya_site_flr is a 32-byte record"


class SiteQuantParams(C.Structure):
    """pya_site_quant_params: the probability a record needs to contribute, the power of two a reading is scaled by, the
    channels of the matrix and the table, PYA_QUANT_COMPLETE_ONLY or 0"""
    _fields_ = [("threshold", C.c_double), ("scale_log2", C.c_int32), ("n_channels", C.c_uint32), ("flags", C.c_uint32),
                ("reserved", C.c_uint32)]


assert C.sizeof(SiteQuantParams) == 24, "pya_site_quant_params is a 24-byte record"
SITE_QUANT_HEAD_DTYPE = [("n_records", "<u4"), ("n_complete", "<u4")]
SITE_QUANT_DTYPE = [("sum", "<u8"), ("n", "<u4"), ("n_saturated", "<u4")]


class Peptidoform(C.Structure):
    """pya_peptidoform: one localised peptidoform -- a peptide (the caller's group) with one site assignment: how many PSMs
    report it, how many confidently, the best of their minimum site probabilities and who has it, the best posterior
    (1 / best_z), the best minimum Ascore, and how many assignments the peptide was seen with"""
    _fields_ = [("sig_bits", C.c_uint64), ("group", C.c_uint32), ("n_psm", C.c_uint32), ("n_confident", C.c_uint32), ("best_psm", C.c_uint32),
                ("best_min_prob", C.c_double), ("best_z", C.c_double), ("best_min_ascore", C.c_float), ("n_isomers", C.c_uint32)]


assert C.sizeof(Peptidoform) == 48, "pya_peptidoform is a 48-byte record"
PEPTIDOFORM_DTYPE = [("sig_bits", "<u8"), ("group", "<u4"), ("n_psm", "<u4"), ("n_confident", "<u4"), ("best_psm", "<u4"),
                     ("best_min_prob", "<f8"), ("best_z", "<f8"), ("best_min_ascore", "<f4"), ("n_isomers", "<u4")]
FLR_DTYPE = [("rank", "<u4"), ("n_decoy", "<u4"), ("err_sum", "<u8"), ("flr", "<f8"), ("decoy_q", "<f8")]


class MzProfileParams(C.Structure):
    """pya_mz_profile_params: bins per Da, bins per ppm, bands per m/z unit, the deepest peak rank counted"""
    _fields_ = [("inv_da", C.c_double), ("inv_ppm", C.c_double), ("inv_band", C.c_double), ("max_rank", C.c_uint32),
                ("reserved", C.c_uint32)]


assert C.sizeof(MzProfileParams) == 32, "pya_mz_profile_params is a 32-byte record"
MZ_PROFILE_DTYPE = [("n_psm", "<u4"), ("n_ions", "<u4"), ("n_rank_skipped", "<u4"), ("out_da", "<u4", (2,)), ("out_ppm", "<u4", (2,)),
                    ("reserved", "<u4"), ("da", "<u4", (PYA_MZP_BANDS, PYA_MZP_BINS)), ("ppm", "<u4", (PYA_MZP_BANDS, PYA_MZP_BINS))]
MZ_CALIBRATION_DTYPE = [("ppm", "<f8", (PYA_MZP_BANDS,)), ("spread_ppm", "<f4", (PYA_MZP_BANDS,)), ("n_signal", "<u4", (PYA_MZP_BANDS,))]


class Coverage(C.Structure):
    """pya_coverage: how much of its spectrum the reported localisation of one PSM explains"""
    _fields_ = [("total_current", C.c_double), ("explained_current", C.c_double), ("nterm_current", C.c_double),
                ("cterm_current", C.c_double), ("n_peaks", C.c_uint32), ("n_retained", C.c_uint32), ("n_explained", C.c_uint32),
                ("n_fragments", C.c_uint32), ("nterm_sizes", C.c_uint16), ("cterm_sizes", C.c_uint16), ("nterm_run", C.c_uint16),
                ("cterm_run", C.c_uint16), ("bonds", C.c_uint16), ("kind", C.c_uint8), ("pad", C.c_uint8 * 5)]


assert C.sizeof(Coverage) == 64 and Coverage.n_peaks.offset == 32 and Coverage.nterm_sizes.offset == 48 and Coverage.bonds.offset == 56 and \
    Coverage.kind.offset == 58 and Coverage.pad.offset == 59, "pya_coverage is a 64-byte record"
COVERAGE_DTYPE = [("total_current", "<f8"), ("explained_current", "<f8"), ("nterm_current", "<f8"), ("cterm_current", "<f8"),
                  ("n_peaks", "<u4"), ("n_retained", "<u4"), ("n_explained", "<u4"), ("n_fragments", "<u4"),
                  ("nterm_sizes", "<u2"), ("cterm_sizes", "<u2"), ("nterm_run", "<u2"), ("cterm_run", "<u2"), ("bonds", "<u2"),
                  ("kind", "u1"), ("pad", "u1", (5,))]

PYA_F64, PYA_F32 = 0, 1

PYA_DEISO_MAX_CHARGE = 8


class DeisotopeParams(C.Structure):
    """pya_deisotope_params: the match width, the intensity ratio, the isotope spacing per charge, the largest charge"""
    _fields_ = [("tol", C.c_double), ("ratio0", C.c_double), ("ratio_per_mz", C.c_double), ("spacing", C.c_double * PYA_DEISO_MAX_CHARGE),
                ("max_charge", C.c_uint32), ("reserved", C.c_uint32)]


assert C.sizeof(DeisotopeParams) == 96, "pya_deisotope_params is a 96-byte record"

PYA_DECHARGE_CARRIER = 1.007825


class DechargeParams(C.Structure):
    """pya_decharge_params: the deisotoping rule, the mass of one charge carrier, the least share of a witness"""
    _fields_ = [("iso", DeisotopeParams), ("carrier", C.c_double), ("witness", C.c_double)]


assert C.sizeof(DechargeParams) == 112, "pya_decharge_params is a 112-byte record"

PYA_STRIP_MAX_CHARGE = 8
PYA_STRIP_MAX_LOSS = 7
PYA_STRIP_MAX_ISOTOPES = 4
PYA_STRIP_STEP = 1.0033548378


class StripParams(C.Structure):
    """pya_strip_params: the half width of a window, the isotope spacing, the range cut, the neutral losses ([0] is 0.0) and
    how many of them, charge-reduced precursors or not, the isotope peaks a window covers"""
    _fields_ = [("tol", C.c_double), ("step", C.c_double), ("mz_lo", C.c_double), ("mz_hi", C.c_double),
                ("loss", C.c_double * (PYA_STRIP_MAX_LOSS + 1)), ("n_loss", C.c_uint32), ("reduced", C.c_uint32), ("isotopes", C.c_uint32),
                ("reserved", C.c_uint32)]


assert C.sizeof(StripParams) == 112, "pya_strip_params is a 112-byte record"


class StripReport(C.Structure):
    """pya_strip_report: which windows of a spectrum held a peak, the peaks removed, the active windows"""
    _fields_ = [("hit", C.c_uint64), ("n_removed", C.c_uint32), ("n_windows", C.c_uint32)]


assert C.sizeof(StripReport) == 16, "pya_strip_report is a 16-byte record"
STRIP_REPORT_DTYPE = [("hit", "<u8"), ("n_removed", "<u4"), ("n_windows", "<u4")]

PYA_MARKER_MAX_TARGETS = 64
PYA_MARKER_ACTIVE = 1
PYA_MARKER_PICKED = 2


class MarkerParams(C.Structure):
    """pya_marker_params: the half width of a window in Da and in ppm of its centre, the value of every target (a fixed m/z, or
    the neutral mass taken off the precursor), which targets are relative to the precursor, and how many targets there are"""
    _fields_ = [("tol", C.c_double), ("tol_ppm", C.c_double), ("value", C.c_double * PYA_MARKER_MAX_TARGETS), ("loss_mask", C.c_uint64),
                ("n_targets", C.c_uint32), ("reserved", C.c_uint32)]


assert C.sizeof(MarkerParams) == 544, "pya_marker_params is a 544-byte record"


class Marker(C.Structure):
    """pya_marker: the peak a target picked in a spectrum, the peaks inside its window, whether it was active and picked"""
    _fields_ = [("mz", C.c_double), ("intensity", C.c_double), ("n_peaks", C.c_uint32), ("flags", C.c_uint32)]


assert C.sizeof(Marker) == 24, "pya_marker is a 24-byte record"
MARKER_DTYPE = [("mz", "<f8"), ("intensity", "<f8"), ("n_peaks", "<u4"), ("flags", "<u4")]


class MarkerSpectrum(C.Structure):
    """pya_marker_spectrum: the ion current and the base peak of a spectrum, which targets picked a peak, the peaks of the
    spectrum and its active targets"""
    _fields_ = [("tic", C.c_double), ("base_peak", C.c_double), ("hit", C.c_uint64), ("n_peaks", C.c_uint32), ("n_active", C.c_uint32)]


assert C.sizeof(MarkerSpectrum) == 32, "pya_marker_spectrum is a 32-byte record"
MARKER_SPECTRUM_DTYPE = [("tic", "<f8"), ("base_peak", "<f8"), ("hit", "<u8"), ("n_peaks", "<u4"), ("n_active", "<u4")]

PYA_PURITY_MAX_CENTRES = 16
PYA_PURITY_MAX_BELOW = 4
PYA_PURITY_ACTIVE = 1
PYA_PURITY_SEEN = 2


class PurityParams(C.Structure):
    """pya_purity_params: the half width of a centre's window in Da and in ppm of the centre, the isotope spacing at charge 1,
    the isotope positions under and above the selected m/z"""
    _fields_ = [("tol", C.c_double), ("tol_ppm", C.c_double), ("step", C.c_double), ("below", C.c_uint32), ("isotopes", C.c_uint32),
                ("reserved", C.c_uint32 * 2)]


assert C.sizeof(PurityParams) == 40, "pya_purity_params is a 40-byte record"


class Purity(C.Structure):
    """pya_purity: the eligible and the precursor intensity of an isolation window, the most intense other peak, the counts,
    which centres held a peak, whether the query was active and its precursor seen"""
    _fields_ = [("window", C.c_double), ("precursor", C.c_double), ("other_mz", C.c_double), ("other_intensity", C.c_double),
                ("n_window", C.c_uint32), ("n_precursor", C.c_uint32), ("iso_hit", C.c_uint32), ("flags", C.c_uint32)]


assert C.sizeof(Purity) == 48, "pya_purity is a 48-byte record"
PURITY_DTYPE = [("window", "<f8"), ("precursor", "<f8"), ("other_mz", "<f8"), ("other_intensity", "<f8"), ("n_window", "<u4"),
                ("n_precursor", "<u4"), ("iso_hit", "<u4"), ("flags", "<u4")]

PYA_XIC_MAX_SCANS = 64
PYA_XIC_MAX_ISOTOPES = 3
PYA_XIC_MAX_GAP = 8
PYA_XIC_ACTIVE, PYA_XIC_SEEN, PYA_XIC_SEED_PRESENT, PYA_XIC_LEFT_VALLEY = 1, 2, 4, 8
PYA_XIC_RIGHT_VALLEY, PYA_XIC_UNSORTED, PYA_XIC_LEFT_OPEN, PYA_XIC_RIGHT_OPEN = 16, 32, 64, 128
PYA_XIC_AREA, PYA_XIC_APEX, PYA_XIC_SEED, PYA_XIC_SUM = 0, 1, 2, 3


class XicParams(C.Structure):
    """pya_xic_params: the half width of an isotope's window in Da and in ppm of its centre, the isotope spacing at charge 1, the
    valley rule's rise, the isotope positions above the selected m/z and the absent scans a trace may bridge"""
    _fields_ = [("tol", C.c_double), ("tol_ppm", C.c_double), ("step", C.c_double), ("rise", C.c_double), ("isotopes", C.c_uint32),
                ("max_gap", C.c_uint32)]


assert C.sizeof(XicParams) == 40, "pya_xic_params is a 40-byte record"


class Xic(C.Structure):
    """pya_xic: area, apex, seed and summed intensity of a precursor's chromatographic peak, its apex, bounds and start as survey
    indices, the present scans of the peak and of the window, the isotopes seen at the apex, the flags"""
    _fields_ = [("area", C.c_double), ("apex_intensity", C.c_double), ("seed_intensity", C.c_double), ("sum_intensity", C.c_double),
                ("apex_scan", C.c_uint32), ("left_scan", C.c_uint32), ("right_scan", C.c_uint32), ("start_scan", C.c_uint32),
                ("n_points", C.c_uint32), ("n_present", C.c_uint32), ("iso_hit", C.c_uint32), ("flags", C.c_uint32)]


assert C.sizeof(Xic) == 64, "pya_xic is a 64-byte record"
XIC_DTYPE = [("area", "<f8"), ("apex_intensity", "<f8"), ("seed_intensity", "<f8"), ("sum_intensity", "<f8"), ("apex_scan", "<u4"),
             ("left_scan", "<u4"), ("right_scan", "<u4"), ("start_scan", "<u4"), ("n_points", "<u4"), ("n_present", "<u4"),
             ("iso_hit", "<u4"), ("flags", "<u4")]

PYA_CENTROID_MAX_HALF_WIDTH = 8


class CentroidParams(C.Structure):
    """pya_centroid_params: the largest distance of two points of one peak (a constant and a share of the m/z), the least
    height of an apex, the points on either side a centroid takes in, apex height or summed area"""
    _fields_ = [("gap0", C.c_double), ("gap_per_mz", C.c_double), ("min_height", C.c_double), ("half_width", C.c_uint32),
                ("area", C.c_uint32), ("reserved", C.c_uint64)]


assert C.sizeof(CentroidParams) == 40, "pya_centroid_params is a 40-byte record"


def spectrum_type(dtype):
    """PYA_F64 / PYA_F32 for a numpy dtype (or its name: 'float64', 'float32'); anything else is no spectrum type."""
    name = getattr(dtype, "name", None) or str(dtype).replace("torch.", "")
    try:
        return {"float64": PYA_F64, "float32": PYA_F32}[name]
    except KeyError:
        raise ValueError("spectrum arrays are float64 or float32, not %s" % name) from None


# every symbol include/pyascore_hip.h declares
SYMBOLS = {
    "pya_create": (C.c_int, [C.POINTER(Config), C.POINTER(_vp)]),
    "pya_destroy": (None, [_vp]),
    "pya_add_neutral_loss": (C.c_int, [_vp, C.c_char_p, C.c_float]),
    "pya_reload_env": (C.c_int, [_vp]),
    "pya_set_debug": (C.c_int, [_vp, C.c_char_p, C.c_char_p]),          # include/pyascore_debug.h (test-only)
    "pya_debug_wave_ops": (C.c_int, [_vp, _vp, _vp]),         # (test-only)
    "pya_debug_last_chunks": (C.c_uint64, [_vp]),             # (test-only)
    "pya_debug_lookup": (C.c_int, [_vp, _vp, _vp, C.c_uint32, C.c_float, _vp, C.c_uint32, _vp, _vp]),   # (test-only)
    "pya_debug_lane_ops": (C.c_int, [_vp, C.c_uint32, _vp, _vp, C.c_uint64, _vp]),             # (test-only)
    "pya_debug_wave64": (C.c_int, [_vp, C.c_uint32, _vp, _vp]),                                # (test-only)
    "pya_debug_block_scan": (C.c_int, [_vp, C.c_uint32, _vp, _vp]),                            # (test-only)
    "pya_debug_ts_scan": (C.c_int, [_vp, C.c_uint32, _vp, C.c_uint64]),                        # (test-only)
    "pya_debug_ions_scan": (C.c_int, [_vp, _vp, C.c_uint32]),                                  # (test-only)
    "pya_debug_table_sizes": (C.c_int, [_vp, _vp]),           # (test-only)
    "pya_debug_span_guard": (C.c_int, [_vp, C.c_char_p, C.c_uint64, _vp, _vp, C.c_uint64, _vp]),   # (test-only)
    "pya_debug_bin_keys": (C.c_int, [_vp, _vp, C.c_uint64, _vp, _vp]),             # (test-only)
    "pya_debug_last_probs_launch": (C.c_int, [_vp, _vp, _vp]),        # (test-only)
    "pya_debug_last_ranked_launch": (C.c_int, [_vp, _vp, _vp]),       # (test-only)
    "pya_debug_last_rollup_launch": (C.c_int, [_vp, _vp, _vp]),       # (test-only)
    "pya_debug_signature_list": (C.c_int, [_vp, C.c_uint64, _vp, C.c_uint64, _vp]),   # (test-only)
    "pya_debug_plan_retained_table": (C.c_int, [_vp, C.c_uint64, _vp, _vp, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_int32)]),  # (test-only)
    "pya_debug_retained_table": (C.c_int, [_vp, C.c_uint64, _vp, _vp, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_int32)]),  # (test-only)
    "pya_score_one": (C.c_int, [_vp, _vp, _vp, C.c_uint64, _vp, C.c_uint64, C.c_int32, C.c_int32, _vp, _vp, C.c_uint64,
                                C.c_uint32, C.POINTER(Results)]),
    "pya_rescore_last_keep": (C.c_int, [_vp]),
    "pya_last_error": (C.c_char_p, [_vp]),
    "pya_error_index": (C.c_int64, [_vp]),
    "pya_score_batch": (C.c_int, [_vp, C.POINTER(Batch), _vp, _vp, C.c_uint32, C.POINTER(Results)]),
    "pya_score_batch_shared": (C.c_int, [_vp, C.POINTER(Batch), _vp, C.c_uint64, _vp, _vp, C.c_uint32, C.POINTER(Results)]),
    "pya_score_batch_typed": (C.c_int, [_vp, C.POINTER(Batch), _vp, C.c_uint64, C.POINTER(TypedSpectra), C.c_uint32, C.POINTER(Results)]),
    "pya_score_batch_named": (C.c_int, [_vp, C.POINTER(Batch), _vp, C.c_uint64, C.POINTER(TypedSpectra), C.c_uint32, C.POINTER(Results),
                                        _vp, _vp, _vp, _vp, _vp]),
    "pya_plan_named": (C.c_int, [_vp, C.POINTER(Results), _vp, _vp, _vp, C.c_uint64, _vp, _vp, _vp]),
    "pya_plan_run_typed": (C.c_int, [_vp, C.POINTER(TypedSpectra), _vp, C.POINTER(Results)]),
    "pya_set_workspace_budget": (C.c_int, [_vp, C.c_uint64]),
    "pya_get_workspace_budget": (C.c_uint64, [_vp]),
    "pya_last_batch_status": (C.c_int, [_vp, _vp, C.c_uint64]),
    "pya_last_batch_evidence": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint32]),
    "pya_plan_evidence": (C.c_int, [_vp, C.POINTER(Results), _vp, _vp]),
    "pya_last_batch_ions": (C.c_int, [_vp, _vp, _vp, C.c_uint64]),
    "pya_plan_ions_count": (C.c_int, [_vp, C.POINTER(Results), _vp, _vp]),
    "pya_plan_ions": (C.c_int, [_vp, C.POINTER(Results), _vp, _vp, _vp, C.c_uint64]),
    "pya_last_batch_sites": (C.c_int, [_vp, _vp, _vp, C.c_uint64]),
    "pya_set_site_sig_cap": (C.c_int, [_vp, C.c_uint32]),
    "pya_get_site_sig_cap": (C.c_uint32, [_vp]),
    "pya_plan_site_offsets": (C.c_int, [_vp, _vp]),
    "pya_plan_sites": (C.c_int, [_vp, C.POINTER(Results), _vp, C.c_uint32, _vp]),
    "pya_last_batch_probs": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint64]),
    "pya_plan_probs": (C.c_int, [_vp, C.POINTER(Results), _vp, C.c_uint32, _vp, _vp]),
    "pya_last_batch_ranked": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint32]),
    "pya_set_ranked_k": (C.c_int, [_vp, C.c_uint32]),
    "pya_get_ranked_k": (C.c_uint32, [_vp]),
    "pya_plan_ranked": (C.c_int, [_vp, C.POINTER(Results), _vp, C.c_uint32, C.c_uint32, _vp]),
    "pya_set_rollup": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint64, C.c_double, _vp]),
    "pya_last_batch_rollup": (C.c_int, [_vp, _vp, C.c_uint64]),
    "pya_rollup_clear": (C.c_int, [_vp, _vp, C.c_uint64, _vp]),
    "pya_plan_rollup": (C.c_int, [_vp, C.POINTER(Results), _vp, _vp, _vp, _vp, C.c_uint64, C.c_double, _vp, C.c_uint32, _vp]),
    "pya_set_peptidoforms": (C.c_int, [_vp, _vp, C.c_uint64, C.c_double, _vp]),
    "pya_last_batch_peptidoforms": (C.c_int, [_vp, _vp, C.c_uint64, _vp]),
    "pya_set_mz_profile": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint64, _vp]),
    "pya_last_batch_mz_profile": (C.c_int, [_vp, _vp, C.c_uint64]),
    "pya_plan_mz_profile": (C.c_int, [_vp, C.POINTER(Results), _vp, _vp, C.c_uint64, _vp, _vp]),
    "pya_set_site_quant": (C.c_int, [_vp, _vp, C.c_uint64, _vp, C.c_uint64, _vp]),
    "pya_last_batch_site_quant": (C.c_int, [_vp, _vp, _vp, C.c_uint64, C.c_uint32]),
    "pya_plan_site_quant": (C.c_int, [_vp, C.POINTER(Results), _vp, _vp, _vp, _vp, C.c_uint64, _vp, C.c_uint64, _vp, C.c_uint32, _vp, _vp, _vp]),
    "pya_marker_values": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint32, C.c_uint64, _vp, _vp]),
    "pya_channel_correct": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint32, _vp, _vp, _vp, _vp]),
    "pya_channel_sums": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint32, _vp, C.c_int32, _vp, _vp]),
    "pya_channel_factors": (C.c_int, [_vp, _vp, C.c_uint32, _vp, _vp]),
    "pya_channel_correct_host": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint32, _vp, _vp, C.c_int32, C.c_uint32, _vp, _vp, _vp]),
    "pya_set_peptidoform_quant": (C.c_int, [_vp, _vp, C.c_uint64, _vp, C.c_uint64, _vp]),
    "pya_last_batch_peptidoform_quant": (C.c_int, [_vp, _vp, _vp, C.c_uint64, C.c_uint32]),
    "pya_peptidoform_quant_workspace_bytes": (C.c_uint64, [C.c_uint64, C.c_uint32]),
    "pya_peptidoform_quant_reduce": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint64, _vp, _vp, _vp, C.c_uint64, C.c_uint32, _vp, _vp, C.c_uint64,
                                               _vp, _vp, _vp, C.c_uint64, _vp]),
    "pya_peptidoform_quant_reduce_host": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint64, _vp, _vp, _vp, C.c_uint64, C.c_uint32, _vp, _vp, _vp,
                                                    C.c_uint64, _vp]),
    "pya_plan_peptidoform_quant": (C.c_int, [_vp, C.POINTER(Results), _vp, _vp, _vp, _vp, C.c_double, _vp, C.c_uint32, _vp, _vp, _vp,
                                             C.c_uint64, _vp, C.c_uint64, _vp, C.c_uint32, _vp, _vp, C.c_uint64, _vp, _vp, _vp, C.c_uint64,
                                             _vp]),
    "pya_last_batch_coverage": (C.c_int, [_vp, _vp, C.c_uint64]),
    "pya_plan_coverage": (C.c_int, [_vp, C.POINTER(Results), C.POINTER(TypedSpectra), _vp, _vp]),
    "pya_mz_profile_fit": (C.c_int, [_vp, _vp, C.c_uint64, _vp, C.c_uint32, _vp, _vp]),
    "pya_mz_profile_fit_host": (C.c_int, [_vp, _vp, C.c_uint64, _vp, C.c_uint32, _vp]),
    "pya_recalibrate_spectra": (C.c_int, [_vp, C.POINTER(TypedSpectra), _vp, C.c_uint64, _vp, _vp, C.c_uint64, C.c_double, _vp, _vp, _vp]),
    "pya_set_recalibration": (C.c_int, [_vp, _vp, C.c_uint64, _vp, C.c_uint64, C.c_double]),
    "pya_deisotope_workspace_bytes": (C.c_uint64, [C.c_uint64, C.c_uint64]),
    "pya_deisotope_spectra": (C.c_int, [_vp, C.POINTER(TypedSpectra), _vp, C.c_uint64, C.POINTER(DeisotopeParams), _vp, _vp, C.c_uint64,
                                        C.POINTER(TypedSpectra), _vp, _vp]),
    "pya_deisotope_spectra_host": (C.c_int, [_vp, C.POINTER(TypedSpectra), _vp, C.c_uint64, C.POINTER(DeisotopeParams),
                                             C.POINTER(TypedSpectra), _vp, _vp]),
    "pya_decharge_workspace_bytes": (C.c_uint64, [C.c_uint64, C.c_uint64]),
    "pya_decharge_spectra": (C.c_int, [_vp, C.POINTER(TypedSpectra), _vp, C.c_uint64, C.POINTER(DechargeParams), _vp, _vp, C.c_uint64,
                                       C.POINTER(TypedSpectra), _vp, _vp, _vp]),
    "pya_decharge_spectra_host": (C.c_int, [_vp, C.POINTER(TypedSpectra), _vp, C.c_uint64, C.POINTER(DechargeParams),
                                            C.POINTER(TypedSpectra), _vp, _vp, _vp]),
    "pya_debug_decharge_passes": (None, [C.c_uint32]),
    "pya_strip_workspace_bytes": (C.c_uint64, [C.c_uint64, C.c_uint64]),
    "pya_strip_spectra": (C.c_int, [_vp, C.POINTER(TypedSpectra), _vp, C.c_uint64, _vp, _vp, C.POINTER(StripParams), _vp, _vp, C.c_uint64,
                                    C.POINTER(TypedSpectra), _vp, _vp, _vp]),
    "pya_strip_spectra_host": (C.c_int, [_vp, C.POINTER(TypedSpectra), _vp, C.c_uint64, _vp, _vp, C.POINTER(StripParams),
                                         C.POINTER(TypedSpectra), _vp, _vp, _vp]),
    "pya_marker_spectra": (C.c_int, [_vp, C.POINTER(TypedSpectra), _vp, C.c_uint64, C.c_uint64, _vp, _vp, C.POINTER(MarkerParams), _vp, _vp, _vp,
                                     _vp]),
    "pya_marker_spectra_host": (C.c_int, [_vp, C.POINTER(TypedSpectra), _vp, C.c_uint64, _vp, _vp, C.POINTER(MarkerParams), _vp, _vp, _vp]),
    "pya_purity_spectra": (C.c_int, [_vp, C.POINTER(TypedSpectra), _vp, C.c_uint64, C.c_uint64, _vp, _vp, _vp, _vp, _vp, C.c_uint64,
                                     C.POINTER(PurityParams), _vp, _vp, _vp]),
    "pya_purity_spectra_host": (C.c_int, [_vp, C.POINTER(TypedSpectra), _vp, C.c_uint64, _vp, _vp, _vp, _vp, _vp, C.c_uint64,
                                          C.POINTER(PurityParams), _vp, _vp]),
    "pya_purity_gate": (C.c_int, [_vp, _vp, C.c_uint64, C.c_double, C.c_uint32, _vp, C.c_uint32, _vp, _vp, _vp]),
    "pya_xic_survey_check": (C.c_int, [_vp, C.POINTER(TypedSpectra), _vp, C.c_uint64, C.c_uint64, _vp, _vp]),
    "pya_xic_spectra": (C.c_int, [_vp, C.POINTER(TypedSpectra), _vp, C.c_uint64, C.c_uint64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_uint64,
                                  C.POINTER(XicParams), _vp, _vp, _vp]),
    "pya_xic_spectra_host": (C.c_int, [_vp, C.POINTER(TypedSpectra), _vp, C.c_uint64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_uint64,
                                       C.POINTER(XicParams), _vp, _vp]),
    "pya_xic_values": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint32, _vp, _vp]),
    "pya_centroid_workspace_bytes": (C.c_uint64, [C.c_uint64, C.c_uint64]),
    "pya_centroid_spectra": (C.c_int, [_vp, C.POINTER(TypedSpectra), _vp, C.c_uint64, _vp, C.POINTER(CentroidParams), _vp, _vp, C.c_uint64,
                                       C.POINTER(TypedSpectra), _vp, _vp]),
    "pya_centroid_spectra_host": (C.c_int, [_vp, C.POINTER(TypedSpectra), _vp, C.c_uint64, _vp, C.POINTER(CentroidParams),
                                            C.POINTER(TypedSpectra), _vp, _vp]),
    "pya_debug_centroid_passes": (None, [C.c_uint32]),
    "pya_peptidoform_workspace_bytes": (C.c_uint64, [C.c_uint64]),
    "pya_peptidoform_reduce": (C.c_int, [_vp, _vp, C.c_uint64, _vp, C.c_uint64, _vp, _vp, C.c_uint64, _vp, C.c_uint64, _vp]),
    "pya_peptidoform_reduce_host": (C.c_int, [_vp, _vp, C.c_uint64, _vp, C.c_uint64, _vp, C.c_uint64, _vp]),
    "pya_plan_peptidoforms": (C.c_int, [_vp, C.POINTER(Results), _vp, _vp, _vp, _vp, C.c_double, _vp, C.c_uint32, _vp, C.c_uint64, _vp,
                                        C.c_uint64, _vp, C.c_uint64, _vp]),
    "pya_debug_peptidoform_timing": (C.c_int, [_vp, C.c_int]),        # (test-only)
    "pya_debug_last_peptidoform_ms": (C.c_int, [_vp, _vp]),           # (test-only)
    "pya_flr_workspace_bytes": (C.c_uint64, [C.c_uint64]),
    "pya_rollup_flr": (C.c_int, [_vp, _vp, C.c_uint64, _vp, C.c_uint32, _vp, _vp, C.c_uint64, _vp, _vp, _vp]),
    "pya_rollup_flr_host": (C.c_int, [_vp, _vp, C.c_uint64, _vp, C.c_uint32, _vp, _vp, _vp]),
    "pya_debug_rollup_flr_timed": (C.c_int, [_vp, _vp, C.c_uint64, _vp, C.c_uint32, _vp, _vp, C.c_uint64, _vp, _vp, _vp, _vp]),   # (test-only)
    "pya_plan_create": (C.c_int, [_vp, C.POINTER(Batch), C.c_uint32, C.POINTER(_vp)]),
    "pya_plan_create_shared": (C.c_int, [_vp, C.POINTER(Batch), _vp, C.c_uint64, C.c_uint32, C.POINTER(_vp)]),
    "pya_plan_run": (C.c_int, [_vp, _vp, _vp, _vp, C.POINTER(Results)]),
    "pya_plan_timings": (C.c_int, [_vp, C.POINTER(C.c_float * 4)]),
    "pya_one_times": (C.c_int, [_vp, C.POINTER(C.c_double * 12)]),
    "pya_plan_timings_sum": (C.c_int, [_vp, C.POINTER(C.c_double * 4), C.POINTER(C.c_uint32)]),
    "pya_plan_check": (C.c_int, [_vp]),
    "pya_pack_records": (C.c_int, [_vp, C.POINTER(Results), C.c_uint64, C.c_uint32, _vp, _vp]),
    "pya_plan_workspace_bytes": (C.c_uint64, [_vp]),
    "pya_plan_total_signatures": (C.c_uint64, [_vp]),
    "pya_plan_destroy": (None, [_vp]),
    "pya_get_pep_scores": (C.c_int, [_vp, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), _vp, _vp,
                                     _vp, _vp, _vp]),
    "pya_get_pep_scores_range": (C.c_int, [_vp, C.c_uint64, C.c_uint64, C.c_uint64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pya_calculate_ambiguity": (C.c_int, [_vp, C.c_uint64, C.c_uint64, _vp, C.c_float, C.c_uint64,
                                          _vp, C.c_float, C.POINTER(C.c_float)]),
    "pya_format_peptide": (C.c_int, [_vp, _vp, C.c_uint64, C.c_int32, _vp, _vp, C.c_uint64,
                                     C.c_uint64, C.c_int32, C.c_char_p, C.c_uint64]),
    "pya_format_peptides": (C.c_int, [_vp, C.POINTER(Batch), C.c_uint64, _vp, _vp, _vp, _vp, _vp, C.c_uint64]),
    "pya_count_sites": (C.c_int, [_vp, _vp, C.c_uint64, C.POINTER(C.c_int32), _vp]),
    "pya_debug_sort": (C.c_int, [_vp, _vp, C.c_uint32, _vp]),
    "pya_version": (C.c_char_p, []),
    # include/pyascore_aux.h
    "pya_spectra_create": (_vp, [C.c_float, C.c_uint64]),
    "pya_spectra_destroy": (None, [_vp]),
    "pya_spectra_consume": (C.c_int, [_vp, _vp, _vp, C.c_uint64]),
    "pya_spectra_info": (None, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "pya_spectra_window_size": (C.c_int64, [_vp, C.c_uint64]),
    "pya_spectra_peak": (C.c_int, [_vp, C.c_uint64, C.c_uint64, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "pya_modpep_create": (_vp, [C.c_char_p, C.c_float, C.c_float, C.c_char_p]),
    "pya_modpep_destroy": (None, [_vp]),
    "pya_modpep_last_error": (C.c_char_p, [_vp]),
    "pya_modpep_add_neutral_loss": (C.c_int, [_vp, C.c_char_p, C.c_float]),
    "pya_modpep_consume_peptide": (C.c_int, [_vp, C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, _vp, _vp, C.c_uint64]),
    "pya_modpep_n_modifiable": (C.c_int64, [_vp]),
    "pya_modpep_consume_peak": (C.c_int, [_vp, C.c_float, C.c_uint64]),
    "pya_modpep_get_match": (C.c_int, [_vp, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_uint64)]),
    "pya_modpep_get_peptide": (C.c_int64, [_vp, _vp, C.c_uint64, C.c_char_p, C.c_uint64]),
    "pya_modpep_site_ions": (C.c_int, [_vp, _vp, _vp, C.c_uint64, C.c_char, C.c_uint64, _vp, C.c_uint64,
                                       C.POINTER(C.c_uint64), _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "pya_fgraph_create": (_vp, [_vp, C.c_char, C.c_uint64]),
    "pya_fgraph_destroy": (None, [_vp]),
    "pya_fgraph_type": (C.c_char, [_vp]),
    "pya_fgraph_charge": (C.c_uint64, [_vp]),
    "pya_fgraph_reset_iterator": (C.c_int, [_vp]),
    "pya_fgraph_incr_signature": (C.c_int, [_vp]),
    "pya_fgraph_is_signature_end": (C.c_int, [_vp]),
    "pya_fgraph_reset_fragment": (C.c_int, [_vp]),
    "pya_fgraph_incr_fragment": (C.c_int, [_vp]),
    "pya_fgraph_is_fragment_end": (C.c_int, [_vp]),
    "pya_fgraph_is_loss": (C.c_int, [_vp]),
    "pya_fgraph_set_signature": (C.c_int, [_vp, _vp, C.c_uint64]),
    "pya_fgraph_get_signature": (C.c_int64, [_vp, _vp, C.c_uint64]),
    "pya_fgraph_fragment_mz": (C.c_int, [_vp, C.POINTER(C.c_float)]),
    "pya_fgraph_fragment_size": (C.c_uint64, [_vp]),
    "pya_fgraph_fragment_seq": (C.c_int64, [_vp, C.c_char_p, C.c_uint64]),
    "pya_log_sum": (C.c_float, [C.c_float, C.c_float]),
    "pya_log_bin_coef": (C.c_int, [C.c_uint64, C.c_uint64, C.POINTER(C.c_float)]),
    "pya_binomial": (C.c_int, [C.c_float, C.c_int, C.c_uint64, C.c_uint64, C.POINTER(C.c_float)]),
    "pya_power_set_sums": (C.c_int64, [_vp, C.c_uint64, C.c_uint64, _vp, C.c_uint64]),
}

_lib = None


def _share_torch_hip_runtime():
    """A process must hold ONE HIP runtime.  PyTorch-ROCm ships its own copy (torch/lib/libamdhip64.so,
    soname libamdhip64.so.7) and asks for it by FILE name; this library asks for the soname.  Loaded
    torch-first, the loader hands us torch's copy; loaded the other way round it would bring in a second
    runtime next to /opt/rocm's, torch would then find "No HIP GPUs", and device.DevicePlan could not
    take torch's device pointers.  So when a ROCm torch is installed, its copy goes in first (without
    importing torch)."""
    if any("libamdhip64" in line for line in open("/proc/self/maps")):
        return                                    # a runtime is already in the process: the loader reuses it
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        C.CDLL(cand, mode=C.RTLD_GLOBAL)


def load():
    """Loads the HIP library (no device needed for loading; pya_create needs one)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "pyascore_amd: %s is missing. Build it with `python -m pyascore_amd.build` "
            "(hipcc, gfx950). There is no CPU fallback." % LIB_PATH)
    _share_torch_hip_runtime()
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        if os.environ.get("PYA_LIB_OLD") and not hasattr(lib, name):
            continue                     # (A/B against an older build of the library: bench.py only)
        fn = getattr(lib, name)          # AttributeError = header/library mismatch: fail loudly
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib
