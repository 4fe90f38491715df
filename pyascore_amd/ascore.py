"""``PyAscore`` -- the reference's Python surface for the PTM-localisation scorer
(pyascore/ptm_scoring/Ascore.pyx:12-288), backed by the MI355X kernels through the C ABI of
include/pyascore_hip.h.  Same constructor, ``add_neutral_loss``, ``score``, properties and
``calculate_ambiguity``; plus ``score_batch`` (``score`` is a batch of one).

Deviations, all towards *more* defined behaviour: inputs the reference
would abort or read out of bounds on (unknown residue, empty spectrum, ``n_top < 10``,
``max_fragment_charge < 1``, mismatched array lengths) raise ``ValueError`` here.
"""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np

from . import _lib


def _as_ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _typed_spectra(mz, intensity):
    """The spectrum arrays of a batch as the library takes them: contiguous, float32 arrays as they are (no widening
    copy), everything else float64 -- and float64 for both when only the m/z are float32 (a combination the library
    refuses)."""
    mz, intensity = np.asarray(mz), np.asarray(intensity)
    it_t = np.float32 if intensity.dtype == np.float32 else np.float64
    mz_t = np.float32 if mz.dtype == np.float32 and it_t == np.float32 else np.float64
    return np.ascontiguousarray(mz, mz_t), np.ascontiguousarray(intensity, it_t)


def _n_spectra(batch):
    """the spectra a batch holds: one per PSM, or the shared ones of a batch with ``spec_of``"""
    return int(batch.get("n_spectra", batch["n_psm"])) if batch.get("spec_of") is not None else int(batch["n_psm"])


def _batch_peak_off(batch):
    """the int64 offsets of the spectra of a batch, ``_n_spectra(batch) + 1`` of them"""
    peak_off = np.ascontiguousarray(batch["peak_off"], np.int64)
    if peak_off.size != _n_spectra(batch) + 1:
        raise ValueError("offset arrays must have n_psm + 1 entries" if batch.get("spec_of") is None else
                         "a shared batch has one spec_of entry per PSM and n_spectra + 1 peak offsets")
    return peak_off


def _transform_call(who, mz, intensity, peak_off):
    """What ``PyAscore.{deisotope,decharge,strip,centroid}_spectra`` (``who``) do alike in front of the library: the spectrum
    arrays as it takes them, cut to ``peak_off[0]:peak_off[-1]``, the offsets from 0, the arrays it writes and the two
    ``TypedSpectra``.  ``n_peaks == 0``: ``mz`` / ``intensity`` / ``out_mz`` / ``out_it`` are one-element stand-ins (an empty
    array may have no address to pass)."""
    mz, intensity = _typed_spectra(mz, intensity)
    peak_off = np.ascontiguousarray(peak_off, np.int64)
    if mz.ndim != 1 or intensity.ndim != 1 or peak_off.ndim != 1 or peak_off.size < 1:
        raise ValueError("%s: mz, intensity and peak_off are one-dimensional, peak_off has n_spectra + 1 entries" % who)
    if peak_off[0] < 0 or (np.diff(peak_off) < 0).any():
        raise ValueError("%s: peak_off must not be negative or descend" % who)
    lo, hi = int(peak_off[0]), int(peak_off[-1])
    if mz.size < hi or intensity.size < hi:
        raise ValueError("peak_off runs past the end of the spectrum arrays")
    mz, intensity = (mz[lo:hi], intensity[lo:hi]) if hi > lo else (np.zeros(1, mz.dtype), np.zeros(1, intensity.dtype))
    out_mz, out_it = np.empty_like(mz), np.empty_like(intensity)
    t_in = _lib.TypedSpectra(_as_ptr(mz), _as_ptr(intensity), _lib.spectrum_type(mz.dtype), _lib.spectrum_type(intensity.dtype))
    t_out = _lib.TypedSpectra(_as_ptr(out_mz), _as_ptr(out_it), t_in.mz_type, t_in.intensity_type)
    return SimpleNamespace(n_spec=peak_off.size - 1, n_peaks=hi - lo, peak_off=np.ascontiguousarray(peak_off - lo), mz=mz,
                           intensity=intensity, out_mz=out_mz, out_it=out_it, new_off=np.zeros(peak_off.size, np.int64),
                           over=np.zeros(2, np.uint32), t_in=t_in, t_out=t_out)


def _transform_result(c):
    """``((mz, intensity, peak_off), over)`` of a ``_transform_call`` the library has answered (or that was not made: no peak
    is kept): the ``new_off[-1]`` output peaks with their offsets, and ``over = (count, first)``"""
    kept = int(c.new_off[-1])
    first = None if not c.over[0] else 0xFFFFFFFF - int(c.over[1])
    return (c.out_mz[:kept], c.out_it[:kept], c.new_off), (int(c.over[0]), first)


def _renumber_psm(message, perm):
    """'PSM <j>: ...' of a batch that was scored in the order ``perm`` -> the caller's number of that PSM."""
    import re
    return re.sub(r"^PSM (\d+)", lambda m: "PSM %d" % perm[int(m.group(1))] if int(m.group(1)) < len(perm) else m.group(0), message)


def _check_f64(name, a):
    if a is None:
        raise TypeError("Argument '%s' must not be None" % name)
    if not isinstance(a, np.ndarray):
        raise TypeError("Argument '%s' has incorrect type (expected numpy.ndarray, got %s)"
                        % (name, type(a).__name__))
    if a.ndim != 1:
        raise ValueError("Buffer has wrong number of dimensions (expected 1, got %d)" % a.ndim)
    if a.dtype != np.float64:
        raise ValueError("Buffer dtype mismatch, expected 'double' but got '%s'" % a.dtype)
    if not a.flags["C_CONTIGUOUS"]:
        raise ValueError("ndarray is not C-contiguous")
    return a


def _check_typed(name, a, dtype, cname):
    if not isinstance(a, np.ndarray):
        raise TypeError("Argument '%s' has incorrect type (expected numpy.ndarray, got %s)"
                        % (name, type(a).__name__))
    if a.ndim != 1:
        raise ValueError("Buffer has wrong number of dimensions (expected 1, got %d)" % a.ndim)
    if a.dtype != dtype:
        raise ValueError("Buffer dtype mismatch, expected '%s' but got '%s'" % (cname, a.dtype))
    if not a.flags["C_CONTIGUOUS"]:
        raise ValueError("ndarray is not C-contiguous")
    return a


try:                                  # the compiled way into pya_score_one (csrc/pyfast.c); ctypes without it
    from . import _fast
    _fast.setup(np.ndarray)
except ImportError:                   # not built for this interpreter
    _fast = None

EVIDENCE_DTYPE = np.dtype(_lib.EVIDENCE_DTYPE)      # pya_evidence, 16 bytes
COVERAGE_DTYPE = np.dtype(_lib.COVERAGE_DTYPE)      # pya_coverage, 64 bytes
SITE_DTYPE = np.dtype(_lib.SITE_DTYPE)              # pya_site, 32 bytes
SITE_PROB_DTYPE = np.dtype(_lib.SITE_PROB_DTYPE)    # pya_site_prob, 16 bytes
PSM_PROB_DTYPE = np.dtype(_lib.PSM_PROB_DTYPE)      # pya_psm_prob, 16 bytes
assert SITE_PROB_DTYPE.itemsize == 16 and PSM_PROB_DTYPE.itemsize == 16
RANKED_DTYPE = np.dtype(_lib.RANKED_DTYPE)          # pya_ranked, 16 bytes
assert RANKED_DTYPE.itemsize == 16
ROLLUP_DTYPE = np.dtype(_lib.ROLLUP_DTYPE)          # pya_site_rollup, 32 bytes
FLR_DTYPE = np.dtype(_lib.FLR_DTYPE)                # pya_site_flr, 32 bytes
assert ROLLUP_DTYPE.itemsize == 32
PEPTIDOFORM_DTYPE = np.dtype(_lib.PEPTIDOFORM_DTYPE)    # pya_peptidoform, 48 bytes
assert PEPTIDOFORM_DTYPE.itemsize == 48
assert EVIDENCE_DTYPE.itemsize == 16
ION_DTYPE = np.dtype(_lib.ION_DTYPE)                # pya_ion, 16 bytes
assert ION_DTYPE.itemsize == 16
from .named import NAMED_DTYPE, query_csr, sig_bits_batch, sig_bits_of, take_queries  # noqa: E402,F401
from .ranked import check_k as check_ranked_k  # noqa: E402
_NO_U32 = np.zeros(0, np.uint32)

_NO_F32 = np.zeros(0, np.float32)


def _peptidoform_request(req, n_psm):
    """``score_batch(peptidoforms=...)`` as contiguous arrays: dict(group int32, threshold, psm_id uint32 | None)"""
    if not isinstance(req, dict):
        raise ValueError("peptidoforms takes a dict: group and optionally threshold and psm_id")
    unknown = set(req) - {"group", "threshold", "psm_id"}
    if unknown or "group" not in req:
        raise ValueError("peptidoforms takes group and optionally threshold and psm_id%s"
                         % ("; unknown: " + ", ".join(sorted(unknown)) if unknown else ""))
    group = np.asarray(req["group"])
    if group.ndim != 1 or (group.size and group.dtype.kind not in "iu") or group.size != n_psm:
        raise ValueError("peptidoforms: group is one integer per PSM")
    if group.size and (group.max() > 0x7FFFFFFF or group.min() < -0x80000000):
        raise ValueError("peptidoforms: group does not fit int32")
    psm_id = req.get("psm_id")
    if psm_id is not None:
        psm_id = np.ascontiguousarray(psm_id, np.uint32)
        if psm_id.shape != (n_psm,):
            raise ValueError("peptidoforms: psm_id has one entry per PSM")
    return dict(group=np.ascontiguousarray(group, np.int32), threshold=float(req.get("threshold", 0.75)), psm_id=psm_id)


def _mz_profile_request(req, n_psm, mz_error, n_top):
    """``score_batch(mz_profile=...)`` with its defaults resolved: dict(run int32 | None, n_slots, params, c_params)"""
    from .rollup import mz_profile_params
    if req is True:
        req = {}
    if not isinstance(req, dict):
        raise ValueError("mz_profile takes a dict: run, n_slots, da_half_width, ppm_half_width, band_width, max_rank")
    unknown = set(req) - {"run", "n_slots", "da_half_width", "ppm_half_width", "band_width", "max_rank"}
    if unknown:
        raise ValueError("mz_profile takes run, n_slots, da_half_width, ppm_half_width, band_width and max_rank; unknown: "
                         + ", ".join(sorted(unknown)))
    run = req.get("run")
    if run is not None:
        run = np.asarray(run)
        if run.ndim != 1 or run.size != n_psm or (run.size and run.dtype.kind not in "iu"):
            raise ValueError("mz_profile: run is one integer per PSM")
        if run.size and (int(run.max()) > 0x7FFFFFFF or int(run.min()) < -0x80000000):
            raise ValueError("mz_profile: run does not fit int32")
        run = np.ascontiguousarray(run, np.int32)
    n_slots = int(req.get("n_slots", 1))
    if not 0 <= n_slots <= 0x7FFFFFFF:
        raise ValueError("mz_profile: n_slots must be in 0 .. 2^31 - 1")
    da = req.get("da_half_width")
    rank = req.get("max_rank")
    params = mz_profile_params(mz_error if da is None else da, req.get("ppm_half_width", 50.0), req.get("band_width", 250.0),
                               n_top - 1 if rank is None else rank)
    c_params = _lib.MzProfileParams(params["inv_da"], params["inv_ppm"], params["inv_band"], params["max_rank"], 0)
    return dict(run=run, n_slots=n_slots, params=params, c_params=c_params)


def _recalibrate_request(req, n_psm):
    """``score_batch(recalibrate=...)`` checked: dict(cal MZ_CALIBRATION_DTYPE, run int32 | None, band_width, inv_band)"""
    from .rollup import MZ_CALIBRATION_DTYPE, MZC_MAX_PPM
    if not isinstance(req, dict):
        raise ValueError("recalibrate takes a dict: calibration, run, band_width")
    unknown = set(req) - {"calibration", "run", "band_width"}
    if unknown:
        raise ValueError("recalibrate takes calibration, run and band_width; unknown: " + ", ".join(sorted(unknown)))
    if req.get("calibration") is None:
        raise ValueError("recalibrate: calibration is missing (pyascore_amd.rollup.MZ_CALIBRATION_DTYPE records, one per run slot)")
    cal = np.ascontiguousarray(req["calibration"], MZ_CALIBRATION_DTYPE).reshape(-1)
    if not (np.abs(cal["ppm"]) <= float(MZC_MAX_PPM)).all():
        raise ValueError("recalibrate: a knot of the calibration is not finite or beyond %d ppm" % MZC_MAX_PPM)
    run = req.get("run")
    if run is not None:
        run = np.asarray(run)
        if run.ndim != 1 or run.size != n_psm or (run.size and run.dtype.kind not in "iu"):
            raise ValueError("recalibrate: run is one integer per PSM")
        if run.size and (int(run.max()) > 0x7FFFFFFF or int(run.min()) < -0x80000000):
            raise ValueError("recalibrate: run does not fit int32")
        run = np.ascontiguousarray(run, np.int32)
    band_width = float(req.get("band_width", 250.0))
    inv_band = 1.0 / band_width if band_width else float("inf")
    if not (np.isfinite(inv_band) and inv_band > 0.0):
        raise ValueError("recalibrate: band_width = %r has no finite positive inverse" % band_width)
    return dict(cal=cal, run=run, band_width=band_width, inv_band=inv_band)


def _deisotope_request(req):
    """``score_batch(deisotope=...)`` checked: the dict of ``pyascore_amd.rollup.deisotope_params``"""
    from .rollup import deisotope_params
    if req is True:
        req = {}
    if not isinstance(req, dict):
        raise ValueError("deisotope takes a dict: tol, max_charge, step, ratio, ratio_per_mz")
    unknown = set(req) - {"tol", "max_charge", "step", "ratio", "ratio_per_mz"}
    if unknown:
        raise ValueError("deisotope takes tol, max_charge, step, ratio and ratio_per_mz; unknown: " + ", ".join(sorted(unknown)))
    try:
        return deisotope_params(**req)
    except TypeError:
        raise ValueError("deisotope: tol, step, ratio and ratio_per_mz are numbers, max_charge an integer") from None


_RECALIBRATE_FIRST = ("decharge moves peaks, and a calibration is a function of the measured m/z: correct the spectra first "
                      "(pya_recalibrate_spectra, DevicePlan.recalibrate or pyascore_amd.rollup.recalibrate), then pass the corrected "
                      "arrays with decharge=")


def _decharge_request(req):
    """``score_batch(decharge=...)`` checked: the dict of ``pyascore_amd.rollup.decharge_params``"""
    from .rollup import decharge_params
    if req is True:
        req = {}
    names = ("tol", "max_charge", "step", "ratio", "ratio_per_mz", "carrier", "witness")
    if not isinstance(req, dict):
        raise ValueError("decharge takes a dict: " + ", ".join(names))
    unknown = set(req) - set(names)
    if unknown:
        raise ValueError("decharge takes " + ", ".join(names) + "; unknown: " + ", ".join(sorted(unknown)))
    try:
        return decharge_params(**req)
    except TypeError:
        raise ValueError("decharge: tol, step, ratio, ratio_per_mz, carrier and witness are numbers, max_charge an integer") from None


def _strip_request(req, mz_error, n_spec=None):
    """``score_batch(strip=...)`` checked: ``(params, precursor_mz, precursor_charge)`` -- the dict of
    ``pyascore_amd.rollup.strip_params`` (``tol=None``: the scorer's ``mz_error``) and the precursors as float64 / int32 arrays,
    one entry per spectrum (``n_spec`` entries when it is given)"""
    from .rollup import strip_params
    names = ("precursor_mz", "precursor_charge", "tol", "losses", "reduced", "isotopes", "step", "mz_lo", "mz_hi")
    if not isinstance(req, dict):
        raise ValueError("strip takes a dict: " + ", ".join(names))
    unknown = set(req) - set(names)
    if unknown:
        raise ValueError("strip takes " + ", ".join(names) + "; unknown: " + ", ".join(sorted(unknown)))
    if req.get("precursor_mz") is None or req.get("precursor_charge") is None:
        raise ValueError("strip needs precursor_mz and precursor_charge, one entry per spectrum")
    rule = {k: v for k, v in req.items() if k not in ("precursor_mz", "precursor_charge")}
    if rule.get("tol") is None:
        rule["tol"] = float(mz_error)
    try:
        params = strip_params(**rule)
        prec_mz = np.ascontiguousarray(req["precursor_mz"], np.float64)
        charge = np.asarray(req["precursor_charge"])
        if charge.dtype.kind not in "iu":
            raise TypeError
        prec_z = np.ascontiguousarray(np.clip(charge, -1, 0x7FFFFFFF), np.int32)     # (every charge outside 1 .. 8 means "no windows")
    except TypeError:
        raise ValueError("strip: tol, step, mz_lo and mz_hi are numbers, losses a sequence of numbers, isotopes an integer, "
                         "precursor_mz numbers and precursor_charge integers") from None
    if prec_mz.ndim != 1 or prec_z.shape != prec_mz.shape or (n_spec is not None and prec_mz.size != n_spec):
        raise ValueError("strip: precursor_mz and precursor_charge have one entry per spectrum (per PSM in a batch without spec_of)")
    return params, prec_mz, prec_z


def _markers_request(req, mz_error, n_spec=None):
    """``score_batch(markers=...)`` checked: ``(params, precursor_mz, precursor_charge)`` -- the dict of
    ``pyascore_amd.rollup.marker_params`` (``tol=None``: the scorer's ``mz_error``) and the precursors as float64 / int32 arrays,
    one entry per spectrum (``n_spec`` entries when it is given), or None / None when none were passed"""
    from .rollup import marker_params
    names = ("mz", "losses", "tol", "tol_ppm", "precursor_mz", "precursor_charge")
    if not isinstance(req, dict):
        raise ValueError("markers takes a dict: " + ", ".join(names))
    unknown = set(req) - set(names)
    if unknown:
        raise ValueError("markers takes " + ", ".join(names) + "; unknown: " + ", ".join(sorted(unknown)))
    rule = {k: v for k, v in req.items() if k not in ("precursor_mz", "precursor_charge")}
    if rule.get("tol") is None:
        rule["tol"] = float(mz_error)
    given = req.get("precursor_mz") is not None, req.get("precursor_charge") is not None
    if given[0] != given[1]:
        raise ValueError("markers: precursor_mz and precursor_charge come together, one entry per spectrum")
    try:
        params = marker_params(**rule)
        prec_mz = prec_z = None
        if given[0]:
            prec_mz = np.ascontiguousarray(req["precursor_mz"], np.float64)
            charge = np.asarray(req["precursor_charge"])
            if charge.dtype.kind not in "iu":
                raise TypeError
            prec_z = np.ascontiguousarray(np.clip(charge, -1, 0x7FFFFFFF), np.int32)  # (every charge outside 1 .. 8 means "no precursor")
    except TypeError:
        raise ValueError("markers: tol and tol_ppm are numbers, mz and losses sequences of numbers, precursor_mz numbers and "
                         "precursor_charge integers") from None
    if params["loss_mask"] and prec_mz is None:
        raise ValueError("markers: losses need precursor_mz and precursor_charge, one entry per spectrum")
    if prec_mz is not None and (prec_mz.ndim != 1 or prec_z.shape != prec_mz.shape or (n_spec is not None and prec_mz.size != n_spec)):
        raise ValueError("markers: precursor_mz and precursor_charge have one entry per spectrum (per PSM in a batch without spec_of)")
    return params, prec_mz, prec_z


def _purity_request(req, n_spec=None, have_quant=True):
    """``score_batch(purity=...)`` checked: ``(params, spectra, queries, gate)`` -- the dict of
    ``pyascore_amd.rollup.purity_params``, ``(ms1_mz, ms1_intensity, ms1_peak_off)`` as given, the five query arrays of
    ``pyascore_amd.rollup.purity_queries`` (``n_spec`` entries each when it is given) and ``(threshold, keep_unknown)`` or None"""
    from .rollup import check_purity_gate, purity_params, purity_queries
    rule_names = ("tol", "tol_ppm", "isotopes", "below", "step")
    names = ("ms1_mz", "ms1_intensity", "ms1_peak_off", "survey", "precursor_mz", "precursor_charge", "window_lo", "window_hi") + rule_names + \
        ("gate",)
    if not isinstance(req, dict):
        raise ValueError("purity takes a dict: " + ", ".join(names))
    unknown = set(req) - set(names)
    if unknown:
        raise ValueError("purity takes " + ", ".join(names) + "; unknown: " + ", ".join(sorted(unknown)))
    missing = [k for k in names[:8] if req.get(k) is None]
    if missing:
        raise ValueError("purity needs " + ", ".join(missing))
    try:
        params = purity_params(**{k: req[k] for k in rule_names if req.get(k) is not None})
    except TypeError:
        raise ValueError("purity: tol, tol_ppm and step are numbers, isotopes and below integers") from None
    queries = purity_queries(req["survey"], req["precursor_mz"], req["precursor_charge"], req["window_lo"], req["window_hi"])
    if n_spec is not None and queries[0].size != n_spec:
        raise ValueError("purity: survey, precursor_mz, precursor_charge, window_lo and window_hi have one entry per spectrum (per PSM in a "
                         "batch without spec_of)")
    gate = req.get("gate")
    if gate is not None:
        if not isinstance(gate, dict) or set(gate) - {"threshold", "keep_unknown"} or gate.get("threshold") is None:
            raise ValueError("purity: gate takes a dict: threshold, keep_unknown")
        gate = check_purity_gate(gate["threshold"], gate.get("keep_unknown", True), "purity: gate")
        if not have_quant:
            raise ValueError("purity: gate needs quant= or peptidoform_quant= in the same call: it is their matrix that is gated")
    return params, (req["ms1_mz"], req["ms1_intensity"], req["ms1_peak_off"]), queries, gate


XIC_CHANNELS = {"xic_area": "area", "xic_apex": "apex"}     # ``values=`` of quant= / peptidoform_quant= beside xic=


def _xic_request(req, n_spec=None):
    """``score_batch(xic=...)`` checked: ``(params, spectra, rt, queries)`` -- the dict of ``pyascore_amd.rollup.xic_params``,
    ``(ms1_mz, ms1_intensity, ms1_peak_off)`` and ``rt`` as given, the five query arrays of ``pyascore_amd.rollup.xic_queries``
    (``n_spec`` entries each when it is given)"""
    from .rollup import xic_params, xic_queries
    rule_names = ("tol", "tol_ppm", "isotopes", "step", "rise", "max_gap")
    names = ("ms1_mz", "ms1_intensity", "ms1_peak_off", "rt", "seed", "scan_lo", "scan_hi", "precursor_mz", "precursor_charge") + rule_names
    if not isinstance(req, dict):
        raise ValueError("xic takes a dict: " + ", ".join(names))
    unknown = set(req) - set(names)
    if unknown:
        raise ValueError("xic takes " + ", ".join(names) + "; unknown: " + ", ".join(sorted(unknown)))
    missing = [k for k in names[:9] if req.get(k) is None]
    if missing:
        raise ValueError("xic needs " + ", ".join(missing))
    try:
        params = xic_params(**{k: req[k] for k in rule_names if req.get(k) is not None})
    except TypeError:
        raise ValueError("xic: tol, tol_ppm, step and rise are numbers, isotopes and max_gap integers") from None
    queries = xic_queries(req["seed"], req["scan_lo"], req["scan_hi"], req["precursor_mz"], req["precursor_charge"])
    if n_spec is not None and queries[0].size != n_spec:
        raise ValueError("xic: seed, scan_lo, scan_hi, precursor_mz and precursor_charge have one entry per spectrum (per PSM in a batch "
                         "without spec_of)")
    return params, (req["ms1_mz"], req["ms1_intensity"], req["ms1_peak_off"]), req["rt"], queries


def _centroid_request(req, n_spec=None):
    """``score_batch(centroid=...)`` checked: ``(params, select)`` -- the dict of ``pyascore_amd.rollup.centroid_params`` and
    the uint8 ``select`` array (one entry per spectrum; ``n_spec`` entries when it is given) or None"""
    from .rollup import centroid_params, centroid_select
    names = ("gap", "gap_ppm", "half_width", "min_height", "area", "select")
    if not isinstance(req, dict):
        raise ValueError("centroid takes a dict: " + ", ".join(names))
    unknown = set(req) - set(names)
    if unknown:
        raise ValueError("centroid takes " + ", ".join(names) + "; unknown: " + ", ".join(sorted(unknown)))
    if req.get("gap") is None:
        raise ValueError("centroid needs gap: the largest distance of two samples of one peak, in m/z (2 to 3 sampling steps)")
    try:
        params = centroid_params(**{k: v for k, v in req.items() if k != "select"})
    except TypeError:
        raise ValueError("centroid: gap, gap_ppm and min_height are numbers, half_width an integer, area a boolean") from None
    select = req.get("select")
    if select is not None:
        select = centroid_select(select, np.size(select) if n_spec is None else n_spec, "centroid")
    return params, select


def _rollup_request(rollup, n_psm):
    """``score_batch(rollup=...)`` as contiguous arrays: dict(slot int32, n_slots, threshold, psm_id uint32 | None,
    site_off int64 | None)"""
    unknown = set(rollup) - {"slot", "n_slots", "threshold", "psm_id", "site_off"}
    if unknown or "slot" not in rollup or "n_slots" not in rollup:
        raise ValueError("rollup takes slot, n_slots and optionally threshold, psm_id and site_off%s"
                         % ("; not " + ", ".join(sorted(unknown)) if unknown else ""))
    slot = np.asarray(rollup["slot"])
    if slot.ndim != 1 or (slot.size and slot.dtype.kind not in "iu"):
        raise ValueError("rollup: slot is one integer per residue record")
    if slot.size and (int(slot.max()) > 0x7FFFFFFF or int(slot.min()) < -0x80000000):
        raise ValueError("rollup: slot does not fit int32")
    n_slots = int(rollup["n_slots"])
    if not 0 <= n_slots <= 0x7FFFFFFF:
        raise ValueError("rollup: n_slots must be in 0 .. 2^31 - 1")
    psm_id = rollup.get("psm_id")
    if psm_id is not None:
        psm_id = np.ascontiguousarray(psm_id, np.uint32)
        if psm_id.shape != (n_psm,):
            raise ValueError("rollup: psm_id has one entry per PSM")
    site_off = rollup.get("site_off")
    if site_off is not None:
        site_off = np.ascontiguousarray(site_off, np.int64)
    return dict(slot=np.ascontiguousarray(slot, np.int32), n_slots=n_slots, threshold=float(rollup.get("threshold", 0.75)),
                psm_id=psm_id, site_off=site_off)


def _marker_channels(name, req, params, records, spec_of):
    """``quant=`` / ``peptidoform_quant=`` with ``values=None`` beside ``markers=``, filled in: the channels are the fixed targets
    of ``markers=`` (its marker records ``records``), the rows the spectra"""
    from .rollup import marker_matrix
    fixed = [t for t in range(len(params["value"])) if not (params["loss_mask"] >> t) & 1]
    if not fixed:
        raise ValueError(name + ": markers= has no fixed target to take as a channel")
    row = req.get("row")
    if row is None and spec_of is not None:
        row = np.asarray(spec_of).astype(np.int32)
    return dict(req, values=np.ascontiguousarray(marker_matrix(records)[:, fixed]), row=row)


def _channels_request(name, req, markers=None):
    """The ``channels=`` entry of ``score_batch(quant=...)`` / ``peptidoform_quant=`` checked, against ``values`` where the
    request holds them already and against the fixed targets of ``markers`` (the ``markers=`` request) where they come from
    there, so that a matrix of another shape is refused before any device work: None when there is none, else dict(matrix float64
    [n_channels, n_channels] | None, normalize bool, select uint8 [n_rows] | None)"""
    from .rollup import QUANT_MAX_CHANNELS, check_channel_matrix
    if not isinstance(req, dict) or req.get("channels") is None:
        return None
    ch = req["channels"]
    what = name + ": channels"
    names = ("matrix", "normalize", "select")
    if not isinstance(ch, dict):
        raise ValueError(what + " takes a dict: " + ", ".join(names))
    unknown = set(ch) - set(names)
    if unknown:
        raise ValueError(what + " takes " + ", ".join(names) + "; unknown: " + ", ".join(sorted(unknown)))
    normalize = ch.get("normalize", False)
    if not isinstance(normalize, (bool, np.bool_)):
        raise ValueError(what + ": normalize = %r is not a boolean" % (normalize,))
    matrix, select = ch.get("matrix"), ch.get("select")
    if matrix is None and not normalize:
        raise ValueError(what + " names neither a matrix nor normalize=True")
    if select is not None and not normalize:
        raise ValueError(what + ": select names the rows the loading factors are taken from; it needs normalize=True")
    shape = None
    if req.get("values") is not None:
        try:
            shape = np.shape(req["values"])
        except (TypeError, ValueError):
            shape = None
        if shape is None or len(shape) != 2:
            raise ValueError(name + ": values is a matrix, one row per spectrum and one column per channel")
    if matrix is not None:
        try:
            matrix = np.ascontiguousarray(matrix, np.float64)
        except (TypeError, ValueError):
            raise ValueError(what + ": matrix is a square matrix of numbers") from None
        if matrix.ndim != 2 or matrix.shape[0] != matrix.shape[1] or not 1 <= matrix.shape[0] <= QUANT_MAX_CHANNELS:
            raise ValueError(what + ": matrix is a square matrix of 1 .. %d channels" % QUANT_MAX_CHANNELS)
        if shape is not None:
            matrix = check_channel_matrix(matrix, shape[1], what)
        elif isinstance(markers, dict):
            try:
                n_fixed = len(tuple(markers.get("mz", ())))
            except TypeError:
                n_fixed = 0                                  # (markers= itself is refused where it is checked)
            if n_fixed:
                matrix = check_channel_matrix(matrix, n_fixed, what)
    if select is not None:
        select = np.asarray(select)
        if select.ndim != 1 or (shape is not None and select.size != shape[0]) or (select.size and select.dtype.kind not in "biu"):
            raise ValueError(what + ": select is one boolean per row of values")
        select = np.ascontiguousarray(select != 0, np.uint8)
    return dict(matrix=matrix, normalize=bool(normalize), select=select)


def _quant_request(req, n_psm, have_rollup, name="quant"):
    """``score_batch(quant=...)`` checked -- under the name ``peptidoform_quant`` that option, whose companion is
    ``peptidoforms=`` --: dict(values float64 [n_rows, n_channels], row int32 | None, params, c_params), ``params`` the dict of
    ``pyascore_amd.rollup.site_quant_params``"""
    from .rollup import site_quant_c_params, site_quant_params
    names = ("values", "row", "threshold", "scale_log2", "complete_only")
    if not isinstance(req, dict):
        raise ValueError(name + " takes a dict: " + ", ".join(names))
    unknown = set(req) - set(names)
    if unknown:
        raise ValueError(name + " takes " + ", ".join(names) + "; unknown: " + ", ".join(sorted(unknown)))
    if not have_rollup and name == "peptidoform_quant":
        raise ValueError("peptidoform_quant needs peptidoforms= in the same call: the table is row-aligned with its list")
    if not have_rollup:
        raise ValueError("quant needs rollup= in the same call: the channel sums go to the slots of the roll-up")
    if req.get("values") is None:
        raise ValueError(name + ": values is missing (a float64 matrix, one row per spectrum and one column per channel); only beside "
                         "markers= it may be None -- the channels are then the fixed targets of markers=")
    try:
        values = np.ascontiguousarray(req["values"], np.float64)
    except (TypeError, ValueError):
        raise ValueError(name + ": values is a matrix of numbers") from None
    if values.ndim != 2:
        raise ValueError(name + ": values is a matrix, one row per spectrum and one column per channel")
    if values.shape[0] > 0x7FFFFFFF:
        raise ValueError(name + ": values has more than 2^31 - 1 rows")
    row = req.get("row")
    if row is not None:
        row = np.asarray(row)
        if row.ndim != 1 or row.size != n_psm or (row.size and row.dtype.kind not in "iu"):
            raise ValueError(name + ": row is one integer per PSM")
        if row.size and (int(row.max()) > 0x7FFFFFFF or int(row.min()) < -0x80000000):
            raise ValueError(name + ": row does not fit int32")
        row = np.ascontiguousarray(row, np.int32)
    params = site_quant_params(req.get("threshold", 0.75), req.get("scale_log2", 10), values.shape[1], req.get("complete_only", False))
    return dict(values=values, row=row, params=params, c_params=site_quant_c_params(params))


class _Last(dict):
    """What the last score() call left: the scalars as they came back, the arrays made from the raw bytes the first
    time something reads them (a loop that only reads best_score never builds them)."""

    def __missing__(self, key):
        if key == "pep":
            v = np.frombuffer(self["peptide"].encode("utf8"), dtype=np.uint8)
        elif key == "ascores":
            v = np.frombuffer(self["_asc"], dtype=np.float32)
        elif key == "alt_mask":
            v = np.frombuffer(self["_alt"], dtype=np.uint64)
        else:
            raise KeyError(key)
        self[key] = v
        return v


class PyAscore:
    """Scores the localization of post translational modifications (Ascore.pyx:12-59).

    Parameters
    ----------
    bin_size : float
        Size in MZ of each bin
    n_top : int
        Number of top peaks to retain in each bin: 10 (what everything is built for and the reference's command
        line passes) to 16 (every PSM then goes through the general kernel: same results, far slower)
    mod_group : str
        Residues that can carry the unlocalized modification, e.g. "STY" ('n'/'c' = termini)
    mod_mass : float
        Mass of the unlocalized modification, e.g. 79.966331
    mz_error : float
        Matching tolerance in Da (default 0.5)
    fragment_types : str
        Ion types to score, subset of b, c, y, z, Z (default "by")
    device : int, optional (keyword only)
        HIP device ordinal; defaults to LOCAL_RANK or 0.
    """

    def __init__(self, bin_size, n_top, mod_group, mod_mass, mz_error=.5, fragment_types="by", *,
                 device=None):
        if not isinstance(mod_group, str) or not isinstance(fragment_types, str):
            raise TypeError("mod_group and fragment_types must be str")
        self._lib = _lib.load()
        self._h = None
        if device is None:
            device = int(os.environ.get("LOCAL_RANK", "0"))
        self._mod_group = mod_group
        self._cfg_strings = (mod_group.encode("utf8"), fragment_types.encode("utf8"))
        cfg = _lib.Config(float(bin_size), int(n_top), self._cfg_strings[0], float(mod_mass),
                          float(mz_error), self._cfg_strings[1], int(device))
        h = C.c_void_p()
        rc = self._lib.pya_create(C.byref(cfg), C.byref(h))
        self._h = h if h.value else None
        if rc:
            self._raise(rc)
        self._h_addr = int(h.value)
        self._score_one_addr = C.cast(self._lib.pya_score_one, C.c_void_p).value
        self.device = int(device)
        self._n_top = int(n_top)
        self._mz_error = float(np.float32(mz_error))     # (as the library holds it: a float32)
        self._last = None            # summary of the last score() call
        self._batch_n = None         # PSMs of the batch retained by score_batch(keep=True)
        self._budget = 0             # set_workspace_budget (0 = the library's default, 6 GiB)
        self._lazy_batch = None      # a retained batch too big for the device: re-scored range by range on demand
        self._one = None             # preallocated batch-of-one scaffolding of score()

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and getattr(self, "_lib", None) is not None:
            self._lib.pya_destroy(h)
            self._h = None
            self._h_addr = 0

    def _raise(self, rc):
        msg = self._lib.pya_last_error(self._h).decode("utf8", "replace") if self._h else "pya_create failed"
        if rc in (_lib.PYA_ERR_ARG, _lib.PYA_ERR_PSM, _lib.PYA_ERR_LIMIT):
            raise ValueError(msg)
        raise RuntimeError(msg)

    # ------------------------------------------------------------------------------------------
    def add_neutral_loss(self, group, mass):
        """Add a neutral loss ion to any fragment containing specified amino acids
        (Ascore.pyx:81-99).  Upper case = unmodified residue, lower case = modified residue.  Every later call scores
        under the new settings; what was made under the old ones -- a ``DevicePlan``, the retained batch of ``score_batch(...,
        keep=True)``, the records of the last ``score()`` PSM -- can still be READ (``batch_pep_scores``, ``pep_scores``) but
        no longer launched over: ``DevicePlan.run`` and its stages and ``calculate_ambiguity`` raise ``RuntimeError``."""
        if not isinstance(group, str):
            raise TypeError("Argument 'group' has incorrect type (expected str)")
        self._ensure_kept()      # (the last score() PSM's records, if they are still to be produced: under the old settings)
        rc = self._lib.pya_add_neutral_loss(self._h, group.encode("utf8"), float(mass))
        if rc:
            self._raise(rc)

    def reload_env(self):
        """Re-reads the four environment variables the library knows (PYA_WORKSPACE_MB, PYA_CHUNK_MB, PYA_HOST_TIMING,
        PYA_STAMPS: sizes and diagnostics, read once when the scorer is created) and puts every debug switch back to
        its production default."""
        self._ensure_kept()
        rc = self._lib.pya_reload_env(self._h)
        if rc:
            self._raise(rc)

    def set_debug(self, key, value=None):
        """TEST-ONLY (include/pyascore_debug.h): one debug switch of this scorer -- force a kernel route, make a kernel
        decline its work, resize a table.  ``value=None`` restores the production default.  Nothing in the
        environment selects a route; the parity suite sets the switches through this call."""
        self._ensure_kept()
        rc = self._lib.pya_set_debug(self._h, key.encode("ascii"), None if value is None else str(value).encode("ascii"))
        if rc:
            self._raise(rc)

    def set_workspace_budget(self, n_bytes):
        """Device memory one ``score_batch`` call may hold at a time (default 6 GiB; 0 restores it).
        Bigger calls are cut into chunks of consecutive PSMs and pipelined (upload of the next chunk
        under the kernels of the current one); results do not depend on the cut."""
        rc = self._lib.pya_set_workspace_budget(self._h, int(n_bytes))
        if rc:
            self._raise(rc)
        self._budget = int(n_bytes)

    def _retained_bytes(self, arrs, peak_bytes=16):
        """Device bytes a retained (keep=True) plan of this batch holds, per PSM: ``peak_bytes`` per raw peak (spectra:
        16 for float64 arrays, 12 or 8 for typed ones) + 8 per peak (retained table) + per site assignment the score, the order and the count record (4 + 4 + 4 x its words:
        32 bytes for n_top = 10, 44 for 16; with n_top > 10 also the general kernel's sort area, 8 more) + grid,
        descriptor, results."""
        from .shard import comb_table, count_sites
        n_sites = np.clip(count_sites(arrs, self._mod_group), 0, 64)
        k = arrs["n_of_mod"].astype(np.int64)
        sigs = np.where((k >= 0) & (k <= n_sites), comb_table()[n_sites, np.clip(k, 0, 64)], 0.0)
        peaks = np.diff(arrs["peak_off"]).astype(np.float64)
        rec_words = (self._n_top + 1) // 2 + 1
        per_sig = 8.0 + 4.0 * rec_words + (8.5 if self._n_top != 10 else 0.0)
        return (8.0 + peak_bytes) * peaks + per_sig * sigs + 1024.0

    def score(self, mz_arr, int_arr, peptide, n_of_mod, max_fragment_charge=1, aux_mod_pos=None,
              aux_mod_mass=None):
        """Consume spectra and associated peptide information and score PTM localization
        (Ascore.pyx:103-152)."""
        if _fast is not None:
            # the compiled way: arguments as they are; None = something it does not take (types, layouts, lengths,
            # negative numbers, more than 64 modifications): the checked way below raises what the reference raises
            r = _fast.score_one(self._score_one_addr, self._h_addr, mz_arr, int_arr, peptide, n_of_mod, max_fragment_charge,
                                aux_mod_pos, aux_mod_mass)
            if r is not None and r[0] == 0:
                have_aux = aux_mod_pos is not None and aux_mod_mass is not None
                self._batch_n = None
                self._last = _Last(peptide=peptide, k=r[6], aux_pos=aux_mod_pos.copy() if have_aux else _NO_U32,
                                   aux_mass=aux_mod_mass.copy() if have_aux else _NO_F32, best_score=r[1], best_sig=r[2],
                                   n_sig=r[3], _asc=r[4], _alt=r[5], lazy=True, mz=mz_arr, it=int_arr, z=max_fragment_charge)
                return
            # (an error code, or PYA_ERR_STATE = "not for the one-PSM kernel": the way below handles both)
        mz_arr = _check_f64("mz_arr", mz_arr)
        int_arr = _check_f64("int_arr", int_arr)
        if not isinstance(peptide, str):
            raise TypeError("Argument 'peptide' has incorrect type (expected str, got %s)"
                            % type(peptide).__name__)
        if int_arr.size != mz_arr.size:
            raise ValueError("mz_arr and int_arr differ in length (%d vs %d)" % (mz_arr.size, int_arr.size))
        if int(n_of_mod) < 0 or int(max_fragment_charge) < 0:
            raise OverflowError("can't convert negative value to size_t")
        pep = np.frombuffer(peptide.encode("utf8"), dtype=np.uint8)
        if aux_mod_pos is not None and aux_mod_mass is not None:
            ap = _check_typed("aux_mod_pos", aux_mod_pos, np.uint32, "unsigned int")
            am = _check_typed("aux_mod_mass", aux_mod_mass, np.float32, "float")
            if ap.size != am.size:
                raise ValueError("aux_mod_pos and aux_mod_mass differ in length")
        else:
            ap = np.zeros(0, np.uint32)
            am = np.zeros(0, np.float32)
        # One PSM through pya_score_one (no plan, no copies: pinned spectrum block, scalars in the kernel
        # arguments, results polled from pinned memory).  The per-signature records behind ``pep_scores`` and
        # ``calculate_ambiguity`` are retained on demand (_ensure_kept): a loop over PSMs that reads only
        # best_sequence / best_score / ascores / alt_sites, like the reference's command line, never pays for them.
        one = self._one
        k = max(1, int(n_of_mod))
        if one is None or one["k"] < k:
            one = dict(k=k, peak_off=np.zeros(2, np.int64), pep_off=np.zeros(2, np.int64),
                       aux_off=np.zeros(2, np.int64), n_of_mod=np.zeros(1, np.int32),
                       max_charge=np.zeros(1, np.int32), best_score=np.zeros(1, np.float32),
                       best_sig=np.zeros(1, np.uint64), n_sig=np.zeros(1, np.int32),
                       ascores=np.zeros((1, k), np.float32), alt_mask=np.zeros((1, k), np.uint64))
            one["batch"] = _lib.Batch(1, _as_ptr(one["peak_off"]), None, _as_ptr(one["pep_off"]),
                                      _as_ptr(one["n_of_mod"]), _as_ptr(one["max_charge"]), None, None,
                                      _as_ptr(one["aux_off"]))
            one["results"] = _lib.Results(k, _as_ptr(one["best_score"]), _as_ptr(one["best_sig"]),
                                          _as_ptr(one["n_sig"]), _as_ptr(one["ascores"]), _as_ptr(one["alt_mask"]))
            self._one = one
        one["ascores"][:] = 0
        one["alt_mask"][:] = 0
        lazy = True
        rc = _lib.PYA_ERR_STATE
        if one["k"] <= 64:
            rc = self._lib.pya_score_one(self._h, mz_arr.ctypes.data, int_arr.ctypes.data, mz_arr.size, pep.ctypes.data,
                                         pep.size, int(n_of_mod), int(max_fragment_charge), ap.ctypes.data, am.ctypes.data,
                                         ap.size, 0, C.byref(one["results"]))
        if rc == _lib.PYA_ERR_STATE and not self._lib.pya_last_error(self._h):
            # (more than 8 fixed modifications: a retained batch of one through the plan machinery)
            lazy = False
            one["peak_off"][1] = mz_arr.size
            one["pep_off"][1] = pep.size
            one["aux_off"][1] = ap.size
            one["n_of_mod"][0] = n_of_mod
            one["max_charge"][0] = max_fragment_charge
            b = one["batch"]
            b.pep = pep.ctypes.data
            b.aux_pos = ap.ctypes.data
            b.aux_mass = am.ctypes.data
            rc = self._lib.pya_score_batch(self._h, C.byref(b), mz_arr.ctypes.data, int_arr.ctypes.data,
                                           _lib.PYA_FLAG_KEEP, C.byref(one["results"]))
        if rc:
            self._last = None
            self._batch_n = None
            self._raise(rc)
        self._batch_n = None if lazy else 1
        self._last = dict(pep=pep, peptide=peptide, k=int(n_of_mod), aux_pos=ap.copy(), aux_mass=am.copy(),
                          best_score=float(one["best_score"][0]), best_sig=int(one["best_sig"][0]),
                          n_sig=int(one["n_sig"][0]), ascores=one["ascores"][0].copy(),
                          alt_mask=one["alt_mask"][0].copy(), lazy=lazy, mz=mz_arr, it=int_arr, z=int(max_fragment_charge))

    def _ensure_kept(self):
        """Retains the per-signature records of the last ``score()`` PSM (its inputs are still where
        pya_score_one staged them)."""
        last = self._last
        if last is not None and last.get("lazy"):
            rc = self._lib.pya_rescore_last_keep(self._h)
            if rc == _lib.PYA_ERR_STATE and not self._lib.pya_last_error(self._h):
                raise RuntimeError("the records of this PSM do not fit the one-PSM kernel; score it with "
                                   "score_batch(keep=True) to read pep_scores")
            if rc:
                self._raise(rc)
            last["lazy"] = False
            self._batch_n = 1

    def score_batch(self, batch, keep=False, skip_invalid=False, evidence=False, ions=False, named=None, sites=False,
                    site_sig_cap=None, probs=False, ranked=None, rollup=None, peptidoforms=None, mz_profile=None,
                    recalibrate=None, deisotope=None, decharge=None, strip=None, centroid=None, coverage=False, markers=None,
                    quant=None, peptidoform_quant=None, purity=None, xic=None):
        """Scores a CSR batch (see pyascore_amd.synth) in one call.

        Returns dict(best_score f32[n], best_sig u64[n], n_sig i32[n], ascores f32[n, max_k],
        alt_mask u64[n, max_k]); row i holds what the reference's properties would hold after
        ``score()`` of PSM i (ascores beyond n_of_mod[i] are 0).

        ``skip_invalid=True``: a PSM that is invalid (unknown residue, empty spectrum, ...) or beyond
        a documented limit of this implementation does not fail the call; it gets best_score -1,
        n_sig -1 and a non-zero code in the extra ``status`` array (include/pyascore_hip.h PYA_PSM_*),
        and ``status_message`` describes the first such PSM.

        ``evidence=True`` adds ``evidence``: a structured array ``[n, max_k]`` (``EVIDENCE_DTYPE``, the 16-byte
        ``pya_evidence`` of include/pyascore_hip.h) with what stands behind every Ascore -- the peak depth it was taken at,
        the site-determining ions possible and matched for the winner and for the competitor, the competitor's position and
        PepScore (``kind``: 0 nothing to compare, 1 counted, 2 the competitor ties the winner).  Every other result is what
        it is without the option.

        ``ions=True`` adds ``ion_off`` (int64 ``[n + 1]``) and ``ions`` (``ION_DTYPE``, the 16-byte ``pya_ion``): the
        records of PSM i are ``ions[ion_off[i]:ion_off[i + 1]]`` -- first every fragment of the best localisation that
        matched a retained peak (``site`` 255), then, for every site whose evidence row is counted, the site-determining
        ions of the winner and of that row's competitor (``site`` = the column, ``flags``: 1 loss variant, 2 the
        competitor's, 4 matched at the row's depth).  Every other result is what it is without the option.

        ``named``: localisations the caller names (``pya_score_batch_named``) -- the search engine's reported sites, a
        known site, a runner-up.  Either the CSR pair ``(q_off int64[n + 1], sig_bits uint64)`` as a tuple, or a list with
        one sequence of signatures per PSM (bit j = the j-th modifiable residue from the N-terminus; ``sig_bits_of`` makes
        them from peptide positions).  Adds ``named_off`` (int64 ``[n + 1]``), ``named`` (``NAMED_DTYPE``, the 32-byte
        ``pya_named``, one record per query in query order: the signature's PepScore and total fragments, its ambiguity
        against the winner -- ``calculate_ambiguity(pep_scores[0], rec)`` -- with depth and site-determining ion counts, and
        ``kind``: 0 PSM not scored, 1 not a site assignment of the PSM, 2 it is the winner, 3 it ties the winner, 4 counted)
        and ``named_counts`` / ``named_scores`` (``[n_q, n_top]``, the cumulative counts and depth scores of ``pep_scores``).
        ``sites=True`` adds ``site_off`` (int64 ``[n + 1]``) and ``sites`` (``SITE_DTYPE``, the 32-byte ``pya_site``): one
        record per modifiable residue of PSM i in ``sites[site_off[i]:site_off[i + 1]]``, N- to C-terminus -- the best
        PepScore among the site assignments that modify the residue and among those that do not, and a site assignment
        that attains each (``pyascore_amd.sites`` has ``deltas``, ``runner_up`` and ``table``).  A PSM with more than
        ``site_sig_cap`` site assignments (default: the library's, ``PYA_FAST_SIGNATURES``; 0: no cap) gets
        ``PYA_SITE_OVER`` records; a PSM that was set aside has none.
        ``probs=True`` adds ``site_off`` (the same offsets), ``site_probs`` (``SITE_PROB_DTYPE``, the 16-byte
        ``pya_site_prob``: per modifiable residue the posterior probability that it is modified, ``with_prob``, and that it
        is not, ``without_prob``) and ``psm_probs`` (``PSM_PROB_DTYPE``, ``[n]``: ``z``, the sum of the likelihood ratios
        10^((PepScore - best) / 10) over the site assignments -- the posterior of the reported localisation is ``1 / z`` --,
        ``n_summed`` and ``kind`` as for ``sites``).  A PepScore-based posterior (MaxQuant's construction), not part of the
        Ascore publication; ``pyascore_amd.probs`` has ``best_prob``, ``table`` and ``annotate``.  ``site_sig_cap`` applies.
        ``ranked=K`` (1 .. 64) adds ``ranked`` (``RANKED_DTYPE``, the 16-byte ``pya_ranked``, shape ``[n, K]``): per PSM its K
        best site assignments in order -- row 0 the reported localisation, the others by PepScore descending, equal scores
        by ascending ``sig_bits``; rows at and beyond ``n_sig`` and the rows of a PSM that was not scored are zero
        (``pyascore_amd.ranked`` has ``lengths``, ``within`` and ``best_tie_size``).  ``site_sig_cap`` applies: a PSM with
        more site assignments has row 0 alone, of kind ``PYA_RANK_OVER``.
        ``rollup=dict(slot=..., n_slots=..., threshold=0.75)`` adds ``rollup`` (``ROLLUP_DTYPE``, the 32-byte
        ``pya_site_rollup``, shape ``[n_slots]``): the residue records of the whole batch collapsed on the device onto the
        caller's slots -- ``slot`` has one int32 per residue record in the records' order (``site_off`` of ``probs=True``;
        negative: left out), see ``pyascore_amd.rollup`` for the slot builders and the table.  ``best_psm`` is in the caller's
        PSM numbering, or in ``psm_id`` (uint32 per PSM) when the dict has it.  ``site_off`` in the dict (the record offsets
        per PSM, ``site_offsets(batch)``) spares a shared batch that is out of spectrum order the pre-pass that finds them.
        ``site_sig_cap`` applies: a PSM over it contributes nothing.

        Every other result is what it is without the option.

        Shared spectra: a batch dict with ``spec_of`` (and ``n_spectra``; ``synth.pack_shared_batch``) holds every
        spectrum once, ``peak_off`` describes the spectra and PSM i is scored against spectrum ``spec_of[i]`` -- the hits
        of one scan (`pyascore/__main__.py`, the hit_depth loop).  Each spectrum is uploaded and binned once; the results
        are those of the repeated-spectrum batch (``synth.expand_shared_batch``), bit for bit.  The library wants the PSMs
        of a spectrum consecutive: a batch in any other order is sorted stably by spectrum, scored, and its rows are put
        back, so the caller always sees input order (with ``keep=True`` such a batch is scored in its expanded form
        instead: the retained records are addressed by PSM number).

        ``peptidoforms=dict(group=..., threshold=0.75, psm_id=None)`` adds ``peptidoforms`` (``PEPTIDOFORM_DTYPE``, the
        48-byte ``pya_peptidoform``): one record per distinct (group, best_sig) of the scored PSMs, ordered by group then
        sig_bits, reduced on the device (``group`` is one non-negative int32 per PSM, e.g. from
        ``pyascore_amd.rollup.peptide_groups``; negative: the PSM is left out).  ``best_psm`` is in the caller's numbering.

        ``mz_profile=dict(run=None, n_slots=1, da_half_width=None, ppm_half_width=50.0, band_width=250.0, max_rank=None)`` adds
        ``mz_profile`` (``pyascore_amd.rollup.MZ_PROFILE_DTYPE``, the 4 128-byte ``pya_mz_profile``, shape ``[n_slots]``): per
        run slot (``run``: one int32 per PSM, negative: left out; None: everything is slot 0) the m/z errors of the matched
        fragments of the reported localisations, counted in 64 bins over ``+-da_half_width`` Da (None: the scorer's
        ``mz_error``) and over ``+-ppm_half_width`` ppm, in 8 bands of ``band_width`` m/z; ``max_rank`` is the deepest peak
        rank counted (None: ``n_top - 1``, every match); ``mz_profile_params`` is the dict of the three inverse widths and
        ``max_rank`` the table was binned with (``pyascore_amd.rollup.mz_profile_params``).  ``pyascore_amd.rollup`` has ``mz_profile_summary``, the host
        restatement ``mz_profile`` and ``merge_mz_profiles``.  The profile only sees errors inside ``+-mz_error`` of this
        scorer: run wide, read the profile, re-run narrow.

        ``recalibrate=dict(calibration=, run=None, band_width=250.0)`` corrects the m/z of every spectrum on the device before
        it is scored (``PYA_FLAG_RECALIBRATE``): ``calibration`` is one ``pyascore_amd.rollup.MZ_CALIBRATION_DTYPE`` record per
        run slot (``fit_mz_calibration`` of a profile), ``run`` one slot per PSM (negative: no correction; None: slot 0),
        ``band_width`` the width of the bands the calibration was fitted over.  Every result is bit-equal to scoring arrays
        corrected by ``pyascore_amd.rollup.recalibrate``; the caller's arrays are not written.  PSMs that share a spectrum
        must agree on its slot.  With ``mz_profile=`` the profile is that of the corrected spectra, the residual errors.  Not
        with ``keep=True`` (the retained records are replayed from the caller's arrays): correct the arrays with
        ``pyascore_amd.rollup.recalibrate`` first.

        ``deisotope=dict(tol=0.01, max_charge=3, step=1.0033548378, ratio=1.0, ratio_per_mz=0.0)`` (or True: the defaults)
        removes isotope satellites from every spectrum before it is scored: the spectra go through ``deisotope_spectra`` once
        (a batch with ``spec_of``: each shared spectrum once) and the ordinary call then runs on the filtered arrays with
        everything else unchanged, so every result is bit-equal to scoring the arrays ``pyascore_amd.rollup.deisotope`` returns.
        That is one extra round trip of the spectra over PCIe.  With ``recalibrate=`` deisotoping comes FIRST: satellites are
        found on the m/z as given, the kept peaks are then corrected.  ``keep=True`` retains the filtered batch.  The
        caller's arrays are not written.

        ``decharge=dict(tol=0.01, max_charge=3, step=1.0033548378, ratio=1.0, ratio_per_mz=0.0, carrier=1.007825, witness=0.3)``
        (or True: the defaults) charge-deconvolves every spectrum before it is scored: deisotoping, and every kept peak whose
        satellites show a charge of 2 or more moved to its m/z at 1+ (``pya_decharge_params``), so that b/y at 1+ finds
        multiply charged fragments: leave ``max_fragment_charge`` at 1 with it.  As with ``deisotope=`` the spectra go through
        ``decharge_spectra`` once (a batch with ``spec_of``: each shared spectrum once) and the ordinary call then runs on the
        result, so every result is bit-equal to scoring the arrays ``pyascore_amd.rollup.decharge`` returns.  That is one extra
        round trip of the spectra over PCIe.  ``decharge=`` contains deisotoping: together with ``deisotope=`` it is a
        ValueError.  Together with ``recalibrate=`` it is a ValueError too: a calibration is a function of the measured m/z
        and must be applied before peaks move -- correct the spectra first (``pya_recalibrate_spectra``,
        ``DevicePlan.recalibrate``, ``pyascore_amd.rollup.recalibrate``).  ``keep=True`` retains the transformed batch.  The
        caller's arrays are not written.

        ``strip=dict(precursor_mz=, precursor_charge=, tol=None, losses=(), reduced=False, isotopes=0, mz_lo=-inf, mz_hi=inf)``
        removes the precursor-derived peaks from every spectrum before it is scored (``pya_strip_params``): the peaks within
        ``tol`` (None: the scorer's ``mz_error``) of the precursor, of the precursor minus each of ``losses`` and -- ``reduced``,
        for ETD -- of the same at every lower charge, each window reaching ``isotopes`` isotope peaks upwards, and the peaks
        outside ``[mz_lo, mz_hi]``.  ``precursor_mz`` / ``precursor_charge`` have one entry per spectrum: per PSM in a private
        batch, per shared spectrum with ``spec_of``; a charge outside 1 .. 8 or an m/z that is not finite and positive gives the
        spectrum no windows.  The spectra go through ``strip_spectra`` once and the ordinary call then runs on the result with
        everything else unchanged, so every result is bit-equal to scoring the arrays ``pyascore_amd.rollup.strip`` returns.
        ``strip=`` comes FIRST, in front of ``deisotope=`` / ``decharge=`` / ``recalibrate=``, and goes with each of them: the
        windows are on the measured m/z, and decharging would move a 2+ precursor.  Each of these steps is a host form of its
        own and costs its own round trip of the spectra over PCIe (measured: 9.3 -> 1.3 M PSMs/s on 100 000 cfg2 PSMs with
        ``strip=`` alone); a caller whose spectra are resident chains the device forms (``pyascore_amd.device.strip``,
        ``.deisotope``, ``.decharge``), which cost about two device copies of the spectra.  ``keep=True`` retains the transformed batch.  The
        caller's arrays are not written.

        ``centroid=dict(gap=, gap_ppm=0.0, half_width=4, min_height=0.0, area=False, select=None)`` centroids profile-mode spectra
        before they are scored (``pya_centroid_params``): every local maximum of a run of samples at most ``gap + gap_ppm 1e-6
        mz`` apart becomes one peak at the intensity-weighted mean m/z of its flanks (``half_width`` samples on either side),
        with the apex's intensity or, with ``area``, the sum; ``select`` (one boolean per spectrum: per PSM in a private batch,
        per shared spectrum with ``spec_of``) leaves the spectra it marks False as they are.  An isolated point is copied, so a
        centroided spectrum passes through.  The spectra go through ``centroid_spectra`` once and the ordinary call then runs
        on the result with everything else unchanged, so every result is bit-equal to scoring the arrays
        ``pyascore_amd.rollup.centroid`` returns.  ``centroid=`` comes FIRST, in front of ``strip=``, and goes with each of
        ``strip=``, ``deisotope=``, ``decharge=`` and ``recalibrate=``: their windows and tolerances are on peaks, not on
        samples.  Like each of them it is a host form of its own and costs ONE EXTRA PCIe ROUND TRIP of the spectra; a caller
        whose spectra are resident chains the device forms (``pyascore_amd.device.centroid`` first).  ``keep=True`` retains the
        transformed batch.  The caller's arrays are not written.

        ``markers=dict(mz=(), losses=(), tol=None, tol_ppm=0.0, precursor_mz=None, precursor_charge=None)`` adds ``markers``
        (``pyascore_amd.rollup.MARKER_DTYPE``, the 24-byte ``pya_marker``, shape ``[n_spectra, n_targets]``) and
        ``marker_spectra`` (``MARKER_SPECTRUM_DTYPE``, the 32-byte ``pya_marker_spectrum``, shape ``[n_spectra]``): per spectrum
        and target the most intense peak within ``tol`` (None: the scorer's ``mz_error``) plus ``tol_ppm`` of the target -- the
        fixed m/z of ``mz`` first (reporter ions, immonium ions), then the precursor minus each of ``losses`` -- and per spectrum
        the ion current and the base peak (``pya_marker_params``).  One row per spectrum: per PSM in a private batch, per shared
        spectrum with ``spec_of``, as the precursors of ``strip=`` are; ``precursor_mz`` / ``precursor_charge`` are needed
        iff there are ``losses``.  The stage is READ-ONLY: it runs behind ``centroid=`` and in front of ``strip=``,
        ``deisotope=``, ``decharge=`` and ``recalibrate=`` -- it sees the peaks strip is about to cut --, goes with all of
        them, and every other result of the call is bit-equal with and without it.  It goes through ``marker_spectra`` once,
        which costs ONE EXTRA UPLOAD of the spectra over PCIe (only the records come back; measured: 9.4 -> 3.7 M PSMs/s on
        100 000 cfg2 PSMs with 18 targets); a caller whose spectra are resident
        uses ``pyascore_amd.device.markers``.  ``pyascore_amd.rollup.markers`` gives the same bytes on the host and
        ``pyascore_amd.rollup.marker_matrix`` the intensities as a matrix.

        ``quant=dict(values=, row=None, threshold=0.75, scale_log2=10, complete_only=False)`` -- beside ``rollup=``, whose slots it
        uses; without it a ValueError -- adds ``quant_head`` (``pyascore_amd.rollup.SITE_QUANT_HEAD_DTYPE``, shape ``[n_slots]``),
        ``quant`` (``SITE_QUANT_DTYPE``, shape ``[n_slots, n_channels]``) and ``quant_params``: per slot and channel the summed
        reading of the PSMs that place the modification on the site with ``with_prob >= threshold`` (``PYA_FLAG_QUANT``,
        ``pya_site_quant``).  ``values``: float64 ``[n_rows, n_channels]``, one row per spectrum; ``row``: the row of every PSM
        (negative: left out), None: PSM i has row i.  With ``values=None`` beside ``markers=`` the channels are the fixed targets of
        ``markers=``, the matrix ``marker_matrix`` of that call's records and ``row`` the batch's ``spec_of`` (the PSM index
        without one).  The sums are integers in units of ``2^-scale_log2`` (``pyascore_amd.rollup.site_quant_sums`` turns them
        into intensities), so the table does not depend on chunk cuts, route or order, and tables of several calls merge by
        adding (``merge_site_quant``); ``pyascore_amd.rollup.site_quant`` gives the same bytes on the host.

        ``channels=dict(matrix=None, normalize=False, select=None)`` inside ``quant=`` (and, the same key, inside
        ``peptidoform_quant=``) corrects the channel matrix before it is summed (the channel correction of
        ``include/pyascore_hip.h``): ``matrix`` float64 ``[n_channels, n_channels]``, the inverse of the reagent lot's spill
        matrix (``pyascore_amd.rollup.channel_matrix``), takes the isotope impurities out of every row; ``normalize=True`` then
        brings the column totals -- over the rows ``select`` names, one boolean per row, None: all -- to the largest one.  The
        matrix (given, or made from ``markers=``) goes through ``correct_channels`` first: ONE EXTRA ROUND TRIP OF THE MATRIX to
        the device and back, before the batch call uploads it again (one for both options where they name the same matrix
        and the same ``channels=``, one each otherwise).  Adds ``quant_channel_sums`` (``SITE_QUANT_DTYPE``, shape
        ``[n_channels]``: the column sums behind the factors) and ``quant_channel_factors`` (float64 ``[n_channels]``, None
        without ``normalize``) -- under ``peptidoform_quant_channel_...`` for that option; every other result is what the
        call gives for ``values=`` the corrected matrix.  Unknown keys and a matrix of another shape are a ValueError before
        anything is scored.

        ``peptidoform_quant=dict(values=, row=None, threshold=0.75, scale_log2=10, complete_only=False)`` -- beside
        ``peptidoforms=``, whose list it is row-aligned with; without it a ValueError -- adds ``peptidoform_quant_head``
        (``SITE_QUANT_HEAD_DTYPE``, shape ``[n_list]``), ``peptidoform_quant`` (``SITE_QUANT_DTYPE``, shape ``[n_list,
        n_channels]``) and ``peptidoform_quant_params``: per peptidoform and channel the summed reading of the PSMs that
        contribute to the list with ``min_prob >= threshold`` (``PYA_FLAG_PFORM_QUANT``, the peptidoform quantification of
        ``include/pyascore_hip.h``).  ``values``, ``row`` and the parameters are those of ``quant=``; ``values=None`` beside
        ``markers=`` takes the fixed targets of that call.  ``peptidoforms`` is exactly what the call returns without the
        option; it goes together with ``rollup=`` / ``quant=`` in one call.  Two pairs merge by
        ``peptidoform_quant_reduce`` or ``pyascore_amd.rollup.merge_peptidoform_quant``; ``pyascore_amd.rollup.peptidoform_quant``
        gives the same bytes on the host.

        ``purity=dict(ms1_mz=, ms1_intensity=, ms1_peak_off=, survey=, precursor_mz=, precursor_charge=, window_lo=, window_hi=,
        tol=0.0, tol_ppm=10.0, isotopes=3, below=0, step=, gate=None)`` adds ``purity`` (``pyascore_amd.rollup.PURITY_DTYPE``, the
        48-byte ``pya_purity``, shape ``[n_spectra]``): per spectrum the intensity of its isolation window in the survey (MS1)
        spectrum ``survey`` names and the part of it at the selected m/z and its isotope positions (``pya_purity_params``;
        ``pyascore_amd.rollup.survey_index`` finds ``survey``, ``purity_ratio`` divides).  One entry per spectrum, as ``markers=``
        has its precursors.  It is handled behind ``markers=`` and in front of ``channels=``: without ``gate`` every other result
        of the call is bit-equal with and without it.  ``gate=dict(threshold=, keep_unknown=True)`` also adds ``purity_pass``
        (uint8 ``[n_spectra]``) and sends the matrix of ``quant=`` / ``peptidoform_quant=`` -- given, or made from ``markers=``;
        one row per spectrum -- through ``pyascore_amd.rollup.purity_gate`` on the host, where the matrix is at that point: the
        readings of a failing spectrum become NaN, and ``purity_pass`` is ANDed into the ``select`` of a ``channels=`` that
        normalizes.  A ``gate`` without ``quant=`` / ``peptidoform_quant=`` is a ValueError.  A caller whose spectra are resident
        uses ``pyascore_amd.device.purity`` / ``purity_gate``; ``pyascore_amd.rollup.purity`` gives the same bytes on the host.

        ``xic=dict(ms1_mz=, ms1_intensity=, ms1_peak_off=, rt=, seed=, scan_lo=, scan_hi=, precursor_mz=, precursor_charge=, tol=0.0,
        tol_ppm=10.0, isotopes=2, step=, rise=2.0, max_gap=1)`` adds ``xic`` (``pyascore_amd.rollup.XIC_DTYPE``, the 64-byte
        ``pya_xic``, shape ``[n_spectra]``): per spectrum the label-free MS1 intensity of its precursor -- area, apex and sum of
        its chromatographic peak over the survey scans ``[scan_lo, scan_hi)`` around the survey scan ``seed``
        (``pya_xic_params``; ``rt`` the survey scans' retention times in seconds; ``pyascore_amd.rollup.survey_index`` finds
        ``seed``, ``xic_windows`` the windows).  READ-ONLY over the survey spectra: every other result of the call is bit-equal
        with and without it.  ``quant=dict(values="xic_area" | "xic_apex", ...)`` and the same on ``peptidoform_quant=`` take that
        column (``pyascore_amd.rollup.xic_values``) as their one channel: a label-free site or peptidoform table.  The survey
        spectra are uploaded once per request: ``purity=`` beside ``xic=`` uploads them a second time (sharing the upload is
        not built).  A resident pipeline uses ``pyascore_amd.device.xic_survey_check`` / ``xic`` / ``xic_values``;
        ``pyascore_amd.rollup.xic`` gives the same bytes on the host.

        ``coverage=True`` adds ``coverage`` (``COVERAGE_DTYPE``, the 64-byte ``pya_coverage``, shape ``[n]``): per PSM the ion
        current of its spectrum and the part of it that the matched fragments of the reported localisation explain, in all and
        from either terminus, beside peak, fragment and bond counts (``pyascore_amd.rollup.coverage_ratios`` makes the ratios,
        ``pyascore_amd.rollup.coverage`` is the host restatement).  It is taken on the spectra that were scored: with a
        transform or ``recalibrate=`` on the transformed arrays.  It goes with every other option.

        Typed spectra: ``batch["mz"]`` / ``batch["intensity"]`` of dtype float32 go to the device as they are (float64
        m/z with float32 intensities, as mzML holds them, or both float32: 12 or 8 bytes per peak over PCIe instead of 16;
        ``pya_score_batch_typed``).  float32 -> float64 is exact and the kernels widen at the load, so the results are those
        of the widened arrays, bit for bit.  Any other dtype is converted to float64, as is a float32 m/z array beside
        float64 intensities."""
        def again(done, spectra, **changed):
            """the call itself on what a transform returned, the transform taken out of the request"""
            rest = dict(keep=keep, skip_invalid=skip_invalid, evidence=evidence, ions=ions, named=named, sites=sites,
                        site_sig_cap=site_sig_cap, probs=probs, ranked=ranked, rollup=rollup, peptidoforms=peptidoforms,
                        mz_profile=mz_profile, recalibrate=recalibrate, deisotope=deisotope, decharge=decharge, strip=strip,
                        centroid=centroid, coverage=coverage, markers=markers, quant=quant,
                        peptidoform_quant=peptidoform_quant, purity=purity, xic=xic)
            rest.update(changed)
            if done is not None:
                rest[done] = None
            return self.score_batch(dict(batch, mz=spectra[0], intensity=spectra[1], peak_off=spectra[2]), **rest)

        labelfree = {name: req["values"] for name, req in (("quant", quant), ("peptidoform_quant", peptidoform_quant))
                     if isinstance(req, dict) and isinstance(req.get("values"), str)}
        for name, column in labelfree.items():
            if column not in XIC_CHANNELS:
                raise ValueError(name + ": values is a matrix, or one of " + ", ".join(repr(k) for k in XIC_CHANNELS) + " beside xic=")
            if xic is None or xic is False:
                raise ValueError(name + ": values = %r needs xic= in the same call" % column)
        if xic is not None and xic is not False:
            # (in front of everything: the stage reads the survey spectra alone, and the column it gives is a matrix to all that
            # follows.  What follows is checked on a column of the same shape first, so that a refusal launches nothing.)
            from .rollup import xic_values
            params, survey_spectra, survey_rt, queries = _xic_request(xic, _n_spectra(batch))
            blank = np.zeros((queries[0].size, 1))
            checks = {name: dict(req, values=blank) if name in labelfree else req
                      for name, req in (("quant", quant), ("peptidoform_quant", peptidoform_quant))}
            for name, req in checks.items():
                _channels_request(name, req, markers)
            if purity is not None and purity is not False:
                _purity_request(purity, _n_spectra(batch), any(isinstance(req, dict) for req in checks.values()))
            records, _ = self.precursor_xic(*survey_spectra, survey_rt, *queries, params)
            # (the rows of the column are the spectra, as beside markers=: a shared batch's PSMs name theirs by spec_of)
            spec_row = None if batch.get("spec_of") is None else np.asarray(batch["spec_of"]).astype(np.int32)
            changed = {name: dict(checks[name], values=xic_values(records, XIC_CHANNELS[column]).reshape(-1, 1),
                                  row=spec_row if checks[name].get("row") is None else checks[name]["row"])
                       for name, column in labelfree.items()}
            res = again("xic", (batch["mz"], batch["intensity"], batch["peak_off"]), **changed)
            res["xic"] = records
            return res
        channel_reqs = {name: _channels_request(name, req, markers)
                        for name, req in (("quant", quant), ("peptidoform_quant", peptidoform_quant))}
        if purity is not None and purity is not False:
            # (refused before anything is launched, whatever stands in front of it)
            purity_req = _purity_request(purity, _n_spectra(batch), isinstance(quant, dict) or isinstance(peptidoform_quant, dict))
        if centroid is not None and centroid is not False:
            params, select = _centroid_request(centroid, _n_spectra(batch))
            return again("centroid", self.centroid_spectra(batch["mz"], batch["intensity"], _batch_peak_off(batch), params, select))
        if markers is not None and markers is not False:
            params, prec_mz, prec_z = _markers_request(markers, self._mz_error, _n_spectra(batch))
            records, spectra, _ = self.marker_spectra(batch["mz"], batch["intensity"], _batch_peak_off(batch), params, prec_mz, prec_z)
            changed = {}
            for name, req in (("quant", quant), ("peptidoform_quant", peptidoform_quant)):
                if isinstance(req, dict) and req.get("values") is None:
                    changed[name] = _marker_channels(name, req, params, records, batch.get("spec_of"))
            res = again("markers", (batch["mz"], batch["intensity"], batch["peak_off"]), **changed)
            res["markers"], res["marker_spectra"] = records, spectra
            return res
        if purity is not None and purity is not False:
            # (behind markers=: the matrix is there by now; in front of channels=, which corrects what the gate leaves)
            from .rollup import purity_gate
            params, survey_spectra, queries, gate = purity_req
            records, _ = self.precursor_purity(*survey_spectra, *queries, params)
            changed, extra = {}, {"purity": records}
            if gate is not None:
                passed, _ = purity_gate(records, *gate)
                extra["purity_pass"] = passed
                for name, req in (("quant", quant), ("peptidoform_quant", peptidoform_quant)):
                    if not isinstance(req, dict):
                        continue
                    if req.get("values") is None:
                        raise ValueError(name + ": values is missing (a float64 matrix, one row per spectrum and one column per channel)")
                    try:
                        values = np.ascontiguousarray(req["values"], np.float64)
                    except (TypeError, ValueError):
                        raise ValueError(name + ": values is a matrix of numbers") from None
                    if values.ndim != 2 or values.shape[0] != records.size:
                        raise ValueError(name + ": beside a purity gate values has one row per spectrum, as the purity records have")
                    req = dict(req, values=purity_gate(records, *gate, values=values)[1])
                    ch = channel_reqs[name]
                    if ch is not None and ch["normalize"]:
                        if ch["select"] is not None and ch["select"].size != passed.size:
                            raise ValueError(name + ": channels: select is one boolean per row of values")
                        req["channels"] = dict(req["channels"], select=passed if ch["select"] is None else passed & ch["select"])
                    changed[name] = req
            res = again("purity", (batch["mz"], batch["intensity"], batch["peak_off"]), **changed)
            res.update(extra)
            return res
        if any(ch is not None for ch in channel_reqs.values()):
            # (behind markers=: the matrix is there by now; in front of everything that scores)
            changed, extra, done = {}, {}, []
            for name, req, have in (("quant", quant, rollup is not None), ("peptidoform_quant", peptidoform_quant, peptidoforms is not None)):
                ch = channel_reqs[name]
                if ch is None:
                    continue
                plain = {k: v for k, v in req.items() if k != "channels"}
                checked = _quant_request(plain, int(batch["n_psm"]), have, name)
                key = (checked["values"].shape, checked["values"].tobytes(), None if ch["matrix"] is None else ch["matrix"].tobytes(),
                       ch["normalize"], None if ch["select"] is None else ch["select"].tobytes(), checked["params"]["scale_log2"])
                # (both options over one matrix with one request, as beside markers=: one round trip serves both)
                result = next((r for k, r in done if k == key), None)
                if result is None:
                    result = self.correct_channels(checked["values"], ch["matrix"], ch["normalize"], ch["select"], checked["params"]["scale_log2"])
                    done.append((key, result))
                changed[name] = dict(plain, values=result[0])
                extra[name + "_channel_sums"], extra[name + "_channel_factors"] = result[1], result[2]
            res = again(None, (batch["mz"], batch["intensity"], batch["peak_off"]), **changed)      # (no transform served: the same spectra)
            res.update(extra)
            return res
        if strip is not None and strip is not False:
            params, prec_mz, prec_z = _strip_request(strip, self._mz_error, _n_spectra(batch))
            return again("strip", self.strip_spectra(batch["mz"], batch["intensity"], _batch_peak_off(batch), prec_mz, prec_z,
                                                     params))
        if decharge is not None and decharge is not False:
            if deisotope is not None and deisotope is not False:
                raise ValueError("decharge= contains deisotoping (its kept peaks are those of deisotope=): pass one of the two")
            if recalibrate is not None:
                raise ValueError("decharge= cannot be combined with recalibrate=: " + _RECALIBRATE_FIRST)
            params = _decharge_request(decharge)
            return again("decharge", self.decharge_spectra(batch["mz"], batch["intensity"], _batch_peak_off(batch), params))
        if deisotope is not None and deisotope is not False:
            params = _deisotope_request(deisotope)
            return again("deisotope", self.deisotope_spectra(batch["mz"], batch["intensity"], _batch_peak_off(batch), params))
        ranked_k = None if ranked is None or ranked is False else check_ranked_k(ranked)
        roll = None if rollup is None else _rollup_request(rollup, int(batch["n_psm"]))
        pform = None if peptidoforms is None else _peptidoform_request(peptidoforms, int(batch["n_psm"]))
        mzp = None if mz_profile is None or mz_profile is False else _mz_profile_request(mz_profile, int(batch["n_psm"]), self._mz_error,
                                                                                        self._n_top)
        recal = None if recalibrate is None else _recalibrate_request(recalibrate, int(batch["n_psm"]))
        qu = None if quant is None or quant is False else _quant_request(quant, int(batch["n_psm"]), roll is not None)
        pfq = None if peptidoform_quant is None or peptidoform_quant is False else \
            _quant_request(peptidoform_quant, int(batch["n_psm"]), pform is not None, "peptidoform_quant")
        if recal is not None and keep:
            raise ValueError("recalibrate does not go with keep=True: correct the arrays with pyascore_amd.rollup.recalibrate and "
                             "retain the batch without it")
        if batch.get("spec_of") is not None:
            from .synth import expand_shared_batch, spectrum_order, take_psms
            perm, inv = spectrum_order(batch["spec_of"])
            if perm is not None and keep:
                return self.score_batch(expand_shared_batch(batch), keep=True, skip_invalid=skip_invalid, evidence=evidence, ions=ions,
                                        named=named, sites=sites, site_sig_cap=site_sig_cap, probs=probs, ranked=ranked, rollup=rollup,
                                        peptidoforms=peptidoforms, mz_profile=mz_profile, coverage=coverage, quant=quant,
                                        peptidoform_quant=peptidoform_quant)
            if perm is not None:
                moved = None
                if named is not None:        # the queries travel with their PSMs, the records come back to the caller's order
                    q_off, q_bits = query_csr(named, int(batch["n_psm"]))
                    moved = take_queries(q_off, q_bits, perm)
                roll_moved = None
                if roll is not None:         # the slots travel with their PSMs, the ids say who they were
                    r_off = roll["site_off"]
                    if r_off is None:
                        r_off = self.site_offsets(batch, skip_invalid)
                    if r_off.size != perm.size + 1 or int(r_off[-1]) != roll["slot"].size:
                        raise ValueError("rollup: %d slots do not match the residue records of the batch; pass their offsets "
                                         "per PSM as site_off" % roll["slot"].size)
                    n_rec = np.diff(r_off)[perm]
                    new_off = np.concatenate([[0], np.cumsum(n_rec)]).astype(np.int64)
                    take = np.repeat(r_off[:-1][perm] - new_off[:-1], n_rec) + np.arange(int(n_rec.sum()))
                    ids = perm.astype(np.uint32) if roll["psm_id"] is None else roll["psm_id"][perm]
                    roll_moved = dict(slot=roll["slot"][take], n_slots=roll["n_slots"], threshold=roll["threshold"], psm_id=ids,
                                      site_off=new_off)
                pform_moved = None
                if pform is not None:        # the groups travel with their PSMs, the ids say who they were
                    pform_moved = dict(group=pform["group"][perm], threshold=pform["threshold"],
                                       psm_id=perm.astype(np.uint32) if pform["psm_id"] is None else pform["psm_id"][perm])
                mzp_moved = None
                if mzp is not None:          # the run slots travel with their PSMs
                    mzp_moved = dict(mz_profile if isinstance(mz_profile, dict) else {})
                    if mzp["run"] is not None:
                        mzp_moved["run"] = mzp["run"][perm]
                quant_moved = None
                if qu is not None:           # the rows travel with their PSMs
                    quant_moved = dict(quant, values=qu["values"], row=perm.astype(np.int32) if qu["row"] is None else qu["row"][perm])
                pfq_moved = None
                if pfq is not None:
                    pfq_moved = dict(peptidoform_quant, values=pfq["values"],
                                     row=perm.astype(np.int32) if pfq["row"] is None else pfq["row"][perm])
                recal_moved = None
                if recal is not None:        # ... and so do the slots of the calibration
                    recal_moved = dict(calibration=recal["cal"], band_width=recal["band_width"],
                                       run=None if recal["run"] is None else recal["run"][perm])
                try:
                    res = self.score_batch(take_psms(batch, perm), skip_invalid=skip_invalid, evidence=evidence, ions=ions,
                                           named=None if moved is None else (moved[0], moved[1]), sites=sites,
                                           site_sig_cap=site_sig_cap, probs=probs, ranked=ranked, rollup=roll_moved,
                                           peptidoforms=pform_moved, mz_profile=mzp_moved, recalibrate=recal_moved,
                                           coverage=coverage, quant=quant_moved, peptidoform_quant=pfq_moved)
                except ValueError as e:
                    raise ValueError(_renumber_psm(str(e), perm)) from None
                csr = (res.pop("ion_off"), res.pop("ions")) if ions else None
                site_csr = (res["site_off"], res.pop("sites")) if sites else None
                prob_csr = (res["site_off"], res.pop("site_probs")) if probs else None
                res.pop("site_off", None)
                table = res.pop("rollup", None)         # (per slot, not per PSM)
                forms = res.pop("peptidoforms", None)   # (per peptidoform)
                profile = res.pop("mz_profile", None)   # (per run slot)
                profile_params = res.pop("mz_profile_params", None)
                per_slot = {k: res.pop(k) for k in ("quant_head", "quant", "quant_params", "peptidoform_quant_head", "peptidoform_quant",
                                                    "peptidoform_quant_params") if k in res}   # (per roll-up slot, per peptidoform)
                per_query = {k: res.pop(k) for k in ("named_off", "named", "named_counts", "named_scores") if k in res}
                res = {k: (v[inv] if isinstance(v, np.ndarray) else v) for k, v in res.items()}
                if moved is not None:
                    res["named_off"] = q_off
                    for k in ("named", "named_counts", "named_scores"):
                        res[k] = np.zeros_like(per_query[k])
                        res[k][moved[2]] = per_query[k]
                if ions:                     # the ranges of the PSMs, back in input order
                    n_rec = np.diff(csr[0])[inv]
                    res["ion_off"] = np.concatenate([[0], np.cumsum(n_rec)]).astype(np.int64)
                    take = np.repeat(csr[0][:-1][inv] - res["ion_off"][:-1], n_rec) + np.arange(int(n_rec.sum()))
                    res["ions"] = csr[1][take]
                if sites:
                    n_rec = np.diff(site_csr[0])[inv]
                    res["site_off"] = np.concatenate([[0], np.cumsum(n_rec)]).astype(np.int64)
                    take = np.repeat(site_csr[0][:-1][inv] - res["site_off"][:-1], n_rec) + np.arange(int(n_rec.sum()))
                    res["sites"] = site_csr[1][take]
                if probs:                    # (psm_probs is per PSM: it came back with the other per-PSM arrays)
                    n_rec = np.diff(prob_csr[0])[inv]
                    res["site_off"] = np.concatenate([[0], np.cumsum(n_rec)]).astype(np.int64)
                    take = np.repeat(prob_csr[0][:-1][inv] - res["site_off"][:-1], n_rec) + np.arange(int(n_rec.sum()))
                    res["site_probs"] = prob_csr[1][take]
                if table is not None:
                    res["rollup"] = table
                if forms is not None:
                    res["peptidoforms"] = forms
                if profile is not None:
                    res["mz_profile"], res["mz_profile_params"] = profile, profile_params
                res.update(per_slot)
                if res.get("status_message"):
                    res["status_message"] = _renumber_psm(res["status_message"], perm)
                return res
        # the records behind pep_scores / calculate_ambiguity of the last score() PSM are produced on demand by
        # replaying what score() staged in the library: before another call reuses that staging, produce them
        self._ensure_kept()
        n = int(batch["n_psm"])
        mz, it = _typed_spectra(batch["mz"], batch["intensity"])
        arrs = dict(
            peak_off=np.ascontiguousarray(batch["peak_off"], np.int64),
            pep=np.ascontiguousarray(batch["pep"], np.uint8),
            pep_off=np.ascontiguousarray(batch["pep_off"], np.int64),
            n_of_mod=np.ascontiguousarray(batch["n_of_mod"], np.int32),
            max_charge=np.ascontiguousarray(batch["max_charge"], np.int32),
            aux_pos=np.ascontiguousarray(batch["aux_pos"], np.uint32),
            aux_mass=np.ascontiguousarray(batch["aux_mass"], np.float32),
            aux_off=np.ascontiguousarray(batch["aux_off"], np.int64))
        spec_of = None
        n_spec = n
        if batch.get("spec_of") is not None:
            spec_of = np.ascontiguousarray(batch["spec_of"], np.uint32)
            n_spec = int(batch.get("n_spectra", arrs["peak_off"].size - 1))
            if spec_of.size != n or arrs["peak_off"].size != n_spec + 1:
                raise ValueError("a shared batch has one spec_of entry per PSM and n_spectra + 1 peak offsets")
        if arrs["peak_off"].size != n_spec + 1 or arrs["pep_off"].size != n + 1 or arrs["aux_off"].size != n + 1:
            raise ValueError("offset arrays must have n_psm + 1 entries")
        if n and (mz.size < arrs["peak_off"][-1] or it.size < arrs["peak_off"][-1]):
            raise ValueError("peak_off runs past the end of the spectrum arrays")
        max_k = max(1, int(arrs["n_of_mod"].max())) if n else 1
        out = dict(best_score=np.zeros(n, np.float32), best_sig=np.zeros(n, np.uint64),
                   n_sig=np.zeros(n, np.int32), ascores=np.zeros((n, max_k), np.float32),
                   alt_mask=np.zeros((n, max_k), np.uint64))
        nq = None
        if named is not None:
            q_off, q_bits = query_csr(named, n)
            n_q = max(int(q_off[-1]), 0) if q_off.size else 0
            out["named_off"] = q_off
            out["named"] = np.zeros(n_q, NAMED_DTYPE)
            out["named_counts"] = np.zeros((n_q, self._n_top), np.int32)
            out["named_scores"] = np.zeros((n_q, self._n_top), np.float32)
            nq = (q_off, q_bits, out["named"], out["named_counts"], out["named_scores"])
        if n == 0:
            if evidence:
                out["evidence"] = np.zeros((0, max_k), EVIDENCE_DTYPE)
            if ions:
                out["ion_off"], out["ions"] = np.zeros(1, np.int64), np.zeros(0, ION_DTYPE)
            if sites:
                out["site_off"], out["sites"] = np.zeros(1, np.int64), np.zeros(0, SITE_DTYPE)
            if probs:
                out["site_off"], out["site_probs"], out["psm_probs"] = np.zeros(1, np.int64), np.zeros(0, SITE_PROB_DTYPE), np.zeros(0, PSM_PROB_DTYPE)
            if ranked_k:
                out["ranked"] = np.zeros((0, ranked_k), RANKED_DTYPE)
            if roll is not None:
                if roll["slot"].size:
                    raise ValueError("rollup: %d slots for a batch without residue records" % roll["slot"].size)
                out["rollup"] = np.zeros(roll["n_slots"], ROLLUP_DTYPE)
                out["rollup"]["best_psm"] = _lib.PYA_ROLLUP_NO_PSM
            if pform is not None:
                out["peptidoforms"] = np.zeros(0, PEPTIDOFORM_DTYPE)
            if mzp is not None:
                out["mz_profile"] = np.zeros(mzp["n_slots"], np.dtype(_lib.MZ_PROFILE_DTYPE))
                out["mz_profile_params"] = dict(mzp["params"])
            if coverage:
                out["coverage"] = np.zeros(0, COVERAGE_DTYPE)
            if qu is not None:
                from .rollup import empty_site_quant
                out["quant_head"], out["quant"] = empty_site_quant(roll["n_slots"], qu["params"]["n_channels"])
                out["quant_params"] = dict(qu["params"])
            if pfq is not None:
                from .rollup import empty_site_quant
                out["peptidoform_quant_head"], out["peptidoform_quant"] = empty_site_quant(0, pfq["params"]["n_channels"])
                out["peptidoform_quant_params"] = dict(pfq["params"])
            return out
        b = _lib.Batch(n, _as_ptr(arrs["peak_off"]), _as_ptr(arrs["pep"]), _as_ptr(arrs["pep_off"]),
                       _as_ptr(arrs["n_of_mod"]), _as_ptr(arrs["max_charge"]), _as_ptr(arrs["aux_pos"]),
                       _as_ptr(arrs["aux_mass"]), _as_ptr(arrs["aux_off"]))
        r = _lib.Results(max_k, _as_ptr(out["best_score"]), _as_ptr(out["best_sig"]), _as_ptr(out["n_sig"]),
                         _as_ptr(out["ascores"]), _as_ptr(out["alt_mask"]))
        # A retained batch is ONE plan on the device.  When its records do not fit the workspace budget the batch is
        # scored without them (chunked and pipelined like any big call) and batch_pep_scores() re-scores the range it
        # is asked for, a budget's worth of PSMs at a time: the export works for any batch size.
        self._lazy_batch = None
        lazy_keep = False
        if keep and n > 1:
            budget = int(self._lib.pya_get_workspace_budget(self._h))
            try:
                # (a shared batch: priced, and re-scored by batch_pep_scores(), in its expanded form)
                lazy_arrs = arrs if spec_of is None else dict(arrs, peak_off=np.concatenate(
                    [[0], np.cumsum(np.diff(arrs["peak_off"])[spec_of])]).astype(np.int64))
                per_psm = self._retained_bytes(dict(lazy_arrs, n_of_mod=arrs["n_of_mod"]), mz.itemsize + it.itemsize)
                lazy_keep = float(per_psm.sum()) > 0.8 * budget
            except (IndexError, ValueError):
                lazy_keep = False            # malformed offsets: the library's own validation reports them
        flags = (_lib.PYA_FLAG_KEEP if keep and not lazy_keep else 0) | (_lib.PYA_FLAG_SKIP_INVALID if skip_invalid else 0) | \
            (_lib.PYA_FLAG_EVIDENCE if evidence else 0) | (_lib.PYA_FLAG_IONS if ions else 0) | (_lib.PYA_FLAG_SITES if sites else 0) | \
            (_lib.PYA_FLAG_PROBS if probs else 0) | (_lib.PYA_FLAG_RANKED if ranked_k else 0) | \
            (_lib.PYA_FLAG_ROLLUP if roll is not None else 0) | (_lib.PYA_FLAG_PEPTIDOFORMS if pform is not None else 0) | \
            (_lib.PYA_FLAG_MZ_PROFILE if mzp is not None else 0) | (_lib.PYA_FLAG_RECALIBRATE if recal is not None else 0) | \
            (_lib.PYA_FLAG_COVERAGE if coverage else 0) | (_lib.PYA_FLAG_QUANT if qu is not None else 0) | \
            (_lib.PYA_FLAG_PFORM_QUANT if pfq is not None else 0)
        # for this call; the handle's own settings come back
        cap_before = k_before = None
        if (sites or probs or ranked_k or roll is not None or pform is not None) and site_sig_cap is not None:
            cap_before = int(self._lib.pya_get_site_sig_cap(self._h))
            self._lib.pya_set_site_sig_cap(self._h, int(site_sig_cap))
        if ranked_k:
            k_before = int(self._lib.pya_get_ranked_k(self._h))
            self._lib.pya_set_ranked_k(self._h, ranked_k)
        try:
            # (the library borrows the arrays of `roll` for the call: they live until it returns)
            rc = 0 if roll is None else self._lib.pya_set_rollup(self._h, _as_ptr(roll["slot"]), roll["slot"].size, roll["n_slots"],
                                                                 roll["threshold"], _as_ptr(roll["psm_id"]))
            if not rc and pform is not None:
                rc = self._lib.pya_set_peptidoforms(self._h, _as_ptr(pform["group"]), n, pform["threshold"], _as_ptr(pform["psm_id"]))
            if not rc and mzp is not None:
                rc = self._lib.pya_set_mz_profile(self._h, _as_ptr(mzp["run"]), n, mzp["n_slots"], C.byref(mzp["c_params"]))
            if not rc and recal is not None:
                rc = self._lib.pya_set_recalibration(self._h, _as_ptr(recal["run"]), n, _as_ptr(recal["cal"]), recal["cal"].size,
                                                     recal["inv_band"])
            if not rc and qu is not None:
                rc = self._lib.pya_set_site_quant(self._h, _as_ptr(qu["values"]), qu["values"].shape[0], _as_ptr(qu["row"]), n,
                                                  C.byref(qu["c_params"]))
            if not rc and pfq is not None:
                rc = self._lib.pya_set_peptidoform_quant(self._h, _as_ptr(pfq["values"]), pfq["values"].shape[0], _as_ptr(pfq["row"]), n,
                                                         C.byref(pfq["c_params"]))
            if not rc:
                rc = self._score_batch_call(b, spec_of, n_spec, mz, it, flags, r, nq)
        finally:
            if cap_before is not None:
                self._lib.pya_set_site_sig_cap(self._h, cap_before)
            if k_before is not None:
                self._lib.pya_set_ranked_k(self._h, k_before)
        if rc:
            self._raise(rc)
        self._batch_n = n if keep else None
        if keep:
            self._last = None        # the handle's retained plan now belongs to this batch, not to score()'s PSM
        if lazy_keep:
            # (references, not copies: a batch this size is gigabytes.  The arrays must not be modified before
            # batch_pep_scores() has been read -- it re-scores the ranges it is asked for from them.)
            self._lazy_batch = dict(arrs, mz=mz, intensity=it, n_psm=n, per_psm=per_psm, budget=budget)
            if spec_of is not None:
                from .synth import expand_shared_batch
                self._lazy_batch = expand_shared_batch(dict(self._lazy_batch, spec_of=spec_of))
        if skip_invalid:
            out["status"] = np.zeros(n, np.int32)
            rc = self._lib.pya_last_batch_status(self._h, _as_ptr(out["status"]), n)
            if rc:
                self._raise(rc)
            out["status_message"] = (self._lib.pya_last_error(self._h).decode("utf8", "replace")
                                     if out["status"].any() else "")
        if evidence:
            out["evidence"] = np.zeros((n, max_k), EVIDENCE_DTYPE)
            rc = self._lib.pya_last_batch_evidence(self._h, _as_ptr(out["evidence"]), n, max_k)
            if rc:
                self._raise(rc)
        if ions:
            out["ion_off"], out["ions"] = self._last_batch_ions(n)
        if sites:
            out["site_off"], out["sites"] = self._last_batch_sites(n)
        if probs:
            out["site_off"], out["site_probs"], out["psm_probs"] = self._last_batch_probs(n)
        if ranked_k:
            out["ranked"] = np.zeros((n, ranked_k), RANKED_DTYPE)
            rc = self._lib.pya_last_batch_ranked(self._h, _as_ptr(out["ranked"]), n, ranked_k)
            if rc:
                self._raise(rc)
        if roll is not None:
            out["rollup"] = np.zeros(roll["n_slots"], ROLLUP_DTYPE)
            rc = self._lib.pya_last_batch_rollup(self._h, _as_ptr(out["rollup"]), roll["n_slots"])
            if rc:
                self._raise(rc)
        if pform is not None:
            count = C.c_uint64(0)
            out["peptidoforms"] = np.zeros(n, PEPTIDOFORM_DTYPE)       # (a list is no longer than the batch)
            rc = self._lib.pya_last_batch_peptidoforms(self._h, _as_ptr(out["peptidoforms"]), n, C.byref(count))
            if rc:
                self._raise(rc)
            out["peptidoforms"] = out["peptidoforms"][:count.value].copy()
        if pfq is not None:
            from .rollup import empty_site_quant
            n_list, n_ch = out["peptidoforms"].size, pfq["params"]["n_channels"]
            out["peptidoform_quant_head"], out["peptidoform_quant"] = empty_site_quant(n_list, n_ch)
            rc = self._lib.pya_last_batch_peptidoform_quant(self._h, _as_ptr(out["peptidoform_quant_head"]),
                                                            _as_ptr(out["peptidoform_quant"]), n_list, n_ch)
            if rc:
                self._raise(rc)
            out["peptidoform_quant_params"] = dict(pfq["params"])
        if mzp is not None:
            out["mz_profile"] = np.zeros(mzp["n_slots"], np.dtype(_lib.MZ_PROFILE_DTYPE))
            rc = self._lib.pya_last_batch_mz_profile(self._h, _as_ptr(out["mz_profile"]), mzp["n_slots"])
            if rc:
                self._raise(rc)
            out["mz_profile_params"] = dict(mzp["params"])
        if qu is not None:
            from .rollup import empty_site_quant
            out["quant_head"], out["quant"] = empty_site_quant(roll["n_slots"], qu["params"]["n_channels"])
            rc = self._lib.pya_last_batch_site_quant(self._h, _as_ptr(out["quant_head"]), _as_ptr(out["quant"]), roll["n_slots"],
                                                     qu["params"]["n_channels"])
            if rc:
                self._raise(rc)
            out["quant_params"] = dict(qu["params"])
        if coverage:
            out["coverage"] = np.zeros(n, COVERAGE_DTYPE)
            rc = self._lib.pya_last_batch_coverage(self._h, _as_ptr(out["coverage"]), n)
            if rc:
                self._raise(rc)
        return out

    def peptidoform_reduce(self, a, b=None):
        """The peptidoform list over one or two arrays of ``PEPTIDOFORM_DTYPE`` records, reduced on the device
        (``pya_peptidoform_reduce_host``): the records may be in any order and may repeat keys, records with ``n_psm == 0``
        are skipped, ``n_isomers`` is recomputed.  Merging the lists of two files or two ranks is this call;
        ``pyascore_amd.rollup.merge_peptidoforms`` gives the same bytes on the host."""
        a = np.ascontiguousarray(a, PEPTIDOFORM_DTYPE).reshape(-1)
        b = np.zeros(0, PEPTIDOFORM_DTYPE) if b is None else np.ascontiguousarray(b, PEPTIDOFORM_DTYPE).reshape(-1)
        total = a.size + b.size
        out, count = np.zeros(total, PEPTIDOFORM_DTYPE), C.c_uint64(0)
        rc = self._lib.pya_peptidoform_reduce_host(self._h, _as_ptr(a), a.size, _as_ptr(b), b.size, _as_ptr(out), total, C.byref(count))
        if rc:
            self._raise(rc)
        return out[:count.value].copy()

    def peptidoform_quant_reduce(self, a, b):
        """The merge of two peptidoform quantification pairs on the device (``pya_peptidoform_quant_reduce_host``): ``a`` and
        ``b`` are ``(list, head, cell)`` triples -- ``PEPTIDOFORM_DTYPE`` records, ``SITE_QUANT_HEAD_DTYPE`` ``[n]`` and
        ``SITE_QUANT_DTYPE`` ``[n, n_channels]`` --, a pair whose ``head`` and ``cell`` are None counts as having an all-zero
        table.  Returns the triple of the merged pair: the keys' union in list order, rows of equal keys added field by field.
        ``pyascore_amd.rollup.merge_peptidoform_quant`` gives the same bytes on the host."""
        from .rollup import SITE_QUANT_DTYPE, SITE_QUANT_HEAD_DTYPE
        sides, n_ch = [], None
        for name, pair in (("a", a), ("b", b)):
            if pair is None:
                pair = (np.zeros(0, PEPTIDOFORM_DTYPE), None, None)
            if len(pair) != 3:
                raise ValueError("peptidoform_quant_reduce: %s is a (list, head, cell) triple" % name)
            lst = np.ascontiguousarray(pair[0], PEPTIDOFORM_DTYPE).reshape(-1)
            if (pair[1] is None) != (pair[2] is None):
                raise ValueError("peptidoform_quant_reduce: head and cell of %s are both given or both None" % name)
            head = cell = None
            if pair[1] is not None:
                head = np.ascontiguousarray(pair[1], SITE_QUANT_HEAD_DTYPE).reshape(-1)
                cell = np.ascontiguousarray(pair[2], SITE_QUANT_DTYPE)
                if head.size != lst.size or cell.ndim != 2 or cell.shape[0] != lst.size:
                    raise ValueError("peptidoform_quant_reduce: the table of %s is not row-aligned with its list" % name)
                if n_ch is not None and cell.shape[1] != n_ch:
                    raise ValueError("peptidoform_quant_reduce: the two tables have different channel counts")
                n_ch = cell.shape[1]
            sides.append((lst, head, cell))
        if n_ch is None:
            raise ValueError("peptidoform_quant_reduce: neither side has a table to take the channel count from")
        total = sides[0][0].size + sides[1][0].size
        out, count = np.zeros(total, PEPTIDOFORM_DTYPE), C.c_uint64(0)
        head, cell = np.zeros(total, SITE_QUANT_HEAD_DTYPE), np.zeros((total, n_ch), SITE_QUANT_DTYPE)
        (la, ha, ca), (lb, hb, cb) = sides
        rc = self._lib.pya_peptidoform_quant_reduce_host(self._h, _as_ptr(la), _as_ptr(ha), _as_ptr(ca), la.size, _as_ptr(lb), _as_ptr(hb),
                                                         _as_ptr(cb), lb.size, n_ch, _as_ptr(out), _as_ptr(head), _as_ptr(cell), total,
                                                         C.byref(count))
        if rc:
            self._raise(rc)
        m = count.value
        return out[:m].copy(), head[:m].copy(), cell[:m].copy()

    def site_offsets(self, batch, skip_invalid=False):
        """``site_off`` (int64 ``[n_psm + 1]``) of a batch BEFORE it is scored: where the residue records of every PSM will
        lie -- what ``rollup=`` needs one slot per entry of.  From the host pre-pass of a plan that is never run
        (``pya_plan_create``, ``pya_plan_site_offsets``): no kernel, and with ``skip_invalid`` the PSMs the library will set
        aside have no records here either."""
        n = int(batch["n_psm"])
        if n == 0:
            return np.zeros(1, np.int64)
        arrs = [np.ascontiguousarray(batch[k], t) for k, t in (("peak_off", np.int64), ("pep", np.uint8), ("pep_off", np.int64),
                                                               ("n_of_mod", np.int32), ("max_charge", np.int32), ("aux_pos", np.uint32),
                                                               ("aux_mass", np.float32), ("aux_off", np.int64))]
        b = _lib.Batch(n, *[_as_ptr(a) for a in arrs])
        flags = _lib.PYA_FLAG_ROLLUP | (_lib.PYA_FLAG_SKIP_INVALID if skip_invalid else 0)
        plan = C.c_void_p()
        if batch.get("spec_of") is not None:
            from .synth import spectrum_order, take_psms
            perm, inv = spectrum_order(batch["spec_of"])
            if perm is not None:                 # (the library wants the PSMs of a spectrum together: counted there, put back)
                counts = np.diff(self.site_offsets(take_psms(batch, perm), skip_invalid))[inv]
                return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
            spec_of = np.ascontiguousarray(batch["spec_of"], np.uint32)
            rc = self._lib.pya_plan_create_shared(self._h, C.byref(b), _as_ptr(spec_of), arrs[0].size - 1, flags, C.byref(plan))
        else:
            rc = self._lib.pya_plan_create(self._h, C.byref(b), flags, C.byref(plan))
        if rc:
            self._raise(rc)
        off = np.zeros(n + 1, np.int64)
        rc = self._lib.pya_plan_site_offsets(plan, _as_ptr(off))
        self._lib.pya_plan_destroy(plan)
        if rc:
            self._raise(rc)
        return off

    def fit_mz_calibration(self, table, params, min_ions=20):
        """The m/z calibration of a mass-error profile, fitted on the device (``pya_mz_profile_fit_host``): ``table`` is a
        ``pyascore_amd.rollup.MZ_PROFILE_DTYPE`` array as ``score_batch(mz_profile=...)`` returns it, ``params`` the
        ``mz_profile_params`` it was binned with, ``min_ions`` the signal ions a band needs to be fitted.  Returns one
        ``pyascore_amd.rollup.MZ_CALIBRATION_DTYPE`` record per slot; ``pyascore_amd.rollup.fit_mz_calibration`` gives the
        same bytes on the host."""
        from .rollup import MZ_CALIBRATION_DTYPE, MZ_PROFILE_DTYPE
        table = np.ascontiguousarray(table, MZ_PROFILE_DTYPE).reshape(-1)
        if int(min_ions) != min_ions or not 0 <= int(min_ions) <= 0xFFFFFFFF:
            raise ValueError("fit_mz_calibration: min_ions must be in 1 .. 2^32 - 1")
        c_params = _lib.MzProfileParams(params["inv_da"], params["inv_ppm"], params["inv_band"], params["max_rank"], 0)
        out = np.zeros(table.size, MZ_CALIBRATION_DTYPE)
        rc = self._lib.pya_mz_profile_fit_host(self._h, _as_ptr(table), table.size, C.byref(c_params), int(min_ions), _as_ptr(out))
        if rc:
            self._raise(rc)
        return out

    def deisotope_spectra(self, mz, intensity, peak_off, params):
        """Spectra deisotoped on the device (``pya_deisotope_spectra_host``; the rule is ``pya_deisotope_params``'s in
        include/pyascore_hip.h): ``mz`` / ``intensity`` float64 or float32 arrays as ``score_batch`` takes them (float32 m/z
        beside float64 intensities is widened), ``peak_off[n_spectra + 1]``, ``params`` of
        ``pyascore_amd.rollup.deisotope_params``.  Returns ``(mz, intensity, peak_off, over)``: new arrays with the kept peaks
        of every spectrum, bit for bit and in order, their offsets, and ``over = (count, first)`` of the spectra that were not
        ascending and came back unchanged (``first`` is None when there is none).  ``pyascore_amd.rollup.deisotope`` gives the
        same bytes on the host."""
        from .rollup import deisotope_c_params
        c_params = deisotope_c_params(params)
        c = _transform_call("deisotope_spectra", mz, intensity, peak_off)
        if c.n_peaks:                                        # (no peak anywhere: nothing to filter)
            rc = self._lib.pya_deisotope_spectra_host(self._h, C.byref(c.t_in), _as_ptr(c.peak_off), c.n_spec, C.byref(c_params),
                                                      C.byref(c.t_out), _as_ptr(c.new_off), _as_ptr(c.over))
            if rc:
                self._raise(rc)
        spectra, over = _transform_result(c)
        return spectra + (over,)

    def decharge_spectra(self, mz, intensity, peak_off, params):
        """Spectra charge-deconvolved on the device (``pya_decharge_spectra_host``; the rule is ``pya_decharge_params``'s in
        include/pyascore_hip.h): arguments as ``deisotope_spectra`` takes them, ``params`` of
        ``pyascore_amd.rollup.decharge_params``.  Returns ``(mz, intensity, peak_off, charge, over)``: new arrays with the
        peaks of every spectrum -- those deisotoping keeps, the multiply charged ones moved to 1+, ascending --, their offsets,
        one ``uint8`` per output peak with its charge (1: not moved), and ``over = (count, first)`` of the spectra that were not
        ascending and came back unchanged.  ``pyascore_amd.rollup.decharge`` gives the same bytes on the host."""
        from .rollup import decharge_c_params
        c_params = decharge_c_params(params)
        c = _transform_call("decharge_spectra", mz, intensity, peak_off)
        charge = np.zeros(c.n_peaks, np.uint8)
        if c.n_peaks:                                        # (no peak anywhere: nothing to do)
            rc = self._lib.pya_decharge_spectra_host(self._h, C.byref(c.t_in), _as_ptr(c.peak_off), c.n_spec, C.byref(c_params),
                                                     C.byref(c.t_out), _as_ptr(c.new_off), _as_ptr(charge), _as_ptr(c.over))
            if rc:
                self._raise(rc)
        spectra, over = _transform_result(c)
        return spectra + (charge[:spectra[0].size], over)

    def strip_spectra(self, mz, intensity, peak_off, precursor_mz, precursor_charge, params):
        """Spectra without their precursor-derived peaks, stripped on the device (``pya_strip_spectra_host``; the rule is
        ``pya_strip_params``'s in include/pyascore_hip.h): ``mz`` / ``intensity`` and ``peak_off`` as ``deisotope_spectra`` takes
        them, ``precursor_mz`` (float64) / ``precursor_charge`` (int32) one entry per spectrum, ``params`` of
        ``pyascore_amd.rollup.strip_params``.  Returns ``(mz, intensity, peak_off, report, over)``: new arrays with the kept
        peaks of every spectrum, bit for bit and in order, their offsets, one ``pyascore_amd.rollup.STRIP_REPORT_DTYPE`` record
        per spectrum (which windows held a peak, the peaks removed, the active windows) and ``over = (count, first)``, which is
        ``(0, None)`` here: the host form sizes its own workspace.  ``pyascore_amd.rollup.strip`` gives the same bytes on the
        host."""
        from .rollup import STRIP_REPORT_DTYPE, strip_c_params
        c_params = strip_c_params(params)
        c = _transform_call("strip_spectra", mz, intensity, peak_off)
        charge = np.asarray(precursor_charge)
        if charge.dtype.kind not in "iu":
            raise ValueError("strip_spectra: precursor_charge is one integer per spectrum")
        prec_mz = np.ascontiguousarray(precursor_mz, np.float64)
        prec_z = np.ascontiguousarray(np.clip(charge, -1, 0x7FFFFFFF), np.int32)
        if prec_mz.shape != (c.n_spec,) or prec_z.shape != (c.n_spec,):
            raise ValueError("strip_spectra: precursor_mz and precursor_charge have one entry per spectrum")
        report = np.zeros(c.n_spec, STRIP_REPORT_DTYPE)
        if c.n_spec:                                         # (spectra without a peak are still a call: the report counts the windows)
            rc = self._lib.pya_strip_spectra_host(self._h, C.byref(c.t_in), _as_ptr(c.peak_off), c.n_spec, _as_ptr(prec_mz), _as_ptr(prec_z),
                                                  C.byref(c_params), C.byref(c.t_out), _as_ptr(c.new_off), _as_ptr(report), _as_ptr(c.over))
            if rc:
                self._raise(rc)
        spectra, over = _transform_result(c)
        return spectra + (report, over)

    def correct_channels(self, values, matrix=None, normalize=False, select=None, scale_log2=10):
        """A channel matrix corrected on the device (``pya_channel_correct_host``; the rule is the channel correction's in
        include/pyascore_hip.h): ``values`` float64 ``[n_rows, n_channels]`` (reporter intensities, NaN where there is none),
        ``matrix`` ``[n_channels, n_channels]`` the inverse of the lot's spill matrix (``pyascore_amd.rollup.channel_matrix``) or
        None, ``normalize`` whether the column totals are then made equal, over the rows ``select`` names (one boolean per row;
        None: all), ``scale_log2`` the quantum of the sums as ``quant=`` has it.  Returns ``(values, cell, factors)``: the
        corrected matrix (new), ``pyascore_amd.rollup.SITE_QUANT_DTYPE[n_channels]`` the column sums after the matrix and before
        the factors, and the factors float64 ``[n_channels]`` (None without ``normalize``).  One upload, one download.
        ``pyascore_amd.rollup.correct_channels`` / ``channel_sums`` / ``channel_factors`` give the same bytes on the host."""
        from .rollup import QUANT_MAX_CHANNELS, SITE_QUANT_DTYPE, check_channel_matrix, check_site_quant_params
        v = np.ascontiguousarray(values, np.float64)
        if v.ndim != 2 or not 1 <= v.shape[1] <= QUANT_MAX_CHANNELS or v.shape[0] > 0xFFFFFFFE:
            raise ValueError("correct_channels: values is a float64 matrix, one row per spectrum and 1 .. %d channels" % QUANT_MAX_CHANNELS)
        n_rows, n_ch = v.shape
        if not isinstance(normalize, (bool, np.bool_)):
            raise ValueError("correct_channels: normalize = %r is not a boolean" % (normalize,))
        if matrix is None and not normalize:
            raise ValueError("correct_channels: neither a matrix nor normalize=True")
        m = None if matrix is None else check_channel_matrix(matrix, n_ch)
        scale_log2 = check_site_quant_params(dict(threshold=0.0, scale_log2=scale_log2, n_channels=n_ch, complete_only=False))["scale_log2"]
        sel = None
        if select is not None:
            sel = np.asarray(select)
            if sel.shape != (n_rows,) or (sel.size and sel.dtype.kind not in "biu"):
                raise ValueError("correct_channels: select is one boolean per row")
            sel = np.ascontiguousarray(sel != 0, np.uint8)
        out = np.empty_like(v)
        cell = np.zeros(n_ch, SITE_QUANT_DTYPE)
        factors = np.ones(n_ch, np.float64) if normalize else None
        rc = self._lib.pya_channel_correct_host(self._h, _as_ptr(v) if n_rows else None, n_rows, n_ch, None if m is None else _as_ptr(m),
                                                None if sel is None or not n_rows else _as_ptr(sel), scale_log2,
                                                _lib.PYA_CHANNEL_NORMALIZE if normalize else 0, _as_ptr(out) if n_rows else None,
                                                _as_ptr(cell), None if factors is None else _as_ptr(factors))
        if rc:
            self._raise(rc)
        return out, cell, factors

    def marker_spectra(self, mz, intensity, peak_off, params, precursor_mz=None, precursor_charge=None):
        """The marker ions of spectra, looked up on the device (``pya_marker_spectra_host``; the rule is ``pya_marker_params``'s
        in include/pyascore_hip.h): ``mz`` / ``intensity`` and ``peak_off`` as ``deisotope_spectra`` takes them, ``params`` of
        ``pyascore_amd.rollup.marker_params``, ``precursor_mz`` (float64) / ``precursor_charge`` (int32) one entry per spectrum,
        needed iff ``params`` has loss targets.  Returns ``(markers, spectra, over)``: ``pyascore_amd.rollup.MARKER_DTYPE``
        records of shape ``[n_spectra, n_targets]`` (the peak every target picked), ``MARKER_SPECTRUM_DTYPE`` records of shape
        ``[n_spectra]`` (ion current, base peak, the ``hit`` word) and ``over = (count, first)``, which is ``(0, None)`` here: the
        host form knows the length of its arrays.  The spectra are uploaded once and only the records come back.
        ``pyascore_amd.rollup.markers`` gives the same bytes on the host."""
        from .rollup import MARKER_DTYPE, MARKER_SPECTRUM_DTYPE, marker_c_params
        c_params = marker_c_params(params)
        c = _transform_call("marker_spectra", mz, intensity, peak_off)
        prec_mz = prec_z = None
        if precursor_mz is not None or precursor_charge is not None:
            charge = np.asarray(precursor_charge)
            if precursor_mz is None or precursor_charge is None or charge.dtype.kind not in "iu":
                raise ValueError("marker_spectra: precursor_mz and precursor_charge come together, the charge one integer per spectrum")
            prec_mz = np.ascontiguousarray(precursor_mz, np.float64)
            prec_z = np.ascontiguousarray(np.clip(charge, -1, 0x7FFFFFFF), np.int32)
            if prec_mz.shape != (c.n_spec,) or prec_z.shape != (c.n_spec,):
                raise ValueError("marker_spectra: precursor_mz and precursor_charge have one entry per spectrum")
        elif c_params.loss_mask:
            raise ValueError("marker_spectra: loss targets need precursor_mz and precursor_charge, one entry per spectrum")
        records = np.zeros((c.n_spec, int(c_params.n_targets)), MARKER_DTYPE)
        spectra = np.zeros(c.n_spec, MARKER_SPECTRUM_DTYPE)
        if c.n_spec:                                         # (spectra without a peak are still a call: fixed targets are active)
            rc = self._lib.pya_marker_spectra_host(self._h, C.byref(c.t_in), _as_ptr(c.peak_off), c.n_spec,
                                                   None if prec_mz is None else _as_ptr(prec_mz), None if prec_z is None else _as_ptr(prec_z),
                                                   C.byref(c_params), _as_ptr(records), _as_ptr(spectra), _as_ptr(c.over))
            if rc:
                self._raise(rc)
        return records, spectra, (int(c.over[0]), None if not c.over[0] else 0xFFFFFFFF - int(c.over[1]))

    def precursor_purity(self, ms1_mz, ms1_intensity, ms1_peak_off, survey, precursor_mz, precursor_charge, window_lo, window_hi, params):
        """The precursor purity of isolation windows, read off survey spectra on the device (``pya_purity_spectra_host``; the rule
        is ``pya_purity_params``'s in include/pyascore_hip.h): ``ms1_mz`` / ``ms1_intensity`` / ``ms1_peak_off`` the survey (MS1)
        spectra as ``deisotope_spectra`` takes spectra; per query (one per MS2 spectrum) ``survey`` the index of its survey
        spectrum (negative: none), ``precursor_mz`` / ``precursor_charge`` and ``window_lo`` / ``window_hi``, the absolute m/z
        bounds of the isolation window; ``params`` of ``pyascore_amd.rollup.purity_params``.  Returns ``(records, over)``:
        ``pyascore_amd.rollup.PURITY_DTYPE[n_query]`` and ``over = (count, first)`` for the queries whose ``survey`` lies beyond
        the survey spectra (zero records), ``(0, None)`` when there is none.  The survey spectra and the queries are uploaded
        once and only the records come back.  ``pyascore_amd.rollup.purity`` gives the same bytes on the host."""
        from .rollup import PURITY_DTYPE, purity_c_params, purity_queries
        c_params = purity_c_params(params)
        c = _transform_call("precursor_purity", ms1_mz, ms1_intensity, ms1_peak_off)
        sv, pm, pz, wl, wh = purity_queries(survey, precursor_mz, precursor_charge, window_lo, window_hi, "precursor_purity")
        if sv.size > 0xFFFFFFFE:
            raise ValueError("precursor_purity: more than 2^32 - 2 queries")
        records = np.zeros(sv.size, PURITY_DTYPE)
        if sv.size:
            rc = self._lib.pya_purity_spectra_host(self._h, C.byref(c.t_in), _as_ptr(c.peak_off), c.n_spec, _as_ptr(sv), _as_ptr(pm), _as_ptr(pz),
                                                   _as_ptr(wl), _as_ptr(wh), sv.size, C.byref(c_params), _as_ptr(records), _as_ptr(c.over))
            if rc:
                self._raise(rc)
        return records, (int(c.over[0]), None if not c.over[0] else 0xFFFFFFFF - int(c.over[1]))

    def precursor_xic(self, ms1_mz, ms1_intensity, ms1_peak_off, rt, seed, scan_lo, scan_hi, precursor_mz, precursor_charge, params,
                      scan_ok=None):
        """The precursor XIC -- the label-free MS1 intensity of identified precursors --, read off survey spectra on the device
        (``pya_xic_spectra_host``; the rule is ``pya_xic_params``'s in include/pyascore_hip.h): ``ms1_mz`` / ``ms1_intensity`` /
        ``ms1_peak_off`` the survey (MS1) spectra as ``precursor_purity`` takes them, ``rt`` their retention times in seconds;
        per query (one per MS2 spectrum) ``seed`` the survey scan of the identification (negative: none), ``scan_lo`` /
        ``scan_hi`` the window of at most 64 survey scans around it (``pyascore_amd.rollup.xic_windows``), ``precursor_mz`` /
        ``precursor_charge``; ``params`` of ``pyascore_amd.rollup.xic_params``; ``scan_ok``: the bytes of
        ``pyascore_amd.rollup.survey_ascending`` when they are at hand, None to have the device check the scans.  Returns
        ``(records, over)``: ``pyascore_amd.rollup.XIC_DTYPE[n_query]`` and ``over = (count, first)`` for the queries whose
        window is out of range (zero records), ``(0, None)`` when there is none.  The survey spectra and the queries are
        uploaded once and only the records come back.  ``pyascore_amd.rollup.xic`` gives the same bytes on the host."""
        from .rollup import XIC_DTYPE, xic_c_params, xic_queries
        c_params = xic_c_params(params)
        c = _transform_call("precursor_xic", ms1_mz, ms1_intensity, ms1_peak_off)
        sd, lo, hi, pm, pz = xic_queries(seed, scan_lo, scan_hi, precursor_mz, precursor_charge, "precursor_xic")
        try:
            rt = np.ascontiguousarray(rt, np.float64)
        except (TypeError, ValueError):
            raise ValueError("precursor_xic: rt is a number per survey spectrum") from None
        if rt.shape != (c.n_spec,):
            raise ValueError("precursor_xic: rt has one entry per survey spectrum")
        if scan_ok is not None:
            scan_ok = np.ascontiguousarray(scan_ok, np.uint8)
            if scan_ok.shape != (c.n_spec,):
                raise ValueError("precursor_xic: scan_ok has one byte per survey spectrum")
        if sd.size > 0xFFFFFFFE:
            raise ValueError("precursor_xic: more than 2^32 - 2 queries")
        records = np.zeros(sd.size, XIC_DTYPE)
        if sd.size:
            rc = self._lib.pya_xic_spectra_host(self._h, C.byref(c.t_in), _as_ptr(c.peak_off), c.n_spec, _as_ptr(rt) if c.n_spec else None,
                                                _as_ptr(scan_ok) if c.n_spec else None, _as_ptr(sd), _as_ptr(lo), _as_ptr(hi), _as_ptr(pm),
                                                _as_ptr(pz), sd.size, C.byref(c_params), _as_ptr(records), _as_ptr(c.over))
            if rc:
                self._raise(rc)
        return records, (int(c.over[0]), None if not c.over[0] else 0xFFFFFFFF - int(c.over[1]))

    def purity_gate(self, records, threshold, keep_unknown=True, values=None):
        """THE GATE of the precursor purity on the device (``pya_purity_gate``): ``records`` ``PURITY_DTYPE[n_rows]``,
        ``threshold`` in 0 .. 1, ``values`` float64 ``[n_rows, n_channels]`` or None.  Returns ``(select, values)`` as
        ``pyascore_amd.rollup.purity_gate`` does, with the same bytes: one upload, one launch, one download -- the host
        function is the cheaper one for host arrays; this form is there for parity with the resident chain
        (``pyascore_amd.device.purity_gate``)."""
        import torch
        from . import device as dev
        from .rollup import PURITY_DTYPE, check_purity_gate
        t, keep = check_purity_gate(threshold, keep_unknown)
        rec = np.ascontiguousarray(records, PURITY_DTYPE)
        if rec.ndim != 1:
            raise ValueError("purity_gate: records is one PURITY_DTYPE record per row")
        device = torch.device("cuda", self.device)
        d_rec = torch.from_numpy(rec.view(np.uint8).reshape(rec.size, PURITY_DTYPE.itemsize)).to(device)
        d_values = None
        if values is not None:
            v = np.ascontiguousarray(values, np.float64)
            if v.ndim != 2 or v.shape[0] != rec.size:
                raise ValueError("purity_gate: values is a float64 matrix with one row per record")
            d_values = torch.from_numpy(v).to(device)
        out, select = dev.purity_gate(self, d_rec, t, keep, d_values, select=True)
        torch.cuda.synchronize(device)
        return select.cpu().numpy(), None if out is None else out.cpu().numpy()

    def centroid_spectra(self, mz, intensity, peak_off, params, select=None):
        """Centroided spectra, picked on the device (``pya_centroid_spectra_host``; the rule is ``pya_centroid_params``'s in
        include/pyascore_hip.h): ``mz`` / ``intensity`` and ``peak_off`` as ``deisotope_spectra`` takes them, ``params`` of
        ``pyascore_amd.rollup.centroid_params``, ``select`` one boolean per spectrum (False: copied unchanged) or None for
        all.  Returns ``(mz, intensity, peak_off, over)``: new arrays with one peak per apex of every spectrum, in order, their
        offsets and ``over = (count, first)``, the number of selected spectra that were not ascending (copied unchanged) and
        the first of them, ``(0, None)`` when there is none.  ``pyascore_amd.rollup.centroid`` gives the same bytes on the
        host."""
        from .rollup import centroid_c_params, centroid_select
        c_params = centroid_c_params(params)
        c = _transform_call("centroid_spectra", mz, intensity, peak_off)
        sel = centroid_select(select, c.n_spec, "centroid_spectra")
        if c.n_spec:                                         # (spectra without a point are still a call, as for strip_spectra)
            rc = self._lib.pya_centroid_spectra_host(self._h, C.byref(c.t_in), _as_ptr(c.peak_off), c.n_spec, _as_ptr(sel), C.byref(c_params),
                                                     C.byref(c.t_out), _as_ptr(c.new_off), _as_ptr(c.over))
            if rc:
                self._raise(rc)
        spectra, over = _transform_result(c)
        return spectra + (over,)

    def rollup_flr(self, table, cls=None, reported_only=False):
        """Site FLR of a roll-up table on the device (``pya_rollup_flr_host``): ``table`` is a ``ROLLUP_DTYPE`` array as
        ``score_batch(rollup=...)`` returns it or ``pyascore_amd.rollup.merge`` makes it of several, ``cls`` one byte per slot
        (0 target, 1 decoy, 2 left out; ``pyascore_amd.rollup.decoy_classes``) or None: every slot is a target;
        ``reported_only``: slots no PSM reports (``n_in_best == 0``) are not ranked.  Returns ``(records, order, n_ranked)``:
        ``FLR_DTYPE`` (the 32-byte ``pya_site_flr``) per slot, the ranked slots best first then the others by index
        (uint32), and the number of ranked slots.  ``pyascore_amd.rollup.flr`` gives the same bytes on the host."""
        table = np.ascontiguousarray(table, ROLLUP_DTYPE)
        if table.ndim != 1:
            raise ValueError("rollup_flr: the table is one record per slot")
        n = table.size
        if cls is not None:
            cls = np.ascontiguousarray(cls, np.uint8)
            if cls.shape != (n,):
                raise ValueError("rollup_flr: cls has one byte per slot")
        records, order, n_ranked = np.zeros(n, FLR_DTYPE), np.zeros(n, np.uint32), np.zeros(1, np.uint32)
        rc = self._lib.pya_rollup_flr_host(self._h, _as_ptr(table), n, _as_ptr(cls), _lib.PYA_FLR_REPORTED_ONLY if reported_only else 0,
                                           _as_ptr(records), _as_ptr(order), _as_ptr(n_ranked))
        if rc:
            self._raise(rc)
        return records, order, int(n_ranked[0])

    def _last_batch_probs(self, n):
        """pya_last_batch_probs: the size query, then the records"""
        off = np.zeros(n + 1, np.int64)
        rc = self._lib.pya_last_batch_probs(self._h, _as_ptr(off), None, None, 0)
        if rc:
            self._raise(rc)
        rec, psms = np.zeros(int(off[-1]), SITE_PROB_DTYPE), np.zeros(n, PSM_PROB_DTYPE)
        rc = self._lib.pya_last_batch_probs(self._h, _as_ptr(off), _as_ptr(rec), _as_ptr(psms), max(rec.size, 1))
        if rc:
            self._raise(rc)
        return off, rec, psms

    def _last_batch_sites(self, n):
        """pya_last_batch_sites: the size query, then the records"""
        off = np.zeros(n + 1, np.int64)
        rc = self._lib.pya_last_batch_sites(self._h, _as_ptr(off), None, 0)
        if rc:
            self._raise(rc)
        rec = np.zeros(int(off[-1]), SITE_DTYPE)
        if rec.size:
            rc = self._lib.pya_last_batch_sites(self._h, _as_ptr(off), _as_ptr(rec), rec.size)
            if rc:
                self._raise(rc)
        return off, rec

    def _last_batch_ions(self, n):
        """pya_last_batch_ions: the size query, then the records"""
        off = np.zeros(n + 1, np.int64)
        rc = self._lib.pya_last_batch_ions(self._h, _as_ptr(off), None, 0)
        if rc:
            self._raise(rc)
        rec = np.zeros(int(off[-1]), ION_DTYPE)
        if rec.size:
            rc = self._lib.pya_last_batch_ions(self._h, _as_ptr(off), _as_ptr(rec), rec.size)
            if rc:
                self._raise(rc)
        return off, rec

    def _score_batch_call(self, b, spec_of, n_spec, mz, it, flags, r, nq=None):
        """float64 arrays through the entry points the reference's interface stands beside, float32 ones through the typed;
        with queries (``nq``: offsets, signatures, the three output arrays) through the named entry point, which takes both."""
        if nq is not None:
            sp = _lib.TypedSpectra(_as_ptr(mz), _as_ptr(it), _lib.spectrum_type(mz.dtype), _lib.spectrum_type(it.dtype))
            return self._lib.pya_score_batch_named(self._h, C.byref(b), _as_ptr(spec_of), n_spec, C.byref(sp), flags, C.byref(r),
                                                   *[_as_ptr(a) for a in nq])
        if mz.dtype == np.float32 or it.dtype == np.float32:
            sp = _lib.TypedSpectra(_as_ptr(mz), _as_ptr(it), _lib.spectrum_type(mz.dtype), _lib.spectrum_type(it.dtype))
            return self._lib.pya_score_batch_typed(self._h, C.byref(b), _as_ptr(spec_of), n_spec, C.byref(sp), flags, C.byref(r))
        if spec_of is None:
            return self._lib.pya_score_batch(self._h, C.byref(b), _as_ptr(mz), _as_ptr(it), flags, C.byref(r))
        return self._lib.pya_score_batch_shared(self._h, C.byref(b), _as_ptr(spec_of), n_spec, _as_ptr(mz), _as_ptr(it), flags,
                                                C.byref(r))

    def format_batch(self, batch, sig_bits, valid=None, rec_psm=None):
        """Modified-sequence strings (``best_sequence`` / the ``sequence`` of ``pep_scores`` records) for
        many localisations in ONE library call: record r is the localisation ``sig_bits[r]`` of PSM
        ``rec_psm[r]`` of ``batch`` (default: record r belongs to PSM r).  Records with ``valid[r] <= 0``
        (pass ``n_sig``) come back as ''.  Returns a list of str."""
        sig_bits = np.ascontiguousarray(sig_bits, np.uint64)
        n_rec = sig_bits.size
        rp = None if rec_psm is None else np.ascontiguousarray(rec_psm, np.int64)
        va = None if valid is None else np.ascontiguousarray(valid, np.int32)
        if (rp is not None and rp.size != n_rec) or (va is not None and va.size != n_rec):
            raise ValueError("rec_psm / valid must have one entry per record")
        arrs = [np.ascontiguousarray(batch["peak_off"], np.int64), np.ascontiguousarray(batch["pep"], np.uint8),
                np.ascontiguousarray(batch["pep_off"], np.int64), np.ascontiguousarray(batch["n_of_mod"], np.int32),
                np.ascontiguousarray(batch["max_charge"], np.int32), np.ascontiguousarray(batch["aux_pos"], np.uint32),
                np.ascontiguousarray(batch["aux_mass"], np.float32), np.ascontiguousarray(batch["aux_off"], np.int64)]
        if rp is None and n_rec != int(batch["n_psm"]):
            raise ValueError("one localisation per PSM expected")
        b = _lib.Batch(int(batch["n_psm"]), *[_as_ptr(a) for a in arrs])
        off = np.zeros(n_rec + 1, np.int64)
        rc = self._lib.pya_format_peptides(self._h, C.byref(b), n_rec, _as_ptr(rp), _as_ptr(sig_bits), _as_ptr(va),
                                           _as_ptr(off), None, 0)
        if rc:
            raise ValueError("record refers to a PSM outside the batch")
        buf = np.zeros(max(int(off[-1]), 1), np.uint8)
        rc = self._lib.pya_format_peptides(self._h, C.byref(b), n_rec, _as_ptr(rp), _as_ptr(sig_bits), _as_ptr(va),
                                           _as_ptr(off), _as_ptr(buf), buf.size)
        if rc:
            self._raise(rc)
        text = buf.tobytes().decode("utf8")
        return [text[off[r]:off[r + 1]] for r in range(n_rec)]

    # ------------------------------------------------------------------------------------------
    def _format(self, last, bits, sig_len):
        buf = C.create_string_buffer(1024)
        n = self._lib.pya_format_peptide(self._h, _as_ptr(last["pep"]), last["pep"].size, last["k"],
                                         _as_ptr(last["aux_pos"]), _as_ptr(last["aux_mass"]),
                                         last["aux_pos"].size, int(bits), int(sig_len), buf, 1024)
        if n < 0:
            self._raise(n)
        return buf.value.decode("utf8")

    def _n_sites(self, last):
        ns = C.c_int32()
        self._lib.pya_count_sites(self._h, _as_ptr(last["pep"]), last["pep"].size, C.byref(ns), None)
        return ns.value

    @property
    def best_sequence(self):
        last = self._last
        if last is None or last["n_sig"] <= 0:
            return ""
        return self._format(last, last["best_sig"], self._n_sites(last))

    @property
    def best_score(self):
        return -1.0 if self._last is None else self._last["best_score"]

    @property
    def pep_scores(self):
        last = self._last
        if last is None or last["n_sig"] <= 0:
            return []
        self._ensure_kept()
        n = last["n_sig"]
        ns = self._n_sites(last)
        bits = np.zeros(n, np.uint64)
        counts = np.zeros((n, self._n_top), np.int32)
        scores = np.zeros((n, self._n_top), np.float32)
        ws = np.zeros(n, np.float32)
        nfrag = np.zeros(n, np.int32)
        got = C.c_uint64()
        rc = self._lib.pya_get_pep_scores(self._h, 0, n, C.byref(got), _as_ptr(bits), _as_ptr(counts),
                                          _as_ptr(scores), _as_ptr(ws), _as_ptr(nfrag))
        if rc:
            self._raise(rc)
        out = []
        for i in range(int(got.value)):
            b = int(bits[i])
            out.append(dict(signature=np.array([(b >> j) & 1 for j in range(ns)], dtype=np.int32),
                            counts=counts[i].copy(), scores=scores[i].copy(),
                            weighted_score=float(ws[i]), total_fragments=int(nfrag[i]),
                            sequence=self._format(last, b, ns)))
        return out

    def batch_pep_scores(self, begin=0, end=None, batch=None):
        """All localisations of PSMs [begin, end) of the last ``score_batch(..., keep=True)``, in the
        reference's sorted order, as CSR arrays (bulk form of ``pep_scores``, Ascore.pyx:241-252):
        dict(rec_off i64[n+1], sig_bits u64[R] (bit j = j-th modifiable residue), counts i32[R, n_top],
        scores f32[R, n_top], weighted_score f32[R], total_fragments i32[R]); records of PSM i are
        rows rec_off[i - begin] : rec_off[i - begin + 1].  With ``batch`` (the scored batch) the
        records' ``sequence`` strings are added, all formatted in one library call."""
        if self._batch_n is None:
            raise RuntimeError("no batch retained: call score_batch(batch, keep=True) first")
        end = self._batch_n if end is None else int(end)
        begin = int(begin)
        if not 0 <= begin <= end <= self._batch_n:
            raise ValueError("PSM range outside the retained batch")
        if self._lazy_batch is not None:
            out = self._lazy_pep_scores(begin, end)
        else:
            out = self._range_pep_scores(begin, end)
        if batch is not None:
            rec_psm = np.repeat(np.arange(begin, end, dtype=np.int64), np.diff(out["rec_off"]))
            out["sequence"] = self.format_batch(batch, out["sig_bits"], rec_psm=rec_psm)
        return out

    def _range_pep_scores(self, begin, end):
        off = np.zeros(end - begin + 1, np.int64)
        rc = self._lib.pya_get_pep_scores_range(self._h, begin, end, 0, _as_ptr(off), None, None, None, None, None)
        if rc:
            self._raise(rc)
        total = int(off[-1])
        out = dict(rec_off=off, sig_bits=np.zeros(total, np.uint64), counts=np.zeros((total, self._n_top), np.int32),
                   scores=np.zeros((total, self._n_top), np.float32), weighted_score=np.zeros(total, np.float32),
                   total_fragments=np.zeros(total, np.int32))
        if total:
            rc = self._lib.pya_get_pep_scores_range(self._h, begin, end, total, _as_ptr(off),
                                                    _as_ptr(out["sig_bits"]), _as_ptr(out["counts"]),
                                                    _as_ptr(out["scores"]), _as_ptr(out["weighted_score"]),
                                                    _as_ptr(out["total_fragments"]))
            if rc:
                self._raise(rc)
        return out

    def _lazy_pep_scores(self, begin, end):
        """Records of PSMs [begin, end) of a retained batch that was too big to keep on the device: the range is
        re-scored in pieces that fit the budget, each retained, exported and dropped."""
        from .synth import slice_batch
        lb = self._lazy_batch
        cost = np.concatenate([[0.0], np.cumsum(lb["per_psm"])])
        parts, lo = [], begin
        while lo < end:
            hi = int(np.searchsorted(cost, cost[lo] + 0.5 * lb["budget"], side="right")) - 1
            hi = min(max(hi, lo + 1), end)
            sub = slice_batch(lb, lo, hi)
            arrs = {k: np.ascontiguousarray(sub[k]) for k in ("peak_off", "pep", "pep_off", "n_of_mod", "max_charge",
                                                              "aux_pos", "aux_mass", "aux_off")}
            m = hi - lo
            mk = max(1, int(arrs["n_of_mod"].max()))
            tmp = dict(best_score=np.zeros(m, np.float32), best_sig=np.zeros(m, np.uint64), n_sig=np.zeros(m, np.int32),
                       ascores=np.zeros((m, mk), np.float32), alt_mask=np.zeros((m, mk), np.uint64))
            b = _lib.Batch(m, _as_ptr(arrs["peak_off"]), _as_ptr(arrs["pep"]), _as_ptr(arrs["pep_off"]),
                           _as_ptr(arrs["n_of_mod"]), _as_ptr(arrs["max_charge"]), _as_ptr(arrs["aux_pos"]),
                           _as_ptr(arrs["aux_mass"]), _as_ptr(arrs["aux_off"]))
            r = _lib.Results(mk, _as_ptr(tmp["best_score"]), _as_ptr(tmp["best_sig"]), _as_ptr(tmp["n_sig"]),
                             _as_ptr(tmp["ascores"]), _as_ptr(tmp["alt_mask"]))
            mz = np.ascontiguousarray(sub["mz"])              # (as the batch was scored: float64 or typed)
            it = np.ascontiguousarray(sub["intensity"])
            rc = self._score_batch_call(b, None, m, mz, it, _lib.PYA_FLAG_KEEP | _lib.PYA_FLAG_SKIP_INVALID, r)
            if rc:
                self._raise(rc)
            parts.append(self._range_pep_scores(0, m))
            lo = hi
        off = np.concatenate([[0]] + [p["rec_off"][1:] + sum(int(q["rec_off"][-1]) for q in parts[:i])
                                      for i, p in enumerate(parts)]).astype(np.int64)
        out = {k: np.concatenate([p[k] for p in parts]) for k in ("sig_bits", "counts", "scores", "weighted_score",
                                                                 "total_fragments")}
        out["rec_off"] = off
        return out

    @property
    def ascores(self):
        if self._last is None:
            return np.zeros(0, np.float32)
        return self._last["ascores"][: self._last["k"]].astype(np.float32)

    @property
    def evidence(self):
        """What stands behind the Ascores of the last ``score()`` PSM: one ``EVIDENCE_DTYPE`` record per modified site
        (see ``score_batch(evidence=True)``).  Produced the first time it is read, by sending that PSM -- the arrays
        ``score()`` was given -- through the batch path as a batch of one; ``score()`` itself does nothing for it."""
        last = self._last
        if last is None:
            return np.zeros(0, EVIDENCE_DTYPE)
        self._batch_of_one_records()
        return last["evidence"][: last["k"]].copy()

    @property
    def ions(self):
        """Which ions stand behind the last ``score()`` PSM: its ``ION_DTYPE`` records (see ``score_batch(ions=True)``),
        the winner's matched fragments first, then the site-determining ions of every counted site.  Produced when read,
        like ``evidence``."""
        last = self._last
        if last is None:
            return np.zeros(0, ION_DTYPE)
        self._batch_of_one_records()
        return last["ions"].copy()

    @property
    def coverage(self):
        """How much of its spectrum the last ``score()`` PSM explains: its ``COVERAGE_DTYPE`` record (see
        ``score_batch(coverage=True)``).  Produced when read, like ``evidence``."""
        last = self._last
        if last is None:
            return np.zeros(1, COVERAGE_DTYPE)[0]
        self._batch_of_one_records()
        return last["coverage"].copy()

    @property
    def sites(self):
        """The site table of the last ``score()`` PSM: one ``SITE_DTYPE`` record per modifiable residue (see
        ``score_batch(sites=True)``; no cap on the site assignments).  Produced the first time it is read, by sending that
        PSM through the batch path as a batch of one, like ``evidence``."""
        last = self._last
        if last is None:
            return np.zeros(0, SITE_DTYPE)
        if "sites" not in last:
            mz, it = _check_f64("mz_arr", last["mz"]), _check_f64("int_arr", last["it"])
            psm = dict(n_psm=1, mz=mz, intensity=it, peak_off=np.array([0, mz.size], np.int64), pep=last["pep"],
                       pep_off=np.array([0, last["pep"].size], np.int64), n_of_mod=np.array([int(last["k"])], np.int32),
                       max_charge=np.array([int(last["z"])], np.int32), aux_pos=last["aux_pos"], aux_mass=last["aux_mass"],
                       aux_off=np.array([0, np.size(last["aux_pos"])], np.int64))
            self._ensure_kept()          # (score_batch does: before the state it leaves is put back)
            state = (self._last, self._batch_n, self._lazy_batch)
            res = self.score_batch(psm, sites=True, site_sig_cap=0)
            self._last, self._batch_n, self._lazy_batch = state
            if int(res["best_sig"][0]) != int(last["best_sig"]):
                raise RuntimeError("the arrays passed to score() changed before sites was read")
            last["sites"] = res["sites"]
        return last["sites"].copy()

    @property
    def probs(self):
        """The site probabilities of the last ``score()`` PSM: dict(site_probs, psm_prob) -- one ``SITE_PROB_DTYPE`` record
        per modifiable residue and the PSM's ``PSM_PROB_DTYPE`` record (see ``score_batch(probs=True)``; no cap on the site
        assignments).  Produced the first time it is read, by sending that PSM through the batch path as a batch of one."""
        last = self._last
        if last is None:
            return dict(site_probs=np.zeros(0, SITE_PROB_DTYPE), psm_prob=np.zeros(1, PSM_PROB_DTYPE)[0])
        if "probs" not in last:
            mz, it = _check_f64("mz_arr", last["mz"]), _check_f64("int_arr", last["it"])
            psm = dict(n_psm=1, mz=mz, intensity=it, peak_off=np.array([0, mz.size], np.int64), pep=last["pep"],
                       pep_off=np.array([0, last["pep"].size], np.int64), n_of_mod=np.array([int(last["k"])], np.int32),
                       max_charge=np.array([int(last["z"])], np.int32), aux_pos=last["aux_pos"], aux_mass=last["aux_mass"],
                       aux_off=np.array([0, np.size(last["aux_pos"])], np.int64))
            self._ensure_kept()          # (score_batch does: before the state it leaves is put back)
            state = (self._last, self._batch_n, self._lazy_batch)
            res = self.score_batch(psm, probs=True, site_sig_cap=0)
            self._last, self._batch_n, self._lazy_batch = state
            if int(res["best_sig"][0]) != int(last["best_sig"]):
                raise RuntimeError("the arrays passed to score() changed before probs was read")
            last["probs"] = (res["site_probs"], res["psm_probs"][0])
        return dict(site_probs=last["probs"][0].copy(), psm_prob=last["probs"][1].copy())

    def ranked(self, top_k=5):
        """The ranked localisations of the last ``score()`` PSM: ``RANKED_DTYPE`` ``[top_k]`` -- row 0 the reported
        localisation, then the other site assignments by PepScore (see ``score_batch(ranked=K)``; no cap on the site
        assignments).  Produced by sending that PSM through the batch path as a batch of one, once per ``top_k``."""
        top_k = check_ranked_k(top_k)
        last = self._last
        if last is None:
            return np.zeros(top_k, RANKED_DTYPE)
        got = last.setdefault("ranked", {})
        if top_k not in got:
            mz, it = _check_f64("mz_arr", last["mz"]), _check_f64("int_arr", last["it"])
            psm = dict(n_psm=1, mz=mz, intensity=it, peak_off=np.array([0, mz.size], np.int64), pep=last["pep"],
                       pep_off=np.array([0, last["pep"].size], np.int64), n_of_mod=np.array([int(last["k"])], np.int32),
                       max_charge=np.array([int(last["z"])], np.int32), aux_pos=last["aux_pos"], aux_mass=last["aux_mass"],
                       aux_off=np.array([0, np.size(last["aux_pos"])], np.int64))
            self._ensure_kept()          # (score_batch does: before the state it leaves is put back)
            state = (self._last, self._batch_n, self._lazy_batch)
            res = self.score_batch(psm, ranked=top_k, site_sig_cap=0)
            self._last, self._batch_n, self._lazy_batch = state
            if int(res["best_sig"][0]) != int(last["best_sig"]):
                raise RuntimeError("the arrays passed to score() changed before ranked() was called")
            got[top_k] = res["ranked"][0]
        return got[top_k].copy()

    def named(self, signatures):
        """The named-localisation records (``NAMED_DTYPE``, see ``score_batch(named=...)``) of the last ``score()`` PSM for
        ``signatures`` (signature bits, or 0 / 1 arrays like ``pep_scores[i]["signature"]``): dict(named, counts, scores).
        Produced when called, by sending that PSM through the batch path as a batch of one, like ``evidence``."""
        last = self._last
        if last is None:
            raise RuntimeError("named needs a scored PSM")
        bits = [sum(1 << j for j, v in enumerate(s) if int(v)) if np.ndim(s) else int(s) for s in signatures]
        mz, it = _check_f64("mz_arr", last["mz"]), _check_f64("int_arr", last["it"])
        psm = dict(n_psm=1, mz=mz, intensity=it, peak_off=np.array([0, mz.size], np.int64), pep=last["pep"],
                   pep_off=np.array([0, last["pep"].size], np.int64), n_of_mod=np.array([int(last["k"])], np.int32),
                   max_charge=np.array([int(last["z"])], np.int32), aux_pos=last["aux_pos"], aux_mass=last["aux_mass"],
                   aux_off=np.array([0, np.size(last["aux_pos"])], np.int64))
        self._ensure_kept()          # (score_batch does: before the state it leaves is put back)
        state = (self._last, self._batch_n, self._lazy_batch)
        res = self.score_batch(psm, named=[np.array(bits, np.uint64)])
        self._last, self._batch_n, self._lazy_batch = state
        if int(res["best_sig"][0]) != int(last["best_sig"]):
            raise RuntimeError("the arrays passed to score() changed before named() was called")
        return dict(named=res["named"], counts=res["named_counts"], scores=res["named_scores"])

    def _batch_of_one_records(self):
        """evidence, ions and coverage of score()'s PSM: the arrays it was given, through the batch path as a batch of one"""
        last = self._last
        if "evidence" not in last:
            mz, it = _check_f64("mz_arr", last["mz"]), _check_f64("int_arr", last["it"])
            pep, ap, am = last["pep"], np.ascontiguousarray(last["aux_pos"], np.uint32), np.ascontiguousarray(last["aux_mass"], np.float32)
            k = max(1, int(last["k"]))
            off = {name: np.array([0, v], np.int64) for name, v in (("peak", mz.size), ("pep", pep.size), ("aux", ap.size))}
            kz = np.array([int(last["k"])], np.int32), np.array([int(last["z"])], np.int32)
            res = (np.zeros(1, np.float32), np.zeros(1, np.uint64), np.zeros(1, np.int32), np.zeros((1, k), np.float32),
                   np.zeros((1, k), np.uint64))
            b = _lib.Batch(1, _as_ptr(off["peak"]), _as_ptr(pep), _as_ptr(off["pep"]), _as_ptr(kz[0]), _as_ptr(kz[1]),
                           _as_ptr(ap), _as_ptr(am), _as_ptr(off["aux"]))
            r = _lib.Results(k, *[_as_ptr(a) for a in res])
            # (no PYA_FLAG_KEEP: the plan path leaves the staging and the retained records of score()'s PSM alone)
            rc = self._lib.pya_score_batch(self._h, C.byref(b), _as_ptr(mz), _as_ptr(it), _lib.PYA_FLAG_EVIDENCE | _lib.PYA_FLAG_IONS | _lib.PYA_FLAG_COVERAGE,
                                           C.byref(r))
            ev, cov = np.zeros((1, k), EVIDENCE_DTYPE), np.zeros(1, COVERAGE_DTYPE)
            if not rc:
                rc = self._lib.pya_last_batch_evidence(self._h, _as_ptr(ev), 1, k)
            if not rc:
                rc = self._lib.pya_last_batch_coverage(self._h, _as_ptr(cov), 1)
            if rc:
                self._raise(rc)
            if int(res[1][0]) != int(last["best_sig"]):
                raise RuntimeError("the arrays passed to score() changed before evidence was read")
            last["ions"] = self._last_batch_ions(1)[1]
            last["coverage"] = cov[0]
            last["evidence"] = ev[0]

    @property
    def alt_sites(self):
        if self._last is None:
            return []
        return [np.array(self.alt_positions(self._last["alt_mask"][j], self._last["pep"]), dtype=np.uint32)
                for j in range(self._last["k"])]

    def alt_positions(self, mask, pep):
        """1-based peptide positions named by one ``alt_mask`` word of a PSM with the letters ``pep`` (bytes / uint8
        array).  Bit p = residue p for peptides of up to 64 residues; for longer ones (scored by the general kernel)
        bit j = the j-th modifiable residue (include/pyascore_hip.h: pya_results.alt_mask)."""
        m = int(mask)
        pep = np.frombuffer(bytes(pep), dtype=np.uint8) if not isinstance(pep, np.ndarray) else np.ascontiguousarray(pep, np.uint8)
        if pep.size <= 64:
            return [p + 1 for p in range(64) if (m >> p) & 1]
        ns = C.c_int32(0)
        pos = np.zeros(_lib.PYA_MAX_PEPTIDE_LEN, np.uint16)
        self._lib.pya_count_sites(self._h, _as_ptr(pep), pep.size, C.byref(ns), _as_ptr(pos))
        return [int(pos[j]) + 1 for j in range(min(int(ns.value), 64)) if (m >> j) & 1]

    def calculate_ambiguity(self, ref_score, other_score):
        """Calculate ambiguity between 2 competing localizations of the last scored PSM
        (Ascore.pyx:208-230).  Inputs should come from ``pep_scores``."""
        if self._last is None:
            raise RuntimeError("calculate_ambiguity needs a scored PSM")
        self._ensure_kept()
        from_sig = lambda s: sum(1 << j for j, v in enumerate(s) if int(v))  # noqa: E731
        rs = np.ascontiguousarray(ref_score["scores"], np.float32)
        os_ = np.ascontiguousarray(other_score["scores"], np.float32)
        if rs.size != self._n_top or os_.size != self._n_top:
            raise ValueError("score containers must hold %d depth scores (n_top)" % self._n_top)
        out = C.c_float()
        rc = self._lib.pya_calculate_ambiguity(
            self._h, 0, from_sig(ref_score["signature"]), _as_ptr(rs), float(ref_score["weighted_score"]),
            from_sig(other_score["signature"]), _as_ptr(os_), float(other_score["weighted_score"]),
            C.byref(out))
        if rc:
            self._raise(rc)
        return float(out.value)
