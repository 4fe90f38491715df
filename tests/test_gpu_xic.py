"""The precursor-XIC stage on the GPU (pya_xic_params): pya_xic_survey_check, pya_xic_spectra and pya_xic_values against
pyascore_amd.rollup.survey_ascending / xic / xic_values, the numpy restatements that tests/test_xic_host.py holds against the
plain-Python yardstick -- every comparison is on raw bytes --, the bounds of everything they write and read, their refusals,
the host form, the device forms, the resident chain down to a site table, score_batch(xic=...) and --xic."""
import base64
import ctypes as C
import os

import numpy as np
import pytest

import site_quant_ref as sq_ref
import xic_cases as xc
from oracle import harness
from pyascore_amd import _lib, rollup as ru, synth

pytestmark = pytest.mark.gpu

GUARD = 16
SCALE = 10
NO_READING = 0x7FF8000000000000
A, S, SP, LV, RV, U, LO, RO = (ru.XIC_ACTIVE, ru.XIC_SEEN, ru.XIC_SEED_PRESENT, ru.XIC_LEFT_VALLEY, ru.XIC_RIGHT_VALLEY, ru.XIC_UNSORTED,
                               ru.XIC_LEFT_OPEN, ru.XIC_RIGHT_OPEN)
_cache = {}


def _any_gpu():
    """a scorer for the calls that do not score (one per process)"""
    if "any" not in _cache:
        from pyascore_amd import PyAscore
        _cache["any"] = harness.make_scorer(PyAscore, synth.describe("cfg2", 1, seed=1)["settings"])
    return _cache["any"]


class _Call:
    """One pya_xic_survey_check + pya_xic_spectra pair on torch's current stream with canaries behind everything they may write:
    0xA5 guard bytes behind d_scan_ok and guard records behind d_xic, guard words behind d_over.  ``check()`` waits, looks at the
    canaries and at the inputs and returns (records[n_query], over, scan_ok) of the host."""

    def __init__(self, mz, it, off, rt, queries, params):
        import torch
        self.torch, self.gpu = torch, _any_gpu()
        self.dev = dev = torch.device("cuda", self.gpu.device)
        self.host_in = [np.ascontiguousarray(a) for a in (mz, it, np.asarray(off, np.int64), np.asarray(rt, np.float64)) + tuple(queries)]
        self.n, self.n_survey, self.n_query = mz.size, len(off) - 1, len(queries[0])
        self.rule = params
        to = lambda a: torch.from_numpy(a if a.size else np.zeros(1, a.dtype)).to(dev)      # noqa: E731 (an address for empty arrays too)
        self.dev_in = [to(a) for a in self.host_in]
        self.ok = torch.from_numpy(np.full(self.n_survey + GUARD, 0xA5, np.uint8)).to(dev)
        self.xic = torch.from_numpy(np.full((self.n_query + GUARD, 64), 0xA5, np.uint8)).to(dev)
        over = np.full(2 + GUARD, 0x5A5A, np.int32)
        over[:2] = 0
        self.over = torch.from_numpy(over).to(dev)
        d = self.dev_in
        self.t_in = _lib.TypedSpectra(d[0].data_ptr(), d[1].data_ptr(), _lib.spectrum_type(mz.dtype), _lib.spectrum_type(it.dtype))

    def stream(self):
        return self.torch.cuda.current_stream(self.dev).cuda_stream

    def check_scans(self, **change):
        a = dict(t_in=C.byref(self.t_in), off=self.dev_in[2].data_ptr(), n_survey=self.n_survey, n_peaks=self.n, ok=self.ok.data_ptr())
        a.update(change)
        return self.gpu._lib.pya_xic_survey_check(self.gpu._h, a["t_in"], a["off"], a["n_survey"], a["n_peaks"], self.stream(), a["ok"])

    def run(self, rule=None, **change):
        d = self.dev_in
        a = dict(t_in=C.byref(self.t_in), off=d[2].data_ptr(), n_survey=self.n_survey, n_peaks=self.n, rt=d[3].data_ptr(), ok=self.ok.data_ptr(),
                 seed=d[4].data_ptr(), lo=d[5].data_ptr(), hi=d[6].data_ptr(), pm=d[7].data_ptr(), pz=d[8].data_ptr(), n_query=self.n_query,
                 params=C.byref(ru.xic_c_params(self.rule if rule is None else rule)), xic=self.xic.data_ptr(), over=self.over.data_ptr())
        a.update(change)
        return self.gpu._lib.pya_xic_spectra(self.gpu._h, a["t_in"], a["off"], a["n_survey"], a["n_peaks"], a["rt"], a["ok"], a["seed"], a["lo"],
                                             a["hi"], a["pm"], a["pz"], a["n_query"], a["params"], self.stream(), a["xic"], a["over"])

    def host(self):
        self.torch.cuda.synchronize(self.dev)
        return self.xic.cpu().numpy(), self.over.cpu().numpy(), self.ok.cpu().numpy()

    def untouched(self, ok_too=True):
        xic, over, ok = self.host()
        return (xic == 0xA5).all() and over.tolist() == [0, 0] + [0x5A5A] * GUARD and (not ok_too or (ok == 0xA5).all())

    def check(self, written=True):
        xic, over, ok = self.host()
        n = self.n_query if written else 0
        assert (xic[n:] == 0xA5).all(), "guard behind d_xic"
        assert over[2:].tolist() == [0x5A5A] * GUARD, "guard behind d_over"
        assert (ok[self.n_survey:] == 0xA5).all(), "guard behind d_scan_ok"
        for h, d in zip(self.host_in, self.dev_in):
            assert d.cpu().numpy()[:h.size].tobytes() == h.tobytes(), "the inputs are only read"
        return np.ascontiguousarray(xic[:n]).view(ru.XIC_DTYPE).reshape(-1), over[:2].view(np.uint32), ok[:self.n_survey]


def _equals_restatement(mz, it, off, rt, queries, params, what, want=None):
    """check kernel, then the trace kernel, against survey_ascending and rollup.xic (or ``want`` where it is at hand)"""
    call = _Call(mz, it, off, rt, queries, params)
    assert call.check_scans() == 0 and call.run() == 0, call.gpu._lib.pya_last_error(call.gpu._h)
    got, g_over, g_ok = call.check()
    assert g_ok.tobytes() == ru.survey_ascending(mz, off).tobytes(), what
    want, w_over = ru.xic(mz, it, off, rt, *queries, params) if want is None else want
    assert got.shape == want.shape and got.tobytes() == want.tobytes(), (what, np.flatnonzero(got != want)[:5])
    assert g_over.tolist() == ([0, 0] if not w_over[0] else [w_over[0], 0xFFFFFFFF - w_over[1]]), what
    return got


def _elution(seed=5, n_survey=90, n_query=120, types="f64/f32", **kw):
    key = ("elution", seed, n_survey, n_query, types, tuple(sorted(kw.items())))
    if key not in _cache:
        rng = np.random.default_rng(seed)
        scans, rt, precs = xc.elution(rng, n_survey, background=12, unsorted=0.06)
        _cache[key] = xc.pack(scans, *xc.TYPES[types]) + (rt, xc.elution_queries(rng, n_query, n_survey, precs, **kw))
    return _cache[key]


# ---- the kernels against the restatements ----

def _sized_scans(isotopes=3):
    """scans of 0, 1, 63, 64, 65 and 4 097 peaks with the precursor's isotope cluster (500.0, 500.5, 501.0, 501.5 at charge 2, step
    1.0) as the first elements, the last ones, and on either side of the first search midpoint; fillers well below and above"""
    scans, where = [], []
    cluster = [(xc.PM + 0.5 * i, float(2 ** (10 - i))) for i in range(isotopes + 1)]
    for length in (0, 1, 63, 64, 65, 4097):
        if length < len(cluster):
            scans.append(cluster[:length])
            where.append((length, 0))
            continue
        room = length - len(cluster)
        mid = length // 2
        for start in sorted({0, room, max(0, min(room, mid - len(cluster))), min(room, mid), max(0, min(room, mid - 1))}):
            below = [(300.0 + 0.01 * k, 5.0) for k in range(start)]
            above = [(700.0 + 0.01 * k, 6.0) for k in range(room - start)]
            scans.append(below + cluster + above)
            where.append((length, start))
    return scans, where


@pytest.mark.parametrize("types", sorted(xc.TYPES))
def test_scan_sizes_and_search_midpoints(types):
    scans, where = _sized_scans()
    assert 20 < len(scans) <= 64 and sorted({w[0] for w in where}) == [0, 1, 63, 64, 65, 4097]
    mz, it, off = xc.pack(scans, *xc.TYPES[types])
    n = len(scans)
    rows = [(k, k, k + 1, xc.PM, xc.Z) for k in range(n)] + [(n // 2, 0, n, xc.PM, xc.Z), (1, 0, n, xc.PM, xc.Z)]
    prm = xc.params(isotopes=3, max_gap=1)
    rec = _equals_restatement(mz, it, off, np.arange(float(n)), xc.queries(rows), prm, types)
    full = [k for k, (length, _) in enumerate(where) if length >= 4]
    assert (rec["iso_hit"][full] == 15).all() and (rec["apex_intensity"][full] == 1024.0 + 512.0 + 256.0 + 128.0).all()
    assert rec["flags"][0] == A and rec["iso_hit"][1] == 1 and rec["n_present"][n] == n - 1


@pytest.mark.parametrize("width", [1, 2, 63, 64, 65])
def test_window_sizes(width):
    rng = np.random.default_rng(width)
    trace = [None if rng.uniform() < 0.15 else float(rng.integers(1, 2000)) for _ in range(70)]
    mz, it, off = xc.pack(xc.trace_scans(trace))
    rows = [(lo + min(width - 1, 3), lo, lo + width, xc.PM, xc.Z) for lo in (0, 2, 70 - width)] + \
        [(lo + width - 1, lo, lo + width, xc.PM, xc.Z) for lo in (0, 70 - width)] + [(0, 0, width, xc.PM, xc.Z), (69, 70 - width, 70, xc.PM, xc.Z)]
    rec = _equals_restatement(mz, it, off, np.cumsum(rng.uniform(0.5, 2.0, 70)), xc.queries(rows), xc.params(), width)
    if width == 65:
        assert not rec.tobytes().strip(b"\0")                              # one scan too many: zero records, all reported
    else:
        assert (rec["flags"] & A).all() and (rec["n_present"] <= width).all()


def test_range_errors_silent_seeds_and_clipped_scans():
    mz, it, off = xc.pack(xc.trace_scans(xc.HAND))
    rt = np.arange(9.0)
    rows = [(-1, 0, 9, xc.PM, 2), (2, 0, 10, xc.PM, 2), (2, 3, 9, xc.PM, 2), (9, 0, 9, xc.PM, 2), (2, -1, 9, xc.PM, 2), (2, 0, 9, xc.PM, 0),
            (2, 0, 9, xc.PM, 9), (2, 0, 9, xc.NAN, 2), (2, 0, 9, xc.INF, 2), (2, 0, 9, -1.0, 2), (2, 0, 10, xc.PM, 0), (2, 0, 9, xc.PM, 2),
            (-(1 << 40), 0, 9, xc.PM, 2), (1 << 40, 0, (1 << 40) + 1, xc.PM, 2), (5, (1 << 62), -(1 << 62), xc.PM, 2), (2, 2, 2, xc.PM, 2)]
    rec = _equals_restatement(mz, it, off, rt, xc.queries(rows), xc.params(), "range errors")
    assert not rec[:11].tobytes().strip(b"\0") and rec["area"][11] == 515.0 and not rec[12:].tobytes().strip(b"\0")
    # no survey spectra at all: every query with a seed is out of range
    call = _Call(mz[:0], it[:0], off[:1], rt[:0], xc.queries(rows), xc.params())
    assert call.check_scans() == 0 and call.run() == 0
    rec, over, _ = call.check()
    assert not rec.tobytes().strip(b"\0") and over.tolist() == [14, 0xFFFFFFFF - 1]
    # offsets that run past the elements the arrays hold are clipped, and the query is reported as well
    q = xc.queries([(2, 0, 9, xc.PM, 2), (2, 0, 7, xc.PM, 2), (-1, 0, 9, xc.PM, 2)])
    call = _Call(mz, it, off, rt, q, xc.params())
    assert call.check_scans(n_peaks=7) == 0 and call.run(n_peaks=7) == 0     # scans 7 and 8 are cut to nothing
    rec, over, ok = call.check()
    cut = off.copy()
    cut[8:] = 7
    want, _ = ru.xic(mz[:7], it[:7], cut, rt, *q, xc.params())
    assert rec.tobytes() == want.tobytes() and rec["n_present"].tolist() == [7, 7, 0] and over.tolist() == [1, 0xFFFFFFFF] and ok.all()


@pytest.mark.parametrize("n_query", [1, 255, 256, 257, 8200])
def test_launch_sizes(n_query):
    """8 200 queries: the grid caps at 2 048 workgroups of 4 wavefronts and strides"""
    mz, it, off, rt, q = _elution(n_query=410, max_window=24)
    if "410" not in _cache:
        _cache["410"] = ru.xic(mz, it, off, rt, *q, ru.xic_params())
    rec410, over410 = _cache["410"]
    reps = -(-n_query // 410)
    tiled = tuple(np.tile(a, reps)[:n_query] for a in q)
    outside = np.flatnonzero(np.tile((rec410["flags"] == 0) & (q[0] >= 0) & ((q[2] > 90) | (q[0] >= q[2]) | (q[0] < q[1])), reps)[:n_query])
    want = (np.tile(rec410, reps)[:n_query], (int(outside.size), int(outside[0]) if outside.size else None))
    if n_query == 257:                                                       # (the tiling's own bookkeeping, once against the restatement)
        direct = ru.xic(mz, it, off, rt, *tiled, ru.xic_params())
        assert direct[0].tobytes() == want[0].tobytes() and direct[1] == want[1] and over410[0] > 0
    rec = _equals_restatement(mz, it, off, rt, tiled, ru.xic_params(), n_query, want=want)
    assert n_query < 255 or ((rec["flags"] & S) != 0).sum() > n_query // 4


@pytest.mark.parametrize("types", sorted(xc.TYPES))
@pytest.mark.parametrize("max_gap", [0, 1, 8])
@pytest.mark.parametrize("isotopes", [0, 1, 2, 3])
def test_parameters_and_types(isotopes, max_gap, types):
    mz, it, off, rt, q = _elution(types=types)
    prm = ru.xic_params(isotopes=isotopes, max_gap=max_gap, rise=(1.0, 2.0, 3.5)[isotopes % 3], tol=0.002 * (max_gap % 2))
    rec = _equals_restatement(mz, it, off, rt, q, prm, (isotopes, max_gap, types))
    flags = int(np.bitwise_or.reduce(rec["flags"]))
    assert flags & (LV | RV) and flags & U and flags & LO and ((rec["flags"] & S) != 0).sum() > 40 and int(rec["iso_hit"].max()) < 2 ** (isotopes + 1)


def test_hand_case_and_ulp_cases():
    mz, it, off = xc.pack(xc.trace_scans(xc.HAND))
    rec = _equals_restatement(mz, it, off, np.arange(9.0), xc.queries([(2, 0, 9, xc.PM, xc.Z), (6, 0, 9, xc.PM, xc.Z)]), xc.params(), "by hand")
    assert rec["area"].tolist() == [515.0, 715.0] and rec["sum_intensity"].tolist() == [530.0, 730.0] and rec["apex_scan"].tolist() == [2, 6]
    assert rec["flags"].tolist() == [A | S | SP | RV | LO, A | S | SP | LV | RO]
    assert (rec["left_scan"].tolist(), rec["right_scan"].tolist()) == ([0, 4], [4, 8])
    for t in (np.float64, np.float32):
        scans, expected = xc.edge_scans(t)
        mz, it, off = xc.pack(scans, t, t)
        q = xc.queries((k, k, k + 1, xc.PM, xc.Z) for k in range(len(scans)))
        rec = _equals_restatement(mz, it, off, np.zeros(len(scans)), q, xc.params(isotopes=3), t)
        for k, (i, inside) in enumerate(expected):
            assert bool(rec["iso_hit"][k] >> i & 1) == inside, (t, k, i, inside)
    # equal maxima, NaN / negative / zero / infinite intensities, a NaN m/z alone in a scan, a scan that does not ascend
    x = xc.PM
    scans = [[(x - xc.T, 3.0), (x, 7.0), (x, 7.0), (x, xc.NAN), (x, -5.0), (x, 0.0), (x, -0.0), (x + xc.T, 2.0), (x + 1.0, 100.0)],
             [(xc.NAN, 5.0)], [(x, 1.0), (x, xc.INF)], [(x, 4.0)], [(x + 1.0, 1.0), (x, 50.0)], [(x, 4.0), (xc.NAN, 1.0)], [(x, 9.0)]]
    mz, it, off = xc.pack(scans)
    rows = [(0, 0, 1, x, 2), (1, 1, 2, x, 2), (3, 2, 4, x, 2), (6, 4, 7, x, 2), (0, 0, 7, x, 2)]
    rec = _equals_restatement(mz, it, off, np.arange(7.0) * 2.0, xc.queries(rows), xc.params(max_gap=2), "special values")
    assert rec["apex_intensity"].tolist() == [7.0, 0.0, xc.INF, 9.0, xc.INF] and rec["flags"][3] == A | S | SP | U | RO and rec["area"][2] == xc.INF


def test_survey_check():
    """ascending scans, equal neighbours, one descent at a stride boundary (elements 63 / 64), at the last pair, a NaN"""
    up = lambda n: [(300.0 + k, 1.0) for k in range(n)]                      # noqa: E731
    def swapped(n, j):
        s = up(n)
        s[j], s[j + 1] = s[j + 1], s[j]
        return s
    scans = [[], up(1), up(2), up(64), up(65), up(129), [(5.0, 1.0)] * 70, swapped(65, 63), swapped(129, 63), swapped(129, 127), swapped(2, 0),
             swapped(200, 198), swapped(64, 62), [(xc.NAN, 1.0)], up(3) + [(xc.NAN, 1.0)], [(xc.NAN, 1.0)] + up(3), up(64) + [(xc.NAN, 1.0)],
             swapped(4097, 4032), up(4097), [(xc.INF, 1.0), (xc.INF, 1.0)], [(-xc.INF, 1.0), (0.0, 1.0), (xc.INF, 1.0)]]
    want = [1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 1, 1]
    for mz_t in (np.float64, np.float32):
        mz, it, off = xc.pack(scans, mz_t, np.float32)
        assert ru.survey_ascending(mz, off).tolist() == want
        call = _Call(mz, it, off, np.zeros(len(scans)), xc.queries([(0, 0, 1, xc.PM, 2)]), xc.params())
        assert call.check_scans() == 0
        assert call.check(written=False)[2].tolist() == want
        lib, h = call.gpu._lib, call.gpu._h
        bad = dict(null_in=dict(t_in=None), null_off=dict(off=None), null_ok=dict(ok=None), too_many=dict(n_survey=0xFFFFFFFF),
                   types=dict(t_in=C.byref(_lib.TypedSpectra(call.t_in.mz, call.t_in.intensity, 3, 0))),
                   null_mz=dict(t_in=C.byref(_lib.TypedSpectra(None, call.t_in.intensity, call.t_in.mz_type, call.t_in.intensity_type))))
        fresh = _Call(mz, it, off, np.zeros(len(scans)), xc.queries([(0, 0, 1, xc.PM, 2)]), xc.params())
        for name, change in bad.items():
            assert fresh.check_scans(**change) == _lib.PYA_ERR_ARG and b"pya_xic_survey_check" in lib.pya_last_error(h), name
        assert fresh.check_scans(n_survey=0, off=None, ok=None) == 0 and fresh.untouched()


def test_refusals_launch_nothing():
    mz, it, off = xc.pack(xc.trace_scans(xc.HAND))
    q = xc.queries([(2, 0, 9, xc.PM, 2), (6, 0, 9, xc.PM, 2)])
    call = _Call(mz, it, off, np.arange(9.0), q, xc.params())
    lib, h = call.gpu._lib, call.gpu._h

    def params(**kw):
        p = ru.xic_c_params(xc.params())
        for k, v in kw.items():
            setattr(p, k, v)
        return C.byref(p)

    def typed(mz_ptr, it_ptr, mz_type, it_type):
        return C.byref(_lib.TypedSpectra(mz_ptr, it_ptr, mz_type, it_type))

    i = call.t_in
    nan, inf = float("nan"), float("inf")
    bad = dict(
        null_in=dict(t_in=None), null_off=dict(off=None), null_rt=dict(rt=None), null_ok=dict(ok=None), null_seed=dict(seed=None),
        null_lo=dict(lo=None), null_hi=dict(hi=None), null_pm=dict(pm=None), null_pz=dict(pz=None), null_xic=dict(xic=None),
        null_over=dict(over=None), null_params=dict(params=None), null_mz=dict(t_in=typed(None, i.intensity, i.mz_type, i.intensity_type)),
        null_it=dict(t_in=typed(i.mz, None, i.mz_type, i.intensity_type)), unknown_type=dict(t_in=typed(i.mz, i.intensity, 2, 0)),
        unknown_it_type=dict(t_in=typed(i.mz, i.intensity, 0, 7)), f32_mz_f64_it=dict(t_in=typed(i.mz, i.intensity, _lib.PYA_F32, _lib.PYA_F64)),
        misaligned=dict(xic=call.xic.data_ptr() + 4), too_many_queries=dict(n_query=0xFFFFFFFF), too_many_surveys=dict(n_survey=0xFFFFFFFF),
        tol_negative=dict(params=params(tol=-0.01)), tol_nan=dict(params=params(tol=nan)), tol_inf=dict(params=params(tol=inf)),
        ppm_negative=dict(params=params(tol_ppm=-1.0)), ppm_nan=dict(params=params(tol_ppm=nan)), ppm_inf=dict(params=params(tol_ppm=inf)),
        step_zero=dict(params=params(step=0.0)), step_negative=dict(params=params(step=-1.0)), step_nan=dict(params=params(step=nan)),
        step_inf=dict(params=params(step=inf)), rise_low=dict(params=params(rise=0.999)), rise_nan=dict(params=params(rise=nan)),
        rise_inf=dict(params=params(rise=inf)), isotopes_4=dict(params=params(isotopes=4)), gap_9=dict(params=params(max_gap=9)),
        wrapped=dict(params=params(isotopes=0xFFFFFFFF)),
    )
    for name, change in bad.items():
        assert call.run(**change) == _lib.PYA_ERR_ARG, name
        assert b"pya_xic_spectra" in lib.pya_last_error(h), (name, lib.pya_last_error(h))
    assert call.untouched()                                                  # nothing was launched, nothing was written
    null = C.byref(_lib.TypedSpectra(None, None, 0, 0))
    assert call.run(n_query=0, t_in=null, off=None, rt=None, ok=None, seed=None, lo=None, hi=None, pm=None, pz=None, xic=None, over=None, n_peaks=0) == 0
    assert call.run(n_query=0) == 0 and call.untouched()
    # (the same checks in front of the host form, and of the values column)
    rec, over = np.zeros(2, ru.XIC_DTYPE), np.zeros(2, np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)                              # noqa: E731
    rt = np.arange(9.0)
    h_in = _lib.TypedSpectra(vp(mz), vp(it), 0, 0)
    host = lambda **kw: lib.pya_xic_spectra_host(h, kw.get("t_in", C.byref(h_in)), vp(kw.get("off", off)), off.size - 1,   # noqa: E731
                                                 kw.get("rt", vp(rt)), None, kw.get("seed", vp(q[0])), vp(q[1]), vp(q[2]), vp(q[3]), vp(q[4]), 2,
                                                 kw.get("params", params()), vp(rec), vp(over))
    for name, kw in dict(types=dict(t_in=typed(vp(mz), vp(it), _lib.PYA_F32, _lib.PYA_F64)), params=dict(params=params(rise=0.5)),
                         descending=dict(off=off[::-1].copy()), negative=dict(off=off - 1), null_seed=dict(seed=None), null_rt=dict(rt=None)).items():
        assert host(**kw) == _lib.PYA_ERR_ARG, name
        assert b"pya_xic_spectra_host" in lib.pya_last_error(h), name
    assert not rec.tobytes().strip(b"\0")
    assert host() == 0 and rec["area"].tolist() == [515.0, 715.0] and over.tolist() == [0, 0]
    d_out = call.torch.full((2 + GUARD,), -7.0, dtype=call.torch.float64, device=call.dev)
    values = lambda **kw: lib.pya_xic_values(h, kw.get("xic", call.xic.data_ptr()), kw.get("n", 2), kw.get("which", 0), call.stream(),   # noqa: E731
                                             kw.get("out", d_out.data_ptr()))
    for name, kw in dict(which=dict(which=4), null_xic=dict(xic=None), null_out=dict(out=None), many=dict(n=0xFFFFFFFF),
                         misaligned=dict(out=d_out.data_ptr() + 4)).items():
        assert values(**kw) == _lib.PYA_ERR_ARG and b"pya_xic_values" in lib.pya_last_error(h), name
    assert values(n=0, xic=None, out=None) == 0
    call.torch.cuda.synchronize(call.dev)
    assert (d_out.cpu().numpy() == -7.0).all()


def test_values_kernel():
    import torch
    from pyascore_amd import device
    gpu = _any_gpu()
    dev = torch.device("cuda", gpu.device)
    mz, it, off, rt, q = _elution()
    rec, _ = ru.xic(mz, it, off, rt, *q, ru.xic_params())
    rec = np.concatenate([rec, np.zeros(5, ru.XIC_DTYPE)])
    rec["flags"][-5:] = [A | S, A, A | S, 0, A | S]
    rec["area"][-5:] = [2.5, 3.0, 0.0, 1.0, xc.NAN]
    rec["apex_intensity"][-5:], rec["seed_intensity"][-5:], rec["sum_intensity"][-5:] = 7.0, [0.0, 1.0, 2.0, 3.0, 4.0], xc.INF
    rec = np.tile(rec, 5)                                                    # 625 records: more than two workgroups
    d_rec = torch.from_numpy(rec.view(np.uint8).reshape(-1, 64).copy()).to(dev)
    for which, name in enumerate(("area", "apex", "seed", "sum")):
        want = ru.xic_values(rec, name)
        out = torch.full((rec.size + GUARD, 1), -7.0, dtype=torch.float64, device=dev)
        got = device.xic_values(gpu, d_rec, which, out=out[:rec.size])
        assert got.data_ptr() == out.data_ptr() and out.cpu().numpy()[:rec.size, 0].tobytes() == want.tobytes(), name
        assert (out.cpu().numpy()[rec.size:] == -7.0).all(), "guard behind d_out"
        assert device.xic_values(gpu, d_rec, name).cpu().numpy().tobytes() == want.tobytes()
        assert np.isnan(want).any() and (want > 0).any() and (want.view(np.uint64)[np.isnan(want)] == NO_READING).all()
    assert d_rec.cpu().numpy().tobytes() == rec.tobytes()
    for bad in (4, "height", True, None):
        with pytest.raises(ValueError):
            device.xic_values(gpu, d_rec, bad)
    with pytest.raises(ValueError):
        device.xic_values(gpu, d_rec[:, :48])
    assert tuple(device.xic_values(gpu, d_rec[:0]).shape) == (0, 1)


@pytest.mark.parametrize("types", sorted(xc.TYPES))
def test_the_host_form_and_the_torch_form_equal_the_device_form(types):
    import torch
    from pyascore_amd import device
    gpu = _any_gpu()
    mz, it, off, rt, q = _elution(types=types)
    params = ru.xic_params(isotopes=3, tol=0.001)
    want, w_over = ru.xic(mz, it, off, rt, *q, params)
    got = _equals_restatement(mz, it, off, rt, q, params, types, want=(want, w_over))
    ok = ru.survey_ascending(mz, off)
    for scan_ok in (None, ok):
        h_rec, h_over = gpu.precursor_xic(mz, it, off, rt, *q, params, scan_ok=scan_ok)
        assert h_rec.dtype == ru.XIC_DTYPE and h_rec.shape == (120,) and h_over == w_over and w_over[0] > 0
        assert h_rec.tobytes() == want.tobytes() == got.tobytes()
    none_ok, _ = gpu.precursor_xic(mz, it, off, rt, *q, params, scan_ok=np.zeros_like(ok))       # scan_ok as given decides
    assert none_ok.tobytes() == ru.xic(mz, it, off, rt, *q, params, scan_ok=np.zeros_like(ok))[0].tobytes() and not (none_ok["flags"] & S).any()
    dev = torch.device("cuda", gpu.device)
    d_mz, d_it = torch.from_numpy(mz).to(dev), torch.from_numpy(it).to(dev)
    for peak_off, d_rt, queries in ((off, rt, q), (torch.from_numpy(off).to(dev), torch.from_numpy(rt).to(dev), tuple(torch.from_numpy(a).to(dev) for a in q))):
        d_ok = device.xic_survey_check(gpu, d_mz, d_it, peak_off)
        assert d_ok.dtype == torch.uint8 and d_ok.cpu().numpy().tobytes() == ok.tobytes()
        d_rec, d_over = device.xic(gpu, d_mz, d_it, peak_off, d_rt, d_ok, *queries, params)
        assert d_rec.dtype == torch.uint8 and tuple(d_rec.shape) == (120, 64)
        assert device.xic_records(d_rec.cpu().numpy()).tobytes() == want.tobytes()
        assert d_over.cpu().numpy().view(np.uint32).tolist() == [w_over[0], 0xFFFFFFFF - w_over[1]]
        again = device.xic(gpu, d_mz, d_it, peak_off, d_rt, ok, *queries, params, out=d_rec.zero_())
        assert again[0] is d_rec and device.xic_records(d_rec.cpu().numpy()).tobytes() == want.tobytes()
    assert d_mz.cpu().numpy().tobytes() == mz.tobytes() and d_it.cpu().numpy().tobytes() == it.tobytes()      # read-only
    for bad in (dict(params=dict(params, rise=0.5)), dict(params=params, out=d_rec[:-1]), dict(params=params, seed=q[0][:-1]),
                dict(params=params, seed=q[0].astype(np.float64)), dict(params=params, rt=rt[:-1])):
        sd, r = bad.pop("seed", q[0]), bad.pop("rt", rt)
        with pytest.raises(ValueError):
            device.xic(gpu, d_mz, d_it, off, torch.from_numpy(r).to(dev), d_ok, torch.from_numpy(sd).to(dev), *q[1:], **bad)
    if types == "f32/f32":                                                   # float32 m/z beside float64 intensities is widened by the host form
        assert gpu.precursor_xic(mz, it.astype(np.float64), off, rt, *q, params)[0].tobytes() == want.tobytes()
    # survey scans without any peak are still a call; no query at all is none
    r, o = gpu.precursor_xic(mz[:0], it[:0], [0, 0], [1.0], [0, 1], [0, 0], [1, 2], [500.0, 500.0], [2, 2], params)
    assert r["flags"].tolist() == [1, 0] and o == (1, 1)
    r, o = gpu.precursor_xic(mz, it, off, rt, [], [], [], [], np.zeros(0, np.int32), params)
    assert r.shape == (0,) and o == (0, None)


# ---- down to a site table ----

def _label_free(n=90):
    """n cfg2 PSMs, the peptides of the first third repeated so that PSMs share slots, and 48 survey scans in which the precursor
    of PSM i (charge 2, its own m/z) elutes as an integer triangle around scan 6 + (5 i mod 36) with two isotopes"""
    if "label_free" not in _cache:
        from pyascore_amd import PyAscore
        base, settings = synth.make_batch("cfg2", n_psm=n, seed=9741)
        kws = [synth.unpack_psm(base, i) for i in range(n)]
        m = n // 3
        psms = [dict(mz=kws[i]["mz_arr"], intensity=kws[i]["int_arr"], peptide=kws[i % m]["peptide"], n_of_mod=kws[i % m]["n_of_mod"],
                     max_charge=kws[i % m]["max_fragment_charge"]) for i in range(n)]
        gpu = harness.make_scorer(PyAscore, settings)
        batch = synth.pack_batch(psms)
        plain = gpu.score_batch(batch, probs=True)
        off = plain["site_off"]
        owner = np.repeat(np.arange(off.size - 1), np.diff(off))
        r = (np.arange(int(off[-1])) - off[owner]).astype(np.uint64)
        in_best = ((plain["best_sig"][owner] >> r) & np.uint64(1) != 0) & (plain["psm_probs"]["kind"][owner] == _lib.PYA_SITE_SCORED)
        thr = float(np.median(plain["site_probs"]["with_prob"][in_best]))
        peptides = [p["peptide"] for p in psms]
        slot, n_slots, _ = ru.peptide_slots(peptides, off, residues=settings["mod_group"])
        rng = np.random.default_rng(11)
        pm = 400.0 + 4.25 * np.arange(n)
        pz = np.full(n, 2, np.int32)
        centre = 6 + (5 * np.arange(n)) % 36
        height = rng.integers(4, 40, n)
        scans = []
        for s in range(48):
            peaks = [(float(x), float(np.floor(y))) for x, y in zip(rng.uniform(300.0, 399.0, 30), rng.uniform(1.0, 50.0, 30))]
            for i in range(n):
                level = int(height[i]) * max(0, 5 - abs(s - int(centre[i])))
                if level and not (i % 7 == 3 and s == centre[i] + 1):                 # (a dropout now and then)
                    peaks += [(pm[i], float(16 * level)), (pm[i] + ru.STRIP_STEP / 2, float(8 * level)), (pm[i] + ru.STRIP_STEP, float(4 * level))]
            scans.append(sorted(peaks))
        ms1 = xc.pack(scans, np.float64, np.float32)
        rt = np.cumsum(rng.uniform(0.75, 1.25, 48))
        seed = (centre + rng.integers(-2, 3, n)).astype(np.int64)
        seed[5] = -1                                                          # a spectrum without a survey scan
        lo, hi = ru.xic_windows(rt, seed, 12.0)
        queries = (seed, lo, hi, pm, pz)
        rule = dict(tol=0.0, tol_ppm=8.0, isotopes=2, rise=2.0, max_gap=1)
        records, over = ru.xic(*ms1, rt, *queries, ru.xic_params(**rule))
        assert over == (0, None) and ((records["flags"] & S) != 0).sum() == n - 1 and (records["iso_hit"][records["flags"] != 0] == 7).all()
        _cache["label_free"] = dict(gpu=gpu, settings=settings, batch=batch, plain=plain, thr=thr, slot=slot, n_slots=n_slots, peptides=peptides,
                                    ms1=ms1, rt=rt, queries=queries, rule=rule, records=records)
    return _cache["label_free"]


def test_resident_chain_equals_the_restatement_chain():
    """survey check -> xic -> values -> site table, nothing read in between"""
    import torch
    from pyascore_amd import device
    from pyascore_amd.device import DevicePlan, site_quant_records
    c = _label_free()
    gpu, batch, plain = c["gpu"], c["batch"], c["plain"]
    dev = torch.device("cuda", gpu.device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)         # noqa: E731
    d_mz, d_it = up(batch["mz"]), up(batch["intensity"])
    d_ms1 = [up(a) for a in c["ms1"]]
    d_rt, d_q, d_slot = up(c["rt"]), [up(a) for a in c["queries"]], up(c["slot"])
    rule = ru.xic_params(**c["rule"])
    plan = DevicePlan(gpu, batch, quant=True)
    plan.run(d_mz, d_it)
    _, sp, pp = plan.probs()
    p = ru.site_quant_params(threshold=c["thr"], scale_log2=SCALE, n_channels=1)
    d_ok = device.xic_survey_check(gpu, *d_ms1)
    d_xic, d_over = device.xic(gpu, *d_ms1, d_rt, d_ok, *d_q, rule)
    d_values = device.xic_values(gpu, d_xic, "area")
    table = plan.site_quant(sp, pp, d_slot, d_values, p, n_slots=c["n_slots"])
    plan.check()
    # the restatement of the same chain
    assert d_ok.cpu().numpy().all() and device.xic_records(d_xic.cpu().numpy()).tobytes() == c["records"].tobytes()
    assert d_over.cpu().numpy().tolist() == [0, 0]
    values = ru.xic_values(c["records"], "area").reshape(-1, 1)
    assert d_values.cpu().numpy().tobytes() == values.tobytes() and np.isnan(values[5, 0]) and (values[np.arange(90) != 5] > 0).all()
    got = site_quant_records((table[0].cpu().numpy(), table[1].cpu().numpy()))
    args = (plain["site_probs"], plain["psm_probs"], plain["site_off"], plain["best_sig"], c["slot"], c["n_slots"])
    want = sq_ref.table(*args, values, None, c["thr"], SCALE)
    assert want[0]["n_records"].sum() > 10 and got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    again = ru.site_quant(*args, values, None, p)
    assert got[0].tobytes() == again[0].tobytes() and got[1].tobytes() == again[1].tobytes()


def _equal_but(got, plain, extra, what):
    for key in plain:
        if key not in extra and key != "status_message":
            g, w = got[key], plain[key]
            assert (g.tobytes() == w.tobytes()) if isinstance(w, np.ndarray) else (g == w), (what, key)
    assert set(got) - set(plain) == set(extra) - set(plain), (what, sorted(set(got) ^ set(plain)))


def test_score_batch_with_xic():
    c = _label_free()
    gpu, batch, thr = c["gpu"], c["batch"], c["thr"]
    ms1_mz, ms1_it, ms1_off = c["ms1"]
    sd, lo, hi, pm, pz = c["queries"]
    req = dict(c["rule"], ms1_mz=ms1_mz, ms1_intensity=ms1_it, ms1_peak_off=ms1_off, rt=c["rt"], seed=sd, scan_lo=lo, scan_hi=hi, precursor_mz=pm,
               precursor_charge=pz)
    roll = dict(slot=c["slot"], n_slots=c["n_slots"])
    group, _, _ = ru.peptide_groups(c["peptides"])
    forms = dict(group=group, threshold=0.75)
    stages = dict(rollup=roll, peptidoforms=forms, probs=True, evidence=True)
    # the records are added and nothing else moves
    without = gpu.score_batch(batch, **stages)
    got = gpu.score_batch(batch, xic=req, **stages)
    _equal_but(got, without, ("xic",), "xic")
    assert got["xic"].dtype == ru.XIC_DTYPE and got["xic"].tobytes() == c["records"].tobytes()
    assert gpu.score_batch(batch, xic=req)["xic"].tobytes() == c["records"].tobytes()            # alone, too
    # the label-free tables: the call given the restatement's column
    tables = ("quant_head", "quant", "peptidoform_quant_head", "peptidoform_quant")
    for name in ("area", "apex"):
        q = dict(values="xic_" + name, threshold=thr, scale_log2=SCALE)
        got = gpu.score_batch(batch, xic=req, quant=q, peptidoform_quant=q, **stages)
        column = ru.xic_values(c["records"], name).reshape(-1, 1)
        explicit = dict(q, values=column)
        want = gpu.score_batch(batch, quant=explicit, peptidoform_quant=explicit, **stages)
        for key in tables:
            assert got[key].tobytes() == want[key].tobytes(), (name, key)
        assert got["quant"]["n"].sum() > 10 and got["quant"].shape[1] == 1
        _equal_but(got, want, ("xic",), "label-free " + name)
    assert got["quant"].tobytes() != gpu.score_batch(batch, xic=req, quant=dict(q, values="xic_area"), **stages)["quant"].tobytes()
    for bad in (dict(req, window=1), dict(req, seed=sd[:-1]), dict(req, rise=0.5), {k: v for k, v in req.items() if k != "rt"}, True):
        with pytest.raises(ValueError):
            gpu.score_batch(batch, xic=bad)
    with pytest.raises(ValueError, match="needs xic="):
        gpu.score_batch(batch, rollup=roll, quant=dict(values="xic_area", threshold=thr))
    with pytest.raises(ValueError, match="xic_area"):
        gpu.score_batch(batch, rollup=roll, xic=req, quant=dict(values="xic_height", threshold=thr))


# ---- the command line ----

def _ms1_spectrum(index, scan, minutes, mz, it):
    arr = lambda a, bits, name: (                                            # noqa: E731
        '<binaryDataArray encodedLength="0"><cvParam cvRef="MS" accession="MS:1000523" name="%d-bit float" value=""/>'
        '<cvParam cvRef="MS" accession="MS:1000576" name="no compression" value=""/><cvParam cvRef="MS" accession="MS:1000514" name="%s" value=""/>'
        "<binary>%s</binary></binaryDataArray>" % (bits, name, base64.b64encode(a.tobytes()).decode()))
    return ('<spectrum index="%d" id="controllerType=0 controllerNumber=1 scan=%d" defaultArrayLength="%d">'
            '<cvParam cvRef="MS" accession="MS:1000579" name="MS1 spectrum" value=""/><cvParam cvRef="MS" accession="MS:1000511" name="ms level" value="1"/>'
            '<cvParam cvRef="MS" accession="MS:1000127" name="centroid spectrum" value=""/><scanList count="1"><scan>'
            '<cvParam cvRef="MS" accession="MS:1000016" name="scan start time" value="%r" unitCvRef="UO" unitAccession="UO:0000031" unitName="minute"/>'
            '</scan></scanList><binaryDataArrayList count="2">%s%s</binaryDataArrayList>'
            "</spectrum>\n" % (index, scan, mz.size, minutes, arr(mz.astype("<f8"), 64, "m/z array"), arr(it.astype("<f4"), 32, "intensity array")))


def test_command_line_file(tmp_path):
    from pyascore_amd import __main__ as cli, batch_cli, ingest
    data = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ingest")
    spec, ident = os.path.join(data, "test_spectra.mzML"), os.path.join(data, "test_psms.pep.xml")
    ms2 = ingest.SpectraParser(spec, "mzML").to_list()
    first = ms2[0]
    assert first["parent_scan"] == 14754 and first["scan"] == 14760
    # nine survey scans in front of the first MS2 scan, the hand case of the rule as its precursor's trace (two isotopes, halved
    # each), half a minute apart; the survey scan it names is the third
    pm, z = first["precursor_mz"], first["precursor_charge"]
    env = pm + ru.STRIP_STEP * np.arange(3) / z
    numbers = [14750 + 2 * k for k in range(9)]
    survey_in = [(np.concatenate([[400.0], env, [1200.0]]), np.array([9.0, y, y / 2, y / 4, 7.0])) for y in xc.HAND]
    text = open(spec).read()
    at = text.index("<spectrum ")
    inline = tmp_path / "with_ms1.mzML"
    inline.write_text(text[:at] + "".join(_ms1_spectrum(k, numbers[k], 40.0 + 0.5 * k, *survey_in[k]) for k in range(9)) + text[at:])
    survey = ingest.SpectraParser(str(inline), "mzML", ms_level=1, native_precision=True, times=True).to_list()
    assert [r["scan"] for r in survey] == numbers and [r["rt"] for r in survey] == [(40.0 + 0.5 * k) * 60.0 for k in range(9)]
    out, table = tmp_path / "ascores.tsv", tmp_path / "xic.tsv"
    opts = ["--mz_error", "0.05", "--hit_depth", "2"]
    xic_opts = ["--xic", str(table), "--xic_rt_window", "200", "--xic_tol_ppm", "20", "--xic_isotopes", "2"]
    rows = cli.run(cli.parse_args(opts + xic_opts + [str(inline), ident, str(out)]), log=lambda *_: None)
    plain = cli.run(cli.parse_args(opts + [spec, ident, str(tmp_path / "plain.tsv")]), log=lambda *_: None)
    assert rows == plain                                                     # the main table is unchanged
    spectra = ingest.SpectraParser(str(inline), "mzML", native_precision=True).to_dict()
    psms = sorted(ingest.IdentificationParser(ident, "pepXML").to_list(), key=lambda p: p["scan"])
    picked, scans = batch_cli.select_psms(psms, spectra, "STY", 79.966331, 2, 5)
    lines = table.read_text().splitlines()
    assert lines[0].split("\t") == batch_cli.XIC_TABLE_COLUMNS and len(lines) == 1 + len(picked)
    ms1 = xc.pack([list(zip(x.tolist(), y.tolist())) for x, y in survey_in], np.float64, np.float32)
    rt = np.array([r["rt"] for r in survey])
    params = ru.xic_params(tol_ppm=20.0, isotopes=2)
    for i, line in enumerate(lines[1:]):
        r = spectra[scans[i]]
        sd = 2 if scans[i] == 14760 else 8                                   # named, or the last survey scan in front
        lo, hi = ru.xic_windows(rt, [sd], 200.0)
        rec, _ = ru.xic(*ms1, rt, [sd], lo, hi, [r["precursor_mz"]], [r["precursor_charge"]], params)
        want = [str(v) for v in [scans[i]] + batch_cli.xic_fields(rec[0], survey, sd, int(lo[0]), int(hi[0]))]
        assert line.split("\t") == want, i
    f = lines[1].split("\t")
    # window: 200 s of 30 s scans reach six scans either way: 0 .. 8; the peak of seed 2 is [0, 4]: 1.75 x 515 x 30 s
    assert f[:4] == ["14760", "14754", "14750", "14766"] and float(f[4]) == 1.75 * 515.0 * 30.0 and float(f[5]) == 525.0
    assert f[6] == "14754" and float(f[7]) == 41.0 * 60.0 and f[10:15] == ["14750", "14758", "5", "9", "111"]
    assert f[15] == "active|seen|seed_present|right_valley|left_open"
    assert any(l.split("\t")[15] == "active" for l in lines[2:])              # the later precursors are not in these scans
    # --purity beside --xic: one pass over the survey scans serves both, and neither table moves
    both = [l for l in open(str(table))]
    ptable = tmp_path / "purity.tsv"
    cli.run(cli.parse_args(opts + xic_opts + ["--purity", str(ptable), "--purity_window", "1.0,1.0", str(inline), ident, str(out)]), log=lambda *_: None)
    assert [l for l in open(str(table))] == both and len(ptable.read_text().splitlines()) == 1 + len(picked)
    # label-free tables: --site_quant / --peptidoform_quant without --marker_mz sum the XIC column
    quant = ["--site_table", str(tmp_path / "sites.tsv"), "--site_quant", str(tmp_path / "q.tsv"), "--peptidoform_quant", str(tmp_path / "pq.tsv"),
             "--site_quant_threshold", "0.0", "--peptidoform_quant_threshold", "0.0"]
    cli.run(cli.parse_args(opts + xic_opts + quant + ["--xic_channel", "area", str(inline), ident, str(out)]), log=lambda *_: None)
    q = (tmp_path / "q.tsv").read_text().splitlines()
    assert q[0].split("\t")[-1] == "xic_area" and (tmp_path / "pq.tsv").read_text().splitlines()[0].split("\t")[-1] == "xic_area"
    sums = [float(l.split("\t")[-1]) for l in q[1:] if l.split("\t")[-1]]
    assert sums and all(v % (1.75 * 515.0 * 30.0) == 0.0 for v in sums)       # only the first spectrum's precursor is in the survey scans
    for bad in (["--xic_channel", "area"], xic_opts + ["--xic_rise", "0.5"], xic_opts + ["--xic_gap", "9"], quant):
        with pytest.raises(ValueError):
            cli.parse_args(opts + bad + [str(inline), ident, str(out)])
