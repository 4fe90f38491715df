"""The precursor-purity stage on the GPU (pya_purity_params): pya_purity_spectra and pya_purity_gate against
pyascore_amd.rollup.purity / purity_gate, the numpy restatement that tests/test_purity_host.py holds against the plain-Python
yardstick -- every comparison is on raw bytes --, the bounds of everything they write and read, their refusals, the host form,
the device forms, the resident chain down to a site table, score_batch(purity=...) and --purity."""
import base64
import ctypes as C
import os

import numpy as np
import pytest

import markers_cases as mc
import purity_cases as pc
import site_quant_ref as sq_ref
from oracle import harness
from pyascore_amd import _lib, rollup as ru, synth

pytestmark = pytest.mark.gpu

TYPES = {"f64/f64": (np.float64, np.float64), "f64/f32": (np.float64, np.float32), "f32/f32": (np.float32, np.float32)}
GUARD = 16
SCALE = 10
NO_READING = 0x7FF8000000000000
_cache = {}


def _any_gpu():
    """a scorer for the calls that do not score (one per process)"""
    if "any" not in _cache:
        from pyascore_amd import PyAscore
        _cache["any"] = harness.make_scorer(PyAscore, synth.describe("cfg2", 1, seed=1)["settings"])
    return _cache["any"]


class _Call:
    """One pya_purity_spectra call on torch's current stream with canaries behind everything it may write: 0xA5 guard records
    behind d_purity, guard words behind d_over.  ``check()`` waits, looks at the canaries and at the inputs and returns
    (records[n_query], over) of the host."""

    def __init__(self, mz, it, off, queries, params):
        import torch
        self.torch, self.gpu = torch, _any_gpu()
        self.dev = dev = torch.device("cuda", self.gpu.device)
        self.host_in = [np.ascontiguousarray(a) for a in (mz, it, np.asarray(off, np.int64)) + tuple(queries)]
        self.n, self.n_survey, self.n_query = mz.size, len(off) - 1, len(queries[0])
        self.rule = params
        to = lambda a: torch.from_numpy(a if a.size else np.zeros(1, a.dtype)).to(dev)      # noqa: E731 (an address for empty arrays too)
        self.dev_in = [to(a) for a in self.host_in]
        self.purity = torch.from_numpy(np.full((self.n_query + GUARD, 48), 0xA5, np.uint8)).to(dev)
        over = np.full(2 + GUARD, 0x5A5A, np.int32)
        over[:2] = 0
        self.over = torch.from_numpy(over).to(dev)
        d = self.dev_in
        self.t_in = _lib.TypedSpectra(d[0].data_ptr(), d[1].data_ptr(), _lib.spectrum_type(mz.dtype), _lib.spectrum_type(it.dtype))

    def run(self, rule=None, **change):
        d = self.dev_in
        a = dict(t_in=C.byref(self.t_in), off=d[2].data_ptr(), n_survey=self.n_survey, n_peaks=self.n, survey=d[3].data_ptr(), pm=d[4].data_ptr(),
                 pz=d[5].data_ptr(), wl=d[6].data_ptr(), wh=d[7].data_ptr(), n_query=self.n_query,
                 params=C.byref(ru.purity_c_params(self.rule if rule is None else rule)), purity=self.purity.data_ptr(), over=self.over.data_ptr())
        a.update(change)
        stream = self.torch.cuda.current_stream(self.dev).cuda_stream
        return self.gpu._lib.pya_purity_spectra(self.gpu._h, a["t_in"], a["off"], a["n_survey"], a["n_peaks"], a["survey"], a["pm"], a["pz"], a["wl"],
                                                a["wh"], a["n_query"], a["params"], stream, a["purity"], a["over"])

    def host(self):
        self.torch.cuda.synchronize(self.dev)
        return self.purity.cpu().numpy(), self.over.cpu().numpy()

    def untouched(self):
        purity, over = self.host()
        return (purity == 0xA5).all() and over.tolist() == [0, 0] + [0x5A5A] * GUARD

    def check(self, written=True):
        purity, over = self.host()
        n = self.n_query if written else 0
        assert (purity[n:] == 0xA5).all(), "guard behind d_purity"
        assert over[2:].tolist() == [0x5A5A] * GUARD, "guard behind d_over"
        for h, d in zip(self.host_in, self.dev_in):
            assert d.cpu().numpy()[:h.size].tobytes() == h.tobytes(), "the inputs are only read"
        return np.ascontiguousarray(purity[:n]).view(ru.PURITY_DTYPE).reshape(-1), over[:2].view(np.uint32)


def _equals_restatement(mz, it, off, queries, params, what):
    call = _Call(mz, it, off, queries, params)
    assert call.run() == 0, call.gpu._lib.pya_last_error(call.gpu._h)
    got, g_over = call.check()
    want, w_over = ru.purity(mz, it, off, *queries, params)
    assert got.shape == want.shape and got.tobytes() == want.tobytes(), (what, np.flatnonzero(got != want)[:5])
    assert g_over.tolist() == ([0, 0] if not w_over[0] else [w_over[0], 0xFFFFFFFF - w_over[1]]), what
    return got


def _one_each(n, wl=pc.WL, wh=pc.WH):
    """query i over survey spectrum i, the base precursor and window"""
    return (np.arange(n, dtype=np.int64), np.full(n, pc.PM), np.full(n, pc.Z, np.int32), np.full(n, wl), np.full(n, wh))


# ---- the kernel against the restatement ----

@pytest.mark.parametrize("types", sorted(TYPES))
def test_stride_and_ballot_boundaries(types):
    """survey scans of 0, 1, 2, 63, 64, 65, 127, 128, 129 and 4 097 peaks in one call, window peaks as the first and the last peak
    and on both sides of every 64-peak boundary; a window that holds a whole 129-peak scan"""
    mz_t, it_t = TYPES[types]
    spectra, planted = pc.boundary_spectra()
    mz, it, off = pc.pack(spectra, mz_t, it_t)
    n = len(spectra)
    assert np.diff(off).tolist() == list(pc.BOUNDARY_LENGTHS)
    rec = _equals_restatement(mz, it, off, _one_each(n), pc.P_BASE, types)
    assert rec["n_window"].tolist() == [len(p) for p in planted] and int(rec["n_window"][9]) == 1 + 2 * 64
    assert (rec["flags"][1:] == 3).all() and rec["flags"][0] == 1 and (rec["iso_hit"][8:] == 7).all() and (rec["other_intensity"][2:] > 0).all()
    whole = _equals_restatement(mz, it, off, (np.array([8, 9], np.int64), np.full(2, pc.PM), np.full(2, pc.Z, np.int32), np.full(2, 0.0),
                                              np.full(2, 1e4)), pc.P_BASE, types + ": the whole scan")
    assert whole["n_window"].tolist() == [129, 4097]


@pytest.mark.parametrize("types", sorted(TYPES))
def test_hand_made_scans(types):
    """every case of tests/purity_cases.py, the cases of one parameter set in one call with empty scans between them"""
    mz_t, it_t = TYPES[types]
    groups = {}
    for c in pc.hand_cases():
        if not (mz_t == np.float32 and c["f64_only"]):
            groups.setdefault(pc.params_key(c["params"]), []).append(c)
    assert len(groups) == 4                                                  # 3, 1 and 16 centres and overlapping ones
    for group in groups.values():
        mz, it, off, *queries = pc.pack_cases(group, mz_t, it_t, gaps=True)
        rec = _equals_restatement(mz, it, off, queries, group[0]["params"], (types, group[0]["name"]))
        want = np.array([c["record"] for c in group], ru.PURITY_DTYPE)
        assert rec.tobytes() == want.tobytes(), [c["name"] for c, g, w in zip(group, rec, want) if g.tobytes() != w.tobytes()]


@pytest.mark.parametrize("n_query", [1, 63, 64, 65, 257])
def test_query_counts(n_query):
    spectra, q = pc.random_inputs(n_query, n_survey=9, n_query=max(n_query, 4))
    q = tuple(a[:n_query] for a in q)
    mz, it, off = pc.pack(spectra, np.float64, np.float32)
    _equals_restatement(mz, it, off, q, ru.purity_params(tol=0.01, tol_ppm=20.0, isotopes=4, below=1), n_query)


def test_more_queries_than_wavefronts_and_many_on_one_scan():
    """8 200 queries: the grid caps at 2 048 workgroups of 4 wavefronts and strides; 40 queries that name one survey scan"""
    spectra, q = pc.random_inputs(77, n_survey=30, n_query=8_200, max_peaks=90)
    q[0][100:140] = 7
    q[2][100:140] = 2
    mz, it, off = pc.pack(spectra)
    rec = _equals_restatement(mz, it, off, q, pc.P_BASE, "8 200 queries")
    assert (rec["flags"] == 3).sum() > 500 and (rec["flags"] == 0).sum() > 500
    spectra, _ = pc.boundary_spectra()
    mz, it, off = pc.pack(spectra)
    one = (np.full(40, 9, np.int64), np.full(40, pc.PM), np.full(40, pc.Z, np.int32), pc.WL + np.arange(40) / 64.0, np.full(40, pc.WH))
    rec = _equals_restatement(mz, it, off, one, pc.P_BASE, "40 queries on one scan")
    assert rec["window"][0] > rec["window"][-1] > 0


def test_out_of_range_survey_writes_zero_records_and_reports():
    spectra, _ = pc.boundary_spectra()
    mz, it, off = pc.pack(spectra[:6])
    q = list(_one_each(12))
    q[0] = np.array([0, 5, 6, 3, 1 << 40, -1, 4, 6, -(1 << 40), 2, 7, 5], np.int64)
    q[2][7] = 0                                                              # (beyond AND unusable: inactive, not reported)
    rec = _equals_restatement(mz, it, off, q, pc.P_BASE, "survey >= n_survey")
    beyond = [2, 4, 10]
    assert not rec[beyond + [5, 7, 8]].tobytes().strip(b"\0") and (rec["flags"][[1, 3, 6, 9, 11]] == 3).all()
    call = _Call(mz, it, off, q, pc.P_BASE)
    assert call.run() == 0
    assert call.check()[1].tolist() == [len(beyond), 0xFFFFFFFF - beyond[0]]
    # no survey spectra at all: every active query is beyond them
    call = _Call(mz[:0], it[:0], off[:1], q, pc.P_BASE)
    assert call.run() == 0
    rec, over = call.check()
    assert not rec.tobytes().strip(b"\0") and over.tolist() == [9, 0xFFFFFFFF]
    # offsets that run past the elements the arrays hold are clipped, and the query is reported as well
    call = _Call(mz, it, off, _one_each(6), pc.P_BASE)
    assert call.run(n_peaks=int(off[5])) == 0                                # spectrum 5 (65 peaks) is cut to nothing
    rec, over = call.check()
    want, _ = ru.purity(mz, it, off, *_one_each(6), pc.P_BASE)
    assert rec[:5].tobytes() == want[:5].tobytes() and rec[5].tolist() == (0.0, 0.0, 0.0, 0.0, 0, 0, 0, 1) and over.tolist() == [1, 0xFFFFFFFF - 5]


def test_refusals_launch_nothing():
    spectra, _ = pc.boundary_spectra()
    mz, it, off = pc.pack(spectra[:6])
    q = _one_each(6)
    call = _Call(mz, it, off, q, pc.P_BASE)
    lib, h = call.gpu._lib, call.gpu._h

    def params(**kw):
        p = ru.purity_c_params(pc.P_BASE)
        for k, v in kw.items():
            if k == "reserved":
                p.reserved[v] = 1
            else:
                setattr(p, k, v)
        return C.byref(p)

    def typed(mz_ptr, it_ptr, mz_type, it_type):
        return C.byref(_lib.TypedSpectra(mz_ptr, it_ptr, mz_type, it_type))

    i = call.t_in
    nan, inf = float("nan"), float("inf")
    bad = dict(
        null_in=dict(t_in=None), null_off=dict(off=None), null_survey=dict(survey=None), null_pm=dict(pm=None), null_pz=dict(pz=None),
        null_wl=dict(wl=None), null_wh=dict(wh=None), null_purity=dict(purity=None), null_over=dict(over=None), null_params=dict(params=None),
        null_mz=dict(t_in=typed(None, i.intensity, i.mz_type, i.intensity_type)), null_it=dict(t_in=typed(i.mz, None, i.mz_type, i.intensity_type)),
        unknown_type=dict(t_in=typed(i.mz, i.intensity, 2, 0)), unknown_it_type=dict(t_in=typed(i.mz, i.intensity, 0, 7)),
        f32_mz_f64_it=dict(t_in=typed(i.mz, i.intensity, _lib.PYA_F32, _lib.PYA_F64)), misaligned=dict(purity=call.purity.data_ptr() + 4),
        too_many_queries=dict(n_query=0xFFFFFFFF), too_many_surveys=dict(n_survey=0xFFFFFFFF),
        tol_negative=dict(params=params(tol=-0.01)), tol_nan=dict(params=params(tol=nan)), tol_inf=dict(params=params(tol=inf)),
        ppm_negative=dict(params=params(tol_ppm=-1.0)), ppm_nan=dict(params=params(tol_ppm=nan)), ppm_inf=dict(params=params(tol_ppm=inf)),
        step_zero=dict(params=params(step=0.0)), step_negative=dict(params=params(step=-1.0)), step_nan=dict(params=params(step=nan)),
        step_inf=dict(params=params(step=inf)), below_5=dict(params=params(below=5)), isotopes_16=dict(params=params(isotopes=16)),
        seventeen=dict(params=params(below=4, isotopes=12)), wrapped=dict(params=params(isotopes=0xFFFFFFFF)),
        reserved_0=dict(params=params(reserved=0)), reserved_1=dict(params=params(reserved=1)),
    )
    for name, change in bad.items():
        assert call.run(**change) == _lib.PYA_ERR_ARG, name
        assert b"pya_purity_spectra" in lib.pya_last_error(h), (name, lib.pya_last_error(h))
    assert call.untouched()                                                  # nothing was launched, nothing was written
    # n_query == 0 is PYA_OK with nothing launched, whatever else is NULL
    null = C.byref(_lib.TypedSpectra(None, None, 0, 0))
    assert call.run(n_query=0, t_in=null, off=None, survey=None, pm=None, pz=None, wl=None, wh=None, purity=None, over=None, n_peaks=0) == 0
    assert call.run(n_query=0) == 0 and call.untouched()
    assert call.run(params=params(below=4, isotopes=11)) == 0                # 16 centres are allowed
    first = call.check()[0]
    # (the same checks in front of the host form)
    rec, over = np.zeros(6, ru.PURITY_DTYPE), np.zeros(2, np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)                              # noqa: E731
    h_in = _lib.TypedSpectra(vp(mz), vp(it), 0, 0)
    host = lambda **kw: lib.pya_purity_spectra_host(h, kw.get("t_in", C.byref(h_in)), vp(kw.get("off", off)), off.size - 1,   # noqa: E731
                                                    kw.get("survey", vp(q[0])), vp(q[1]), vp(q[2]), vp(q[3]), vp(q[4]), 6,
                                                    kw.get("params", params()), vp(rec), vp(over))
    for name, kw in dict(types=dict(t_in=typed(vp(mz), vp(it), _lib.PYA_F32, _lib.PYA_F64)), params=dict(params=params(below=5)),
                         descending=dict(off=off[::-1].copy()), negative=dict(off=off - 1), null_survey=dict(survey=None)).items():
        assert host(**kw) == _lib.PYA_ERR_ARG, name
        assert b"pya_purity_spectra_host" in lib.pya_last_error(h), name
    assert not rec.tobytes().strip(b"\0")
    want, _ = ru.purity(mz, it, off, *q, pc.P_BASE)
    assert host() == 0 and rec.tobytes() == want.tobytes() and over.tolist() == [0, 0]
    assert first.tobytes() == ru.purity(mz, it, off, *q, pc.P_16)[0].tobytes()


@pytest.mark.parametrize("types", sorted(TYPES))
def test_the_host_form_and_the_torch_form_equal_the_device_form(types):
    import torch
    from pyascore_amd import device
    mz_t, it_t = TYPES[types]
    gpu = _any_gpu()
    params = ru.purity_params(tol=0.005, tol_ppm=20.0, isotopes=3, below=1, step=1.0)
    spectra, q = pc.random_inputs(3, n_survey=20, n_query=300)
    spectra[4] = pc.boundary_spectra(seed=3)[0][9]                           # one long scan among them
    mz, it, off = pc.pack(spectra, mz_t, it_t)
    want, w_over = ru.purity(mz, it, off, *q, params)
    got = _equals_restatement(mz, it, off, q, params, types)
    h_rec, h_over = gpu.precursor_purity(mz, it, off, *q, params)
    assert h_rec.dtype == ru.PURITY_DTYPE and h_rec.shape == (300,) and h_over == w_over and w_over[0] > 0
    assert h_rec.tobytes() == want.tobytes() == got.tobytes() and (h_rec["flags"] == 3).any()
    dev = torch.device("cuda", gpu.device)
    d_mz, d_it = torch.from_numpy(mz).to(dev), torch.from_numpy(it).to(dev)
    for peak_off, queries in ((off, q), (torch.from_numpy(off).to(dev), tuple(torch.from_numpy(a).to(dev) for a in q))):
        d_rec, d_over = device.purity(gpu, d_mz, d_it, peak_off, *queries, params)
        assert d_rec.dtype == torch.uint8 and tuple(d_rec.shape) == (300, 48)
        assert device.purity_records(d_rec.cpu().numpy()).tobytes() == want.tobytes()
        assert d_over.cpu().numpy().view(np.uint32).tolist() == [w_over[0], 0xFFFFFFFF - w_over[1]]
        again = device.purity(gpu, d_mz, d_it, peak_off, *queries, params, out=d_rec.zero_())
        assert again[0] is d_rec and device.purity_records(d_rec.cpu().numpy()).tobytes() == want.tobytes()
    assert d_mz.cpu().numpy().tobytes() == mz.tobytes() and d_it.cpu().numpy().tobytes() == it.tobytes()      # read-only (NaNs among them)
    for bad in (dict(params=dict(params, tol=-1.0)), dict(params=params, out=d_rec[:-1]), dict(params=params, survey=q[0][:-1]),
                dict(params=params, survey=q[0].astype(np.float64))):
        sv = bad.pop("survey", q[0])
        with pytest.raises(ValueError):
            device.purity(gpu, d_mz, d_it, off, torch.from_numpy(sv).to(dev), *q[1:], **bad)
    if types == "f32/f32":                                                   # float32 m/z beside float64 intensities is widened by the host form
        w = gpu.precursor_purity(mz, it.astype(np.float64), off, *q, params)
        assert w[0].tobytes() == want.tobytes()
    # survey scans without any peak are still a call; no query at all is none
    r, o = gpu.precursor_purity(mz[:0], it[:0], [0, 0], [0, 1], [500.0, 500.0], [2, 2], [499.0, 499.0], [501.0, 501.0], params)
    assert r["flags"].tolist() == [1, 0] and o == (1, 1)
    r, o = gpu.precursor_purity(mz, it, off, [], [], np.zeros(0, np.int32), [], [], params)
    assert r.shape == (0,) and o == (0, None)


# ---- the gate ----

def _gate_records(n_rows, seed):
    """records with known and unknown rows, an exact-threshold row and its lower neighbour among them"""
    rng = np.random.default_rng(seed)
    rec = np.zeros(n_rows, ru.PURITY_DTYPE)
    rec["window"] = rng.choice([0.0, 2048.0, 1000.0, 3.0], size=n_rows)
    rec["precursor"] = rec["window"] * rng.choice([0.0, 0.25, 0.75, 1.0], size=n_rows)
    rec["flags"] = rng.choice([0, 1, 3], size=n_rows)
    if n_rows > 2:
        rec[1] = (2048.0, 1536.0, 0.0, 0.0, 2, 1, 1, 3)                      # precursor == 0.75 * window exactly
        rec[2] = (2048.0, pc.down(1536.0), 0.0, 0.0, 2, 1, 1, 3)             # one ulp below
    return rec


@pytest.mark.parametrize("n_ch", [1, 2, 18, 63, 64])
def test_gate_equals_the_restatement(n_ch):
    import torch
    from pyascore_amd import device
    gpu = _any_gpu()
    dev = torch.device("cuda", gpu.device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)         # noqa: E731
    for n_rows in (0, 1, 63, 64, 65, 257):
        rec = _gate_records(n_rows, 100 * n_ch + n_rows)
        rng = np.random.default_rng(n_rows)
        v = rng.choice([1.5, 0.0, -0.0, np.nan, 1e300, -7.0, 1234.5], size=(n_rows, n_ch))
        if n_rows:
            v.view(np.uint64)[0, 0] = 0x7FF0000000000123                     # (a NaN with a payload: a passing row's bits are copied)
        d_rec, d_v = up(rec.view(np.uint8).reshape(n_rows, 48)), up(v)
        for keep in (True, False):
            what = "%d rows, %d channels, keep_unknown=%s" % (n_rows, n_ch, keep)
            w_select, w_out = ru.purity_gate(rec, 0.75, keep, v)
            # out of place, between guard rows; select between guard bytes
            room = torch.empty((n_rows + 2, n_ch), dtype=torch.float64, device=dev)
            room.view(torch.uint8).fill_(0x5A)
            sel = torch.full((n_rows + 2 * GUARD,), 0x5A, dtype=torch.uint8, device=dev)
            out, select = device.purity_gate(gpu, d_rec, 0.75, keep, d_v, out=room[1:n_rows + 1], select=sel[GUARD:GUARD + n_rows])
            host, h_sel = room.cpu().numpy(), sel.cpu().numpy()
            assert host[1:n_rows + 1].tobytes() == w_out.tobytes() and h_sel[GUARD:GUARD + n_rows].tolist() == w_select.tolist(), what
            assert (host[[0, -1]].view(np.uint8) == 0x5A).all() and (h_sel[:GUARD] == 0x5A).all() and (h_sel[GUARD + n_rows:] == 0x5A).all(), what
            assert d_v.cpu().numpy().tobytes() == v.tobytes() and d_rec.cpu().numpy().tobytes() == rec.tobytes()    # only read
            # exactly in place, without select; select alone
            d_w = d_v.clone()
            assert device.purity_gate(gpu, d_rec, 0.75, keep, d_w, out=d_w)[0] is d_w and d_w.cpu().numpy().tobytes() == w_out.tobytes(), what
            none, only = device.purity_gate(gpu, d_rec, 0.75, keep, select=True)
            assert none is None and only.cpu().numpy().tolist() == w_select.tolist(), what
        if n_rows > 2:
            assert w_select[1] == 1 and w_select[2] == 0                     # the exact-threshold row passes, its lower neighbour fails
            assert w_out.view(np.uint64)[2].tolist() == [NO_READING] * n_ch
    h_select, h_out = gpu.purity_gate(rec, 0.75, True, v)                    # the host-array form, on the last shape
    w = ru.purity_gate(rec, 0.75, True, v)
    assert h_select.tobytes() == w[0].tobytes() and h_out.tobytes() == w[1].tobytes()


def test_gate_refusals_leave_the_output_untouched():
    import torch
    gpu = _any_gpu()
    lib, h = gpu._lib, gpu._h
    dev = torch.device("cuda", gpu.device)
    rec = _gate_records(65, 1)
    d_rec = torch.from_numpy(rec.view(np.uint8).reshape(65, 48).copy()).to(dev)
    d_v = torch.ones((65, 3), dtype=torch.float64, device=dev)
    out = torch.empty((66, 3), dtype=torch.float64, device=dev)
    out.view(torch.uint8).fill_(0x5A)
    sel = torch.full((65 + GUARD,), 0x5A, dtype=torch.uint8, device=dev)
    base = dict(rec=d_rec.data_ptr(), n=65, t=0.5, keep=1, v=d_v.data_ptr(), c=3, out=out.data_ptr(), sel=sel.data_ptr())
    call = lambda **kw: (lambda a: lib.pya_purity_gate(h, a["rec"], a["n"], a["t"], a["keep"], a["v"], a["c"], a["out"], a["sel"], None))(   # noqa: E731
        dict(base, **kw))
    nan = float("nan")
    for name, kw in dict(null_records=dict(rec=None), null_values=dict(v=None), null_out=dict(out=None), channels_65=dict(c=65),
                         too_many=dict(n=0xFFFFFFFF), below_0=dict(t=-0.01), above_1=dict(t=1.01), t_nan=dict(t=nan), keep_2=dict(keep=2),
                         nothing_wanted=dict(c=0, sel=None), misaligned_records=dict(rec=d_rec.data_ptr() + 4),
                         misaligned_values=dict(v=d_v.data_ptr() + 4), misaligned_out=dict(out=out.data_ptr() + 4)).items():
        assert call(**kw) == _lib.PYA_ERR_ARG, name
        assert b"pya_purity_gate" in lib.pya_last_error(h), name
    torch.cuda.synchronize(dev)
    assert (out.view(torch.uint8).cpu().numpy() == 0x5A).all() and (sel.cpu().numpy() == 0x5A).all()
    assert call(n=0, rec=None, v=None, out=None, sel=None) == 0              # no rows: nothing launched
    assert call(c=0, v=None, out=None) == 0                                  # no channels: select alone
    torch.cuda.synchronize(dev)
    assert sel.cpu().numpy()[:65].tolist() == ru.purity_gate(rec, 0.5, True)[0].tolist() and (sel.cpu().numpy()[65:] == 0x5A).all()
    assert (out.view(torch.uint8).cpu().numpy() == 0x5A).all()


# ---- end to end ----

def _planted(n=120):
    """n cfg2 PSMs with ten planted reporters (the marker tests' planting), the peptides of the first third repeated so that PSMs
    share slots, and one survey scan per four spectra: an isotope envelope 4 : 2 : 1 at every precursor (charge 2, step 1.0)
    and, for every second spectrum, an interferer of four times the envelope a quarter m/z above the precursor"""
    if "planted" not in _cache:
        from pyascore_amd import PyAscore
        base, settings = synth.make_batch("cfg2", n_psm=n, seed=9740)
        tol = 0.05
        planted, pm, pz, _ = mc.with_markers(base, tol)
        kws = [synth.unpack_psm(planted, i) for i in range(n)]
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
        peptides = [q["peptide"] for q in psms]
        slot, n_slots, _ = ru.peptide_slots(peptides, off, residues=settings["mod_group"])
        rng = np.random.default_rng(8)
        scans = []
        for s in range(0, n, 4):
            x, y = [rng.uniform(300.0, 1800.0, size=400)], [rng.uniform(1.0, 100.0, size=400)]
            for i in range(s, s + 4):
                unit = float(2 ** int(rng.integers(8, 12)))
                x.append([pm[i], pm[i] + 0.5, pm[i] + 1.0] + ([pm[i] + 0.25] if i % 2 else []))
                y.append([4.0 * unit, 2.0 * unit, unit] + ([28.0 * unit] if i % 2 else []))
            x, y = np.concatenate(x), np.concatenate(y)
            order = np.argsort(x, kind="stable")
            scans.append((x[order], y[order]))
        ms1_mz, ms1_it, ms1_off = pc.pack(scans, np.float64, np.float32)
        rule = dict(tol=0.01, tol_ppm=5.0, isotopes=2, below=0, step=1.0)
        queries = (np.arange(n, dtype=np.int64) // 4, pm.copy(), pz.copy(), pm - 0.75, pm + 1.25)
        spill = ru.channel_spill(10, [(c, t, float(rng.uniform(0.01, 0.08))) for c in range(10) for t in (c - 1, c + 1) if 0 <= t < 10])
        records, _ = ru.purity(ms1_mz, ms1_it, ms1_off, *queries, ru.purity_params(**rule))
        ratio = ru.purity_ratio(records)
        assert (ratio[0::2] > 0.6).mean() > 0.8 and (ratio[1::2] < 0.4).all()   # (a background peak in a window now and then)
        _cache["planted"] = dict(gpu=gpu, settings=settings, batch=batch, plain=plain, thr=thr, slot=slot, n_slots=n_slots, peptides=peptides,
                                 tol=tol, pm=pm, pz=pz, matrix=ru.channel_matrix(spill), ms1=(ms1_mz, ms1_it, ms1_off), queries=queries,
                                 rule=rule, records=records)
    return _cache["planted"]


def test_resident_chain_equals_the_restatement_chain():
    """marker records -> channel matrix -> purity -> gate -> impurity matrix -> sums over the passing rows -> factors -> factor ->
    site table, nothing read in between"""
    import torch
    from pyascore_amd import device
    from pyascore_amd.device import DevicePlan, channel_sum_records, site_quant_records
    c = _planted()
    gpu, batch, plain = c["gpu"], c["batch"], c["plain"]
    dev = torch.device("cuda", gpu.device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)         # noqa: E731
    params, rule = mc.planted_params(c["tol"]), ru.purity_params(**c["rule"])
    d_mz, d_it = up(batch["mz"]), up(batch["intensity"])
    d_ms1 = [up(a) for a in c["ms1"]]
    d_q = [up(a) for a in c["queries"]]
    d_slot, d_matrix = up(c["slot"]), up(c["matrix"])
    plan = DevicePlan(gpu, batch, quant=True)
    plan.run(d_mz, d_it)
    _, sp, pp = plan.probs()
    p = ru.site_quant_params(threshold=c["thr"], scale_log2=SCALE, n_channels=10)
    d_rec, _, _ = device.markers(gpu, d_mz, d_it, batch["peak_off"], params, c["pm"], c["pz"])
    d_values = device.marker_values(gpu, d_rec, 0x3FF)
    d_purity, d_over = device.purity(gpu, *d_ms1, *d_q, rule)
    _, d_select = device.purity_gate(gpu, d_purity, 0.5, True, d_values, out=d_values, select=True)
    device.correct_channels(gpu, d_values, matrix=d_matrix, out=d_values)
    d_cell = device.channel_sums(gpu, d_values, d_select, SCALE)
    d_factor = device.channel_factors(gpu, d_cell)
    device.correct_channels(gpu, d_values, factor=d_factor, out=d_values)
    table = plan.site_quant(sp, pp, d_slot, d_values, p, n_slots=c["n_slots"])
    plan.check()
    # the restatement of the same chain
    rec, _ = ru.markers(batch["mz"], batch["intensity"], batch["peak_off"], params, c["pm"], c["pz"])
    raw = np.ascontiguousarray(ru.marker_matrix(rec)[:, :10])
    assert device.purity_records(d_purity.cpu().numpy()).tobytes() == c["records"].tobytes() and d_over.cpu().numpy().tolist() == [0, 0]
    select, gated = ru.purity_gate(c["records"], 0.5, True, raw)
    assert 40 <= int(select.sum()) <= 70 and select[1::2].sum() == 0          # the planted interference fails, and about half pass
    assert d_select.cpu().numpy().tobytes() == select.tobytes()
    corrected = ru.correct_channels(gated, matrix=c["matrix"])
    cell = ru.channel_sums(corrected, select, SCALE)
    factors = ru.channel_factors(cell)
    values = ru.correct_channels(corrected, factor=factors)
    assert d_values.cpu().numpy().tobytes() == values.tobytes() and np.isnan(values[select == 0]).all() and not np.isnan(values[select == 1]).any()
    assert channel_sum_records(d_cell.cpu().numpy()).tobytes() == cell.tobytes() and d_factor.cpu().numpy().tobytes() == factors.tobytes()
    got = site_quant_records((table[0].cpu().numpy(), table[1].cpu().numpy()))
    args = (plain["site_probs"], plain["psm_probs"], plain["site_off"], plain["best_sig"], c["slot"], c["n_slots"])
    want = sq_ref.table(*args, values, None, c["thr"], SCALE)
    assert want[0]["n_records"].sum() > 10 and got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    # ... which is, cell for cell, the table over the rows that pass alone (a gated row still counts as a record of its slot)
    passing = sq_ref.table(*args, values, np.where(select != 0, np.arange(select.size), -1), c["thr"], SCALE)
    assert got[1].tobytes() == passing[1].tobytes() and passing[1]["n"].sum() > 0
    assert int(got[0]["n_records"].sum()) > int(passing[0]["n_records"].sum())
    ungated = sq_ref.table(*args, ru.correct_channels(raw, matrix=c["matrix"]), None, c["thr"], SCALE)
    assert ungated[1]["n"].sum() > got[1]["n"].sum()


def _equal_but(got, plain, extra, what):
    for key in plain:
        if key not in extra and key != "status_message":
            g, w = got[key], plain[key]
            assert (g.tobytes() == w.tobytes()) if isinstance(w, np.ndarray) else (g == w), (what, key)
    assert set(got) - set(plain) == set(extra) - set(plain), (what, sorted(set(got) ^ set(plain)))


def test_score_batch_with_purity():
    c = _planted()
    gpu, batch, thr = c["gpu"], c["batch"], c["thr"]
    ms1_mz, ms1_it, ms1_off = c["ms1"]
    sv, pm, pz, wl, wh = c["queries"]
    req = dict(c["rule"], ms1_mz=ms1_mz, ms1_intensity=ms1_it, ms1_peak_off=ms1_off, survey=sv, precursor_mz=pm, precursor_charge=pz,
               window_lo=wl, window_hi=wh)
    marks = dict(mz=mc.REPORTERS, losses=(mc.LOSS_H3PO4,), tol=c["tol"], precursor_mz=c["pm"], precursor_charge=c["pz"])
    roll = dict(slot=c["slot"], n_slots=c["n_slots"])
    group, _, _ = ru.peptide_groups(c["peptides"])
    forms = dict(group=group, threshold=0.75)
    q = dict(values=None, threshold=thr, scale_log2=SCALE)
    ch = dict(matrix=c["matrix"], normalize=True)
    stages = dict(rollup=roll, peptidoforms=forms, markers=marks, quant=dict(q, channels=ch), peptidoform_quant=dict(q, channels=ch), probs=True)
    # without a gate: the records are added and nothing else moves
    without = gpu.score_batch(batch, **stages)
    got = gpu.score_batch(batch, purity=req, **stages)
    _equal_but(got, without, ("purity",), "no gate")
    assert got["purity"].dtype == ru.PURITY_DTYPE and got["purity"].tobytes() == c["records"].tobytes()
    assert gpu.score_batch(batch, purity=req)["purity"].tobytes() == c["records"].tobytes()      # alone, too
    # with a gate: the call on rollup.purity_gate's matrix and select
    gate = dict(threshold=0.5, keep_unknown=True)
    got = gpu.score_batch(batch, purity=dict(req, gate=gate), **stages)
    raw = np.ascontiguousarray(ru.marker_matrix(without["markers"])[:, :10])
    select, gated = ru.purity_gate(c["records"], 0.5, True, raw)
    explicit = dict(q, values=gated, channels=dict(ch, select=select))
    want = gpu.score_batch(batch, rollup=roll, peptidoforms=forms, quant=explicit, peptidoform_quant=explicit, probs=True)
    tables = ("quant_head", "quant", "peptidoform_quant_head", "peptidoform_quant", "quant_channel_sums", "quant_channel_factors",
              "peptidoform_quant_channel_sums", "peptidoform_quant_channel_factors")
    for key in tables:
        assert got[key].tobytes() == want[key].tobytes(), key
    assert got["quant"].tobytes() != without["quant"].tobytes() and got["quant_channel_sums"].tobytes() != without["quant_channel_sums"].tobytes()
    assert got["purity_pass"].dtype == np.uint8 and got["purity_pass"].tobytes() == select.tobytes()
    _equal_but(got, without, tables + ("purity", "purity_pass"), "gate")      # nothing else of the run moves
    # a given matrix, no channels=, keep_unknown=False with a spectrum that has no survey scan
    sv2 = sv.copy()
    sv2[0] = -1
    got = gpu.score_batch(batch, rollup=roll, quant=dict(q, values=raw), purity=dict(req, survey=sv2, gate=dict(threshold=0.5, keep_unknown=False)))
    rec2, _ = ru.purity(ms1_mz, ms1_it, ms1_off, sv2, pm, pz, wl, wh, ru.purity_params(**c["rule"]))
    sel2, gated2 = ru.purity_gate(rec2, 0.5, False, raw)
    want = gpu.score_batch(batch, rollup=roll, quant=dict(q, values=gated2))
    assert sel2[0] == 0 and got["purity_pass"].tobytes() == sel2.tobytes() and got["quant"].tobytes() == want["quant"].tobytes()
    for bad in (dict(req, gate=gate), dict(req, window=1), dict(req, survey=sv[:-1]), dict(req, tol=-1.0), True):
        with pytest.raises(ValueError):
            gpu.score_batch(batch, purity=bad)                               # (the first: a gate without a quant request)
    with pytest.raises(ValueError):
        gpu.score_batch(batch, rollup=roll, quant=dict(q, values=raw[:-1]), purity=dict(req, gate=gate))


# ---- the command line ----

def _ms1_spectrum(index, scan, mz, it):
    arr = lambda a, bits, name: (                                            # noqa: E731
        '<binaryDataArray encodedLength="0"><cvParam cvRef="MS" accession="MS:1000523" name="%d-bit float" value=""/>'
        '<cvParam cvRef="MS" accession="MS:1000576" name="no compression" value=""/><cvParam cvRef="MS" accession="MS:1000514" name="%s" value=""/>'
        "<binary>%s</binary></binaryDataArray>" % (bits, name, base64.b64encode(a.tobytes()).decode()))
    return ('<spectrum index="%d" id="controllerType=0 controllerNumber=1 scan=%d" defaultArrayLength="%d">'
            '<cvParam cvRef="MS" accession="MS:1000579" name="MS1 spectrum" value=""/><cvParam cvRef="MS" accession="MS:1000511" name="ms level" value="1"/>'
            '<cvParam cvRef="MS" accession="MS:1000127" name="centroid spectrum" value=""/><binaryDataArrayList count="2">%s%s</binaryDataArrayList>'
            "</spectrum>\n" % (index, scan, mz.size, arr(mz.astype("<f8"), 64, "m/z array"), arr(it.astype("<f4"), 32, "intensity array")))


def test_command_line_file(tmp_path):
    from pyascore_amd import __main__ as cli, batch_cli, ingest
    data = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ingest")
    spec, ident = os.path.join(data, "test_spectra.mzML"), os.path.join(data, "test_psms.pep.xml")
    ms2 = ingest.SpectraParser(spec, "mzML").to_list()
    first = ms2[0]
    assert first["parent_scan"] == 14754 and first["scan"] == 14760
    # two survey scans: the one the first MS2 scan names, with its precursor's envelope and an interferer, and a later one that
    # no MS2 scan names (the MS2 scans behind it name scans the file does not hold: they get it by order)
    pm, z = first["precursor_mz"], first["precursor_charge"]
    env = pm + ru.STRIP_STEP * np.arange(3) / z
    mz_a = np.concatenate([[400.0], env, [first["isolation"][0] + 0.5, 1200.0]])
    it_a = np.array([9.0, 4096.0, 2048.0, 1024.0, 1024.0, 7.0])
    later = [r for r in ms2 if r["scan"] > 16000]
    # (every later precursor with an equal peak 0.4 above it: inside its window, at no isotope position of charge 2, 3 or 4)
    mz_b = np.sort(np.concatenate([[r["precursor_mz"] for r in later], [r["precursor_mz"] + 0.4 for r in later], [300.0]]))
    it_b = np.full(mz_b.size, 512.0)
    text = open(spec).read()
    at = text.index("<spectrum ")
    inline = tmp_path / "with_ms1.mzML"
    inline.write_text(text[:at] + _ms1_spectrum(0, 14754, mz_a, it_a) + _ms1_spectrum(1, 16000, mz_b, it_b) + text[at:])
    survey = ingest.SpectraParser(str(inline), "mzML", ms_level=1, native_precision=True).to_list()
    assert [r["scan"] for r in survey] == [14754, 16000] and survey[0]["intensity_values"].dtype == np.float32
    out, table = tmp_path / "ascores.tsv", tmp_path / "purity.tsv"
    opts = ["--mz_error", "0.05", "--hit_depth", "2"]
    rows = cli.run(cli.parse_args(opts + ["--purity", str(table), "--purity_tol_ppm", "20", "--purity_isotopes", "2", str(inline), ident, str(out)]),
                   log=lambda *_: None)
    plain = cli.run(cli.parse_args(opts + [spec, ident, str(tmp_path / "plain.tsv")]), log=lambda *_: None)
    assert rows == plain                                                     # the main table is unchanged
    spectra = ingest.SpectraParser(str(inline), "mzML", native_precision=True).to_dict()
    psms = sorted(ingest.IdentificationParser(ident, "pepXML").to_list(), key=lambda p: p["scan"])
    picked, scans = batch_cli.select_psms(psms, spectra, "STY", 79.966331, 2, 5)
    lines = table.read_text().splitlines()
    assert lines[0].split("\t") == batch_cli.PURITY_COLUMNS and len(lines) == 1 + len(picked)
    ms1_mz, ms1_it, ms1_off = pc.pack([(mz_a, it_a), (mz_b, it_b)], np.float64, np.float32)
    params = ru.purity_params(tol_ppm=20.0, isotopes=2)
    seen = set()
    for i, line in enumerate(lines[1:]):
        r = spectra[scans[i]]
        sv = 0 if scans[i] < 16000 else 1
        wl, wh = r["isolation"][0] - r["isolation"][1], r["isolation"][0] + r["isolation"][2]
        rec, _ = ru.purity(ms1_mz, ms1_it, ms1_off, [sv], [r["precursor_mz"]], [r["precursor_charge"]], [wl], [wh], params)
        want = [str(v) for v in [scans[i], [14754, 16000][sv], wl, wh] + batch_cli.purity_fields(rec[0])]
        assert line.split("\t") == want, i
        seen.add((sv, int(rec["flags"][0])))
    first_line = lines[1].split("\t")
    assert first_line[:2] == ["14760", "14754"] and float(first_line[6]) == 7168.0 / 8192.0 and first_line[9] == "111"
    assert float(first_line[10]) == first["isolation"][0] + 0.5 and (1, 3) in seen
    # the gate beside --site_quant: the table changes, and equals the one localize gives for the same request
    # (channels: the base peaks of the first picked spectra, so that each of them has a reading)
    tops = sorted({float(p["mz"][int(np.argmax(p["intensity"]))]) for p in picked[:8]})
    quant = ["--site_table", str(tmp_path / "sites.tsv"), "--marker_mz", ",".join(repr(t) for t in tops)]
    cli.run(cli.parse_args(opts + quant + ["--site_quant", str(tmp_path / "q0.tsv"), str(inline), ident, str(out)]), log=lambda *_: None)
    cli.run(cli.parse_args(opts + quant + ["--site_quant", str(tmp_path / "q1.tsv"), "--purity", str(table), "--purity_tol_ppm", "20",
                                           "--purity_isotopes", "2", "--purity_threshold", "0.9", "--purity_drop_unknown", str(inline), ident, str(out)]),
            log=lambda *_: None)
    assert table.read_text().splitlines() == lines                           # the purity table does not depend on the gate
    q0, q1 = (tmp_path / "q0.tsv").read_text().splitlines(), (tmp_path / "q1.tsv").read_text().splitlines()
    assert q0[0] == q1[0] and len(q0) == len(q1) and q0 != q1
