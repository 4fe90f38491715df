"""Precursor stripping on the GPU (pya_strip_params): pya_strip_spectra against pyascore_amd.rollup.strip, the numpy restatement
of the header's rule that tests/test_strip_host.py pins by hand -- every comparison is on raw bytes --, the bounds of everything
it writes, its refusals, the host form, and score_batch(strip=...) / device.strip against the same calls on arrays the
restatement stripped."""
import ctypes as C

import numpy as np
import pytest

import deisotope_cases as dc
import strip_cases as sc
from oracle import harness
from pyascore_amd import _lib, rollup as ru, synth

pytestmark = pytest.mark.gpu

TYPES = {"f64/f64": (np.float64, np.float64), "f64/f32": (np.float64, np.float32), "f32/f32": (np.float32, np.float32)}
GUARD = 16
_scorers = {}


def _gpu(settings):
    from pyascore_amd import PyAscore
    return harness.make_scorer(PyAscore, settings)


def _any_gpu():
    """a scorer for the calls that do not score (one per process)"""
    if "any" not in _scorers:
        _scorers["any"] = _gpu(synth.describe("cfg2", 1, seed=1)["settings"])
    return _scorers["any"]


class _Call:
    """One pya_strip_spectra call on torch's current stream with canaries around everything it may write: the out arrays are
    pre-filled, guard words stand behind d_new_off, d_report, d_over and the workspace.  ``check()`` waits, looks at the canaries
    and returns (mz, intensity, new_off, report, over) of the host."""

    def __init__(self, mz, it, off, prec_mz, prec_z, work_peaks=None):
        import torch
        self.torch, self.gpu = torch, _any_gpu()
        self.dev = dev = torch.device("cuda", self.gpu.device)
        self.mz, self.it, self.off = mz, it, np.ascontiguousarray(off, np.int64)
        self.n, self.n_spec = mz.size, self.off.size - 1
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)             # noqa: E731
        self.d_mz, self.d_it, self.d_off = to(mz), to(it), to(self.off)
        self.d_pm, self.d_pz = to(np.asarray(prec_mz, np.float64)), to(np.asarray(prec_z, np.int32))
        assert self.d_pm.numel() == self.n_spec and self.d_pz.numel() == self.n_spec
        self.o_mz = to(np.full(self.n + GUARD, -7.0, mz.dtype))
        self.o_it = to(np.full(self.n + GUARD, -7.0, it.dtype))
        self.new_off = to(np.full(self.n_spec + 1 + GUARD, -99, np.int64))
        self.report = to(np.full((self.n_spec + GUARD, 16), 0xA5, np.uint8))
        over = np.full(2 + GUARD, 0x5A5A, np.int32)
        over[:2] = 0
        self.over = to(over)
        self.work_bytes = int(self.gpu._lib.pya_strip_workspace_bytes(self.n_spec, self.n if work_peaks is None else work_peaks))
        assert self.work_bytes % 8 == 0 and self.work_bytes >= 8
        self.work = to(np.full(self.work_bytes // 8 + GUARD, 0x1234567, np.int64))
        self.t_in = _lib.TypedSpectra(self.d_mz.data_ptr(), self.d_it.data_ptr(), _lib.spectrum_type(mz.dtype), _lib.spectrum_type(it.dtype))
        self.t_out = _lib.TypedSpectra(self.o_mz.data_ptr(), self.o_it.data_ptr(), self.t_in.mz_type, self.t_in.intensity_type)

    def run(self, rule, **change):
        a = dict(t_in=C.byref(self.t_in), off=self.d_off.data_ptr(), n_spec=self.n_spec, pm=self.d_pm.data_ptr(), pz=self.d_pz.data_ptr(),
                 params=C.byref(ru.strip_c_params(rule)), work=self.work.data_ptr(), work_bytes=self.work_bytes, t_out=C.byref(self.t_out),
                 new_off=self.new_off.data_ptr(), report=self.report.data_ptr(), over=self.over.data_ptr())
        a.update(change)
        stream = self.torch.cuda.current_stream(self.dev).cuda_stream
        return self.gpu._lib.pya_strip_spectra(self.gpu._h, a["t_in"], a["off"], a["n_spec"], a["pm"], a["pz"], a["params"], stream, a["work"],
                                               a["work_bytes"], a["t_out"], a["new_off"], a["report"], a["over"])

    def host(self):
        self.torch.cuda.synchronize(self.dev)
        return [t.cpu().numpy() for t in (self.o_mz, self.o_it, self.new_off, self.report, self.over, self.work)]

    def untouched(self):
        o_mz, o_it, new_off, report, over, work = self.host()
        return (o_mz == -7.0).all() and (o_it == -7.0).all() and (new_off == -99).all() and (report == 0xA5).all() and \
            over.tolist() == [0, 0] + [0x5A5A] * GUARD and (work == 0x1234567).all()

    def check(self, report_written=True):
        o_mz, o_it, new_off, report, over, work = self.host()
        assert (new_off[self.n_spec + 1:] == -99).all(), "guard behind d_new_off"
        assert (report[self.n_spec if report_written else 0:] == 0xA5).all(), "guard behind d_report"
        assert over[2:].tolist() == [0x5A5A] * GUARD, "guard behind d_over"
        assert (work[self.work_bytes // 8:] == 0x1234567).all(), "guard behind the workspace"
        kept = int(new_off[self.n_spec])
        assert 0 <= kept <= self.n
        assert (o_mz[kept:] == -7.0).all() and (o_it[kept:] == -7.0).all(), "out elements from new_off[n] on"
        assert self.d_mz.cpu().numpy().tobytes() == self.mz.tobytes() and self.d_it.cpu().numpy().tobytes() == self.it.tobytes()
        rep = np.ascontiguousarray(report[:self.n_spec]).view(ru.STRIP_REPORT_DTYPE).reshape(-1)
        return o_mz[:kept], o_it[:kept], new_off[:self.n_spec + 1], rep, over[:2].view(np.uint32)


def _equals_restatement(mz, it, off, prec_mz, prec_z, params, what):
    call = _Call(mz, it, off, prec_mz, prec_z)
    assert call.run(params) == 0, call.gpu._lib.pya_last_error(call.gpu._h)
    g_mz, g_it, g_off, g_rep, g_over = call.check()
    w_mz, w_it, w_off, w_rep = ru.strip(mz, it, off, prec_mz, prec_z, params)
    assert g_off.tobytes() == w_off.tobytes(), what
    assert g_mz.dtype == mz.dtype and g_mz.tobytes() == w_mz.tobytes(), what
    assert g_it.dtype == it.dtype and g_it.tobytes() == w_it.tobytes(), what
    assert g_rep.tobytes() == w_rep.tobytes(), what
    assert g_over.tolist() == [0, 0], what
    return g_mz, g_rep


# ---- the kernels against the restatement ----

@pytest.mark.parametrize("types", sorted(TYPES))
def test_stride_and_ballot_boundaries(types):
    """spectra of 0, 1, 2, 63, 64, 65, 127, 128, 129 and 4 097 peaks in one call, peaks inside a window as the first and the last
    peak and on both sides of every 64-peak boundary, two spectra removed entirely"""
    mz_t, it_t = TYPES[types]
    spectra, planted = sc.boundary_spectra()
    mz, it, off = sc.pack(spectra, mz_t, it_t, gaps=False)
    n = len(spectra)
    assert np.diff(off).tolist() == list(sc.BOUNDARY_LENGTHS)
    g_mz, rep = _equals_restatement(mz, it, off, np.full(n, sc.BOUNDARY_PREC[0]), np.full(n, sc.BOUNDARY_PREC[1], np.int32), sc.P_BASE, types)
    # (the planted values are sums of powers of two, exact in float32 too: the device kept what was not planted)
    assert g_mz.tobytes() == mz[~np.concatenate(planted)].tobytes()
    assert rep["n_removed"].tolist() == [int(m.sum()) for m in planted]
    assert int(rep["n_removed"][9]) == 64 + 65                             # of 4 097: peaks 63, 127, .. 4 095 and 0, 64, .. 4 096


@pytest.mark.parametrize("types", sorted(TYPES))
def test_hand_made_spectra(types):
    """every case of tests/strip_cases.py, the cases of one parameter set in one call with empty spectra between them"""
    mz_t, it_t = TYPES[types]
    groups = {}
    for c in sc.hand_cases():
        groups.setdefault(sc.params_key(c["params"]), []).append(c)
    assert len(groups) >= 10
    for group in groups.values():
        mz, it, off, pm, pz = sc.pack_cases(group, mz_t, it_t, gaps=True)
        g_mz, rep = _equals_restatement(mz, it, off, pm, pz, group[0]["params"], (types, group[0]["name"]))
        if mz_t == np.float64:                                             # (the float32 cases hold the same values widened)
            assert g_mz.tobytes() == mz[np.concatenate([c["keep"] for c in group])].tobytes()
            assert rep["hit"][0::2].tolist() == [c["hit"] for c in group]
            assert rep["n_windows"][0::2].tolist() == [c["n_windows"] for c in group]
            assert rep["n_removed"][0::2].tolist() == [int((~c["keep"]).sum()) for c in group]


def _tiny_spectra(n_spec, seed=21):
    """many spectra of 0 .. 8 peaks around precursors of every charge from -1 to 9, a third of the peaks inside a window"""
    rng = np.random.default_rng(seed)
    p = ru.strip_params(0.02, losses=(sc.LOSS_H3PO4, sc.LOSS_WATER, 17.026549, 79.966331, 115.987461, 36.02113, 43.989829), reduced=True,
                        isotopes=1, mz_lo=120.0, mz_hi=1900.0)
    pz = rng.integers(-1, 10, n_spec).astype(np.int32)
    pm = rng.uniform(300.0, 900.0, n_spec)
    pm[rng.random(n_spec) < 0.02] = np.nan
    lo, hi, active = ru.strip_windows(pm, pz, p)
    spectra = []
    for s, n in enumerate(rng.integers(0, 9, n_spec)):
        x = rng.uniform(100.0, 2000.0, size=n)
        ws = np.flatnonzero(active[s])
        if ws.size:
            hitting = rng.random(n) < 0.33
            w = rng.choice(ws, size=n)
            x = np.where(hitting, lo[s, w] + rng.random(n) * (hi[s, w] - lo[s, w]), x)
        spectra.append((x, rng.choice([1.0, 2.0, 3.0], size=n)))
    return spectra, pm, pz, p


def test_more_spectra_than_wavefronts_and_scan_tiles():
    """9 000 small spectra: the grid strides over them (8 192 wavefronts) and the offset scan has 9 tiles"""
    spectra, pm, pz, p = _tiny_spectra(9_000)
    mz, it, off = sc.pack(spectra, np.float64, np.float32, gaps=False)
    g_mz, rep = _equals_restatement(mz, it, off, pm, pz, p, "9 000 spectra")
    assert 0.15 < 1.0 - g_mz.size / mz.size < 0.6 and (rep["hit"] != 0).sum() > 1000 and (rep["hit"] >> np.uint64(32)).any()
    assert set(rep["n_windows"].tolist()) == {0, 8, 16, 24, 32, 40, 48, 56, 64}


def test_a_workspace_for_fewer_peaks_clips_instead_of_writing_past_it():
    """the peak count is on the device: the host cannot refuse, the kernels clip to the peaks the workspace has bits for and
    report the spectra that reach beyond them; no canary is touched"""
    spectra, _ = sc.boundary_spectra()
    mz, it, off = sc.pack(spectra, gaps=False)
    n = len(spectra)
    pm, pz = np.full(n, sc.BOUNDARY_PREC[0]), np.full(n, sc.BOUNDARY_PREC[1], np.int32)
    call = _Call(mz, it, off, pm, pz, work_peaks=256)
    assert call.run(sc.P_BASE) == 0
    g_mz, g_it, g_off, rep, over = call.check()
    cap = 256 + 63                                                        # (the bits of the last word count)
    inside = int(np.searchsorted(off, cap, "right")) - 1                  # spectra that end at or before the cap
    assert inside >= 6
    w_mz, _, w_off, w_rep = ru.strip(mz, it, off[:inside + 1], pm[:inside], pz[:inside], sc.P_BASE)
    assert g_off[:inside + 1].tolist() == w_off.tolist() and g_mz[:int(w_off[-1])].tobytes() == w_mz.tobytes()
    assert rep[:inside].tobytes() == w_rep.tobytes()
    assert over[0] >= 1 and 0xFFFFFFFF - int(over[1]) == inside


def test_refusals_launch_nothing():
    spectra, _ = sc.boundary_spectra()
    mz, it, off = sc.pack(spectra[:6], gaps=False)
    pm, pz = np.full(6, 400.0), np.full(6, 2, np.int32)
    call = _Call(mz, it, off, pm, pz)
    lib, h = call.gpu._lib, call.gpu._h
    f32 = _Call(mz.astype(np.float32), it.astype(np.float32), off, pm, pz)
    ok = sc.P_BASE

    def params(**kw):
        p = ru.strip_c_params(ok)
        for k, v in kw.items():
            if k == "loss":
                for i, s in enumerate(v):
                    p.loss[i] = s
            else:
                setattr(p, k, v)
        return C.byref(p)

    def typed(mz_ptr, it_ptr, mz_type, it_type):
        return C.byref(_lib.TypedSpectra(mz_ptr, it_ptr, mz_type, it_type))

    i, o = call.t_in, call.t_out
    nan, inf = float("nan"), float("inf")
    bad = dict(
        null_in=dict(t_in=None), null_out=dict(t_out=None), null_off=dict(off=None), null_new_off=dict(new_off=None), null_over=dict(over=None),
        null_work=dict(work=None), null_params=dict(params=None), null_prec_mz=dict(pm=None), null_prec_z=dict(pz=None),
        null_mz=dict(t_in=typed(None, i.intensity, i.mz_type, i.intensity_type)), null_out_it=dict(t_out=typed(o.mz, None, o.mz_type, o.intensity_type)),
        in_place_mz=dict(t_out=typed(i.mz, o.intensity, o.mz_type, o.intensity_type)),
        in_place_it=dict(t_out=typed(o.mz, i.intensity, o.mz_type, o.intensity_type)),
        unknown_type=dict(t_in=typed(i.mz, i.intensity, 2, 0), t_out=typed(o.mz, o.intensity, 2, 0)),
        unknown_it_type=dict(t_in=typed(i.mz, i.intensity, 0, 7), t_out=typed(o.mz, o.intensity, 0, 7)),
        mismatched_types=dict(t_out=typed(o.mz, o.intensity, _lib.PYA_F64, _lib.PYA_F32)),
        f32_mz_f64_it=dict(t_in=typed(i.mz, i.intensity, _lib.PYA_F32, _lib.PYA_F64), t_out=typed(o.mz, o.intensity, _lib.PYA_F32, _lib.PYA_F64)),
        small_work=dict(work_bytes=int(lib.pya_strip_workspace_bytes(call.n_spec, 0)) - 8), no_work=dict(work_bytes=0),
        misaligned_work=dict(work=call.work.data_ptr() + 4), misaligned_report=dict(report=call.report.data_ptr() + 4),
        too_many=dict(n_spec=0xFFFFFFFF),
        tol_negative=dict(params=params(tol=-0.01)), tol_nan=dict(params=params(tol=nan)), tol_inf=dict(params=params(tol=inf)),
        step_zero=dict(params=params(step=0.0)), step_negative=dict(params=params(step=-1.0)), step_nan=dict(params=params(step=nan)),
        step_inf=dict(params=params(step=inf)), lo_nan=dict(params=params(mz_lo=nan)), hi_nan=dict(params=params(mz_hi=nan)),
        lo_above_hi=dict(params=params(mz_lo=500.0, mz_hi=499.0)), n_loss_8=dict(params=params(n_loss=8)),
        loss0_not_0=dict(params=params(loss=[1.0])), loss_negative=dict(params=params(loss=[0.0, -1.0])),
        loss_nan=dict(params=params(loss=[0.0, nan])), loss_inf=dict(params=params(loss=[0.0, inf])), reduced_2=dict(params=params(reduced=2)),
        isotopes_5=dict(params=params(isotopes=5)), reserved=dict(params=params(reserved=1)),
    )
    for name, change in bad.items():
        assert call.run(ok, **change) == _lib.PYA_ERR_ARG, name
        assert b"pya_strip_spectra" in lib.pya_last_error(h), (name, lib.pya_last_error(h))
    assert call.untouched()                                               # nothing was launched, nothing was written
    # (a loss above n_loss is not read, whatever it holds)
    assert call.run(ok, params=params(loss=[0.0, 32.0, nan])) == 0
    first = call.check()
    # (the same checks in front of the float32 instantiation and of the host form)
    assert f32.run(ok, work_bytes=0) == _lib.PYA_ERR_ARG and f32.untouched()
    out_mz, out_it, new_off, over = np.zeros_like(mz), np.zeros_like(it), np.zeros(off.size, np.int64), np.zeros(2, np.uint32)
    rep = np.zeros(off.size - 1, ru.STRIP_REPORT_DTYPE)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)                           # noqa: E731
    h_in = _lib.TypedSpectra(vp(mz), vp(it), 0, 0)
    h_out = _lib.TypedSpectra(vp(out_mz), vp(out_it), 0, 0)
    host = lambda **kw: lib.pya_strip_spectra_host(h, kw.get("t_in", C.byref(h_in)), vp(kw.get("off", off)), off.size - 1,   # noqa: E731
                                                   kw.get("pm", vp(pm)), vp(pz), kw.get("params", params()), kw.get("t_out", C.byref(h_out)),
                                                   vp(new_off), vp(rep), vp(over))
    for name, kw in dict(in_place=dict(t_out=C.byref(h_in)), params=dict(params=params(isotopes=9)), descending=dict(off=off[::-1].copy()),
                         negative=dict(off=off - 1), null_prec=dict(pm=None)).items():
        assert host(**kw) == _lib.PYA_ERR_ARG, name
        assert b"pya_strip_spectra_host" in lib.pya_last_error(h), name
    assert not out_mz.any() and not new_off.any() and not rep["n_windows"].any()
    want = ru.strip(mz, it, off, pm, pz, ok)
    assert host() == 0 and new_off.tolist() == want[2].tolist() and rep.tobytes() == want[3].tobytes()
    # a good call still works on the same buffers
    assert call.run(ok) == 0
    again = call.check()
    assert again[2].tolist() == new_off.tolist() and again[3].tobytes() == first[3].tobytes() == rep.tobytes()


def test_no_spectra_is_a_no_op_that_writes_the_first_offset():
    e = np.zeros(0)
    call = _Call(e, e, np.zeros(1, np.int64), e, np.zeros(0, np.int32))
    null = C.byref(_lib.TypedSpectra(None, None, 0, 0))
    assert call.run(sc.P_BASE, t_in=null, t_out=null, work=None, work_bytes=0, over=None, off=None, pm=None, pz=None, report=None) == 0
    _, _, new_off, _, over = call.check(report_written=False)
    assert new_off.tolist() == [0] and over.tolist() == [0, 0]
    assert _any_gpu()._lib.pya_strip_workspace_bytes(0, 0) == 8


def test_a_null_report_writes_no_report():
    spectra, _ = sc.boundary_spectra()
    mz, it, off = sc.pack(spectra, np.float64, np.float32, gaps=False)
    n = len(spectra)
    pm, pz = np.full(n, 400.0), np.full(n, 2, np.int32)
    call = _Call(mz, it, off, pm, pz)
    assert call.run(sc.P_BASE, report=None) == 0
    g_mz, g_it, g_off, _, over = call.check(report_written=False)
    want = ru.strip(mz, it, off, pm, pz, sc.P_BASE)
    assert g_mz.tobytes() == want[0].tobytes() and g_it.tobytes() == want[1].tobytes() and g_off.tobytes() == want[2].tobytes()


@pytest.mark.parametrize("types", sorted(TYPES))
def test_the_host_form_and_the_torch_form_equal_the_device_form(types):
    import torch
    from pyascore_amd import device
    mz_t, it_t = TYPES[types]
    gpu = _any_gpu()
    spectra, pm, pz, p = _tiny_spectra(300, seed=3)
    spectra[4] = sc.boundary_spectra(seed=3)[0][9]                         # one long spectrum among them
    pm[4], pz[4] = sc.BOUNDARY_PREC
    mz, it, off = sc.pack(spectra, mz_t, it_t, gaps=False)
    want = ru.strip(mz, it, off, pm, pz, p)
    h_mz, h_it, h_off, h_rep, h_over = gpu.strip_spectra(mz, it, off, pm, pz, p)
    assert h_mz.dtype == mz_t and h_it.dtype == it_t and h_over == (0, None) and h_rep.dtype == ru.STRIP_REPORT_DTYPE
    assert h_mz.tobytes() == want[0].tobytes() and h_it.tobytes() == want[1].tobytes() and h_off.tobytes() == want[2].tobytes()
    assert h_rep.tobytes() == want[3].tobytes() and (h_rep["hit"] != 0).any()
    dev = torch.device("cuda", gpu.device)
    d_mz, d_it = torch.from_numpy(mz).to(dev), torch.from_numpy(it).to(dev)
    for peak_off, prec in ((off, (pm, pz)), (torch.from_numpy(off).to(dev), (torch.from_numpy(pm).to(dev), torch.from_numpy(pz).to(dev)))):
        for with_report in (True, False):
            o_mz, o_it, d_new, d_rep, d_over = device.strip(gpu, d_mz, d_it, peak_off, prec[0], prec[1], p, report=with_report)
            new = d_new.cpu().numpy()
            kept = int(new[-1])
            assert new.tobytes() == want[2].tobytes() and d_over.cpu().numpy().tolist() == [0, 0]
            assert o_mz.dtype == d_mz.dtype and o_mz.cpu().numpy()[:kept].tobytes() == want[0].tobytes()
            assert o_it.dtype == d_it.dtype and o_it.cpu().numpy()[:kept].tobytes() == want[1].tobytes()
            assert (d_rep is None) if not with_report else d_rep.cpu().numpy().tobytes() == want[3].tobytes()
    with pytest.raises(ValueError):
        device.strip(gpu, d_mz, d_it, off, pm, pz, p, out=(d_mz, d_it))    # not in place
    with pytest.raises(ValueError):
        device.strip(gpu, d_mz, d_it, off, pm, pz, dict(p, tol=-1.0))
    with pytest.raises(ValueError):
        device.strip(gpu, d_mz, d_it, off, pm[:-1], pz[:-1], p)
    # float32 m/z beside float64 intensities is widened by the host form, as score_batch does
    if types == "f32/f32":
        w = gpu.strip_spectra(mz, it.astype(np.float64), off, pm, pz, p)
        assert w[0].dtype == np.float64 and w[2].tobytes() == want[2].tobytes()
    # spectra without any peak still have windows
    r = gpu.strip_spectra(mz[:0], it[:0], [0, 0, 0], [400.0, 0.0], [2, 0], sc.P_BASE)
    assert r[2].tolist() == [0, 0, 0] and r[3]["n_windows"].tolist() == [2, 0]
    assert gpu.strip_spectra(mz[:0], it[:0], [0], [], np.zeros(0, np.int32), sc.P_BASE)[2].tolist() == [0]


# ---- end to end ----

RULE = dict(tol=0.5, losses=(sc.LOSS_H3PO4, sc.LOSS_WATER), reduced=True, isotopes=2, mz_lo=150.0)


def _precursors(batch, seed=17):
    """one precursor per spectrum inside its own m/z range, charge 2 or 3; a few spectra without one"""
    rng = np.random.default_rng(seed)
    off = np.asarray(batch["peak_off"], np.int64)
    mz = np.asarray(batch["mz"], np.float64)
    lo = np.array([mz[a:b].min() for a, b in zip(off[:-1], off[1:])])
    hi = np.array([mz[a:b].max() for a, b in zip(off[:-1], off[1:])])
    pm = rng.uniform(lo + 0.3 * (hi - lo), lo + 0.6 * (hi - lo))
    pz = rng.integers(2, 4, pm.size).astype(np.int32)
    pz[::11] = 0
    return pm, pz


def _stripped(batch, pm, pz, rule=RULE):
    mz, it, off, _ = ru.strip(batch["mz"], batch["intensity"], batch["peak_off"], pm, pz, ru.strip_params(**rule))
    return dict(batch, mz=mz, intensity=it, peak_off=off)


def _same(got, want, what):
    assert set(got) == set(want), what
    for key in want:
        if isinstance(want[key], np.ndarray):
            assert got[key].dtype == want[key].dtype and got[key].tobytes() == want[key].tobytes(), (what, key)
        else:
            assert got[key] == want[key], (what, key)


def _shared(batch, hits=5):
    """the spectrum of every ``hits``-th PSM held once and shared by the PSMs behind it"""
    n = int(batch["n_psm"])
    po = batch["peak_off"]
    parts = [(batch["mz"][po[i]:po[i + 1]], batch["intensity"][po[i]:po[i + 1]]) for i in range(0, n, hits)]
    mz, it, off = dc.pack(parts, batch["mz"].dtype, batch["intensity"].dtype, gaps=False)
    return dict(batch, mz=mz, intensity=it, peak_off=off, spec_of=(np.arange(n) // hits).astype(np.uint32), n_spectra=len(parts))


@pytest.fixture(scope="module")
def dense():
    batch, settings = dc.dense_batch()
    pm, pz = _precursors(batch)
    return batch, settings, _gpu(settings), pm, pz


def test_score_batch_private(dense):
    batch, settings, gpu, pm, pz = dense
    before = (batch["mz"].copy(), batch["intensity"].copy(), batch["peak_off"].copy())
    req = dict(RULE, precursor_mz=pm, precursor_charge=pz)
    got = gpu.score_batch(batch, strip=req)
    want_batch = _stripped(batch, pm, pz)
    assert 0.0 < 1.0 - want_batch["mz"].size / batch["mz"].size < 0.5      # (the rule has work to do, and leaves work for the scorer)
    _same(got, gpu.score_batch(want_batch), "private")
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, (batch["mz"], batch["intensity"], batch["peak_off"])))
    assert gpu.score_batch(batch)["best_score"].tobytes() != got["best_score"].tobytes() and (got["n_sig"] > 0).all()
    # tol=None is the scorer's mz_error
    plain = dict(precursor_mz=pm, precursor_charge=pz)
    _same(gpu.score_batch(batch, strip=plain), gpu.score_batch(_stripped(batch, pm, pz, dict(tol=gpu._mz_error))), "tol=None")
    for bad in (dict(RULE), dict(req, isotopes=7), dict(req, precursor_mz=pm[:-1]), True):
        with pytest.raises(ValueError):
            gpu.score_batch(batch, strip=bad)


def test_score_batch_shared_typed_and_kept(dense):
    batch, settings, gpu, pm, pz = dense
    shared = _shared(synth.slice_batch(batch, 0, 40))
    s_pm, s_pz = pm[0:40:5], pz[0:40:5]                                   # one precursor per shared spectrum
    req = dict(RULE, precursor_mz=s_pm, precursor_charge=s_pz)
    _same(gpu.score_batch(shared, strip=req), gpu.score_batch(_stripped(shared, s_pm, s_pz)), "shared")
    back = synth.take_psms(shared, np.arange(40)[::-1].copy())             # PSMs out of spectrum order: rows come back in input order
    _same(gpu.score_batch(back, strip=req), gpu.score_batch(_stripped(back, s_pm, s_pz)), "shared, out of order")
    with pytest.raises(ValueError):
        gpu.score_batch(shared, strip=dict(RULE, precursor_mz=pm[:40], precursor_charge=pz[:40]))    # per spectrum, not per PSM
    full = dict(RULE, precursor_mz=pm, precursor_charge=pz)
    f32 = synth.narrow_batch(batch)
    _same(gpu.score_batch(f32, strip=full), gpu.score_batch(_stripped(f32, pm, pz)), "float32")
    mixed = synth.narrow_batch(batch, np.float64, np.float32)
    _same(gpu.score_batch(mixed, strip=full), gpu.score_batch(_stripped(mixed, pm, pz)), "float64 m/z, float32 intensities")
    stages = dict(probs=True, mz_profile=dict(n_slots=1), skip_invalid=True)
    _same(gpu.score_batch(batch, strip=full, **stages), gpu.score_batch(_stripped(batch, pm, pz), **stages), "probs and mz_profile")
    # keep=True retains the stripped batch
    sub = synth.slice_batch(batch, 0, 6)
    want = gpu.score_batch(_stripped(sub, pm[:6], pz[:6]))
    _same(gpu.score_batch(sub, strip=dict(RULE, precursor_mz=pm[:6], precursor_charge=pz[:6]), keep=True), want, "keep")
    kept = gpu.batch_pep_scores(0, 6)
    gpu.score_batch(_stripped(sub, pm[:6], pz[:6]), keep=True)
    _same(kept, gpu.batch_pep_scores(0, 6), "the retained records")


def test_score_batch_strips_first_beside_the_other_filters(dense):
    """strip= in front of decharge=, and in front of deisotope= + recalibrate=: each equals the restatements applied in that
    order; the refusals between the other three stand with strip= beside them"""
    batch, settings, gpu, pm, pz = dense
    req = dict(RULE, precursor_mz=pm, precursor_charge=pz)
    base = _stripped(batch, pm, pz)
    d_mz, d_it, d_off, _, _ = ru.decharge(base["mz"], base["intensity"], base["peak_off"], ru.decharge_params())
    _same(gpu.score_batch(batch, strip=req, decharge=True), gpu.score_batch(dict(base, mz=d_mz, intensity=d_it, peak_off=d_off)),
          "strip, then decharge")
    i_mz, i_it, i_off, _ = ru.deisotope(base["mz"], base["intensity"], base["peak_off"], ru.deisotope_params())
    cal = np.zeros(1, ru.MZ_CALIBRATION_DTYPE)
    cal["ppm"][0] = [20.0, 15.0, 10.0, 5.0, 0.0, -5.0, -10.0, -15.0]
    _same(gpu.score_batch(batch, strip=req, deisotope=True, recalibrate=dict(calibration=cal)),
          gpu.score_batch(dict(base, mz=i_mz, intensity=i_it, peak_off=i_off), recalibrate=dict(calibration=cal)),
          "strip, then deisotope, then recalibrate")
    _same(gpu.score_batch(batch, strip=req, deisotope=True), gpu.score_batch(dict(base, mz=i_mz, intensity=i_it, peak_off=i_off)),
          "strip, then deisotope")
    with pytest.raises(ValueError):
        gpu.score_batch(batch, strip=req, decharge=True, deisotope=True)
    with pytest.raises(ValueError):
        gpu.score_batch(batch, strip=req, decharge=True, recalibrate=dict(calibration=cal))


def test_device_form_feeds_a_plan(dense):
    """device.strip -> read the offsets -> DevicePlan(...).run, against the same plan on host-stripped arrays"""
    import torch
    from pyascore_amd import device
    batch, settings, gpu, pm, pz = dense
    dev = torch.device("cuda", gpu.device)
    p = ru.strip_params(**RULE)
    d_mz, d_it = torch.from_numpy(batch["mz"]).to(dev), torch.from_numpy(batch["intensity"]).to(dev)
    o_mz, o_it, d_new, d_rep, d_over = device.strip(gpu, d_mz, d_it, batch["peak_off"], pm, pz, p)
    new_off = d_new.cpu().numpy()
    want = _stripped(batch, pm, pz)
    assert new_off.tobytes() == want["peak_off"].tobytes() and d_over.cpu().numpy().tolist() == [0, 0]
    results = []
    for mz_t, it_t in ((o_mz, o_it), (torch.from_numpy(want["mz"]).to(dev), torch.from_numpy(want["intensity"]).to(dev))):
        plan = device.DevicePlan(gpu, dict(batch, peak_off=new_off))
        plan.run(mz_t, it_t)
        plan.check()
        results.append([t.cpu().numpy().tobytes() for t in (plan.best_score, plan.best_sig, plan.n_sig, plan.ascores, plan.alt_mask)])
        plan.close()
    assert results[0] == results[1]
    host = gpu.score_batch(want)
    assert results[0][0] == host["best_score"].tobytes() and results[0][3] == host["ascores"].tobytes()


def test_deisotoping_is_what_it_was():
    """the fill kernel is now launched through an exported launcher: pya_deisotope_spectra on the deisotope boundary spectra
    still equals the restatement, byte for byte"""
    gpu = _any_gpu()
    for mz_t, it_t in TYPES.values():
        mz, it, off = dc.pack(dc.boundary_spectra(), mz_t, it_t, gaps=False)
        want = ru.deisotope(mz, it, off, dc.P0)
        got = gpu.deisotope_spectra(mz, it, off, dc.P0)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and got[2].tobytes() == want[2].tobytes()
        assert got[3] == (0, None) and not want[3].all()
