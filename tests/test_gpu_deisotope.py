"""Deisotoping on the GPU (pya_deisotope_params): pya_deisotope_spectra against pyascore_amd.rollup.deisotope, the numpy
restatement of the header's rule that tests/test_deisotope_host.py pins by hand -- every comparison is on raw bytes --, the
bounds of everything it writes, its refusals, the host form, and score_batch(deisotope=...) / device.deisotope against the
same calls on arrays the restatement filtered."""
import ctypes as C

import numpy as np
import pytest

import deisotope_cases as dc
from conftest import checker_kind
from oracle import harness, par_check
from pyascore_amd import _lib, rollup as ru, synth

pytestmark = pytest.mark.gpu

KEYS = ("best_score", "best_sig", "n_sig", "ascores", "alt_mask")
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
    """One pya_deisotope_spectra call on torch's current stream with canaries around everything it may write: the out arrays
    are pre-filled, guard words stand behind d_new_off, d_over and the workspace.  ``check()`` waits, looks at the canaries
    and returns (mz, intensity, new_off, over) of the host."""

    def __init__(self, mz, it, off, work_peaks=None):
        import torch
        self.torch, self.gpu = torch, _any_gpu()
        self.dev = dev = torch.device("cuda", self.gpu.device)
        self.mz, self.it, self.off = mz, it, np.ascontiguousarray(off, np.int64)
        self.n, self.n_spec = mz.size, self.off.size - 1
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)             # noqa: E731
        self.d_mz, self.d_it, self.d_off = to(mz), to(it), to(self.off)
        self.o_mz = to(np.full(self.n + GUARD, -7.0, mz.dtype))
        self.o_it = to(np.full(self.n + GUARD, -7.0, it.dtype))
        self.new_off = to(np.full(self.n_spec + 1 + GUARD, -99, np.int64))
        over = np.full(2 + GUARD, 0x5A5A, np.int32)
        over[:2] = 0
        self.over = to(over)
        self.work_bytes = int(self.gpu._lib.pya_deisotope_workspace_bytes(self.n_spec, self.n if work_peaks is None else work_peaks))
        assert self.work_bytes % 8 == 0 and self.work_bytes >= 8
        self.work = to(np.full(self.work_bytes // 8 + GUARD, 0x1234567, np.int64))
        self.t_in = _lib.TypedSpectra(self.d_mz.data_ptr(), self.d_it.data_ptr(), _lib.spectrum_type(mz.dtype), _lib.spectrum_type(it.dtype))
        self.t_out = _lib.TypedSpectra(self.o_mz.data_ptr(), self.o_it.data_ptr(), self.t_in.mz_type, self.t_in.intensity_type)

    def run(self, rule, **change):
        a = dict(t_in=C.byref(self.t_in), off=self.d_off.data_ptr(), n_spec=self.n_spec, params=C.byref(ru.deisotope_c_params(rule)),
                 work=self.work.data_ptr(), work_bytes=self.work_bytes, t_out=C.byref(self.t_out), new_off=self.new_off.data_ptr(),
                 over=self.over.data_ptr())
        a.update(change)
        stream = self.torch.cuda.current_stream(self.dev).cuda_stream
        return self.gpu._lib.pya_deisotope_spectra(self.gpu._h, a["t_in"], a["off"], a["n_spec"], a["params"], stream, a["work"], a["work_bytes"],
                                                   a["t_out"], a["new_off"], a["over"])

    def host(self):
        self.torch.cuda.synchronize(self.dev)
        return [t.cpu().numpy() for t in (self.o_mz, self.o_it, self.new_off, self.over, self.work)]

    def untouched(self):
        o_mz, o_it, new_off, over, work = self.host()
        return (o_mz == -7.0).all() and (o_it == -7.0).all() and (new_off == -99).all() and over.tolist() == [0, 0] + [0x5A5A] * GUARD and \
            (work == 0x1234567).all()

    def check(self):
        o_mz, o_it, new_off, over, work = self.host()
        assert (new_off[self.n_spec + 1:] == -99).all(), "guard behind d_new_off"
        assert over[2:].tolist() == [0x5A5A] * GUARD, "guard behind d_over"
        assert (work[self.work_bytes // 8:] == 0x1234567).all(), "guard behind the workspace"
        kept = int(new_off[self.n_spec])
        assert 0 <= kept <= self.n
        assert (o_mz[kept:] == -7.0).all() and (o_it[kept:] == -7.0).all(), "out elements from new_off[n] on"
        assert self.d_mz.cpu().numpy().tobytes() == self.mz.tobytes() and self.d_it.cpu().numpy().tobytes() == self.it.tobytes()
        return o_mz[:kept], o_it[:kept], new_off[:self.n_spec + 1], over[:2].view(np.uint32)


def _equals_restatement(mz, it, off, params, what):
    call = _Call(mz, it, off)
    assert call.run(params) == 0, call.gpu._lib.pya_last_error(call.gpu._h)
    g_mz, g_it, g_off, g_over = call.check()
    w_mz, w_it, w_off, keep = ru.deisotope(mz, it, off, params)
    assert g_off.tobytes() == w_off.tobytes(), what
    assert g_mz.dtype == mz.dtype and g_mz.tobytes() == w_mz.tobytes(), what
    assert g_it.dtype == it.dtype and g_it.tobytes() == w_it.tobytes(), what
    return keep, g_over


# ---- the kernels against the restatement ----

@pytest.mark.parametrize("types", sorted(TYPES))
def test_stride_and_ballot_boundaries(types):
    """spectra of 0, 1, 2, 63, 64, 65, 127, 128, 129 and 4 097 peaks in one call, parents and satellites on both sides of every
    64-peak boundary"""
    mz_t, it_t = TYPES[types]
    mz, it, off = dc.pack(dc.boundary_spectra(), mz_t, it_t, gaps=False)
    assert np.diff(off).tolist() == list(dc.BOUNDARY_LENGTHS)
    keep, over = _equals_restatement(mz, it, off, dc.P0, types)
    assert over.tolist() == [0, 0]
    big = slice(int(off[9]), int(off[10]))
    assert 0.2 < keep[big].mean() < 0.8                                   # (the filter has work on both sides)
    k = keep[big]
    at_edges = np.concatenate([k[63::64], k[64::64]])                     # removed and kept peaks right at the boundaries
    assert at_edges.any() and not at_edges.all()


@pytest.mark.parametrize("types", sorted(TYPES))
def test_hand_made_spectra(types):
    """every case of tests/deisotope_cases.py, the cases of one parameter set in one call with empty spectra between them"""
    mz_t, it_t = TYPES[types]
    cases = dc.hand_cases()
    groups = {}
    for c in cases:
        groups.setdefault(dc.params_key(c["params"]), []).append(c)
    assert len(groups) >= 6
    for group in groups.values():
        mz, it, off = dc.pack([(c["mz"], c["intensity"]) for c in group], mz_t, it_t, gaps=True)
        keep, over = _equals_restatement(mz, it, off, group[0]["params"], (types, group[0]["name"]))
        if types == "f64/f64":                                             # (the float32 cases hold the same values widened)
            assert keep.tolist() == np.concatenate([c["keep"] for c in group]).tolist()
        if mz_t == np.float64:
            bad = [2 * i for i, c in enumerate(group) if c["unordered"]]
            assert over.tolist() == ([len(bad), 0xFFFFFFFF - bad[0]] if bad else [0, 0])


@pytest.mark.parametrize("types", sorted(TYPES))
def test_dense_psms(types):
    mz_t, it_t = TYPES[types]
    batch, _ = dc.dense_batch()
    keep, over = _equals_restatement(batch["mz"].astype(mz_t), batch["intensity"].astype(it_t), batch["peak_off"], dc.P0, types)
    assert over.tolist() == [0, 0] and 0.25 < keep.mean() < 0.6


def test_more_spectra_than_wavefronts_and_scan_tiles():
    """9 000 small spectra: the grid strides over them (8 192 wavefronts) and the offset scan has 9 tiles; the other parameter
    sets on the first 700 of them"""
    rng = np.random.default_rng(21)
    spectra = []
    for n in rng.integers(0, 9, 9_000):
        kind = rng.integers(0, 4, size=n)
        spectra.append((100.0 + np.cumsum(np.choose(kind, [dc.S, dc.S / 2, 0.7313, 0.0])), rng.choice([1.0, 2.0, 3.0], size=n)))
    mz, it, off = dc.pack(spectra, np.float64, np.float32, gaps=False)
    keep, over = _equals_restatement(mz, it, off, dc.P0, "9 000 spectra")
    assert over.tolist() == [0, 0] and not keep.all()
    for p in (dc.P_HALF, dc.P_PER_MZ, ru.deisotope_params(max_charge=8, tol=0.002)):
        keep, over = _equals_restatement(mz[:off[700]], it[:off[700]], off[:701], p, "700 spectra")
        assert over.tolist() == [0, 0] and not keep.all()


def test_a_descending_spectrum_among_good_ones():
    spectra = dc.boundary_spectra(seed=9)
    s = 5
    x, y = spectra[s]
    x = x.copy()
    x[40] = x[38] - 0.5                                                   # one descending pair inside a 65-peak spectrum
    spectra[s] = (x, y)
    mz, it, off = dc.pack(spectra, gaps=False)
    keep, over = _equals_restatement(mz, it, off, dc.P0, "descending")
    assert over.tolist() == [1, 0xFFFFFFFF - s]
    assert keep[off[s]:off[s + 1]].all()
    clean = dc.pack(dc.boundary_spectra(seed=9), gaps=False)
    keep_clean = ru.deisotope(*clean, dc.P0)[3]
    assert not keep_clean[off[s]:off[s + 1]].all()
    others = np.ones(keep.size, bool)
    others[off[s]:off[s + 1]] = False
    assert keep[others].tolist() == keep_clean[others].tolist()          # the neighbours are not affected
    # two of them: the count, and the smaller spectrum number
    x2, y2 = spectra[8]
    spectra[8] = (x2[::-1].copy(), y2)
    mz, it, off = dc.pack(spectra, gaps=False)
    _, over = _equals_restatement(mz, it, off, dc.P0, "two descending")
    assert over.tolist() == [2, 0xFFFFFFFF - s]


def test_a_workspace_for_fewer_peaks_clips_instead_of_writing_past_it():
    """the peak count is on the device: the host cannot refuse, the kernels clip to the peaks the workspace has bits for and
    report the spectra that reach beyond them; no canary is touched"""
    mz, it, off = dc.pack(dc.boundary_spectra(), gaps=False)
    call = _Call(mz, it, off, work_peaks=256)
    assert call.run(dc.P0) == 0
    g_mz, g_it, g_off, over = call.check()
    cap = 256 + 63                                                        # (the bits of the last word count)
    inside = int(np.searchsorted(off, cap, "right")) - 1                  # spectra that end at or before the cap
    assert inside >= 6
    w_mz, _, w_off, _ = ru.deisotope(mz, it, off[:inside + 1], dc.P0)
    assert g_off[:inside + 1].tolist() == w_off.tolist() and g_mz[:int(w_off[-1])].tobytes() == w_mz.tobytes()
    assert over[0] >= 1 and 0xFFFFFFFF - int(over[1]) == inside


def test_refusals_launch_nothing():
    mz, it, off = dc.pack(dc.boundary_spectra()[:6], gaps=False)
    call = _Call(mz, it, off)
    lib, h = call.gpu._lib, call.gpu._h
    f32 = _Call(mz.astype(np.float32), it.astype(np.float32), off)
    ok = ru.deisotope_params()

    def params(**kw):
        p = ru.deisotope_c_params(ok)
        for k, v in kw.items():
            if k == "spacing":
                for i, s in enumerate(v):
                    p.spacing[i] = s
            else:
                setattr(p, k, v)
        return C.byref(p)

    def typed(mz_ptr, it_ptr, mz_type, it_type):
        return C.byref(_lib.TypedSpectra(mz_ptr, it_ptr, mz_type, it_type))

    i, o = call.t_in, call.t_out
    bad = dict(
        null_in=dict(t_in=None), null_out=dict(t_out=None), null_off=dict(off=None), null_new_off=dict(new_off=None), null_over=dict(over=None),
        null_work=dict(work=None), null_params=dict(params=None),
        null_mz=dict(t_in=typed(None, i.intensity, i.mz_type, i.intensity_type)), null_out_it=dict(t_out=typed(o.mz, None, o.mz_type, o.intensity_type)),
        in_place_mz=dict(t_out=typed(i.mz, o.intensity, o.mz_type, o.intensity_type)),
        in_place_it=dict(t_out=typed(o.mz, i.intensity, o.mz_type, o.intensity_type)),
        unknown_type=dict(t_in=typed(i.mz, i.intensity, 2, 0), t_out=typed(o.mz, o.intensity, 2, 0)),
        unknown_it_type=dict(t_in=typed(i.mz, i.intensity, 0, 7), t_out=typed(o.mz, o.intensity, 0, 7)),
        mismatched_types=dict(t_out=typed(o.mz, o.intensity, _lib.PYA_F64, _lib.PYA_F32)),
        f32_mz_f64_it=dict(t_in=typed(i.mz, i.intensity, _lib.PYA_F32, _lib.PYA_F64), t_out=typed(o.mz, o.intensity, _lib.PYA_F32, _lib.PYA_F64)),
        small_work=dict(work_bytes=int(lib.pya_deisotope_workspace_bytes(call.n_spec, 0)) - 8), no_work=dict(work_bytes=0),
        misaligned_work=dict(work=call.work.data_ptr() + 4),
        too_many=dict(n_spec=0xFFFFFFFF),
        tol_negative=dict(params=params(tol=-0.01)), tol_nan=dict(params=params(tol=float("nan"))), tol_inf=dict(params=params(tol=float("inf"))),
        ratio_nan=dict(params=params(ratio0=float("nan"))), per_mz_inf=dict(params=params(ratio_per_mz=float("inf"))),
        charge_0=dict(params=params(max_charge=0)), charge_9=dict(params=params(max_charge=9)), reserved=dict(params=params(reserved=1)),
        spacing_rising=dict(params=params(spacing=[0.5, 1.0])), spacing_equal=dict(params=params(spacing=[1.0, 1.0])),
        spacing_zero=dict(params=params(spacing=[1.0, 0.5, 0.0])), spacing_nan=dict(params=params(spacing=[float("nan")])),
        spacing_under_2_tol=dict(params=params(tol=0.2)),
    )
    for name, change in bad.items():
        assert call.run(ok, **change) == _lib.PYA_ERR_ARG, name
        assert b"pya_deisotope_spectra" in lib.pya_last_error(h), (name, lib.pya_last_error(h))
    assert call.untouched()                                               # nothing was launched, nothing was written
    # (the same checks in front of the float32 instantiation and of the host form)
    assert f32.run(ok, work_bytes=0) == _lib.PYA_ERR_ARG and f32.untouched()
    out_mz, out_it, new_off, over = np.zeros_like(mz), np.zeros_like(it), np.zeros(off.size, np.int64), np.zeros(2, np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)                           # noqa: E731
    h_in = _lib.TypedSpectra(vp(mz), vp(it), 0, 0)
    h_out = _lib.TypedSpectra(vp(out_mz), vp(out_it), 0, 0)
    host = lambda **kw: lib.pya_deisotope_spectra_host(h, kw.get("t_in", C.byref(h_in)), vp(kw.get("off", off)), off.size - 1,   # noqa: E731
                                                       kw.get("params", params()), kw.get("t_out", C.byref(h_out)), vp(new_off), vp(over))
    for name, kw in dict(in_place=dict(t_out=C.byref(h_in)), params=dict(params=params(max_charge=0)), descending=dict(off=off[::-1].copy()),
                         negative=dict(off=off - 1)).items():
        assert host(**kw) == _lib.PYA_ERR_ARG, name
        assert b"pya_deisotope_spectra_host" in lib.pya_last_error(h), name
    assert not out_mz.any() and not new_off.any()
    assert host() == 0 and new_off.tolist() == ru.deisotope(mz, it, off, ok)[2].tolist()
    # a good call still works on the same buffers
    assert call.run(ok) == 0
    assert call.check()[2].tolist() == new_off.tolist()


def test_no_spectra_is_a_no_op_that_writes_the_first_offset():
    e = np.zeros(0)
    call = _Call(e, e, np.zeros(1, np.int64))
    assert call.run(dc.P0, t_in=C.byref(_lib.TypedSpectra(None, None, 0, 0)), t_out=C.byref(_lib.TypedSpectra(None, None, 0, 0)), work=None,
                    work_bytes=0, over=None, off=None) == 0
    _, _, new_off, over = call.check()
    assert new_off.tolist() == [0] and over.tolist() == [0, 0]
    assert _any_gpu()._lib.pya_deisotope_workspace_bytes(0, 0) == 8


@pytest.mark.parametrize("types", sorted(TYPES))
def test_the_host_form_and_the_torch_form_equal_the_device_form(types):
    import torch
    from pyascore_amd import device
    mz_t, it_t = TYPES[types]
    gpu = _any_gpu()
    spectra = dc.boundary_spectra(seed=3)
    x, y = spectra[4]
    spectra[4] = (x[::-1].copy(), y)                                      # one spectrum that is not ascending
    mz, it, off = dc.pack(spectra, mz_t, it_t, gaps=False)
    want = ru.deisotope(mz, it, off, dc.P0)
    h_mz, h_it, h_off, h_over = gpu.deisotope_spectra(mz, it, off, dc.P0)
    assert h_mz.dtype == mz_t and h_it.dtype == it_t and h_over == (1, 4)
    assert h_mz.tobytes() == want[0].tobytes() and h_it.tobytes() == want[1].tobytes() and h_off.tobytes() == want[2].tobytes()
    dev = torch.device("cuda", gpu.device)
    d_mz, d_it = torch.from_numpy(mz).to(dev), torch.from_numpy(it).to(dev)
    for peak_off in (off, torch.from_numpy(off).to(dev)):
        o_mz, o_it, d_new, d_over = device.deisotope(gpu, d_mz, d_it, peak_off, dc.P0)
        new = d_new.cpu().numpy()
        kept = int(new[-1])
        assert new.tobytes() == want[2].tobytes() and d_over.cpu().numpy().view(np.uint32).tolist() == [1, 0xFFFFFFFF - 4]
        assert o_mz.dtype == d_mz.dtype and o_mz.cpu().numpy()[:kept].tobytes() == want[0].tobytes()
        assert o_it.dtype == d_it.dtype and o_it.cpu().numpy()[:kept].tobytes() == want[1].tobytes()
    with pytest.raises(ValueError):
        device.deisotope(gpu, d_mz, d_it, off, dc.P0, out=(d_mz, d_it))   # not in place
    with pytest.raises(ValueError):
        device.deisotope(gpu, d_mz, d_it, off, dict(dc.P0, tol=1.0))
    # float32 m/z beside float64 intensities is widened by the host form, as score_batch does
    if types == "f32/f32":
        w = gpu.deisotope_spectra(mz, it.astype(np.float64), off, dc.P0)
        assert w[0].dtype == np.float64 and w[2].tobytes() == want[2].tobytes()
    # spectra without any peak
    assert gpu.deisotope_spectra(mz[:0], it[:0], [0, 0, 0], dc.P0)[2].tolist() == [0, 0, 0]


# ---- end to end ----

def _filtered(batch, params):
    mz, it, off, _ = ru.deisotope(batch["mz"], batch["intensity"], batch["peak_off"], params)
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
    return batch, settings, _gpu(settings)


def test_score_batch_private(dense):
    batch, settings, gpu = dense
    before = (batch["mz"].copy(), batch["intensity"].copy(), batch["peak_off"].copy())
    got = gpu.score_batch(batch, deisotope=dict(tol=0.01, max_charge=3))
    want = gpu.score_batch(_filtered(batch, dc.P0))
    _same(got, want, "private")
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, (batch["mz"], batch["intensity"], batch["peak_off"])))
    plain = gpu.score_batch(batch)
    assert plain["best_score"].tobytes() != got["best_score"].tobytes() and (got["n_sig"] > 0).all()
    assert float(got["best_score"].mean()) > float(plain["best_score"].mean())       # satellites cost score; the rule gives it back
    _same(gpu.score_batch(batch, deisotope=True), want, "deisotope=True")
    other = dict(tol=0.004, max_charge=2, ratio=0.7, ratio_per_mz=1e-4)
    _same(gpu.score_batch(batch, deisotope=other), gpu.score_batch(_filtered(batch, ru.deisotope_params(**other))), "other parameters")
    with pytest.raises(ValueError):
        gpu.score_batch(batch, deisotope=dict(max_charge=9))


def test_score_batch_shared_typed_and_beside_other_stages(dense):
    batch, settings, gpu = dense
    shared = _shared(synth.slice_batch(batch, 0, 40))
    _same(gpu.score_batch(shared, deisotope=True), gpu.score_batch(_filtered(shared, dc.P0)), "shared")
    back = synth.take_psms(shared, np.arange(40)[::-1].copy())             # PSMs out of spectrum order: rows come back in input order
    _same(gpu.score_batch(back, deisotope=True), gpu.score_batch(_filtered(back, dc.P0)), "shared, out of order")
    f32 = synth.narrow_batch(batch)
    got = gpu.score_batch(f32, deisotope=True)
    _same(got, gpu.score_batch(_filtered(f32, dc.P0)), "float32")
    mixed = synth.narrow_batch(batch, np.float64, np.float32)
    _same(gpu.score_batch(mixed, deisotope=True), gpu.score_batch(_filtered(mixed, dc.P0)), "float64 m/z, float32 intensities")
    stages = dict(probs=True, mz_profile=dict(n_slots=1), skip_invalid=True)
    _same(gpu.score_batch(batch, deisotope=True, **stages), gpu.score_batch(_filtered(batch, dc.P0), **stages), "probs and mz_profile")
    # with recalibrate=: deisotoping first, the kept peaks are then corrected
    cal = np.zeros(1, ru.MZ_CALIBRATION_DTYPE)
    cal["ppm"][0] = [20.0, 15.0, 10.0, 5.0, 0.0, -5.0, -10.0, -15.0]
    _same(gpu.score_batch(batch, deisotope=True, recalibrate=dict(calibration=cal)),
          gpu.score_batch(_filtered(batch, dc.P0), recalibrate=dict(calibration=cal)), "deisotope, then recalibrate")
    # keep=True retains the filtered batch
    sub = synth.slice_batch(batch, 0, 6)
    want = gpu.score_batch(_filtered(sub, dc.P0))
    _same(gpu.score_batch(sub, deisotope=True, keep=True), want, "keep")
    kept = gpu.batch_pep_scores(0, 6)
    gpu.score_batch(_filtered(sub, dc.P0), keep=True)
    again = gpu.batch_pep_scores(0, 6)
    _same(kept, again, "the retained records")


def test_device_form_feeds_a_plan(dense):
    """device.deisotope -> read the offsets -> DevicePlan(...).run, against the same plan on host-filtered arrays"""
    import torch
    from pyascore_amd import device
    batch, settings, gpu = dense
    dev = torch.device("cuda", gpu.device)
    d_mz, d_it = torch.from_numpy(batch["mz"]).to(dev), torch.from_numpy(batch["intensity"]).to(dev)
    o_mz, o_it, d_new, d_over = device.deisotope(gpu, d_mz, d_it, batch["peak_off"], dc.P0)
    new_off = d_new.cpu().numpy()
    want = _filtered(batch, dc.P0)
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


def test_filtered_batch_against_the_reference():
    """64 PSMs with satellites: score_batch(deisotope=...) against the reference's own core on the arrays the restatement
    filtered (the reference sees deisotoped spectra only through the restatement, which the host file pins)"""
    desc = synth.describe("cfg2", n_psm=64, n_noise=300, isotopes=True, seed=77)
    batch, settings = synth.make_slice(desc), desc["settings"]
    got = _gpu(settings).score_batch(batch, deisotope=True)
    sub = {k: (np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v) for k, v in _filtered(batch, dc.P0).items()}
    want = par_check.score_batch_parallel(settings, sub, got["ascores"].shape[1], kind=checker_kind())
    for key in KEYS:
        assert np.array_equal(got[key], want[key]), key
