"""Centroiding on the GPU (pya_centroid_params): pya_centroid_spectra against pyascore_amd.rollup.centroid, the numpy
restatement of the header's rule that tests/test_centroid_host.py pins by hand -- every comparison is on raw bytes --, the bounds
of everything it writes, its refusals, the host form, and score_batch(centroid=...) / device.centroid against the same calls on
arrays the restatement centroided."""
import ctypes as C

import numpy as np
import pytest

import centroid_cases as cc
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
    """One pya_centroid_spectra call on torch's current stream with canaries around everything it may write: the out arrays are
    pre-filled, guard words stand behind d_new_off, d_over and the workspace.  ``check()`` waits, looks at the canaries and
    returns (mz, intensity, new_off, over) of the host."""

    def __init__(self, mz, it, off, select=None, work_peaks=None):
        import torch
        self.torch, self.gpu = torch, _any_gpu()
        self.dev = dev = torch.device("cuda", self.gpu.device)
        self.mz, self.it, self.off = mz, it, np.ascontiguousarray(off, np.int64)
        self.n, self.n_spec = mz.size, self.off.size - 1
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)             # noqa: E731
        self.d_mz, self.d_it, self.d_off = to(mz), to(it), to(self.off)
        self.d_sel = None if select is None else to(np.asarray(select, np.uint8))
        self.o_mz = to(np.full(self.n + GUARD, -7.0, mz.dtype))
        self.o_it = to(np.full(self.n + GUARD, -7.0, it.dtype))
        self.new_off = to(np.full(self.n_spec + 1 + GUARD, -99, np.int64))
        over = np.full(2 + GUARD, 0x5A5A, np.int32)
        over[:2] = 0
        self.over = to(over)
        self.work_bytes = int(self.gpu._lib.pya_centroid_workspace_bytes(self.n_spec, self.n if work_peaks is None else work_peaks))
        assert self.work_bytes % 8 == 0 and self.work_bytes >= 8
        self.work = to(np.full(self.work_bytes // 8 + GUARD, 0x1234567, np.int64))
        self.t_in = _lib.TypedSpectra(self.d_mz.data_ptr(), self.d_it.data_ptr(), _lib.spectrum_type(mz.dtype), _lib.spectrum_type(it.dtype))
        self.t_out = _lib.TypedSpectra(self.o_mz.data_ptr(), self.o_it.data_ptr(), self.t_in.mz_type, self.t_in.intensity_type)

    def run(self, rule, **change):
        a = dict(t_in=C.byref(self.t_in), off=self.d_off.data_ptr(), n_spec=self.n_spec, select=None if self.d_sel is None else self.d_sel.data_ptr(),
                 params=C.byref(ru.centroid_c_params(rule)), work=self.work.data_ptr(), work_bytes=self.work_bytes, t_out=C.byref(self.t_out),
                 new_off=self.new_off.data_ptr(), over=self.over.data_ptr())
        a.update(change)
        stream = self.torch.cuda.current_stream(self.dev).cuda_stream
        return self.gpu._lib.pya_centroid_spectra(self.gpu._h, a["t_in"], a["off"], a["n_spec"], a["select"], a["params"], stream, a["work"],
                                                  a["work_bytes"], a["t_out"], a["new_off"], a["over"])

    def host(self):
        self.torch.cuda.synchronize(self.dev)
        return [t.cpu().numpy() for t in (self.o_mz, self.o_it, self.new_off, self.over, self.work)]

    def untouched(self):
        o_mz, o_it, new_off, over, work = self.host()
        return (o_mz == -7.0).all() and (o_it == -7.0).all() and (new_off == -99).all() and \
            over.tolist() == [0, 0] + [0x5A5A] * GUARD and (work == 0x1234567).all()

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


def _equals_restatement(mz, it, off, params, what, select=None):
    call = _Call(mz, it, off, select)
    assert call.run(params) == 0, call.gpu._lib.pya_last_error(call.gpu._h)
    g_mz, g_it, g_off, g_over = call.check()
    w_mz, w_it, w_off, w_bad = ru.centroid(mz, it, off, params, select)
    assert g_off.tobytes() == w_off.tobytes(), what
    assert g_mz.dtype == mz.dtype and g_mz.tobytes() == w_mz.tobytes(), what
    assert g_it.dtype == it.dtype and g_it.tobytes() == w_it.tobytes(), what
    bad = np.flatnonzero(w_bad)
    assert g_over.tolist() == ([int(bad.size), 0xFFFFFFFF - int(bad[0])] if bad.size else [0, 0]), what
    return g_mz, g_it, g_off


# ---- the kernels against the restatement ----

@pytest.mark.parametrize("area", [0, 1])
@pytest.mark.parametrize("types", sorted(TYPES))
def test_stride_and_ballot_boundaries(types, area):
    """spectra of 0, 1, 2, 63, 64, 65, 127, 128, 129 and 4 097 points in one call, apexes planted at 0, 62, 63, 64, 65 and the
    last point, footprints of every shape on both sides of every 64-point boundary; with select NULL and given"""
    mz_t, it_t = TYPES[types]
    spectra, planted = cc.boundary_spectra()
    mz, it, off = cc.pack(spectra, mz_t, it_t, gaps=False)
    assert np.diff(off).tolist() == list(cc.BOUNDARY_LENGTHS)
    for p in (dict(cc.P, area=area), dict(cc.P_W1, area=area), dict(cc.P_W8_AREA, area=area)):
        g_mz, g_it, g_off = _equals_restatement(mz, it, off, p, (types, p))
        assert np.diff(g_off).sum() < mz.size // 2 and int(np.diff(g_off)[9]) > 500
        if not area:
            assert [int((g_it[a:b] == 16.0).sum()) for a, b in zip(g_off[:-1], g_off[1:])] == [len(at) for at in planted]
    select = np.arange(len(spectra)) % 3 != 1                              # (the 64-, 128- and 0-point spectra are copied)
    g_mz, g_it, g_off = _equals_restatement(mz, it, off, dict(cc.P, area=area), (types, "select"), select)
    assert np.diff(g_off)[~select].tolist() == np.diff(off)[~select].tolist()


@pytest.mark.parametrize("types", sorted(TYPES))
def test_hand_made_spectra(types):
    """every case of tests/centroid_cases.py, the cases of one parameter set in one call with empty spectra between them, with
    area 0 and 1; in float64 the bytes are the ones written out by hand"""
    mz_t, it_t = TYPES[types]
    groups = {}
    for c in cc.hand_cases():
        groups.setdefault(cc.params_key(dict(c["params"], area=0)), []).append(c)
    assert len(groups) >= 6
    for group in groups.values():
        mz, it, off = cc.pack([(c["mz"], c["intensity"]) for c in group], mz_t, it_t, gaps=True)
        select = np.repeat([c["select"] for c in group], 2)
        for area in (0, 1):
            p = dict(group[0]["params"], area=area)
            g_mz, g_it, g_off = _equals_restatement(mz, it, off, p, (types, group[0]["name"], area), select)
            if mz_t == np.float64 and it_t == np.float64:                  # (the float32 cases hold the same values widened)
                assert g_mz.tobytes() == np.concatenate([c["out_mz"].astype(np.float64) for c in group]).tobytes()
                assert g_it.tobytes() == np.concatenate([cc.expected(c, area)[1].astype(np.float64) for c in group]).tobytes()
                assert np.diff(g_off)[0::2].tolist() == [len(c["apex"]) for c in group]
        if all(c["select"] for c in group):
            _equals_restatement(mz, it, off, group[0]["params"], (types, group[0]["name"], "select NULL"))


def _tiny_spectra(n_spec, seed=21):
    """many spectra of 0 .. 12 points on the DX grid, steps of 0, 1 or 3 DX, intensities from a few values"""
    rng = np.random.default_rng(seed)
    spectra = []
    for n in rng.integers(0, 13, n_spec):
        x = 100.0 + np.cumsum(rng.choice([0.0, 1.0, 1.0, 1.0, 3.0], size=n)) * cc.DX
        spectra.append((x, rng.choice([0.0, 1.0, 2.0, 3.0, 8.0], size=n)))
    return spectra


def test_more_spectra_than_wavefronts_and_scan_tiles():
    """9 000 small spectra: the grid strides over them (8 192 wavefronts) and the offset scan has 9 tiles; every seventh
    spectrum is not selected, a few are not ascending"""
    spectra = _tiny_spectra(9_000)
    for s in range(100, 9_000, 997):
        if len(spectra[s][0]) > 2:
            spectra[s][0][1] = 99.0
    mz, it, off = cc.pack(spectra, np.float64, np.float32, gaps=False)
    select = np.arange(9_000) % 7 != 3
    g_mz, g_it, g_off = _equals_restatement(mz, it, off, cc.P_AREA, "9 000 spectra", select)
    assert 0.2 < g_mz.size / mz.size < 0.6


def test_a_workspace_for_fewer_peaks_clips_instead_of_writing_past_it():
    """the point count is on the device: the host cannot refuse, the kernels clip to the points the workspace has bits for and
    report the spectra that reach beyond them; no canary is touched"""
    spectra, _ = cc.boundary_spectra()
    mz, it, off = cc.pack(spectra, gaps=False)
    call = _Call(mz, it, off, work_peaks=256)
    assert call.run(cc.P) == 0
    g_mz, g_it, g_off, over = call.check()
    cap = 256 + 63                                                        # (the bits of the last word count)
    inside = int(np.searchsorted(off, cap, "right")) - 1                  # spectra that end at or before the cap
    assert inside >= 6
    w_mz, w_it, w_off, _ = ru.centroid(mz, it, off[:inside + 1], cc.P)
    assert g_off[:inside + 1].tolist() == w_off.tolist() and g_mz[:int(w_off[-1])].tobytes() == w_mz.tobytes()
    assert g_it[:int(w_off[-1])].tobytes() == w_it.tobytes()
    assert over[0] >= 1 and 0xFFFFFFFF - int(over[1]) == inside


def test_refusals_launch_nothing():
    spectra, _ = cc.boundary_spectra()
    mz, it, off = cc.pack(spectra[:6], gaps=False)
    call = _Call(mz, it, off)
    lib, h = call.gpu._lib, call.gpu._h
    f32 = _Call(mz.astype(np.float32), it.astype(np.float32), off)
    ok = cc.P

    def params(**kw):
        p = ru.centroid_c_params(ok)
        for k, v in kw.items():
            setattr(p, k, v)
        return C.byref(p)

    def typed(mz_ptr, it_ptr, mz_type, it_type):
        return C.byref(_lib.TypedSpectra(mz_ptr, it_ptr, mz_type, it_type))

    i, o = call.t_in, call.t_out
    nan, inf = float("nan"), float("inf")
    bad = dict(
        null_in=dict(t_in=None), null_out=dict(t_out=None), null_off=dict(off=None), null_new_off=dict(new_off=None), null_over=dict(over=None),
        null_work=dict(work=None), null_params=dict(params=None),
        null_mz=dict(t_in=typed(None, i.intensity, i.mz_type, i.intensity_type)), null_out_it=dict(t_out=typed(o.mz, None, o.mz_type, o.intensity_type)),
        in_place_mz=dict(t_out=typed(i.mz, o.intensity, o.mz_type, o.intensity_type)),
        in_place_it=dict(t_out=typed(o.mz, i.intensity, o.mz_type, o.intensity_type)),
        unknown_type=dict(t_in=typed(i.mz, i.intensity, 2, 0), t_out=typed(o.mz, o.intensity, 2, 0)),
        mismatched_types=dict(t_out=typed(o.mz, o.intensity, _lib.PYA_F64, _lib.PYA_F32)),
        f32_mz_f64_it=dict(t_in=typed(i.mz, i.intensity, _lib.PYA_F32, _lib.PYA_F64), t_out=typed(o.mz, o.intensity, _lib.PYA_F32, _lib.PYA_F64)),
        small_work=dict(work_bytes=int(lib.pya_centroid_workspace_bytes(call.n_spec, 0)) - 8), no_work=dict(work_bytes=0),
        misaligned_work=dict(work=call.work.data_ptr() + 4), too_many=dict(n_spec=0xFFFFFFFF),
        gap_negative=dict(params=params(gap0=-0.01)), gap_nan=dict(params=params(gap0=nan)), gap_inf=dict(params=params(gap0=inf)),
        gap_both_zero=dict(params=params(gap0=0.0)), per_mz_negative=dict(params=params(gap_per_mz=-1e-6)), per_mz_nan=dict(params=params(gap_per_mz=nan)),
        per_mz_inf=dict(params=params(gap_per_mz=inf)), height_negative=dict(params=params(min_height=-1.0)), height_nan=dict(params=params(min_height=nan)),
        height_inf=dict(params=params(min_height=inf)), width_0=dict(params=params(half_width=0)), width_9=dict(params=params(half_width=9)),
        area_2=dict(params=params(area=2)), reserved=dict(params=params(reserved=1)),
    )
    for name, change in bad.items():
        assert call.run(ok, **change) == _lib.PYA_ERR_ARG, name
        assert b"pya_centroid_spectra" in lib.pya_last_error(h), (name, lib.pya_last_error(h))
    assert call.untouched()                                               # nothing was launched, nothing was written
    assert f32.run(ok, work_bytes=0) == _lib.PYA_ERR_ARG and f32.untouched()
    assert lib.pya_centroid_workspace_bytes(6, 1000) == lib.pya_deisotope_workspace_bytes(6, 1000)
    # the same checks in front of the host form
    out_mz, out_it, new_off, over = np.zeros_like(mz), np.zeros_like(it), np.zeros(off.size, np.int64), np.zeros(2, np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)                           # noqa: E731
    h_in = _lib.TypedSpectra(vp(mz), vp(it), 0, 0)
    h_out = _lib.TypedSpectra(vp(out_mz), vp(out_it), 0, 0)
    host = lambda **kw: lib.pya_centroid_spectra_host(h, kw.get("t_in", C.byref(h_in)), vp(kw.get("off", off)), off.size - 1, None,   # noqa: E731
                                                      kw.get("params", params()), kw.get("t_out", C.byref(h_out)), vp(new_off), vp(over))
    for name, kw in dict(in_place=dict(t_out=C.byref(h_in)), params=dict(params=params(half_width=99)), descending=dict(off=off[::-1].copy()),
                         negative=dict(off=off - 1)).items():
        assert host(**kw) == _lib.PYA_ERR_ARG, name
        assert b"pya_centroid_spectra_host" in lib.pya_last_error(h), name
    assert not out_mz.any() and not new_off.any()
    want = ru.centroid(mz, it, off, ok)
    assert host() == 0 and new_off.tolist() == want[2].tolist() and out_mz[:want[0].size].tobytes() == want[0].tobytes()
    # a good call still works on the same buffers
    assert call.run(ok) == 0
    assert call.check()[2].tolist() == new_off.tolist()


def test_no_spectra_is_a_no_op_that_writes_the_first_offset():
    e = np.zeros(0)
    call = _Call(e, e, np.zeros(1, np.int64))
    null = C.byref(_lib.TypedSpectra(None, None, 0, 0))
    assert call.run(cc.P, t_in=null, t_out=null, work=None, work_bytes=0, over=None, off=None) == 0
    _, _, new_off, over = call.check()
    assert new_off.tolist() == [0] and over.tolist() == [0, 0]
    assert _any_gpu()._lib.pya_centroid_workspace_bytes(0, 0) == 8


@pytest.mark.parametrize("types", sorted(TYPES))
def test_the_host_form_and_the_torch_form_equal_the_device_form(types):
    import torch
    from pyascore_amd import device
    mz_t, it_t = TYPES[types]
    gpu = _any_gpu()
    spectra = _tiny_spectra(300, seed=3)
    spectra[4] = cc.boundary_spectra(seed=3)[0][9]                         # one long spectrum among them
    spectra[7] = (np.array([100.0 + 2 * cc.DX, 100.0 + cc.DX, 100.0]), np.array([1.0, 2.0, 1.0]))      # ... and one that descends
    mz, it, off = cc.pack(spectra, mz_t, it_t, gaps=False)
    select = np.arange(300) % 5 != 3
    dev = torch.device("cuda", gpu.device)
    d_mz, d_it = torch.from_numpy(mz).to(dev), torch.from_numpy(it).to(dev)
    for p, sel in ((cc.P, None), (cc.P_W8_AREA, select)):
        want = ru.centroid(mz, it, off, p, sel)
        assert want[3].sum() == 1 and want[3][7]
        h_mz, h_it, h_off, h_over = gpu.centroid_spectra(mz, it, off, p, sel)
        assert h_mz.dtype == mz_t and h_it.dtype == it_t and h_over == (1, 7)
        assert h_mz.tobytes() == want[0].tobytes() and h_it.tobytes() == want[1].tobytes() and h_off.tobytes() == want[2].tobytes()
        for peak_off, d_sel in ((off, sel), (torch.from_numpy(off).to(dev), None if sel is None else torch.from_numpy(sel).to(dev))):
            o_mz, o_it, d_new, d_over = device.centroid(gpu, d_mz, d_it, peak_off, p, d_sel)
            new = d_new.cpu().numpy()
            kept = int(new[-1])
            assert new.tobytes() == want[2].tobytes() and d_over.cpu().numpy().view(np.uint32).tolist() == [1, 0xFFFFFFFF - 7]
            assert o_mz.dtype == d_mz.dtype and o_mz.cpu().numpy()[:kept].tobytes() == want[0].tobytes()
            assert o_it.dtype == d_it.dtype and o_it.cpu().numpy()[:kept].tobytes() == want[1].tobytes()
    with pytest.raises(ValueError):
        device.centroid(gpu, d_mz, d_it, off, cc.P, out=(d_mz, d_it))      # not in place
    with pytest.raises(ValueError):
        device.centroid(gpu, d_mz, d_it, off, dict(cc.P, half_width=0))
    with pytest.raises(ValueError):
        device.centroid(gpu, d_mz, d_it, off, cc.P, select[:-1])
    # float32 m/z beside float64 intensities is widened by the host form, as score_batch does
    if types == "f32/f32":
        w = gpu.centroid_spectra(mz, it.astype(np.float64), off, cc.P)
        assert w[0].dtype == np.float64 and w[2].tobytes() == ru.centroid(mz, it, off, cc.P)[2].tobytes()
    r = gpu.centroid_spectra(mz[:0], it[:0], [0, 0, 0], cc.P)
    assert r[2].tolist() == [0, 0, 0] and r[3] == (0, None)
    assert gpu.centroid_spectra(mz[:0], it[:0], [0], cc.P)[2].tolist() == [0]


def test_a_spectrum_too_long_for_the_scorer_comes_out_under_its_limit():
    """200 000 points in one spectrum: nothing limits the points of a spectrum; 13 000 peaks come out"""
    gpu = _any_gpu()
    rng = np.random.default_rng(5)
    centres = np.sort(150.0 + 0.15 * np.arange(13_000) + rng.uniform(0.0, 0.04, 13_000))
    prof = cc.profile_of(dict(mz=centres, intensity=rng.uniform(10.0, 1e4, centres.size), peak_off=np.array([0, centres.size])), 0.008, 0.004)
    assert prof["mz"].size > 200_000
    p = ru.centroid_params(0.01, half_width=8)
    want = ru.centroid(prof["mz"], prof["intensity"], prof["peak_off"], p)
    got = gpu.centroid_spectra(prof["mz"], prof["intensity"], prof["peak_off"], p)
    assert got[2].tolist() == [0, 13_000] and got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


# ---- end to end ----

SIGMA, STEP = 0.008, 0.004
RULE = dict(gap=2.5 * STEP, half_width=8)


def _same(got, want, what):
    assert set(got) == set(want), what
    for key in want:
        if isinstance(want[key], np.ndarray):
            assert got[key].dtype == want[key].dtype and got[key].tobytes() == want[key].tobytes(), (what, key)
        else:
            assert got[key] == want[key], (what, key)


def _picked(batch, rule=RULE, select=None):
    mz, it, off, _ = ru.centroid(batch["mz"], batch["intensity"], batch["peak_off"], ru.centroid_params(**rule), select)
    return dict(batch, mz=mz, intensity=it, peak_off=off)


@pytest.fixture(scope="module")
def profile():
    batch, settings = synth.make_batch("cfg2", n_psm=64, seed=5, mz_error=0.05)
    return batch, cc.profile_of(batch, SIGMA, STEP), settings, _gpu(dict(settings, mz_error=0.05))


def test_score_batch_on_profile_spectra(profile):
    clean, prof, settings, gpu = profile
    assert prof["mz"].size > 14 * clean["mz"].size
    before = (prof["mz"].copy(), prof["intensity"].copy(), prof["peak_off"].copy())
    got = gpu.score_batch(prof, centroid=RULE)
    _same(got, gpu.score_batch(_picked(prof)), "private")
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, (prof["mz"], prof["intensity"], prof["peak_off"])))
    assert (got["n_sig"] > 0).all() and (got["best_sig"] == gpu.score_batch(clean)["best_sig"]).mean() >= 0.95
    select = np.arange(64) % 4 != 1
    _same(gpu.score_batch(prof, centroid=dict(RULE, select=select, area=True)), gpu.score_batch(_picked(prof, dict(RULE, area=True), select)),
          "select and area")
    f32 = synth.narrow_batch(prof, np.float64, np.float32)
    _same(gpu.score_batch(f32, centroid=RULE), gpu.score_batch(_picked(f32)), "float64 m/z, float32 intensities")
    for bad in (dict(), dict(RULE, half_width=9), dict(RULE, select=select[:-1]), True):
        with pytest.raises(ValueError):
            gpu.score_batch(prof, centroid=bad)


def test_score_batch_centroids_first_beside_the_other_transforms(profile):
    """centroid= in front of strip= and decharge=, and in front of deisotope=: each equals the restatements applied in that order"""
    clean, prof, settings, gpu = profile
    base = _picked(prof)
    rng = np.random.default_rng(3)
    pm, pz = rng.uniform(400.0, 900.0, 64), rng.integers(2, 4, 64).astype(np.int32)
    strip = dict(tol=0.5, losses=(97.976896,), isotopes=1, mz_lo=150.0)
    s_mz, s_it, s_off, _ = ru.strip(base["mz"], base["intensity"], base["peak_off"], pm, pz, ru.strip_params(**strip))
    d_mz, d_it, d_off, _, _ = ru.decharge(s_mz, s_it, s_off, ru.decharge_params())
    _same(gpu.score_batch(prof, centroid=RULE, strip=dict(strip, precursor_mz=pm, precursor_charge=pz), decharge=True),
          gpu.score_batch(dict(base, mz=d_mz, intensity=d_it, peak_off=d_off)), "centroid, then strip, then decharge")
    i_mz, i_it, i_off, _ = ru.deisotope(base["mz"], base["intensity"], base["peak_off"], ru.deisotope_params())
    _same(gpu.score_batch(prof, centroid=RULE, deisotope=True), gpu.score_batch(dict(base, mz=i_mz, intensity=i_it, peak_off=i_off)),
          "centroid, then deisotope")


def test_a_centroided_batch_is_scored_as_it_is(profile):
    """min_height 0 on spectra whose peaks are further apart than the gap: bit-equal to the plain call"""
    clean, prof, settings, gpu = profile
    gap = 0.5 * float(np.diff(clean["mz"])[np.diff(clean["mz"]) > 0].min())
    _same(gpu.score_batch(clean, centroid=dict(gap=gap, half_width=8)), gpu.score_batch(clean), "pass-through")
