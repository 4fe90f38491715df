"""The marker-ion stage on the GPU (pya_marker_params): pya_marker_spectra against pyascore_amd.rollup.markers, the numpy
restatement of the header's rule that tests/test_markers_host.py pins by hand -- every comparison is on raw bytes --, the bounds
of everything it writes and reads, its refusals, the host form, device.markers, score_batch(markers=...) and --markers."""
import ctypes as C

import numpy as np
import pytest

import deisotope_cases as dc
import markers_cases as mc
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
    """One pya_marker_spectra call on torch's current stream with canaries behind everything it may write: guard records stand
    behind d_markers and d_spectra, guard words behind d_over.  ``check()`` waits, looks at the canaries and at the inputs and
    returns (markers[n_spec, n_targets], spectra[n_spec], over) of the host."""

    def __init__(self, mz, it, off, params, prec_mz=None, prec_z=None, n_spec=None):
        import torch
        self.torch, self.gpu = torch, _any_gpu()
        self.dev = dev = torch.device("cuda", self.gpu.device)
        self.mz, self.it, self.off = mz, it, np.ascontiguousarray(off, np.int64)
        self.n, self.n_spec = mz.size, self.off.size - 1 if n_spec is None else n_spec
        self.rule, self.n_t = params, len(params["value"])
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)             # noqa: E731
        self.d_mz, self.d_it, self.d_off = to(mz), to(it), to(self.off)
        self.d_pm = None if prec_mz is None else to(np.asarray(prec_mz, np.float64))
        self.d_pz = None if prec_z is None else to(np.asarray(prec_z, np.int32))
        self.markers = to(np.full((self.n_spec * self.n_t + GUARD, 24), 0xA5, np.uint8))
        self.spectra = to(np.full((self.n_spec + GUARD, 32), 0xA5, np.uint8))
        over = np.full(2 + GUARD, 0x5A5A, np.int32)
        over[:2] = 0
        self.over = to(over)
        self.t_in = _lib.TypedSpectra(self.d_mz.data_ptr(), self.d_it.data_ptr(), _lib.spectrum_type(mz.dtype), _lib.spectrum_type(it.dtype))

    def run(self, rule=None, **change):
        a = dict(t_in=C.byref(self.t_in), off=self.d_off.data_ptr(), n_spec=self.n_spec, n_peaks=self.n,
                 pm=None if self.d_pm is None else self.d_pm.data_ptr(), pz=None if self.d_pz is None else self.d_pz.data_ptr(),
                 params=C.byref(ru.marker_c_params(self.rule if rule is None else rule)), markers=self.markers.data_ptr(),
                 spectra=self.spectra.data_ptr(), over=self.over.data_ptr())
        a.update(change)
        stream = self.torch.cuda.current_stream(self.dev).cuda_stream
        return self.gpu._lib.pya_marker_spectra(self.gpu._h, a["t_in"], a["off"], a["n_spec"], a["n_peaks"], a["pm"], a["pz"], a["params"], stream,
                                                a["markers"], a["spectra"], a["over"])

    def host(self):
        self.torch.cuda.synchronize(self.dev)
        return [t.cpu().numpy() for t in (self.markers, self.spectra, self.over)]

    def untouched(self):
        markers, spectra, over = self.host()
        return (markers == 0xA5).all() and (spectra == 0xA5).all() and over.tolist() == [0, 0] + [0x5A5A] * GUARD

    def check(self, spectra_written=True, written=True):
        markers, spectra, over = self.host()
        n_rec = self.n_spec * self.n_t if written else 0
        assert (markers[n_rec:] == 0xA5).all(), "guard behind d_markers"
        assert (spectra[self.n_spec if spectra_written and written else 0:] == 0xA5).all(), "guard behind d_spectra"
        assert over[2:].tolist() == [0x5A5A] * GUARD, "guard behind d_over"
        assert self.d_mz.cpu().numpy().tobytes() == self.mz.tobytes() and self.d_it.cpu().numpy().tobytes() == self.it.tobytes()
        assert self.d_off.cpu().numpy().tobytes() == self.off.tobytes()
        rec = np.ascontiguousarray(markers[:n_rec]).view(ru.MARKER_DTYPE).reshape(-1, self.n_t)
        spec = np.ascontiguousarray(spectra[:self.n_spec]).view(ru.MARKER_SPECTRUM_DTYPE).reshape(-1)
        return rec, spec, over[:2].view(np.uint32)


def _equals_restatement(mz, it, off, params, prec_mz, prec_z, what):
    call = _Call(mz, it, off, params, prec_mz, prec_z)
    assert call.run() == 0, call.gpu._lib.pya_last_error(call.gpu._h)
    g_rec, g_spec, g_over = call.check()
    w_rec, w_spec = ru.markers(mz, it, off, params, prec_mz, prec_z)
    assert g_rec.shape == w_rec.shape and g_rec.tobytes() == w_rec.tobytes(), what
    assert g_spec.tobytes() == w_spec.tobytes(), what
    assert g_over.tolist() == [0, 0], what
    return g_rec, g_spec


# ---- the kernel against the restatement ----

@pytest.mark.parametrize("types", sorted(TYPES))
def test_stride_and_ballot_boundaries(types):
    """spectra of 0, 1, 2, 63, 64, 65, 127, 128, 129 and 4 097 peaks in one call, planted peaks as the first and the last peak
    and on both sides of every 64-peak boundary: candidates of one target in one stride and in two, equal ones among them"""
    mz_t, it_t = TYPES[types]
    spectra, planted = mc.boundary_spectra()
    mz, it, off = mc.pack(spectra, mz_t, it_t, gaps=False)
    n = len(spectra)
    assert np.diff(off).tolist() == list(mc.BOUNDARY_LENGTHS)
    rec, spec = _equals_restatement(mz, it, off, mc.P_BASE, np.full(n, mc.BOUNDARY_PREC[0]), np.full(n, mc.BOUNDARY_PREC[1], np.int32), types)
    # (the planted values are sums of powers of two, exact in float32 too: every planted peak is inside, nothing else is)
    assert rec["n_peaks"].sum(axis=1).tolist() == [int(m.sum()) for m in planted]
    assert int(rec["n_peaks"][9].sum()) == 64 + 65 and (rec["n_peaks"][9] > 40).all()      # of 4 097: peaks 63, 127, .. and 0, 64, ..
    assert spec["n_peaks"].tolist() == list(mc.BOUNDARY_LENGTHS) and (spec["hit"][[9, 11]] == 3).all()
    assert (rec["intensity"][9] == 3.0).all()                                               # the largest of the three values, in some stride


@pytest.mark.parametrize("types", sorted(TYPES))
def test_hand_made_spectra(types):
    """every case of tests/markers_cases.py, the cases of one parameter set in one call with empty spectra between them"""
    mz_t, it_t = TYPES[types]
    groups = {}
    for c in mc.hand_cases():
        groups.setdefault(mc.params_key(c["params"]), []).append(c)
    assert len(groups) >= 9
    for group in groups.values():
        mz, it, off, pm, pz = mc.pack_cases(group, mz_t, it_t, gaps=True)
        rec, spec = _equals_restatement(mz, it, off, group[0]["params"], pm, pz, (types, group[0]["name"]))
        if mz_t == np.float64 and it_t == np.float64:                       # (the float32 cases hold the same values widened)
            assert rec[0::2].tobytes() == np.stack([c["markers"] for c in group]).tobytes()
            assert spec[0::2].tobytes() == np.concatenate([c["spectrum"] for c in group]).tobytes()


def _crowded(params, n_peaks, seed):
    """one spectrum whose peaks all lie among the targets of ``params`` (fixed ones at 100 .. 352): every stride has candidates"""
    rng = np.random.default_rng(seed)
    return rng.uniform(96.0, 392.0, size=n_peaks), rng.choice([1.0, 2.0, 2.0, 3.0], size=n_peaks)


def _on_every_target(params, seed):
    """one spectrum with two peaks of every target of ``params`` for the precursor 400.0 / 2: its centre and a step beside it"""
    rng = np.random.default_rng(seed)
    cen, _, _, active = ru.marker_windows(400.0, 2, params)
    assert active.all()
    x = rng.permutation(np.concatenate([cen, cen + mc.D / 2]))
    return x, rng.choice([1.0, 2.0, 2.0, 3.0], size=x.size)


WIDE_64 = ru.check_marker_params(dict(mc.P_64, tol=3.0))                      # windows of 6 on a grid of 4: neighbours overlap
LOSS_0_AND_63 = ru.check_marker_params(dict(tol=mc.TOL, tol_ppm=0.0, value=(32.0,) + tuple(100.0 + 4.0 * k for k in range(62)) + (18.0,),
                                            loss_mask=(1 << 63) | 1))
TARGET_SETS = {
    "1 target": mc.P_FIXED,
    "2 targets, the loss in lane 0": mc.P_LOSS_FIRST,
    # (the kernel takes a stride's m/z span first with more than 8 active targets: 8, and 9 that are 8 without a precursor)
    "8 targets": ru.marker_params(mz=tuple(100.0 + 4.0 * k for k in range(7)), losses=(32.0,), tol=mc.TOL),
    "9 targets": ru.marker_params(mz=tuple(100.0 + 4.0 * k for k in range(8)), losses=(32.0,), tol=mc.TOL),
    "9 overlapping windows": ru.marker_params(mz=tuple(100.0 + 4.0 * k for k in range(8)), losses=(32.0,), tol=3.0),
    "63 targets": ru.marker_params(mz=tuple(100.0 + 4.0 * k for k in range(62)), losses=(32.0,), tol=mc.TOL),
    "64 targets, the loss in lane 63": mc.P_64,
    "64 targets, losses in lanes 0 and 63": LOSS_0_AND_63,
    "64 overlapping windows": WIDE_64,
    "64 overlapping windows in ppm": ru.check_marker_params(dict(mc.P_64, tol=0.5, tol_ppm=9000.0)),
    "only losses": ru.marker_params(losses=(32.0, 18.0, 0.0), tol=mc.TOL),
}


@pytest.mark.parametrize("name", sorted(TARGET_SETS))
def test_target_counts_loss_lanes_and_overlapping_windows(name):
    params = TARGET_SETS[name]
    spectra, pm, pz = mc.tiny_spectra(300, params, seed=len(name))
    spectra[7] = _crowded(params, 333, 1)
    spectra[8] = _on_every_target(params, 2)
    pm[7:9], pz[7:9] = 400.0, 2
    mz, it, off = mc.pack(spectra, np.float64, np.float32, gaps=False)
    rec, spec = _equals_restatement(mz, it, off, params, pm, pz, name)
    n_t = len(params["value"])
    assert rec.shape == (300, n_t) and int(spec["n_active"].max()) == n_t and (spec["hit"] != 0).sum() > 20
    if n_t == 64:
        assert (spec["hit"] >> np.uint64(63)).any() and (spec["n_active"] < 64).any()
    if "overlapping" in name:
        _, lo, hi, _ = ru.marker_windows(400.0, 2, params)
        x = spectra[7][0]
        in_any = int(((lo[None, :] <= x[:, None]) & (x[:, None] <= hi[None, :])).any(axis=1).sum())
        assert int(rec["n_peaks"][7].sum()) > in_any > 20                            # a peak counts for every window it is in
    assert (rec["flags"][8] == 3).all() and (rec["n_peaks"][8] >= 2).all()


def test_all_targets_inactive():
    """only loss targets and no usable precursor anywhere: every record is written, and every one is zero"""
    params = ru.marker_params(losses=(32.0, 18.0), tol=mc.TOL)
    spectra, _ = mc.boundary_spectra()
    mz, it, off = mc.pack(spectra, gaps=False)
    n = len(spectra)
    rec, spec = _equals_restatement(mz, it, off, params, np.full(n, 400.0), np.zeros(n, np.int32), "inactive")
    assert not rec.tobytes().strip(b"\0") and not spec["n_active"].any() and not spec["hit"].any() and spec["tic"][9] > 0.0


def test_more_spectra_than_wavefronts():
    """8 200 spectra of 0 .. 3 peaks: the grid caps at 2 048 workgroups of 4 wavefronts and strides; a hit in spectrum 8 199"""
    params = ru.marker_params(mz=mc.REPORTERS, losses=(mc.LOSS_H3PO4, 18.010565), tol=0.02)
    spectra, pm, pz = mc.tiny_spectra(8_200, params, last_hit=9)
    mz, it, off = mc.pack(spectra, np.float64, np.float32, gaps=False)
    rec, spec = _equals_restatement(mz, it, off, params, pm, pz, "8 200 spectra")
    assert rec[8_199, 9].tolist() == (mc.REPORTERS[9], 7.0, 1, 3) and int(spec["hit"][8_199]) == 1 << 9
    assert (spec["hit"] != 0).sum() > 1000 and set(spec["n_active"].tolist()) == {10, 12}


def _clipped(off, total):
    a, b = off[:-1], off[1:]
    lo = np.clip(a, 0, total)
    hi = np.where(b < lo, lo, np.minimum(b, total))
    return lo, hi, (lo != a) | (hi != b)


def test_clipped_and_descending_offsets():
    """offsets that run past n_peaks, descend or are negative: the kernel clips them as the transforms do, reports the spectra
    in over and reads nothing beyond n_peaks -- the elements behind it hold peaks that every target would pick"""
    rng = np.random.default_rng(4)
    n_peaks, n_behind = 500, 300
    x = rng.uniform(100.0, 1500.0, size=n_peaks + n_behind)
    x[rng.random(x.size) < 0.2] = mc.C
    x[rng.random(x.size) < 0.2] = mc.L
    y = rng.choice([1.0, 2.0, 3.0], size=x.size)
    y[n_peaks:] = 1000.0
    off = np.array([0, 64, 64, 200, 150, 300, -5, 10, 450, 520, 800, 700], np.int64)       # off[-1]: beyond n_peaks too
    n = off.size - 1
    pm, pz = np.full(n, 400.0), np.full(n, 2, np.int32)
    call = _Call(x, y, off, mc.P_BASE, pm, pz)
    assert call.run(n_peaks=n_peaks) == 0
    rec, spec, over = call.check()
    lo, hi, clipped = _clipped(off, min(max(int(off[-1]), 0), n_peaks))
    assert clipped.tolist() == [False, False, False, True, False, True, True, False, True, True, True]
    for s in range(n):
        w_rec, w_spec = ru.markers(x, y, [int(lo[s]), int(hi[s])], mc.P_BASE, pm[s:s + 1], pz[s:s + 1])
        assert rec[s].tobytes() == w_rec[0].tobytes() and spec[s].tobytes() == w_spec[0].tobytes(), s
    assert spec["base_peak"].max() == 3.0 and rec["intensity"].max() == 3.0
    assert over.tolist() == [int(clipped.sum()), 0xFFFFFFFF - 3]
    # n_peaks = 0: every spectrum is empty and every spectrum with an offset that is not 0 is reported
    call = _Call(x, y, off, mc.P_BASE, pm, pz)
    assert call.run(n_peaks=0) == 0
    rec, spec, over = call.check()
    assert not rec["n_peaks"].any() and (rec["flags"] == 1).all() and not spec["n_peaks"].any() and over.tolist() == [n, 0xFFFFFFFF]


def test_optional_arguments():
    spectra, _ = mc.boundary_spectra()
    mz, it, off = mc.pack(spectra, np.float64, np.float32, gaps=False)
    n = len(spectra)
    pm, pz = np.full(n, 400.0), np.full(n, 2, np.int32)
    want = ru.markers(mz, it, off, mc.P_BASE, pm, pz)
    # d_spectra == NULL
    call = _Call(mz, it, off, mc.P_BASE, pm, pz)
    assert call.run(spectra=None) == 0
    rec, _, over = call.check(spectra_written=False)
    assert rec.tobytes() == want[0].tobytes() and over.tolist() == [0, 0]
    # NULL precursors with loss_mask == 0
    call = _Call(mz, it, off, mc.P_FIXED)
    assert call.run() == 0
    rec, spec, _ = call.check()
    w_rec, w_spec = ru.markers(mz, it, off, mc.P_FIXED)
    assert rec.tobytes() == w_rec.tobytes() == want[0][:, :1].tobytes() and spec["tic"].tobytes() == w_spec["tic"].tobytes()
    # ... and their refusal with loss_mask != 0
    for change in (dict(pm=None), dict(pz=None), dict(pm=None, pz=None)):
        call = _Call(mz, it, off, mc.P_BASE, pm, pz)
        assert call.run(**change) == _lib.PYA_ERR_ARG and b"pya_marker_spectra" in call.gpu._lib.pya_last_error(call.gpu._h)
        assert call.untouched()
    # n_spectra == 0 writes nothing, whatever else is NULL
    call = _Call(mz, it, off, mc.P_BASE, pm, pz)
    null = C.byref(_lib.TypedSpectra(None, None, 0, 0))
    assert call.run(n_spec=0, t_in=null, off=None, pm=None, pz=None, markers=None, spectra=None, over=None, n_peaks=0) == 0
    assert call.run(n_spec=0) == 0
    assert call.untouched()


def test_refusals_launch_nothing():
    spectra, _ = mc.boundary_spectra()
    mz, it, off = mc.pack(spectra[:6], gaps=False)
    pm, pz = np.full(6, 400.0), np.full(6, 2, np.int32)
    call = _Call(mz, it, off, mc.P_BASE, pm, pz)
    lib, h = call.gpu._lib, call.gpu._h

    def params(**kw):
        p = ru.marker_c_params(mc.P_BASE)
        for k, v in kw.items():
            if k == "value":
                for i, s in enumerate(v):
                    p.value[i] = s
            else:
                setattr(p, k, v)
        return C.byref(p)

    def typed(mz_ptr, it_ptr, mz_type, it_type):
        return C.byref(_lib.TypedSpectra(mz_ptr, it_ptr, mz_type, it_type))

    i = call.t_in
    nan, inf = float("nan"), float("inf")
    bad = dict(
        null_in=dict(t_in=None), null_off=dict(off=None), null_markers=dict(markers=None), null_over=dict(over=None), null_params=dict(params=None),
        null_prec_mz=dict(pm=None), null_prec_z=dict(pz=None), null_mz=dict(t_in=typed(None, i.intensity, i.mz_type, i.intensity_type)),
        null_it=dict(t_in=typed(i.mz, None, i.mz_type, i.intensity_type)), unknown_type=dict(t_in=typed(i.mz, i.intensity, 2, 0)),
        unknown_it_type=dict(t_in=typed(i.mz, i.intensity, 0, 7)), f32_mz_f64_it=dict(t_in=typed(i.mz, i.intensity, _lib.PYA_F32, _lib.PYA_F64)),
        misaligned_markers=dict(markers=call.markers.data_ptr() + 4), misaligned_spectra=dict(spectra=call.spectra.data_ptr() + 4),
        too_many=dict(n_spec=0xFFFFFFFF),
        tol_negative=dict(params=params(tol=-0.01)), tol_nan=dict(params=params(tol=nan)), tol_inf=dict(params=params(tol=inf)),
        ppm_negative=dict(params=params(tol_ppm=-1.0)), ppm_nan=dict(params=params(tol_ppm=nan)), ppm_inf=dict(params=params(tol_ppm=inf)),
        no_targets=dict(params=params(n_targets=0, loss_mask=0)), n_targets_65=dict(params=params(n_targets=65)),
        mask_beyond=dict(params=params(loss_mask=0b110)), mask_63=dict(params=params(loss_mask=(1 << 63) | 0b10)),
        fixed_zero=dict(params=params(value=[0.0])), fixed_negative=dict(params=params(value=[-1.0])), fixed_nan=dict(params=params(value=[nan])),
        fixed_inf=dict(params=params(value=[inf])), loss_negative=dict(params=params(value=[126.0, -1.0])),
        loss_nan=dict(params=params(value=[126.0, nan])), loss_inf=dict(params=params(value=[126.0, inf])), reserved=dict(params=params(reserved=1)),
    )
    for name, change in bad.items():
        assert call.run(**change) == _lib.PYA_ERR_ARG, name
        assert b"pya_marker_spectra" in lib.pya_last_error(h), (name, lib.pya_last_error(h))
    assert call.untouched()                                               # nothing was launched, nothing was written
    # (a value from n_targets on is not looked at, whatever it holds; a loss of 0.0 is the precursor itself)
    assert call.run(params=params(value=[mc.C, 32.0, nan])) == 0
    first = call.check()
    assert call.run(params=params(value=[mc.C, 0.0])) == 0
    assert (call.check()[0]["flags"][:, 1] & 1).all()
    # (the same checks in front of the host form)
    rec, spec, over = np.zeros((6, 2), ru.MARKER_DTYPE), np.zeros(6, ru.MARKER_SPECTRUM_DTYPE), np.zeros(2, np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)                           # noqa: E731
    h_in = _lib.TypedSpectra(vp(mz), vp(it), 0, 0)
    host = lambda **kw: lib.pya_marker_spectra_host(h, kw.get("t_in", C.byref(h_in)), vp(kw.get("off", off)), off.size - 1,   # noqa: E731
                                                    kw.get("pm", vp(pm)), vp(pz), kw.get("params", params()), vp(rec), vp(spec), vp(over))
    for name, kw in dict(types=dict(t_in=typed(vp(mz), vp(it), _lib.PYA_F32, _lib.PYA_F64)), params=dict(params=params(n_targets=65)),
                         descending=dict(off=off[::-1].copy()), negative=dict(off=off - 1), null_prec=dict(pm=None)).items():
        assert host(**kw) == _lib.PYA_ERR_ARG, name
        assert b"pya_marker_spectra_host" in lib.pya_last_error(h), name
    assert not rec["flags"].any() and not spec["n_active"].any()
    want = ru.markers(mz, it, off, mc.P_BASE, pm, pz)
    assert host() == 0 and rec.tobytes() == want[0].tobytes() == first[0].tobytes() and spec.tobytes() == want[1].tobytes()
    assert over.tolist() == [0, 0]


@pytest.mark.parametrize("types", sorted(TYPES))
def test_the_host_form_and_the_torch_form_equal_the_device_form(types):
    import torch
    from pyascore_amd import device
    mz_t, it_t = TYPES[types]
    gpu = _any_gpu()
    params = ru.marker_params(mz=mc.REPORTERS, losses=(mc.LOSS_H3PO4, 18.010565), tol=0.02, tol_ppm=20.0)
    spectra, pm, pz = mc.tiny_spectra(300, params, seed=3)
    spectra[4] = mc.boundary_spectra(seed=3)[0][9]                         # one long spectrum among them
    mz, it, off = mc.pack(spectra, mz_t, it_t, gaps=False)
    want = ru.markers(mz, it, off, params, pm, pz)
    call = _Call(mz, it, off, params, pm, pz)
    assert call.run() == 0
    c_rec, c_spec, _ = call.check()
    assert c_rec.tobytes() == want[0].tobytes() and c_spec.tobytes() == want[1].tobytes()
    h_rec, h_spec, h_over = gpu.marker_spectra(mz, it, off, params, pm, pz)
    assert h_rec.dtype == ru.MARKER_DTYPE and h_rec.shape == (300, 12) and h_spec.dtype == ru.MARKER_SPECTRUM_DTYPE and h_over == (0, None)
    assert h_rec.tobytes() == want[0].tobytes() and h_spec.tobytes() == want[1].tobytes() and (h_spec["hit"] != 0).any()
    dev = torch.device("cuda", gpu.device)
    d_mz, d_it = torch.from_numpy(mz).to(dev), torch.from_numpy(it).to(dev)
    before = (d_mz.clone(), d_it.clone())
    for peak_off, prec in ((off, (pm, pz)), (torch.from_numpy(off).to(dev), (torch.from_numpy(pm).to(dev), torch.from_numpy(pz).to(dev)))):
        d_rec, d_spec, d_over = device.markers(gpu, d_mz, d_it, peak_off, params, prec[0], prec[1])
        assert d_rec.dtype == torch.uint8 and tuple(d_rec.shape) == (300, 12, 24) and tuple(d_spec.shape) == (300, 32)
        assert device.marker_records(d_rec.cpu().numpy()).tobytes() == want[0].tobytes()
        assert device.marker_spectrum_records(d_spec.cpu().numpy()).tobytes() == want[1].tobytes()
        assert d_over.cpu().numpy().tolist() == [0, 0]
        again = device.markers(gpu, d_mz, d_it, peak_off, params, prec[0], prec[1], out=(d_rec.zero_(), d_spec.zero_()))
        assert again[0] is d_rec and device.marker_records(d_rec.cpu().numpy()).tobytes() == want[0].tobytes()
    assert torch.equal(d_mz, before[0]) and torch.equal(d_it, before[1])   # read-only
    fixed = ru.marker_params(mz=mc.REPORTERS, tol=0.02)
    d_rec, _, _ = device.markers(gpu, d_mz, d_it, off, fixed)              # no loss target: no precursors
    assert device.marker_records(d_rec.cpu().numpy()).tobytes() == ru.markers(mz, it, off, fixed)[0].tobytes()
    for bad in (dict(params=params), dict(params=params, d_prec_mz=pm), dict(params=dict(params, tol=-1.0), d_prec_mz=pm, d_prec_z=pz),
                dict(params=params, d_prec_mz=pm[:-1], d_prec_z=pz[:-1]), dict(params=fixed, out=(d_rec, d_rec))):
        with pytest.raises(ValueError):
            device.markers(gpu, d_mz, d_it, off, **bad)
    # float32 m/z beside float64 intensities is widened by the host form, as score_batch does
    if types == "f32/f32":
        w = gpu.marker_spectra(mz, it.astype(np.float64), off, params, pm, pz)
        assert w[0].tobytes() == want[0].tobytes()
    # spectra without any peak still have targets; no spectra at all is no call
    r = gpu.marker_spectra(mz[:0], it[:0], [0, 0, 0], mc.P_BASE, [400.0, 0.0], [2, 0])
    assert r[0]["flags"].tolist() == [[1, 1], [1, 0]] and r[1]["n_active"].tolist() == [2, 1]
    r = gpu.marker_spectra(mz[:0], it[:0], [0], mc.P_BASE, [], np.zeros(0, np.int32))
    assert r[0].shape == (0, 2) and r[1].shape == (0,)
    with pytest.raises(ValueError):
        gpu.marker_spectra(mz, it, off, params)                            # loss targets without precursors


# ---- end to end ----

STRIP = dict(tol=0.5, losses=(97.976896, 18.010565), reduced=True, isotopes=2, mz_lo=150.0)
KEYS = ("best_score", "best_sig", "n_sig", "ascores", "alt_mask")


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


def _same_but_for_markers(got, plain, what):
    assert set(got) == set(plain) | {"markers", "marker_spectra"}, what
    for key in plain:
        if isinstance(plain[key], np.ndarray):
            assert got[key].dtype == plain[key].dtype and got[key].tobytes() == plain[key].tobytes(), (what, key)
        else:
            assert got[key] == plain[key], (what, key)


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
    # targets where the spectra have peaks: the most intense peak of the first three spectra, and two losses
    off = batch["peak_off"]
    fixed = tuple(float(batch["mz"][off[s] + int(np.argmax(batch["intensity"][off[s]:off[s + 1]]))]) for s in range(3))
    return batch, settings, _gpu(settings), pm, pz, dict(mz=fixed, losses=(97.976896, 18.010565), tol=0.4, tol_ppm=10.0)


def test_score_batch_alone_and_shared(dense):
    batch, settings, gpu, pm, pz, rule = dense
    before = (batch["mz"].copy(), batch["intensity"].copy(), batch["peak_off"].copy())
    req = dict(rule, precursor_mz=pm, precursor_charge=pz)
    params = ru.marker_params(**rule)
    stages = dict(probs=True, coverage=True, skip_invalid=True)
    plain = gpu.score_batch(batch, **stages)
    got = gpu.score_batch(batch, markers=req, **stages)
    _same_but_for_markers(got, plain, "private")
    want = ru.markers(batch["mz"], batch["intensity"], batch["peak_off"], params, pm, pz)
    assert got["markers"].tobytes() == want[0].tobytes() and got["marker_spectra"].tobytes() == want[1].tobytes()
    assert got["markers"].shape == (int(batch["n_psm"]), 5) and (got["marker_spectra"]["hit"] != 0).any()
    assert (got["markers"]["flags"][:, 3:] == 0).any() and (got["markers"]["flags"][:, 3:] == 3).any()      # pz[::11] = 0; a loss peak seen
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, (batch["mz"], batch["intensity"], batch["peak_off"])))
    # tol=None is the scorer's mz_error; fixed targets need no precursors
    fixed = dict(mz=rule["mz"])
    got = gpu.score_batch(batch, markers=fixed)
    want = ru.markers(batch["mz"], batch["intensity"], batch["peak_off"], ru.marker_params(mz=rule["mz"], tol=gpu._mz_error))
    assert got["markers"].tobytes() == want[0].tobytes() and got["marker_spectra"].tobytes() == want[1].tobytes()
    # shared spectra: one row per spectrum, not per PSM
    shared = _shared(synth.slice_batch(batch, 0, 40))
    s_pm, s_pz = pm[0:40:5], pz[0:40:5]
    got = gpu.score_batch(shared, markers=dict(rule, precursor_mz=s_pm, precursor_charge=s_pz))
    _same_but_for_markers(got, gpu.score_batch(shared), "shared")
    want = ru.markers(shared["mz"], shared["intensity"], shared["peak_off"], params, s_pm, s_pz)
    assert got["markers"].shape == (8, 5) and got["markers"].tobytes() == want[0].tobytes() and got["marker_spectra"].tobytes() == want[1].tobytes()
    f32 = synth.narrow_batch(batch)
    got = gpu.score_batch(f32, markers=req)
    want = ru.markers(f32["mz"], f32["intensity"], f32["peak_off"], params, pm, pz)
    assert got["markers"].tobytes() == want[0].tobytes() and got["marker_spectra"].tobytes() == want[1].tobytes()
    for bad in (dict(rule), dict(req, window=1), dict(req, precursor_mz=pm[:-1]), dict(req, tol=-1.0), True,
                dict(rule, precursor_mz=pm[:40], precursor_charge=pz[:40])):
        with pytest.raises(ValueError):
            gpu.score_batch(batch, markers=bad)


def test_score_batch_sees_the_spectra_in_front_of_strip_and_behind_centroid(dense):
    batch, settings, gpu, pm, pz, rule = dense
    req = dict(rule, precursor_mz=pm, precursor_charge=pz)
    params = ru.marker_params(**rule)
    strip = dict(STRIP, precursor_mz=pm, precursor_charge=pz)
    # strip= cuts the loss peaks the markers report: the records are those of the spectra in front of it
    plain = gpu.score_batch(batch, strip=strip, deisotope=True)
    got = gpu.score_batch(batch, strip=strip, deisotope=True, markers=req)
    _same_but_for_markers(got, plain, "strip and deisotope")
    want = ru.markers(batch["mz"], batch["intensity"], batch["peak_off"], params, pm, pz)
    assert got["markers"].tobytes() == want[0].tobytes() and got["marker_spectra"].tobytes() == want[1].tobytes()
    s_mz, s_it, s_off, _ = ru.strip(batch["mz"], batch["intensity"], batch["peak_off"], pm, pz, ru.strip_params(**STRIP))
    behind = ru.markers(s_mz, s_it, s_off, params, pm, pz)
    assert not (behind[0]["flags"][:, 3:] & ru.MARKER_PICKED).any() and (want[0]["flags"][:, 3:] & ru.MARKER_PICKED).any()
    # centroid= comes first: the records are those of the centroided spectra
    cen = dict(gap=0.02, half_width=2)
    c_mz, c_it, c_off, _ = ru.centroid(batch["mz"], batch["intensity"], batch["peak_off"], ru.centroid_params(**cen))
    assert c_mz.size < batch["mz"].size
    plain = gpu.score_batch(batch, centroid=cen, strip=strip, decharge=True)
    got = gpu.score_batch(batch, centroid=cen, strip=strip, decharge=True, markers=req)
    _same_but_for_markers(got, plain, "centroid, strip and decharge")
    want = ru.markers(c_mz, c_it, c_off, params, pm, pz)
    assert got["markers"].tobytes() == want[0].tobytes() and got["marker_spectra"].tobytes() == want[1].tobytes()


def test_command_line_file(tmp_path):
    import os
    from pyascore_amd import __main__ as cli, batch_cli, ingest
    data = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ingest")
    out, table = tmp_path / "ascores.tsv", tmp_path / "markers.tsv"
    spec, ident = os.path.join(data, "test_spectra.mzML"), os.path.join(data, "test_psms.pep.xml")
    spectra = ingest.SpectraParser(spec, "mzML", native_precision=True).to_dict()
    psms = sorted(ingest.IdentificationParser(ident, "pepXML").to_list(), key=lambda p: p["scan"])
    picked, scans = batch_cli.select_psms(psms, spectra, "STY", 79.966331, 2, 5)
    # targets the file has peaks at: the base peak of the first picked spectrum, and the phosphate losses
    first = picked[0]
    target = float(first["mz"][int(np.argmax(first["intensity"]))])
    opts = ["--mz_error", "0.05", "--hit_depth", "2"]
    rows = cli.run(cli.parse_args(opts + ["--markers", str(table), "--marker_mz", "%r,216.0426" % target, "--marker_losses", "97.976896,79.966331",
                                          "--marker_tol", "0.02", "--marker_tol_ppm", "10", "--strip_precursor", spec, ident, str(out)]),
                   log=lambda *_: None)
    plain = cli.run(cli.parse_args(opts + ["--strip_precursor", spec, ident, str(tmp_path / "plain.tsv")]), log=lambda *_: None)
    assert rows == plain                                                         # the main table is unchanged
    batch = batch_cli.pack_hits(picked, scans)
    pm, pz = batch_cli.hit_precursors(picked, scans)
    params = ru.marker_params(mz=(target, 216.0426), losses=(97.976896, 79.966331), tol=0.02, tol_ppm=10.0)
    rec, spectrum = ru.markers(batch["mz"], batch["intensity"], batch["peak_off"], params, pm, pz)
    lines = table.read_text().splitlines()
    assert lines[0].split("\t") == list(batch_cli.marker_columns((target, 216.0426), (97.976896, 79.966331))) and len(lines) == 1 + len(picked)
    assert len(lines[0].split("\t")) == 3 + 3 * 4 and (rec["flags"][:, 0] == 3).any()
    for i, line in enumerate(lines[1:]):
        s = i if batch.get("spec_of") is None else int(batch["spec_of"][i])
        want = [str(scans[i])] + batch_cli.marker_fields(rec[s], spectrum[s])
        assert line.split("\t") == want, i
        assert float(want[1]) == spectrum["tic"][s]                              # (repr round-trips)
