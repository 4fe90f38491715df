"""Charge deconvolution on the GPU (pya_decharge_params): pya_decharge_spectra against pyascore_amd.rollup.decharge, the numpy
restatement of the header's rule that tests/test_decharge_host.py pins by hand and against an all-pairs form -- every comparison
is on raw bytes --, against pya_deisotope_spectra where the two must agree, the bounds of everything it writes, its refusals,
the host form, and score_batch(decharge=...) / device.decharge against the same calls on arrays the restatement made."""
import ctypes as C

import numpy as np
import pytest

import decharge_cases as cc
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
    """One pya_decharge_spectra call on torch's current stream with canaries around everything it may write: the out arrays
    and the charges are pre-filled, guard words stand behind d_new_off, d_over and the workspace.  ``check()`` waits, looks at the
    canaries and returns (mz, intensity, new_off, charge, over) of the host."""

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
        self.o_chg = to(np.full(self.n + GUARD, 0xEE, np.uint8))
        self.new_off = to(np.full(self.n_spec + 1 + GUARD, -99, np.int64))
        over = np.full(2 + GUARD, 0x5A5A, np.int32)
        over[:2] = 0
        self.over = to(over)
        self.work_bytes = int(self.gpu._lib.pya_decharge_workspace_bytes(self.n_spec, self.n if work_peaks is None else work_peaks))
        assert self.work_bytes % 8 == 0 and self.work_bytes >= 8
        self.work = to(np.full(self.work_bytes // 8 + GUARD, 0x1234567, np.int64))
        self.t_in = _lib.TypedSpectra(self.d_mz.data_ptr(), self.d_it.data_ptr(), _lib.spectrum_type(mz.dtype), _lib.spectrum_type(it.dtype))
        self.t_out = _lib.TypedSpectra(self.o_mz.data_ptr(), self.o_it.data_ptr(), self.t_in.mz_type, self.t_in.intensity_type)

    def run(self, rule, **change):
        a = dict(t_in=C.byref(self.t_in), off=self.d_off.data_ptr(), n_spec=self.n_spec, params=C.byref(ru.decharge_c_params(rule)),
                 work=self.work.data_ptr(), work_bytes=self.work_bytes, t_out=C.byref(self.t_out), new_off=self.new_off.data_ptr(),
                 charge=self.o_chg.data_ptr(), over=self.over.data_ptr())
        a.update(change)
        stream = self.torch.cuda.current_stream(self.dev).cuda_stream
        return self.gpu._lib.pya_decharge_spectra(self.gpu._h, a["t_in"], a["off"], a["n_spec"], a["params"], stream, a["work"], a["work_bytes"],
                                                  a["t_out"], a["new_off"], a["charge"], a["over"])

    def host(self):
        self.torch.cuda.synchronize(self.dev)
        return [t.cpu().numpy() for t in (self.o_mz, self.o_it, self.new_off, self.o_chg, self.over, self.work)]

    def untouched(self):
        o_mz, o_it, new_off, chg, over, work = self.host()
        return (o_mz == -7.0).all() and (o_it == -7.0).all() and (new_off == -99).all() and (chg == 0xEE).all() and \
            over.tolist() == [0, 0] + [0x5A5A] * GUARD and (work == 0x1234567).all()

    def check(self, charges=True):
        o_mz, o_it, new_off, chg, over, work = self.host()
        assert (new_off[self.n_spec + 1:] == -99).all(), "guard behind d_new_off"
        assert over[2:].tolist() == [0x5A5A] * GUARD, "guard behind d_over"
        assert (work[self.work_bytes // 8:] == 0x1234567).all(), "guard behind the workspace"
        kept = int(new_off[self.n_spec])
        assert 0 <= kept <= self.n
        assert (o_mz[kept:] == -7.0).all() and (o_it[kept:] == -7.0).all(), "out elements from new_off[n] on"
        assert (chg[kept if charges else 0:] == 0xEE).all(), "charges from new_off[n] on"
        assert self.d_mz.cpu().numpy().tobytes() == self.mz.tobytes() and self.d_it.cpu().numpy().tobytes() == self.it.tobytes()
        return o_mz[:kept], o_it[:kept], new_off[:self.n_spec + 1], chg[:kept], over[:2].view(np.uint32)


def _equals_restatement(mz, it, off, params, what):
    call = _Call(mz, it, off)
    assert call.run(params) == 0, call.gpu._lib.pya_last_error(call.gpu._h)
    g_mz, g_it, g_off, g_chg, g_over = call.check()
    w_mz, w_it, w_off, w_chg, keep = ru.decharge(mz, it, off, params)
    assert g_off.tobytes() == w_off.tobytes(), what
    assert g_chg.tobytes() == w_chg.tobytes(), what
    assert g_mz.dtype == mz.dtype and g_mz.tobytes() == w_mz.tobytes(), what
    assert g_it.dtype == it.dtype and g_it.tobytes() == w_it.tobytes(), what
    return keep, w_chg, w_off, g_over


# ---- the kernels against the restatement ----

@pytest.mark.parametrize("types", sorted(TYPES))
def test_stride_and_ballot_boundaries(types):
    """spectra of 0, 1, 2, 63, 64, 65, 127, 128, 129 and 4 097 peaks: deisotope's ladders, then the ladders with half of the
    steps S / 2 or S / 3 (moved peaks cross 64-peak strides in MARK and in PLACE), a spectrum whose every kept peak moves and
    one where none does"""
    mz_t, it_t = TYPES[types]
    spectra = dc.boundary_spectra() + cc.charged_boundary_spectra() + [cc.all_moved_spectrum(), cc.none_moved_spectrum()]
    mz, it, off = cc.pack(spectra, mz_t, it_t, gaps=False)
    n = len(dc.BOUNDARY_LENGTHS)
    assert np.diff(off).tolist() == list(dc.BOUNDARY_LENGTHS) * 2 + [300, 300]
    keep, chg, new_off, over = _equals_restatement(mz, it, off, cc.P0, types)
    assert over.tolist() == [0, 0]
    big = chg[new_off[n + 9]:new_off[n + 10]]                             # the 4 097-peak ladder of the charged variant
    assert 0.1 < (big > 1).mean() < 0.9 and big.size > 1000
    moved_at = np.flatnonzero(big > 1)
    assert np.unique(moved_at // 64).size > 10                            # moved peaks land in many strides of the output
    assert (chg[new_off[2 * n]:new_off[2 * n + 1]] == 2).all() and new_off[2 * n + 1] - new_off[2 * n] == 150
    assert (chg[new_off[2 * n + 1]:new_off[2 * n + 2]] == 1).all() and new_off[2 * n + 2] - new_off[2 * n + 1] == 150


@pytest.mark.parametrize("types", sorted(TYPES))
def test_hand_made_spectra(types):
    """every case of tests/decharge_cases.py, the cases of one parameter set in one call with empty spectra between them"""
    mz_t, it_t = TYPES[types]
    groups = {}
    for c in cc.hand_cases():
        if c["params"] is cc.P_HUGE and mz_t == np.float32 and c["mz"].dtype == np.float64:
            continue
        groups.setdefault((cc.params_key(c["params"]), c["mz"].dtype.name), []).append(c)
    assert len(groups) >= 6
    for group in groups.values():
        native = group[0]["mz"].dtype == mz_t and it_t == mz_t
        mz, it, off = cc.pack([(c["mz"], c["intensity"]) for c in group], mz_t, it_t, gaps=True)
        keep, chg, new_off, over = _equals_restatement(mz, it, off, group[0]["params"], (types, group[0]["name"]))
        if native:                                                         # (the case as written: the hand-made outcome holds)
            assert keep.tolist() == np.concatenate([c["keep"] for c in group]).tolist()
            assert chg.tolist() == np.concatenate([c["charge"] for c in group]).tolist()
            bad = [2 * i for i, c in enumerate(group) if c["unordered"]]
            assert over.tolist() == ([len(bad), 0xFFFFFFFF - bad[0]] if bad else [0, 0])


@pytest.mark.parametrize("types", sorted(TYPES))
def test_dense_psms(types):
    mz_t, it_t = TYPES[types]
    batch, _ = dc.dense_batch()
    keep, chg, _, over = _equals_restatement(batch["mz"].astype(mz_t), batch["intensity"].astype(it_t), batch["peak_off"], cc.P0, types)
    assert over.tolist() == [0, 0] and 0.25 < keep.mean() < 0.6 and (chg > 1).any()


@pytest.mark.parametrize("types", sorted(TYPES))
def test_max_charge_1_equals_pya_deisotope_spectra(types):
    """device against device: with one charge there is nothing to move, and the bytes are deisotoping's"""
    import torch
    from pyascore_amd import device
    mz_t, it_t = TYPES[types]
    gpu = _any_gpu()
    dev = torch.device("cuda", gpu.device)
    mz, it, off = cc.pack(cc.charged_boundary_spectra(seed=4), mz_t, it_t, gaps=False)
    d_mz, d_it = torch.from_numpy(mz).to(dev), torch.from_numpy(it).to(dev)
    a_mz, a_it, a_off, a_chg, a_over = device.decharge(gpu, d_mz, d_it, off, ru.decharge_params(max_charge=1))
    b_mz, b_it, b_off, b_over = device.deisotope(gpu, d_mz, d_it, off, ru.deisotope_params(max_charge=1))
    kept = int(b_off.cpu().numpy()[-1])
    assert 0 < kept < mz.size and a_off.cpu().numpy().tobytes() == b_off.cpu().numpy().tobytes()
    assert a_mz.cpu().numpy()[:kept].tobytes() == b_mz.cpu().numpy()[:kept].tobytes()
    assert a_it.cpu().numpy()[:kept].tobytes() == b_it.cpu().numpy()[:kept].tobytes()
    assert (a_chg.cpu().numpy()[:kept] == 1).all() and a_over.cpu().numpy().tolist() == b_over.cpu().numpy().tolist() == [0, 0]
    # and with three charges the offsets are still deisotoping's
    c_off = device.decharge(gpu, d_mz, d_it, off, cc.P0)[2].cpu().numpy()
    assert c_off.tobytes() == device.deisotope(gpu, d_mz, d_it, off, dc.P0)[2].cpu().numpy().tobytes()


def test_more_spectra_than_wavefronts_and_scan_tiles():
    """9 000 small spectra: the grid strides over them (8 192 wavefronts) and the offset scan has 9 tiles; the other parameter
    sets on the first 700 of them"""
    rng = np.random.default_rng(21)
    spectra = []
    for n in rng.integers(0, 9, 9_000):
        kind = rng.integers(0, 4, size=n)
        spectra.append((100.0 + np.cumsum(np.choose(kind, [dc.S, dc.S / 2, 0.7313, dc.S / 3])), rng.choice([1.0, 2.0, 3.0], size=n)))
    mz, it, off = cc.pack(spectra, np.float64, np.float32, gaps=False)
    keep, chg, _, over = _equals_restatement(mz, it, off, cc.P0, "9 000 spectra")
    assert over.tolist() == [0, 0] and not keep.all() and (chg == 2).any() and (chg == 3).any()
    for p in (ru.decharge_params(witness=0.0), ru.decharge_params(ratio=0.5, witness=0.5), ru.decharge_params(max_charge=8, tol=0.002),
              ru.decharge_params(carrier=1.00728, ratio_per_mz=0.001)):
        keep, chg, _, over = _equals_restatement(mz[:off[700]], it[:off[700]], off[:701], p, "700 spectra")
        assert over.tolist() == [0, 0] and not keep.all() and (chg > 1).any()


def test_a_descending_spectrum_among_good_ones():
    spectra = cc.charged_boundary_spectra(seed=9)
    s = 5
    x, y = spectra[s]
    x = x.copy()
    x[40] = x[38] - 0.5                                                   # one descending pair inside a 65-peak spectrum
    spectra[s] = (x, y)
    mz, it, off = cc.pack(spectra, gaps=False)
    call = _Call(mz, it, off)
    assert call.run(cc.P0) == 0
    g_mz, g_it, g_off, g_chg, over = call.check()
    w = ru.decharge(mz, it, off, cc.P0)
    assert g_mz.tobytes() == w[0].tobytes() and g_it.tobytes() == w[1].tobytes() and g_off.tobytes() == w[2].tobytes() and g_chg.tobytes() == w[3].tobytes()
    assert over.tolist() == [1, 0xFFFFFFFF - s]
    a, b = int(g_off[s]), int(g_off[s + 1])
    assert b - a == 65 and g_mz[a:b].tobytes() == x.tobytes() and g_it[a:b].tobytes() == y.tobytes() and (g_chg[a:b] == 1).all()
    clean = ru.decharge(*cc.pack(cc.charged_boundary_spectra(seed=9), gaps=False), cc.P0)
    assert clean[2][s + 1] - clean[2][s] < 65                             # (it would have lost peaks)
    assert g_mz[b:].tobytes() == clean[0][clean[2][s + 1]:].tobytes() and g_mz[:a].tobytes() == clean[0][:clean[2][s]].tobytes()
    x2, y2 = spectra[8]
    spectra[8] = (x2[::-1].copy(), y2)
    mz, it, off = cc.pack(spectra, gaps=False)
    over = _equals_restatement(mz, it, off, cc.P0, "two descending")[3]
    assert over.tolist() == [2, 0xFFFFFFFF - s]


def test_a_workspace_for_fewer_peaks_clips_instead_of_writing_past_it():
    """the peak count is on the device: the host cannot refuse, the kernels clip to the peaks the workspace has room for (whole
    groups of 64) and report the spectra that reach beyond them; no canary is touched"""
    mz, it, off = cc.pack(cc.charged_boundary_spectra(), gaps=False)
    call = _Call(mz, it, off, work_peaks=256)
    assert call.run(cc.P0) == 0
    g_mz, g_it, g_off, g_chg, over = call.check()
    cap = 64 * (256 // 64 + 1)                                            # (256 peaks need five groups of 64)
    inside = int(np.searchsorted(off, cap, "right")) - 1                  # spectra that end at or before the cap
    assert inside >= 6
    w_mz, _, w_off, w_chg, _ = ru.decharge(mz, it, off[:inside + 1], cc.P0)
    assert g_off[:inside + 1].tolist() == w_off.tolist() and g_mz[:int(w_off[-1])].tobytes() == w_mz.tobytes()
    assert g_chg[:int(w_off[-1])].tobytes() == w_chg.tobytes()
    assert over[0] >= 1 and 0xFFFFFFFF - int(over[1]) == inside


def test_refusals_launch_nothing():
    mz, it, off = cc.pack(cc.charged_boundary_spectra()[:6], gaps=False)
    call = _Call(mz, it, off)
    lib, h = call.gpu._lib, call.gpu._h
    f32 = _Call(mz.astype(np.float32), it.astype(np.float32), off)
    ok = ru.decharge_params()

    def params(**kw):
        p = ru.decharge_c_params(ok)
        for k, v in kw.items():
            if k == "spacing":
                for i, s in enumerate(v):
                    p.iso.spacing[i] = s
            elif k in ("carrier", "witness"):
                setattr(p, k, v)
            else:
                setattr(p.iso, k, v)
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
        charge_is_out=dict(charge=o.mz), charge_is_in=dict(charge=i.intensity),
        unknown_type=dict(t_in=typed(i.mz, i.intensity, 2, 0), t_out=typed(o.mz, o.intensity, 2, 0)),
        unknown_it_type=dict(t_in=typed(i.mz, i.intensity, 0, 7), t_out=typed(o.mz, o.intensity, 0, 7)),
        mismatched_types=dict(t_out=typed(o.mz, o.intensity, _lib.PYA_F64, _lib.PYA_F32)),
        f32_mz_f64_it=dict(t_in=typed(i.mz, i.intensity, _lib.PYA_F32, _lib.PYA_F64), t_out=typed(o.mz, o.intensity, _lib.PYA_F32, _lib.PYA_F64)),
        small_work=dict(work_bytes=int(lib.pya_decharge_workspace_bytes(call.n_spec, 0)) - 8), no_work=dict(work_bytes=0),
        misaligned_work=dict(work=call.work.data_ptr() + 4),
        too_many=dict(n_spec=0xFFFFFFFF),
        tol_negative=dict(params=params(tol=-0.01)), tol_nan=dict(params=params(tol=nan)), tol_inf=dict(params=params(tol=inf)),
        ratio_nan=dict(params=params(ratio0=nan)), per_mz_inf=dict(params=params(ratio_per_mz=inf)),
        charge_0=dict(params=params(max_charge=0)), charge_9=dict(params=params(max_charge=9)), reserved=dict(params=params(reserved=1)),
        spacing_rising=dict(params=params(spacing=[0.5, 1.0])), spacing_equal=dict(params=params(spacing=[1.0, 1.0])),
        spacing_zero=dict(params=params(spacing=[1.0, 0.5, 0.0])), spacing_nan=dict(params=params(spacing=[nan])),
        spacing_under_2_tol=dict(params=params(tol=0.2)),
        carrier_0=dict(params=params(carrier=0.0)), carrier_negative=dict(params=params(carrier=-1.0)), carrier_nan=dict(params=params(carrier=nan)),
        carrier_inf=dict(params=params(carrier=inf)), witness_negative=dict(params=params(witness=-0.1)), witness_nan=dict(params=params(witness=nan)),
        witness_inf=dict(params=params(witness=inf)),
    )
    for name, change in bad.items():
        assert call.run(ok, **change) == _lib.PYA_ERR_ARG, name
        assert b"pya_decharge_spectra" in lib.pya_last_error(h), (name, lib.pya_last_error(h))
    assert call.untouched()                                               # nothing was launched, nothing was written
    # (the same checks in front of the float32 instantiation and of the host form)
    assert f32.run(ok, work_bytes=0) == _lib.PYA_ERR_ARG and f32.untouched()
    out_mz, out_it, new_off, over = np.zeros_like(mz), np.zeros_like(it), np.zeros(off.size, np.int64), np.zeros(2, np.uint32)
    chg = np.zeros(mz.size, np.uint8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)                           # noqa: E731
    h_in = _lib.TypedSpectra(vp(mz), vp(it), 0, 0)
    h_out = _lib.TypedSpectra(vp(out_mz), vp(out_it), 0, 0)
    host = lambda **kw: lib.pya_decharge_spectra_host(h, kw.get("t_in", C.byref(h_in)), vp(kw.get("off", off)), off.size - 1,   # noqa: E731
                                                      kw.get("params", params()), kw.get("t_out", C.byref(h_out)), vp(new_off), vp(chg), vp(over))
    for name, kw in dict(in_place=dict(t_out=C.byref(h_in)), params=dict(params=params(max_charge=0)), witness=dict(params=params(witness=-1.0)),
                         carrier=dict(params=params(carrier=0.0)), descending=dict(off=off[::-1].copy()), negative=dict(off=off - 1)).items():
        assert host(**kw) == _lib.PYA_ERR_ARG, name
        assert b"pya_decharge_spectra_host" in lib.pya_last_error(h), name
    assert not out_mz.any() and not new_off.any() and not chg.any()
    want = ru.decharge(mz, it, off, ok)
    assert host() == 0 and new_off.tolist() == want[2].tolist() and chg[:want[3].size].tobytes() == want[3].tobytes()
    # a good call still works on the same buffers
    assert call.run(ok) == 0
    assert call.check()[2].tolist() == new_off.tolist()


def test_no_spectra_is_a_no_op_that_writes_the_first_offset():
    e = np.zeros(0)
    call = _Call(e, e, np.zeros(1, np.int64))
    assert call.run(cc.P0, t_in=C.byref(_lib.TypedSpectra(None, None, 0, 0)), t_out=C.byref(_lib.TypedSpectra(None, None, 0, 0)), work=None,
                    work_bytes=0, over=None, off=None, charge=None) == 0
    _, _, new_off, _, over = call.check()
    assert new_off.tolist() == [0] and over.tolist() == [0, 0]
    assert _any_gpu()._lib.pya_decharge_workspace_bytes(0, 0) == 8 * (131 + 3)


def test_without_charges():
    """d_charge = NULL: the same spectra, and the charge array is not written"""
    mz, it, off = cc.pack(cc.charged_boundary_spectra(seed=2), gaps=False)
    call = _Call(mz, it, off)
    assert call.run(cc.P0, charge=None) == 0
    g_mz, g_it, g_off, _, over = call.check(charges=False)
    w = ru.decharge(mz, it, off, cc.P0)
    assert g_mz.tobytes() == w[0].tobytes() and g_it.tobytes() == w[1].tobytes() and g_off.tobytes() == w[2].tobytes() and over.tolist() == [0, 0]


@pytest.mark.parametrize("types", sorted(TYPES))
def test_the_host_form_and_the_torch_form_equal_the_device_form(types):
    import torch
    from pyascore_amd import device
    mz_t, it_t = TYPES[types]
    gpu = _any_gpu()
    spectra = cc.charged_boundary_spectra(seed=3)
    x, y = spectra[4]
    spectra[4] = (x[::-1].copy(), y)                                      # one spectrum that is not ascending
    mz, it, off = cc.pack(spectra, mz_t, it_t, gaps=False)
    want = ru.decharge(mz, it, off, cc.P0)
    h_mz, h_it, h_off, h_chg, h_over = gpu.decharge_spectra(mz, it, off, cc.P0)
    assert h_mz.dtype == mz_t and h_it.dtype == it_t and h_chg.dtype == np.uint8 and h_over == (1, 4)
    assert h_mz.tobytes() == want[0].tobytes() and h_it.tobytes() == want[1].tobytes() and h_off.tobytes() == want[2].tobytes()
    assert h_chg.tobytes() == want[3].tobytes()
    dev = torch.device("cuda", gpu.device)
    d_mz, d_it = torch.from_numpy(mz).to(dev), torch.from_numpy(it).to(dev)
    for peak_off in (off, torch.from_numpy(off).to(dev)):
        o_mz, o_it, d_new, d_chg, d_over = device.decharge(gpu, d_mz, d_it, peak_off, cc.P0)
        new = d_new.cpu().numpy()
        kept = int(new[-1])
        assert new.tobytes() == want[2].tobytes() and d_over.cpu().numpy().view(np.uint32).tolist() == [1, 0xFFFFFFFF - 4]
        assert o_mz.dtype == d_mz.dtype and o_mz.cpu().numpy()[:kept].tobytes() == want[0].tobytes()
        assert o_it.dtype == d_it.dtype and o_it.cpu().numpy()[:kept].tobytes() == want[1].tobytes()
        assert d_chg.dtype == torch.uint8 and d_chg.cpu().numpy()[:kept].tobytes() == want[3].tobytes()
    o_mz, _, _, none, _ = device.decharge(gpu, d_mz, d_it, off, cc.P0, charge=False)
    assert none is None and o_mz.cpu().numpy()[:kept].tobytes() == want[0].tobytes()
    with pytest.raises(ValueError):
        device.decharge(gpu, d_mz, d_it, off, cc.P0, out=(d_mz, d_it))    # not in place
    with pytest.raises(ValueError):
        device.decharge(gpu, d_mz, d_it, off, dict(cc.P0, witness=-1.0))
    if types == "f32/f32":                                                 # widened by the host form, as score_batch does
        w = gpu.decharge_spectra(mz, it.astype(np.float64), off, cc.P0)
        assert w[0].dtype == np.float64 and w[2].tobytes() == want[2].tobytes()
    r = gpu.decharge_spectra(mz[:0], it[:0], [0, 0, 0], cc.P0)             # spectra without any peak
    assert r[2].tolist() == [0, 0, 0] and r[3].size == 0


# ---- end to end ----

def _decharged(batch, params):
    mz, it, off, _, _ = ru.decharge(batch["mz"], batch["intensity"], batch["peak_off"], params)
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
    mz, it, off = cc.pack(parts, batch["mz"].dtype, batch["intensity"].dtype, gaps=False)
    return dict(batch, mz=mz, intensity=it, peak_off=off, spec_of=(np.arange(n) // hits).astype(np.uint32), n_spectra=len(parts))


@pytest.fixture(scope="module")
def charged():
    """120 cfg2 PSMs whose peaks are 2+ or 3+ with probability 0.6, two satellites behind every peak (the host file's batch)"""
    batch, settings = synth.make_batch("cfg2", n_psm=120, seed=5, mz_error=0.05)
    settings = dict(settings, mz_error=0.05)
    return cc.charged(batch, 0.6), settings, _gpu(settings)


def test_score_batch_private_shared_and_typed(charged):
    batch, settings, gpu = charged
    before = (batch["mz"].copy(), batch["intensity"].copy(), batch["peak_off"].copy())
    got = gpu.score_batch(batch, decharge=dict(tol=0.01, max_charge=3, witness=0.3))
    want = gpu.score_batch(_decharged(batch, cc.P0))
    _same(got, want, "private")
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, (batch["mz"], batch["intensity"], batch["peak_off"])))
    plain, deiso = gpu.score_batch(batch), gpu.score_batch(batch, deisotope=True)
    m_got, m_deiso, m_plain = (float(r["best_score"].mean()) for r in (got, deiso, plain))
    assert m_got > m_deiso + 150.0 and m_got > m_plain + 150.0            # deisotoping alone does not find the charged fragments
    _same(gpu.score_batch(batch, decharge=True), want, "decharge=True")
    other = dict(tol=0.004, max_charge=2, ratio=0.7, ratio_per_mz=1e-4, witness=0.1, carrier=1.00728)
    _same(gpu.score_batch(batch, decharge=other), gpu.score_batch(_decharged(batch, ru.decharge_params(**other))), "other parameters")
    shared = _shared(synth.slice_batch(batch, 0, 40))
    _same(gpu.score_batch(shared, decharge=True), gpu.score_batch(_decharged(shared, cc.P0)), "shared")
    f32 = synth.narrow_batch(batch)
    _same(gpu.score_batch(f32, decharge=True), gpu.score_batch(_decharged(f32, cc.P0)), "float32")
    mixed = synth.narrow_batch(batch, np.float64, np.float32)
    _same(gpu.score_batch(mixed, decharge=True), gpu.score_batch(_decharged(mixed, cc.P0)), "float64 m/z, float32 intensities")
    stages = dict(probs=True, mz_profile=dict(n_slots=1), skip_invalid=True)
    _same(gpu.score_batch(batch, decharge=True, **stages), gpu.score_batch(_decharged(batch, cc.P0), **stages), "probs and mz_profile")
    for bad in (dict(decharge=dict(max_charge=9)), dict(decharge=True, deisotope=True),
                dict(decharge=True, recalibrate=dict(calibration=np.zeros(1, ru.MZ_CALIBRATION_DTYPE)))):
        with pytest.raises(ValueError):
            gpu.score_batch(batch, **bad)


def test_device_form_feeds_a_plan(charged):
    """device.decharge -> read the offsets -> DevicePlan(...).run, against the same plan on host-made arrays"""
    import torch
    from pyascore_amd import device
    batch, settings, gpu = charged
    dev = torch.device("cuda", gpu.device)
    d_mz, d_it = torch.from_numpy(batch["mz"]).to(dev), torch.from_numpy(batch["intensity"]).to(dev)
    o_mz, o_it, d_new, d_chg, d_over = device.decharge(gpu, d_mz, d_it, batch["peak_off"], cc.P0)
    new_off = d_new.cpu().numpy()
    want = _decharged(batch, cc.P0)
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


def test_decharged_batch_against_the_reference(charged):
    """the charged batch (share 0.6, 120 PSMs) scored on the device after decharge=, against the reference's own core on the
    arrays the restatement made (the reference sees decharged spectra only through the restatement, which the host file pins)"""
    batch, settings, gpu = charged
    got = gpu.score_batch(batch, decharge=True)
    sub = {k: (np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v) for k, v in _decharged(batch, cc.P0).items()}
    want = par_check.score_batch_parallel(settings, sub, got["ascores"].shape[1], kind=checker_kind())
    for key in KEYS:
        assert np.array_equal(got[key], want[key]), key
