"""64-bit addressing on the GPU: real spectra placed where a 32-bit byte offset or a 32-bit element index would wrap
(tests/faroffsets.py has the layouts; tests/test_faroffsets_host.py proves them on the CPU).  Marks: HARNESS = 2^16 (float64:
everything here is also checked by the reference core on a host), M1 = 2^29 (float64: byte offset 2^32), M2 = 2^31 (float32: an
int32 element index wraps), M3 = 2^32 (float32: a uint32 element index wraps).  Every comparison is on bytes; nothing has a
tolerance.

One module-scoped fixture holds the filled device tensors of one mark at a time and frees them before the next mark is filled.
Each test computes the device bytes it needs from the layout before it allocates (faroffsets.Layout.device_bytes; a plan adds its
exact pya_plan_workspace_bytes) and prints them; the cap is faroffsets.CAP_BYTES = 40 GB per test.  The one skip there is: less
free device memory than the test still needs plus one tenth.

What does not fit the cap is left out, never shrunk:
  * a plan over the M3 layout.  A plan keeps an 8-byte retained entry for every raw peak of its spectra, so its workspace is
    34.4 GB beside the 34.4 GB of the two float32 arrays.  The resident plan and its stages run at HARNESS, M1 and M2 (at M2 the
    retained entries pass byte offset 2^34 and element 2^31); M3 is reached by the transforms and the recalibration only.
  * far output at M3 (four arrays of 17.2 GB) and the out-of-place recalibration at M3 (three): recalibrate runs in place there.
  * device.decharge beyond HARNESS: its workspace is 16.4 bytes per peak of peak_off[n_spectra] -- 8.8 GB at M1 (25 GB with the two
    float64 arrays and full-size outputs the wrapper makes), 35 GB at M2 before the 17.2 GB of input arrays.

The far-input tests read the fixture's tensors with offsets that begin at the straddler, just below the mark: everything in
front of peak_off[0] is never touched by the call, and the outputs are sized by the spectra, not by the arrays (the C ABI is
called directly where a wrapper would allocate outputs of the input's capacity)."""
import ctypes as C
import resource
import time

import numpy as np
import pytest

import faroffsets as fo
from conftest import checker_kind
from oracle import harness, orc
from pyascore_amd import _lib, rollup as ru, synth

pytestmark = pytest.mark.gpu

KEYS = ("best_score", "best_sig", "n_sig", "ascores", "alt_mask")
STAGES = dict(evidence=True, ions=True, probs=True, mz_profile=True, coverage=True)
P_MZ = ru.mz_profile_params(0.05, ppm_half_width=50.0, band_width=250.0, max_rank=9)
GUARD = 4096
ROUTES = {"lean_localize": {"PYA_NO_FUSED": "1"}, "general_localize": {"PYA_NO_PLAIN": "1"},
          "hash_declines": {"PYA_NO_PLAIN": "1", "PYA_DEBUG": "8192"}}
ROUTE_VARS = ("PYA_NO_PLAIN", "PYA_NO_LOC_HASH", "PYA_HASH_PP", "PYA_NO_NODES", "PYA_NODE_CAP", "PYA_NO_FUSED", "PYA_DEBUG",
              "PYA_NO_BIG_INLINE")


def _gpu(setting):
    from pyascore_amd import PyAscore
    return harness.make_scorer(PyAscore, fo.SETTINGS[setting])


def _dev():
    import torch
    return torch.device("cuda", 0)


# ---- the fixture: one mark resident at a time ----

class Far:
    def __init__(self, lay, d_mz, d_it, fill_s):
        self.lay, self.d_mz, self.d_it, self.fill_s = lay, d_mz, d_it, fill_s
        self.resident = lay.array_bytes()


def _room(far, test, more=0):
    """prints what ``test`` needs on the device at this mark, holds it against the cap, and skips only where the device has
    less free memory than what is still to be allocated plus one tenth"""
    import torch
    lay = far.lay
    need = lay.device_bytes(test) + more
    print("\ndevice bytes %s[%s]: %d (%.2f GB), %d of them resident; the fill took %.2f s" % (
        test, lay.name, need, need / 1e9, far.resident, far.fill_s))
    assert need <= fo.CAP_BYTES, "%s at %s needs %d bytes: over the cap, leave the shape out" % (test, lay.name, need)
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    still = max(0, need - far.resident)
    if free < still + still // 10:
        pytest.skip("%s at %s still needs %d device bytes plus one tenth; %d are free" % (test, lay.name, still, free))


@pytest.fixture(scope="module")
def far(request):
    import torch
    lay = fo.layout(request.param)
    torch.cuda.empty_cache()
    free, need = torch.cuda.mem_get_info()[0], lay.array_bytes()
    if free < need + need // 10:
        pytest.skip("the arrays of %s need %d device bytes plus one tenth; %d are free" % (lay.name, need, free))
    t0 = time.perf_counter()
    d_mz, d_it = fo.fill(lay, _dev())
    torch.cuda.synchronize()
    held = Far(lay, d_mz, d_it, time.perf_counter() - t0)
    del d_mz, d_it
    yield held
    del held.d_mz, held.d_it
    torch.cuda.empty_cache()


ALL = pytest.mark.parametrize("far", ["HARNESS", "M1", "M2", "M3"], indirect=True)
TO_M2 = pytest.mark.parametrize("far", ["HARNESS", "M1", "M2"], indirect=True)
TO_M1 = pytest.mark.parametrize("far", ["HARNESS", "M1"], indirect=True)


# ---- yardsticks, computed once and never changed ----

_wanted = {}


def _reference(lay, setting, which):
    """the reference core on the 39 real PSMs alone (``real``), or on the four filler patterns and the short last filler"""
    key = (lay.mz_dtype.name, lay.last_len, lay.n_filler % 4, setting, which)
    if key not in _wanted:
        batch = lay.alone(lay.real_spectra()[:fo.N_NEAR + 1]) if which == "real" else lay.filler_alone()
        wide = {k: (np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v) for k, v in synth.widen_batch(batch).items()}
        want = harness.make_scorer(orc.OracleAscore, fo.SETTINGS[setting], kind=checker_kind()).score_batch(wide, 3)
        for a in want.values():
            a.setflags(write=False)
        _wanted[key] = want
    return _wanted[key]


def _upload(batch):
    import torch
    return torch.from_numpy(np.ascontiguousarray(batch["mz"])).to(_dev()), torch.from_numpy(np.ascontiguousarray(batch["intensity"])).to(_dev())


def _rows(plan):
    return dict(best_score=plan.best_score.cpu().numpy(), best_sig=plan.best_sig.cpu().numpy().view(np.uint64),
                n_sig=plan.n_sig.cpu().numpy(), ascores=plan.ascores.cpu().numpy(), alt_mask=plan.alt_mask.cpu().numpy().view(np.uint64))


def _same_rows(got, want, k, what, pick=None):
    """the five result arrays, per-site columns up to every PSM's own n_of_mod (a plan leaves the others unwritten)"""
    cols = np.arange(3)[None, :] < np.asarray(k)[:, None]
    for key in KEYS:
        g = got[key] if pick is None else got[key][pick]
        w = want[key]
        if g.ndim == 2:
            width = min(g.shape[1], w.shape[1])
            assert (cols[:, width:] == False).all(), what                                       # noqa: E712
            g, w = (np.where(cols[:, :width], a[:, :width], np.zeros((), a.dtype)) for a in (g, w))
        bad = np.flatnonzero(np.any(np.atleast_2d((g.view(np.uint8).reshape(g.shape[0], -1) != w.view(np.uint8).reshape(w.shape[0], -1)).T),
                                    axis=0))
        assert bad.size == 0, "%s: %s differs for rows %s" % (what, key, bad[:10])


def _run(gpu, batch, d_mz, d_it, **flags):
    from pyascore_amd.device import DevicePlan
    plan = DevicePlan(gpu, batch, **flags)
    plan.run(d_mz, d_it)
    plan.check()
    return plan


def _fillers_on_device(lay, plan, pats, first):
    """the rows of filler j equal those of pattern j mod 4 scored once alone (the short last one: its own), compared on the
    device; ``first``: the row of filler 0"""
    import torch
    n = lay.n_filler
    idx = torch.arange(n, device=_dev()) % 4
    idx[n - 1] = 4
    for name in ("best_score", "best_sig", "n_sig"):
        got, want = getattr(plan, name)[first:first + n], getattr(pats, name)[idx]
        got, want = (got.view(torch.int32), want.view(torch.int32)) if got.dtype == torch.float32 else (got, want)
        assert torch.equal(got, want), name
    assert torch.equal(plan.ascores[first:first + n, :1].contiguous().view(torch.int32), pats.ascores[idx][:, :1].contiguous().view(torch.int32))
    assert torch.equal(plan.alt_mask[first:first + n, :1], pats.alt_mask[idx][:, :1])


def _plan_against_everything(far, gpu, setting, test="plan"):
    """a. the resident plan over the whole layout: every filler spectrum gets the trivial PSM, distance comes from the filler"""
    lay = far.lay
    _room(far, test)
    batch = lay.batch()
    plan = _run(gpu, batch, far.d_mz, far.d_it)
    ws = plan.workspace_bytes
    print("plan workspace %s: %d bytes (estimate %d)" % (lay.name, ws, lay.plan_bytes()))
    assert lay.array_bytes() + ws + lay.n_spectra * 52 <= fo.CAP_BYTES
    real = lay.real_spectra()
    k = batch["n_of_mod"][real]
    got = _rows(plan)
    ref = _reference(lay, setting, "real")
    _same_rows(got, {key: ref[key][lay.real_of[real]] for key in KEYS}, k, "%s %s against the reference core" % (lay.name, setting), real)
    sel = real[fo.N_NEAR:]                                              # the straddler and the far block
    al = lay.alone(real)
    alone = _run(gpu, al, *_upload(al))
    _same_rows(got, _rows(alone), k, "%s %s against the same PSMs alone from offset 0" % (lay.name, setting), real)
    assert sel[0] == lay.straddler and lay.peak_off[sel[1]] >= lay.mark
    fa = lay.filler_alone()
    pats = _run(gpu, fa, *_upload(fa))
    want = _reference(lay, setting, "filler")
    _same_rows(_rows(pats), want, np.ones(5, np.int64), "%s %s filler patterns against the reference core" % (lay.name, setting))
    _fillers_on_device(lay, plan, pats, lay.filler[0])
    for p in (plan, alone, pats):
        p.close()


# ---- a. the resident plan ----

@TO_M2
@pytest.mark.parametrize("setting", ["cfg2", "cfg4"])
def test_resident_plan(far, setting):
    _plan_against_everything(far, _gpu(setting), setting)


@TO_M1
@pytest.mark.parametrize("setting", ["cfg2", "cfg4"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_resident_plan_on_other_routes(far, setting, route, monkeypatch):
    """the same on the routes of tests/test_gpu_parity.py that address spectra and retained tables in kernels of their own"""
    for v in ROUTE_VARS:
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("PYA_PLAIN_MIN", "0")
    monkeypatch.setenv("PYA_NO_TINY", "1")
    for name, value in ROUTES[route].items():
        monkeypatch.setenv(name, value)
    _plan_against_everything(far, _gpu(setting), setting)


def _shared(batch, double, partner):
    """``batch`` (one PSM per spectrum) as a shared batch: every spectrum keeps its PSM, the spectra ``double`` get a second one
    with the peptide of the spectrum ``partner`` names"""
    n = int(batch["n_psm"])
    reps = np.ones(n, np.int64)
    reps[double] = 2
    spec_of = np.repeat(np.arange(n), reps)
    perm = spec_of.copy()
    second = np.flatnonzero(np.concatenate([[False], spec_of[1:] == spec_of[:-1]]))
    perm[second] = partner
    base = dict(batch, spec_of=np.arange(n, dtype=np.uint32), n_spectra=n)
    out = synth.take_psms(base, perm)
    out["spec_of"] = spec_of.astype(np.uint32)
    return out


@TO_M1
@pytest.mark.parametrize("setting", ["cfg2", "cfg4"])
def test_resident_shared_plan(far, setting):
    """pya_plan_create_shared: spec_of over the whole layout, two PSMs per far spectrum (its own and its neighbour's peptide)"""
    lay = far.lay
    _room(far, "plan")
    gpu = _gpu(setting)
    far_specs = np.asarray(lay.far)
    whole = _shared(lay.batch(), far_specs, np.roll(far_specs, -1))
    plan = _run(gpu, whole, far.d_mz, far.d_it)
    assert lay.array_bytes() + plan.workspace_bytes + whole["n_psm"] * 52 <= fo.CAP_BYTES
    sel = np.arange(lay.straddler, lay.n_spectra)
    al = lay.alone(sel)
    local = np.arange(1, sel.size)
    al_shared = _shared(al, local, np.roll(local, -1))
    alone = _run(gpu, al_shared, *_upload(al_shared))
    rows = np.flatnonzero(whole["spec_of"] >= lay.straddler)
    assert rows.size == al_shared["n_psm"] == 1 + 2 * fo.N_NEAR
    k = al_shared["n_of_mod"]
    got = _rows(plan)
    _same_rows(got, _rows(alone), k, "%s %s shared, against the same PSMs alone" % (lay.name, setting), rows)
    wide = synth.widen_batch(synth.expand_shared_batch(al_shared))
    wide = {key: (np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v) for key, v in wide.items()}
    ref = harness.make_scorer(orc.OracleAscore, fo.SETTINGS[setting], kind=checker_kind()).score_batch(wide, 3)
    _same_rows(got, ref, k, "%s %s shared, against the reference core" % (lay.name, setting), rows)
    fa = lay.filler_alone()
    pats = _run(gpu, fa, *_upload(fa))
    _fillers_on_device(lay, plan, pats, lay.filler[0])
    for p in (plan, alone, pats):
        p.close()


# ---- b. the stages behind that plan ----

def _stage_outputs(plan, d_mz, d_it, slots=None):
    import torch
    ev = plan.evidence()
    ion_off, ions = plan.ions()
    site_off, site_probs, psm_probs = plan.probs()
    cov = plan.coverage(d_mz, d_it)
    run = None if slots is None else torch.from_numpy(np.asarray(slots, np.int32)).to(_dev())
    prof = plan.mz_profile(P_MZ, run=run, n_slots=1 if slots is None else int(max(slots)) + 1)
    plan.check()
    return dict(ev=ev, ion_off=ion_off, ions=ions, site_off=site_off, site_probs=site_probs, psm_probs=psm_probs, cov=cov, prof=prof)


@TO_M2
@pytest.mark.parametrize("setting", ["cfg2", "cfg4"])
def test_stages_behind_the_plan(far, setting):
    """coverage strides the raw peaks again; evidence, ions, probs and mz_profile index per-PSM tables over all the PSMs of the
    layout.  The rows of the straddler and the far PSMs equal the rows of the same PSMs run alone (those are pinned to their
    yardsticks by the stages' own tests); the mass-error profile is the sum of the parts, word for word."""
    import torch
    lay = far.lay
    _room(far, "stages")
    gpu = _gpu(setting)
    batch = lay.batch()
    t0 = time.perf_counter()
    plan = _run(gpu, batch, far.d_mz, far.d_it, **STAGES)
    t1 = time.perf_counter()
    got = _stage_outputs(plan, far.d_mz, far.d_it)
    torch.cuda.synchronize()
    print("stages[%s %s]: plan and run %.3f s, the five stages %.3f s, %d ion records" % (lay.name, setting, t1 - t0, time.perf_counter() - t1,
                                                                                     got["ions"].shape[0]))
    assert lay.array_bytes() + plan.workspace_bytes + lay.n_spectra * 400 + got["ions"].numel() <= fo.CAP_BYTES
    s0, n = lay.straddler, lay.n_spectra
    sel = np.arange(s0, n)
    al = lay.alone(sel)
    a_mz, a_it = _upload(al)
    alone = _run(gpu, al, a_mz, a_it, **STAGES)
    want = _stage_outputs(alone, a_mz, a_it)
    k = torch.from_numpy(batch["n_of_mod"][sel].astype(np.int64)).to(_dev())
    cols = (torch.arange(3, device=_dev())[None, :] < k[:, None])[:, :, None]
    assert torch.equal(got["ev"][s0:] * cols, want["ev"] * cols), "evidence"
    off = got["ion_off"]
    assert torch.equal(off[s0:] - off[s0], want["ion_off"]), "ion offsets"
    assert torch.equal(got["ions"][int(off[s0].item()):int(off[n].item())], want["ions"]), "ion records"
    so = got["site_off"]
    assert np.array_equal(so[s0:] - so[s0], want["site_off"])
    assert torch.equal(got["site_probs"][int(so[s0]):].view(torch.int64), want["site_probs"].view(torch.int64)), "site probabilities"
    assert torch.equal(got["psm_probs"][s0:], want["psm_probs"]), "PSM probabilities"
    assert torch.equal(got["cov"][s0:], want["cov"]), "coverage"
    # the profile: (the real PSMs alone) + (fillers of a pattern) x (that pattern's profile) + the short last filler's
    real = lay.real_spectra()
    al_real = lay.alone(real)
    r_mz, r_it = _upload(al_real)
    p_real = _run(gpu, al_real, r_mz, r_it, **STAGES)
    prof_real = _stage_outputs(p_real, r_mz, r_it)["prof"].cpu().numpy().view(np.uint32).astype(np.uint64)
    fa = lay.filler_alone()
    f_mz, f_it = _upload(fa)
    p_fill = _run(gpu, fa, f_mz, f_it, **STAGES)
    prof_fill = _stage_outputs(p_fill, f_mz, f_it, slots=np.arange(5))["prof"].cpu().numpy().view(np.uint32).astype(np.uint64)
    full = lay.n_filler - 1
    count = np.array([(full - p + 3) // 4 for p in range(4)] + [1], np.uint64)
    assert count[:4].sum() == full
    total = prof_real[0] + (prof_fill * count[:, None]).sum(axis=0)
    assert total.max() < 2 ** 32
    got_prof = got["prof"].cpu().numpy().view(np.uint32).astype(np.uint64)[0]
    bad = np.flatnonzero(got_prof != total)
    assert bad.size == 0, "mass-error profile: words %s differ" % bad[:10]
    for p in (plan, alone, p_real, p_fill):
        p.close()


# ---- c. / d. the transforms ----

def _typed(d_mz, d_it):
    return _lib.TypedSpectra(d_mz.data_ptr(), d_it.data_ptr(), _lib.spectrum_type(d_mz.dtype), _lib.spectrum_type(d_it.dtype))


def _raw_transform(gpu, kind, d_mz, d_it, d_off, n_end, out_len, prec=None):
    """pya_{deisotope,strip,centroid}_spectra called directly, with outputs of ``out_len`` elements and GUARD elements of 7.0
    behind them, and a workspace sized for offsets that end at ``n_end``.  Returns (out_mz, out_it, new_off, over, report)."""
    import torch
    dev, lib = _dev(), gpu._lib
    n_spec = d_off.numel() - 1
    sizer = getattr(lib, "pya_%s_workspace_bytes" % kind)
    work = torch.empty((int(sizer(n_spec, n_end)) + 7) // 8, dtype=torch.int64, device=dev)
    o_mz = torch.full((out_len + GUARD,), 7.0, dtype=d_mz.dtype, device=dev)
    o_it = torch.full((out_len + GUARD,), 7.0, dtype=d_it.dtype, device=dev)
    new_off = torch.empty(n_spec + 1, dtype=torch.int64, device=dev)
    over = torch.zeros(2, dtype=torch.int32, device=dev)
    t_in, t_out = _typed(d_mz, d_it), _typed(o_mz, o_it)
    stream = torch.cuda.current_stream(dev).cuda_stream
    report = None
    if kind == "deisotope":
        prm = ru.deisotope_c_params(fo.DEISOTOPE)
        rc = lib.pya_deisotope_spectra(gpu._h, C.byref(t_in), d_off.data_ptr(), n_spec, C.byref(prm), stream, work.data_ptr(), work.numel() * 8,
                                       C.byref(t_out), new_off.data_ptr(), over.data_ptr())
    elif kind == "strip":
        prm = ru.strip_c_params(fo.STRIP)
        d_pm, d_pz = torch.from_numpy(prec[0]).to(dev), torch.from_numpy(prec[1]).to(dev)
        report = torch.empty((n_spec, 16), dtype=torch.uint8, device=dev)
        rc = lib.pya_strip_spectra(gpu._h, C.byref(t_in), d_off.data_ptr(), n_spec, d_pm.data_ptr(), d_pz.data_ptr(), C.byref(prm), stream,
                                   work.data_ptr(), work.numel() * 8, C.byref(t_out), new_off.data_ptr(), report.data_ptr(), over.data_ptr())
    else:
        prm = ru.centroid_c_params(fo.CENTROID)
        rc = lib.pya_centroid_spectra(gpu._h, C.byref(t_in), d_off.data_ptr(), n_spec, None, C.byref(prm), stream, work.data_ptr(),
                                      work.numel() * 8, C.byref(t_out), new_off.data_ptr(), over.data_ptr())
    if rc:
        gpu._raise(rc)
    torch.cuda.synchronize()
    return o_mz, o_it, new_off, over, report


def _restated(kind, mz, it, off, prec=None):
    """(mz, intensity, new_off, report) of pyascore_amd.rollup on host arrays"""
    if kind == "deisotope":
        return ru.deisotope(mz, it, off, fo.DEISOTOPE)[:3] + (None,)
    if kind == "strip":
        return ru.strip(mz, it, off, prec[0], prec[1], fo.STRIP)
    return ru.centroid(mz, it, off, fo.CENTROID)[:3] + (None,)


@ALL
@pytest.mark.parametrize("kind", ["strip", "deisotope", "centroid"])
def test_transform_far_input(far, kind):
    """c. peak_off[0] sits just below the mark: the straddler and the far block go through the device form; outputs, offsets
    and report equal pyascore_amd.rollup on those spectra alone, d_over is zero, nothing is written behind the outputs"""
    import torch
    lay = far.lay
    _room(far, "far_input")
    gpu = _gpu("cfg2")
    sel = np.arange(lay.straddler, lay.n_spectra)
    al = lay.alone(sel)
    prec = lay.precursors(sel)
    w_mz, w_it, w_off, w_rep = _restated(kind, al["mz"], al["intensity"], al["peak_off"], prec)
    d_off = torch.from_numpy(lay.peak_off[lay.straddler:].copy()).to(_dev())
    assert lay.peak_off[lay.straddler] < lay.mark < lay.peak_off[lay.straddler + 1]
    n_in = int(al["peak_off"][-1])
    o_mz, o_it, new_off, over, report = _raw_transform(gpu, kind, far.d_mz, far.d_it, d_off, lay.total, n_in, prec)
    assert np.array_equal(new_off.cpu().numpy(), w_off), kind
    kept = int(w_off[-1])
    assert 0 < kept < n_in
    assert o_mz[:kept].cpu().numpy().tobytes() == w_mz.tobytes() and o_it[:kept].cpu().numpy().tobytes() == w_it.tobytes(), kind
    assert bool((o_mz[n_in:] == 7.0).all()) and bool((o_it[n_in:] == 7.0).all()), "written behind the outputs"
    assert over.cpu().numpy().tolist() == [0, 0]
    if kind == "strip":
        assert report.cpu().numpy().tobytes() == w_rep.tobytes()


@ALL
def test_markers_far_input(far):
    import torch
    from pyascore_amd import device
    lay = far.lay
    _room(far, "far_input")
    gpu = _gpu("cfg2")
    sel = np.arange(lay.straddler, lay.n_spectra)
    al = lay.alone(sel)
    pm, pz = lay.precursors(sel)
    w_rec, w_spec = ru.markers(al["mz"], al["intensity"], al["peak_off"], fo.MARKERS, pm, pz)
    d_off = torch.from_numpy(lay.peak_off[lay.straddler:].copy()).to(_dev())
    d_rec, d_spec, over = device.markers(gpu, far.d_mz, far.d_it, d_off, fo.MARKERS, pm, pz)
    assert d_rec.cpu().numpy().tobytes() == w_rec.tobytes() and d_spec.cpu().numpy().tobytes() == w_spec.tobytes()
    assert over.cpu().numpy().tolist() == [0, 0]


@ALL
def test_recalibrate_far_input(far):
    """DevicePlan.recalibrate on the straddler and the far block: out of place where a third array fits the cap (not at M3),
    and in place at every mark -- the elements in front of peak_off[0] and the corrected spectra are put back afterwards"""
    import torch
    from pyascore_amd.device import DevicePlan
    lay = far.lay
    gpu = _gpu("cfg2")
    plan = DevicePlan(gpu, synth.slice_batch(synth.make_batch("cfg2", n_psm=2, seed=1)[0], 0, 2))
    sel = np.arange(lay.straddler, lay.n_spectra)
    al = lay.alone(sel)
    rng = np.random.default_rng(5)
    cal = np.zeros(3, ru.MZ_CALIBRATION_DTYPE)
    cal["ppm"][0] = fo.CAL_KNOTS
    cal["ppm"][1:] = rng.uniform(-200.0, 200.0, (2, 8))
    run = rng.integers(-1, 3, sel.size).astype(np.int32)
    run[0] = 1                                                          # the straddler is corrected
    want = ru.recalibrate(al["mz"], al["peak_off"], run, cal)
    assert want.tobytes() != al["mz"].tobytes()
    a, b = int(lay.peak_off[lay.straddler]), lay.total
    d_off = torch.from_numpy(lay.peak_off[lay.straddler:].copy()).to(_dev())
    d_cal = torch.from_numpy(cal.view(np.uint8).reshape(3, -1)).to(_dev())
    d_run = torch.from_numpy(run).to(_dev())
    if lay.device_bytes("recalibrate") <= fo.CAP_BYTES:
        _room(far, "recalibrate")
        out = plan.recalibrate(far.d_mz, d_off, d_cal, run=d_run)
        assert out[a:b].cpu().numpy().tobytes() == want.tobytes(), "out of place"
        assert plan.last_recalibrate_over.cpu().numpy().tolist() == [0, 0]
        del out
    else:
        assert lay.name == "M3"
    _room(far, "recalibrate_in_place")
    keep = far.d_mz[a:b].clone()
    before = far.d_mz[a - GUARD:a].clone()
    try:
        assert plan.recalibrate(far.d_mz, d_off, d_cal, run=d_run, out=far.d_mz) is far.d_mz
        assert far.d_mz[a:b].cpu().numpy().tobytes() == want.tobytes(), "in place"
        assert torch.equal(far.d_mz[a - GUARD:a], before), "written in front of peak_off[0]"
        assert plan.last_recalibrate_over.cpu().numpy().tolist() == [0, 0]
    finally:
        far.d_mz[a:b] = keep
    plan.close()


@pytest.mark.parametrize("far", ["HARNESS"], indirect=True)
def test_decharge_far_input_at_the_harness_mark(far):
    """device.decharge at HARNESS only (the module docstring has the sizes of its workspace at the other marks)"""
    import torch
    from pyascore_amd import device
    lay = far.lay
    gpu = _gpu("cfg2")
    sel = np.arange(lay.straddler, lay.n_spectra)
    al = lay.alone(sel)
    w_mz, w_it, w_off, w_charge, _ = ru.decharge(al["mz"], al["intensity"], al["peak_off"], fo.DECHARGE)
    d_off = torch.from_numpy(lay.peak_off[lay.straddler:].copy()).to(_dev())
    o_mz, o_it, new_off, charge, over = device.decharge(gpu, far.d_mz, far.d_it, d_off, fo.DECHARGE)
    kept = int(w_off[-1])
    assert np.array_equal(new_off.cpu().numpy(), w_off)
    assert o_mz[:kept].cpu().numpy().tobytes() == w_mz.tobytes() and o_it[:kept].cpu().numpy().tobytes() == w_it.tobytes()
    assert charge[:kept].cpu().numpy().tobytes() == w_charge.tobytes() and (w_charge > 1).any()
    assert over.cpu().numpy().tolist() == [0, 0]


@TO_M2
@pytest.mark.parametrize("kind", ["strip", "deisotope", "centroid"])
def test_transform_far_output(far, kind):
    """d. the whole layout goes in, so d_new_off itself passes the mark.  The filler is kept unchanged (the filler rules of
    tests/test_faroffsets_host.py), so new_off is known in closed form: the offsets of the input less what the real spectra in
    front lost.  The filler region of the output equals the input's, compared on the device in chunks; the real spectra's
    outputs equal the restatement at new_off; the guard elements behind new_off[n_spectra] keep their fill."""
    import torch
    lay = far.lay
    _room(far, "far_output")
    gpu = _gpu("cfg2")
    real = lay.real_spectra()
    al = lay.alone(real)
    prec_all = lay.precursors()
    w_mz, w_it, w_off, w_rep = _restated(kind, al["mz"], al["intensity"], al["peak_off"], (prec_all[0][real], prec_all[1][real]))
    kept = np.diff(lay.peak_off)
    kept[real] = np.diff(w_off)
    want_off = np.concatenate([[0], np.cumsum(kept)]).astype(np.int64)
    d_off = torch.from_numpy(lay.peak_off).to(_dev())
    o_mz, o_it, new_off, over, report = _raw_transform(gpu, kind, far.d_mz, far.d_it, d_off, lay.total, lay.total, prec_all)
    assert torch.equal(new_off, torch.from_numpy(want_off).to(_dev())), kind
    assert over.cpu().numpy().tolist() == [0, 0]
    f0, f1, end = int(want_off[lay.filler[0]]), int(want_off[lay.straddler]), int(want_off[-1])
    assert f1 - f0 == lay.filler_end - lay.filler_begin and (lay.name == "HARNESS" or f1 > lay.mark - 2 ** 20)
    step = 1 << 27
    for src, dst in ((far.d_mz, o_mz), (far.d_it, o_it)):
        for c in range(0, f1 - f0, step):
            m = min(step, f1 - f0 - c)
            assert torch.equal(dst[f0 + c:f0 + c + m], src[lay.filler_begin + c:lay.filler_begin + c + m]), (kind, "filler", c)
    near_kept = int(w_off[fo.N_NEAR])
    assert f0 == near_kept
    for dst, w in ((o_mz, w_mz), (o_it, w_it)):
        assert dst[:f0].cpu().numpy().tobytes() == w[:near_kept].tobytes(), (kind, "near block")
        assert dst[f1:end].cpu().numpy().tobytes() == w[near_kept:].tobytes(), (kind, "straddler and far block")
        assert bool((dst[end:end + GUARD] == 7.0).all()), (kind, "guard")
    if kind == "strip":
        rep = report.cpu().numpy().view(ru.STRIP_REPORT_DTYPE).reshape(-1)
        assert rep[real].tobytes() == w_rep.tobytes()
        fill = np.arange(lay.filler[0], lay.straddler)
        assert not rep["n_removed"][fill].any() and not rep["n_windows"][fill].any()


# ---- e. host arrays with a far base ----

def _far_host_batch(batch, base):
    """``batch`` with its spectrum arrays behind ``base`` untouched zero elements (np.zeros: the pages of the gap are never
    resident; only the tail is written)"""
    n = int(batch["peak_off"][-1])
    out = dict(batch, peak_off=np.asarray(batch["peak_off"], np.int64) + base)
    for key in ("mz", "intensity"):
        a = np.zeros(base + n, batch[key].dtype)
        a[base:] = batch[key]
        out[key] = a
    return out


@pytest.mark.parametrize("form", ["private", "shared", "typed"])
def test_host_arrays_with_a_far_base(form):
    """e. score_batch on host arrays whose peak_off[0] is 2^29 + 5 (float64: byte offset 2^32) or 2^31 + 5 (float32): results
    equal the same batch rebased to 0, and the call does not copy or convert the gap (peak RSS grows by less than 1 GB over a
    gap of more than 4 GB)"""
    batch, settings = synth.make_batch("cfg2", n_psm=96, seed=fo.SEED + 7)
    if form == "shared":
        spectra = [dict(mz=kw["mz_arr"], intensity=kw["int_arr"]) for kw in (synth.unpack_psm(batch, i) for i in range(32))]
        psms = []
        for i in range(96):
            kw = synth.unpack_psm(batch, i)
            psms.append(dict(spectrum=i // 3, peptide=kw["peptide"], n_of_mod=kw["n_of_mod"], max_charge=kw["max_fragment_charge"]))
        batch = synth.pack_shared_batch(spectra, psms)
    base = 2 ** 29 + 5
    if form == "typed":
        batch, base = synth.narrow_batch(batch), 2 ** 31 + 5
    from pyascore_amd import PyAscore
    gpu = harness.make_scorer(PyAscore, settings)
    want = gpu.score_batch(batch)
    moved = _far_host_batch(batch, base)
    assert moved["mz"].nbytes > 2 ** 32 and moved["peak_off"][0] == base
    before = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    got = gpu.score_batch(moved)
    grown = (resource.getrusage(resource.RUSAGE_SELF).ru_maxrss - before) * 1024
    print("\npeak RSS grew by %d bytes over score_batch[%s] with a gap of %d bytes per array" % (grown, form, base * moved["mz"].itemsize))
    for key in KEYS:
        assert np.array_equal(got[key], want[key]), (form, key)
    assert grown < 10 ** 9, "score_batch copied or converted the gap in front of peak_off[0]"
    wide = synth.widen_batch(synth.expand_shared_batch(batch) if form == "shared" else batch)
    wide = {k: (np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v) for k, v in wide.items()}
    ref = harness.make_scorer(orc.OracleAscore, settings, kind=checker_kind()).score_batch(wide, got["ascores"].shape[1])
    for key in KEYS:
        assert np.array_equal(got[key], ref[key]), (form, key, "reference core")
