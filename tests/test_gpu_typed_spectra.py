"""Typed spectra on the GPU: float32 m/z and intensity arrays go to the device and through the binning kernels as they are
(pya_score_batch_typed / pya_plan_run_typed).  float32 -> float64 is exact and the kernels widen every value where they load
it, so the yardstick everywhere is the SAME batch with its arrays widened on the host (synth.widen_batch(narrow_batch(b)))
through the float64 entry points: every result must be bit-equal -- for the three type combinations, on every binning kernel
and its hand-over, for shared, chunked, retained, device-resident and tiny batches.  A sample of every batch is also checked
against the reference's own C++ core fed the widened arrays."""
import ctypes as C

import numpy as np
import pytest

import switches
from conftest import checker_kind
from oracle import harness, par_check
from pyascore_amd import _lib, synth
from test_gpu_shared_spectra import _psm, _share, _sizes, _dense_spectrum, _ambiguity

pytestmark = pytest.mark.gpu

KEYS = ("best_score", "best_sig", "n_sig", "ascores", "alt_mask")
TYPES = {"f64_f32": (np.float64, np.float32), "f32_f32": (np.float32, np.float32), "f64_f64": (np.float64, np.float64)}
ROUTE_VARS = ("PYA_DEBUG", "PYA_BIN_SELECT_MIN", "PYA_BIN_SELECT_SCAP", "PYA_CHUNK_MB", "PYA_NO_CHUNKS", "PYA_NO_UPLOAD_THREAD",
              "PYA_NO_TINY", "PYA_WORKSPACE_MB")


def _gpu(settings):
    from pyascore_amd import PyAscore
    return harness.make_scorer(PyAscore, settings)


def _same(got, want, what, keys=KEYS):
    for key in keys:
        assert got[key].shape == want[key].shape, "%s: %s has another shape" % (what, key)
        bad = np.flatnonzero(np.any(np.atleast_2d((got[key] != want[key]).T), axis=0))
        assert bad.size == 0, "%s: %s differs for PSMs %s" % (what, key, bad[:10])


def _against_reference(settings, wide, got, n=32):
    """the first and the last n PSMs of the widened batch through the reference's own C++ core"""
    if wide.get("spec_of") is not None:
        wide = synth.expand_shared_batch(wide)
    total = wide["n_psm"]
    for lo in sorted({0, max(0, total - n)}):
        hi = min(total, lo + n)
        sub = synth.slice_batch(wide, lo, hi)
        sub = {k: (np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v) for k, v in sub.items()}
        want = par_check.score_batch_parallel(settings, sub, got["ascores"].shape[1], kind=checker_kind())
        for key in KEYS:
            assert np.array_equal(got[key][lo:hi], want[key]), "%s differs from the reference for PSMs %d..%d" % (key, lo, hi)


def _typed_equals_widened(gpu, settings, batch, what, types=("f64_f32", "f32_f32", "f64_f64"), reference=True, **kw):
    """every type combination of `batch` through the typed path against its widened form through the float64 entry points"""
    out = {}
    for t in types:
        nb = synth.narrow_batch(batch, *TYPES[t])
        wide = synth.widen_batch(nb)
        want = gpu.score_batch(wide, **kw)
        got = gpu.score_batch(nb, **kw)
        _same(got, want, "%s %s" % (what, t), KEYS + (("status",) if kw.get("skip_invalid") else ()))
        if reference and t != "f64_f64":
            _against_reference(settings, wide, got)
        out[t] = got
    return out


def _ties_below_float32(batch, seed):
    """intensities that differ only below float32 precision inside a window: distinct in float64, EQUAL once narrowed"""
    rng = np.random.default_rng(seed)
    it = batch["intensity"].astype(np.float32).astype(np.float64)
    po = batch["peak_off"]
    for i in range(batch["n_psm"]):
        a, b = int(po[i]), int(po[i + 1])
        for j in range(a, b - 1, 7):                       # neighbours in m/z: almost always in one window
            it[j + 1] = it[j] * (1.0 + 2.0 ** -30 * (1 + rng.integers(0, 8)))
    out = dict(batch, intensity=it)
    assert np.any(np.diff(it) != 0) and np.any(np.diff(it.astype(np.float32)) == 0)
    return out


CASES = {
    "cfg2": lambda: synth.make_batch("cfg2", n_psm=700, seed=701),
    "cfg3": lambda: synth.make_batch("cfg3", n_psm=500, seed=702),
    "cfg4": lambda: synth.make_batch("cfg4", n_psm=260, seed=703),
    "cfg5": lambda: synth.make_batch("cfg5", n_psm=200, seed=704),
    "realistic": lambda: synth.make_realistic(260, seed=705),
    "realistic_plain": lambda: synth.make_realistic(400, seed=706, general=False),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_typed_batches_equal_the_widened_batches(name):
    batch, settings = CASES[name]()
    gpu = _gpu(settings)
    out = _typed_equals_widened(gpu, settings, batch, name)
    assert (out["f32_f32"]["n_sig"] > 0).sum() > batch["n_psm"] // 2            # (scored, not set aside)
    # float64 arrays through the typed path ARE the old path
    _same(out["f64_f64"], gpu.score_batch(batch), name + " float64")


def test_golden_cfg1_batch_typed():
    import os
    from conftest import GOLDEN
    settings, batch, _ = harness.load_case(os.path.join(GOLDEN, "synth_cfg1.npz"))
    _typed_equals_widened(_gpu(settings), settings, batch, "cfg1 golden")


def test_narrowing_creates_ties_inside_a_window():
    """equal intensities are where the tie order of std::nth_element / std::sort decides what is retained: in float32 far more
    intensities tie than in float64 -- the fast kernel hands such spectra to the exact one, which must be launched with the
    same types"""
    base, settings = synth.make_batch("cfg2", n_psm=300, seed=711)
    tied = _ties_below_float32(base, 1)
    gpu = _gpu(settings)
    out = _typed_equals_widened(gpu, settings, tied, "ties below float32")
    assert (out["f32_f32"]["n_sig"] > 0).all()
    real, rs = synth.make_realistic(200, seed=712)
    _typed_equals_widened(_gpu(rs), rs, _ties_below_float32(real, 2), "realistic ties")


def test_every_binning_kernel_reads_typed_spectra(monkeypatch):
    """sparse (bin_fast, both bodies), ~1 570 and ~4 070 peaks (bin_select), more than 8 192 (the global kernel, general
    scoring), equal intensities, equal m/z and unsorted peaks (declined, redone by the exact kernel with the same types), all
    peaks in one window, no windows at all -- then every spectrum through the exact kernel (PYA_DEBUG=128), selection forced on
    every class, selection with too few slots (its hand-over), and all-pairs ranking for every class."""
    for v in ROUTE_VARS:
        monkeypatch.delenv(v, raising=False)
    rng = np.random.default_rng(43)
    base, settings = synth.make_batch("cfg2", n_psm=48, seed=43)
    kinds = [(None, "sorted"), (1570, "sorted"), (4070, "sorted"), (9000, "sorted"), (1570, "counts"), (300, "counts"),
             (400, "shuffled"), (12000, "counts"), (None, "sorted"), (4070, "counts"), (700, "sorted"), (1000, "shuffled")]
    psms = []
    for s, (P, mode) in enumerate(kinds):
        p = _psm(base, 3 * s)
        if P is not None:
            p.update(_dense_spectrum(rng, p, max(P, p["mz"].size + 1), mode))
        psms.append(p)
    dup = _psm(base, 40)                                   # equal m/z (and, narrowed, more of them): sorted, not strictly
    dup["mz"] = np.repeat(dup["mz"][::2], 2)[:dup["mz"].size]
    psms.append(dup)
    one = _psm(base, 41)                                   # every peak in one window
    keep = (one["mz"] > 500.0) & (one["mz"] < 600.0)
    one["mz"], one["intensity"] = one["mz"][keep], one["intensity"][keep]
    assert one["mz"].size > 3
    psms.append(one)
    none = _psm(base, 42)                                  # PYA_PSM_NO_WINDOWS: min == max at a multiple of 100
    none["mz"], none["intensity"] = np.array([500.0, 500.0]), np.array([1.0, 2.0])
    psms.append(none)
    batch = synth.pack_batch(psms)
    gpu = _gpu(settings)
    out = _typed_equals_widened(gpu, settings, batch, "production binning", reference=False, skip_invalid=True)
    assert out["f32_f32"]["status"][-1] == 1 and (out["f32_f32"]["status"][:-1] == 0).all()
    ok = synth.pack_batch(psms[:-1])
    _against_reference(settings, synth.widen_batch(synth.narrow_batch(ok)), {k: out["f32_f32"][k][:-1] for k in KEYS}, n=ok["n_psm"])
    for label, env in (("exact", {"PYA_DEBUG": "128"}), ("select_forced", {"PYA_BIN_SELECT_MIN": "0"}),
                       ("select_overflow", {"PYA_BIN_SELECT_MIN": "0", "PYA_BIN_SELECT_SCAP": "64"}),
                       ("all_pairs", {"PYA_BIN_SELECT_MIN": "1000000"})):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        switches.from_env(gpu)
        for t in ("f64_f32", "f32_f32"):
            _same(gpu.score_batch(synth.narrow_batch(batch, *TYPES[t]), skip_invalid=True), out[t], "%s %s" % (label, t), KEYS + ("status",))
        for k in env:
            monkeypatch.delenv(k)
    switches.from_env(gpu)


@pytest.mark.parametrize("hits", [1, 2, 5, 10])
def test_shared_typed_batches(hits):
    base, settings = synth.make_batch("cfg2", n_psm=240, seed=720 + hits)
    shared = _share(base, [hits] * (240 // hits))
    spare = dict(shared, n_spectra=shared["n_spectra"] + 1,                    # a spectrum nobody uses
                 mz=np.concatenate([shared["mz"], [321.5, 400.25]]), intensity=np.concatenate([shared["intensity"], [3.0, 4.0]]),
                 peak_off=np.concatenate([shared["peak_off"], [shared["peak_off"][-1] + 2]]))
    gpu = _gpu(settings)
    out = _typed_equals_widened(gpu, settings, spare, "%d hits" % hits)
    # ... and against the repeated-spectrum form, typed as well
    ex = synth.expand_shared_batch(synth.narrow_batch(spare))
    assert ex["mz"].dtype == np.float32
    _same(gpu.score_batch(ex), out["f32_f32"], "expanded, typed")
    # a shared batch that is not sorted by spectrum is reordered with its typed arrays
    perm = np.random.default_rng(hits).permutation(spare["n_psm"])
    shuffled = synth.take_psms(synth.narrow_batch(spare), perm)
    got = gpu.score_batch(shuffled)
    for key in KEYS:
        assert np.array_equal(got[key], out["f32_f32"][key][perm]), key


def _chunks(gpu):
    return int(gpu._lib.pya_debug_last_chunks(gpu._h))


def test_chunked_and_pipelined_typed_calls(monkeypatch):
    """the upload ring, the upload thread's buffer and the cuts count the arrays' real bytes: a typed call is cut into no more
    chunks than the widened one for the same budget, and results do not depend on the cut"""
    for v in ROUTE_VARS:
        monkeypatch.delenv(v, raising=False)
    desc = synth.describe("cfg2", 9000, seed=33)
    base, settings = synth.make_slice(desc), desc["settings"]
    assert base["mz"].size * 16 > (32 << 20) > base["mz"].size * 8            # (chunked as float64, one plan as float32)
    gpu = _gpu(settings)
    wide32 = synth.widen_batch(synth.narrow_batch(base))
    monkeypatch.setenv("PYA_NO_CHUNKS", "1")
    switches.from_env(gpu)
    one = gpu.score_batch(wide32)
    assert _chunks(gpu) == 1
    for t in ("f64_f32", "f32_f32"):                                           # one plan, upload thread on ...
        nb = synth.narrow_batch(base, *TYPES[t])
        want = one if t == "f32_f32" else gpu.score_batch(synth.widen_batch(nb))
        _same(gpu.score_batch(nb), want, "one plan " + t)
        monkeypatch.setenv("PYA_NO_UPLOAD_THREAD", "1")                        # ... and off
        switches.from_env(gpu)
        _same(gpu.score_batch(nb), want, "one plan, no upload thread " + t)
        monkeypatch.delenv("PYA_NO_UPLOAD_THREAD")
        switches.from_env(gpu)
    monkeypatch.delenv("PYA_NO_CHUNKS")
    switches.from_env(gpu)
    _against_reference(settings, wide32, one)
    # (12 bytes per peak: above the 32 MB from which a call is pipelined; 8 bytes per peak: below, one plan whatever the target)
    nb12, nb8 = synth.narrow_batch(base, np.float64, np.float32), synth.narrow_batch(base)
    wide12 = synth.widen_batch(nb12)
    for label, env, budget in (("default", {}, 0), ("9 MB chunks", {"PYA_CHUNK_MB": "9"}, 0), ("3 MB chunks", {"PYA_CHUNK_MB": "3"}, 0),
                               ("24 MB budget", {}, 24 << 20)):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        switches.from_env(gpu)
        gpu.set_workspace_budget(budget)
        want12 = gpu.score_batch(wide12)
        n_wide = _chunks(gpu)
        _same(gpu.score_batch(wide32), one, label + " widened")
        assert _chunks(gpu) == n_wide
        _same(gpu.score_batch(nb12), want12, label + " float32 intensities")
        n12 = _chunks(gpu)
        _same(gpu.score_batch(nb8), one, label + " float32")
        n8 = _chunks(gpu)
        assert 1 <= n8 <= n12 <= n_wide, (label, n8, n12, n_wide)
        if label != "default":
            assert 1 < n12 < n_wide, (label, n12, n_wide)
        for k in env:
            monkeypatch.delenv(k)
    gpu.set_workspace_budget(0)
    switches.from_env(gpu)


def test_a_shared_group_cut_by_a_chunk_border_typed(monkeypatch):
    for v in ROUTE_VARS:
        monkeypatch.delenv(v, raising=False)
    desc = synth.describe("cfg2", 9000, seed=35)
    base, settings = synth.make_slice(desc), desc["settings"]
    sizes = _sizes(9000, seed=9, big=12000)
    rng = np.random.default_rng(6)
    pick = rng.integers(0, base["n_psm"], sum(sizes))
    shared = synth.take_psms(dict(base, spec_of=np.arange(9000, dtype=np.uint32), n_spectra=9000), pick)
    shared["spec_of"] = np.repeat(np.arange(9000), sizes).astype(np.uint32)
    nb = synth.narrow_batch(shared, np.float64, np.float32)
    assert nb["mz"].size * 12 > (32 << 20)                                     # (pipelined at 12 bytes per peak too)
    gpu = _gpu(settings)
    monkeypatch.setenv("PYA_NO_CHUNKS", "1")
    switches.from_env(gpu)
    one = gpu.score_batch(synth.widen_batch(nb))
    monkeypatch.delenv("PYA_NO_CHUNKS")
    monkeypatch.setenv("PYA_CHUNK_MB", "7")
    switches.from_env(gpu)
    gpu.set_workspace_budget(16 << 20)                                         # the group of 12 000 alone needs more: cut inside it
    _same(gpu.score_batch(nb), one, "typed, 7 MB chunks, 16 MB budget")
    assert _chunks(gpu) > 3
    gpu.set_workspace_budget(0)
    monkeypatch.delenv("PYA_CHUNK_MB")
    switches.from_env(gpu)


def _records_equal(got, want, what):
    assert got.keys() == want.keys()
    for key in want:
        assert np.array_equal(got[key], want[key]), "%s: %s" % (what, key)


def test_retained_records_of_a_typed_batch():
    base, settings = synth.make_batch("cfg3", n_psm=120, seed=741)
    nb, gpu = synth.narrow_batch(base), _gpu(settings)
    wide = synth.widen_batch(nb)
    want_res = gpu.score_batch(wide, keep=True)
    want = gpu.batch_pep_scores()
    psm = int(np.flatnonzero(np.diff(want["rec_off"]) > 1)[0])
    rec_w = gpu.batch_pep_scores(psm, psm + 1)
    want_amb = _ambiguity(gpu, psm, rec_w, 0, 1)
    got_res = gpu.score_batch(nb, keep=True)
    _same(got_res, want_res, "keep")
    _records_equal(gpu.batch_pep_scores(), want, "keep")
    assert _ambiguity(gpu, psm, gpu.batch_pep_scores(psm, psm + 1), 0, 1) == want_amb
    shared = synth.narrow_batch(_share(base, [3] * 40))
    s_want = gpu.score_batch(synth.widen_batch(shared), keep=True)
    rec_want = gpu.batch_pep_scores()
    _same(gpu.score_batch(shared, keep=True), s_want, "keep, shared")
    _records_equal(gpu.batch_pep_scores(), rec_want, "keep, shared")
    # over the budget: scored without the records, which are then re-scored range by range from the TYPED arrays
    gpu.set_workspace_budget(16 << 20)
    big, _ = synth.make_batch("cfg2", n_psm=6000, seed=742)
    nbig = synth.narrow_batch(big, np.float64, np.float32)
    gpu.score_batch(synth.widen_batch(nbig), keep=True)
    assert gpu._lazy_batch is not None
    lazy_want = gpu.batch_pep_scores(5900, 6000)
    gpu.score_batch(nbig, keep=True)
    assert gpu._lazy_batch is not None and gpu._lazy_batch["intensity"].dtype == np.float32
    _records_equal(gpu.batch_pep_scores(5900, 6000), lazy_want, "lazy export")
    gpu.set_workspace_budget(0)


def test_one_plan_runs_float64_then_float32_then_float64():
    import torch
    from pyascore_amd.device import DevicePlan
    base, settings = synth.make_batch("cfg2", n_psm=500, seed=751)
    nb = synth.narrow_batch(base)
    wide = synth.widen_batch(nb)
    gpu = _gpu(settings)
    want = gpu.score_batch(wide)
    dev = torch.device("cuda", gpu.device)
    plan = DevicePlan(gpu, wide)
    ws = plan.workspace_bytes
    t64 = [torch.from_numpy(wide[k]).to(dev) for k in ("mz", "intensity")]
    t32 = [torch.from_numpy(nb[k]).to(dev) for k in ("mz", "intensity")]
    runs = []
    for mz, it in (t64, t32, t64, (t64[0], t32[1])):
        plan.run(mz, it)
        plan.check()
        runs.append({k: getattr(plan, k).cpu().numpy().copy() for k in KEYS})
    for i, r in enumerate(runs):
        r["best_sig"], r["alt_mask"] = r["best_sig"].view(np.uint64), r["alt_mask"].view(np.uint64)
        _same(r, want, "run %d" % i)
    assert plan.workspace_bytes == ws
    fresh = _gpu(settings)
    other = DevicePlan(fresh, nb)                          # (the plan itself knows nothing of the types)
    assert other.workspace_bytes <= DevicePlan(_gpu(settings), wide).workspace_bytes
    for bad in ((t64[0][::2], t64[1][::2]), (t64[0].to(torch.float16), t64[1].to(torch.float16)), (t32[0], t64[1]),
                (t64[0].cpu(), t64[1].cpu())):
        with pytest.raises(ValueError, match="contiguous float64 device tensors"):
            plan.run(*bad)
    plan.close()
    other.close()
    shared = _share(base, [5] * 100)
    snb = synth.narrow_batch(shared, np.float64, np.float32)
    swant = gpu.score_batch(synth.widen_batch(snb))
    splan = DevicePlan(gpu, snb)
    splan.run(torch.from_numpy(snb["mz"]).to(dev), torch.from_numpy(snb["intensity"]).to(dev))
    splan.check()
    got = {k: getattr(splan, k).cpu().numpy().copy() for k in KEYS}
    got["best_sig"], got["alt_mask"] = got["best_sig"].view(np.uint64), got["alt_mask"].view(np.uint64)
    _same(got, swant, "shared plan, typed run")
    splan.close()


@pytest.mark.parametrize("n", [1, 2, 63])
def test_tiny_typed_batches(n):
    base, settings = synth.make_batch("cfg2", n_psm=n, seed=760 + n)
    _typed_equals_widened(_gpu(settings), settings, base, "%d PSMs" % n)


def _raw_typed(gpu, batch, mz_type, it_type, spec_of=None):
    """pya_score_batch_typed as a C caller would call it"""
    n = batch["n_psm"]
    arrs = [np.ascontiguousarray(batch[k]) for k in ("peak_off", "pep", "pep_off", "n_of_mod", "max_charge", "aux_pos", "aux_mass", "aux_off")]
    b = _lib.Batch(n, *[a.ctypes.data_as(C.c_void_p) for a in arrs])
    out = dict(best_score=np.zeros(n, np.float32), best_sig=np.zeros(n, np.uint64), n_sig=np.zeros(n, np.int32),
               ascores=np.zeros((n, 4), np.float32), alt_mask=np.zeros((n, 4), np.uint64))
    r = _lib.Results(4, *[out[k].ctypes.data_as(C.c_void_p) for k in KEYS])
    sp = _lib.TypedSpectra(batch["mz"].ctypes.data_as(C.c_void_p), batch["intensity"].ctypes.data_as(C.c_void_p), mz_type, it_type)
    rc = gpu._lib.pya_score_batch_typed(gpu._h, C.byref(b), None if spec_of is None else spec_of.ctypes.data_as(C.c_void_p),
                                        0 if spec_of is None else int(spec_of.max()) + 1, C.byref(sp), 0, C.byref(r))
    return rc, gpu._lib.pya_last_error(gpu._h).decode(), out


def test_refusals():
    base, settings = synth.make_batch("cfg2", n_psm=8, seed=770)
    gpu = _gpu(settings)
    rc, msg, _ = _raw_typed(gpu, base, 7, 0)
    assert rc == _lib.PYA_ERR_ARG and "spectrum types (7, 0)" in msg
    rc, msg, _ = _raw_typed(gpu, base, 0, 2)
    assert rc == _lib.PYA_ERR_ARG and "spectrum types (0, 2)" in msg
    rc, msg, _ = _raw_typed(gpu, dict(base, mz=base["mz"].astype(np.float32)), _lib.PYA_F32, _lib.PYA_F64)
    assert rc == _lib.PYA_ERR_ARG and "float32 m/z with float64 intensities is not supported" in msg
    rc, msg, got = _raw_typed(gpu, base, _lib.PYA_F64, _lib.PYA_F64)             # (F64, F64) behaves as pya_score_batch
    assert rc == 0
    want = gpu.score_batch(base)
    for k in ("best_score", "best_sig", "n_sig"):
        assert np.array_equal(got[k], want[k])
    # PyAscore.score_batch never sends the refused combination: float32 m/z beside float64 intensities are widened
    mixed = dict(base, mz=base["mz"].astype(np.float32))
    _same(gpu.score_batch(mixed), gpu.score_batch(dict(base, mz=mixed["mz"].astype(np.float64))), "float32 m/z alone")
    # ... and integer intensities are converted to float64, as before
    ints = dict(base, intensity=np.floor(base["intensity"]).astype(np.int64))
    _same(gpu.score_batch(ints), gpu.score_batch(dict(base, intensity=ints["intensity"].astype(np.float64))), "integer intensities")
    # a shared typed call validates spec_of as pya_score_batch_shared does
    nb = synth.narrow_batch(base)
    rc, msg, _ = _raw_typed(gpu, dict(nb, peak_off=nb["peak_off"][:3]), _lib.PYA_F32, _lib.PYA_F32,
                            spec_of=np.array([0, 1, 0, 1, 1, 1, 1, 1], np.uint32))
    assert rc == _lib.PYA_ERR_ARG and msg.startswith("PSM 2: spec_of decreases")


def test_score_still_wants_float64():
    base, settings = synth.make_batch("cfg2", n_psm=2, seed=780)
    gpu = _gpu(settings)
    kw = synth.unpack_psm(base, 0)
    gpu.score(**kw)
    want = gpu.best_score
    for bad in (dict(kw, mz_arr=kw["mz_arr"].astype(np.float32)), dict(kw, int_arr=kw["int_arr"].astype(np.float32))):
        with pytest.raises(ValueError, match="Buffer dtype mismatch"):
            gpu.score(**bad)
    gpu.score(**kw)
    assert gpu.best_score == want
