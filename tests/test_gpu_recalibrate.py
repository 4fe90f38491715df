"""Fragment m/z recalibration on the GPU (pya_mz_calibration): the fit of a mass-error profile, the correction of m/z arrays on
the device, and the batch path behind PYA_FLAG_RECALIBRATE.  Yardsticks: pyascore_amd.rollup.fit_mz_calibration and
.recalibrate, the numpy restatements of the header's definitions -- every comparison is on raw bytes; a flagged batch is
compared with the same batch scored without the flag on arrays corrected by the restatement."""
import ctypes as C
import os

import numpy as np
import pytest

import switches
from conftest import GOLDEN
from oracle import harness
from pyascore_amd import _lib, rollup as ru, synth

pytestmark = pytest.mark.gpu

KEYS = ("best_score", "best_sig", "n_sig", "ascores", "alt_mask")
DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ingest")
BINS, BANDS, HALF = ru.MZP_BINS, ru.MZP_BANDS, ru.MZP_BINS // 2
P = ru.mz_profile_params(0.05, ppm_half_width=50.0, band_width=250.0, max_rank=9)
KNOTS = [32.0, 28.0, 22.0, 15.0, 9.0, 4.0, 0.0, -3.0]
vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
_scorers = {}


def _gpu(settings):
    from pyascore_amd import PyAscore
    return harness.make_scorer(PyAscore, settings)


def _any_gpu():
    """a scorer for the calls that do not score (one per process)"""
    if "any" not in _scorers:
        _scorers["any"] = _gpu(synth.describe("cfg2", 1, seed=1)["settings"])
    return _scorers["any"]


def _cal(knots=KNOTS, n=1):
    c = np.zeros(n, ru.MZ_CALIBRATION_DTYPE)
    c["ppm"][:] = knots
    return c


def _same_cal(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == ru.MZ_CALIBRATION_DTYPE, what
    a, b = got.view(np.uint32).reshape(got.size, -1), want.view(np.uint32).reshape(want.size, -1)
    bad = np.argwhere(a != b)
    assert bad.size == 0, "%s: %d words differ, first (slot, word) %s: got %s, want %s" % (
        what, len(bad), bad[0].tolist(), got[bad[0][0]], want[bad[0][0]])


def _cparams(p):
    return C.byref(_lib.MzProfileParams(p["inv_da"], p["inv_ppm"], p["inv_band"], p["max_rank"], 0))


# ---- the fit ----

def _hand_made_tables():
    """the tables of tests/test_recalibrate_host.py, one slot each"""
    t = np.zeros(12, ru.MZ_PROFILE_DTYPE)
    t["ppm"][0, 3, 40] = 100                                              # all counts in one bin
    t["ppm"][1, 2, :] = 7                                                 # flat
    t["ppm"][2, 2, [0, 1, BINS - 2, BINS - 1]] = 1000                     # the four edge bins only
    t["ppm"][3, 5, 20] = 19                                               # one below 4 x min_ions
    t["ppm"][4, 5, 20] = 20                                               # exactly at it
    t["ppm"][5, 5, :] = 3                                                 # ... above a floor
    t["ppm"][5, 5, 20] = 23
    t["ppm"][6, 2, 36] = 50                                               # a tie between two fitted neighbours
    t["ppm"][6, 6, 28] = 50
    t["ppm"][7, 0, 30:34] = [10, 30, 40, 20]                              # interpolation inside the bins
    t["ppm"][8, 4, 33:35] = 0xFFFFFFFF                                    # counts near 2^32
    t["ppm"][8, 7, :] = 0xFFFFFFFF
    t["ppm"][9, 0, 0] = 400                                               # the quantiles in the first and in the last bin
    t["ppm"][10, 7, BINS - 1] = 400
    rng = np.random.default_rng(11)
    t["ppm"][11] = rng.poisson(6.0, (BANDS, BINS))                        # noise over a floor, a peak per band
    for b in range(BANDS):
        t["ppm"][11, b, 20 + 3 * b:24 + 3 * b] += rng.integers(30, 400, 4).astype(np.uint32)
    t["da"] = 77                                                          # (what the fit must not read)
    t["n_ions"] = 5
    return t


def test_fit_hand_made_tables_equal_the_restatement():
    gpu = _any_gpu()
    t = _hand_made_tables()
    for min_ions in (1, 20, 21):
        want = ru.fit_mz_calibration(t, P, min_ions=min_ions)
        _same_cal(gpu.fit_mz_calibration(t, P, min_ions=min_ions), want, "min_ions %d" % min_ions)
    want = ru.fit_mz_calibration(t, P)
    assert want["n_signal"][8, 4] == 0xFFFFFFFF and (want["n_signal"][3] < 20).all() and want["n_signal"][4, 5] == 20
    assert want[11]["spread_ppm"].all()
    for s in range(t.size):                                               # slot by slot: the slots are independent
        _same_cal(gpu.fit_mz_calibration(t[s:s + 1], P), want[s:s + 1], "slot %d alone" % s)
    other = ru.mz_profile_params(0.02, ppm_half_width=20.0, band_width=300.0, max_rank=4)
    _same_cal(gpu.fit_mz_calibration(t, other, min_ions=5), ru.fit_mz_calibration(t, other, min_ions=5), "another axis")


@pytest.mark.parametrize("what", ["cfg2", "cfg4", "realistic"])
def test_fit_of_scored_profiles(what):
    """the profile of a scored batch in 1, 3 and 65 slots with an empty one among them (the batch is scored once, with its ion
    records; the tables are the yardstick's over them, which tests/test_gpu_mz_profile.py holds equal to the stage's); the
    device form on device tensors equals the host form and the restatement"""
    import torch
    from pyascore_amd.device import DevicePlan, mz_calibration_records, mz_profile_records
    if what == "realistic":
        batch, settings = synth.make_realistic(40, seed=9210, general=True)
    else:
        batch, settings = synth.make_batch(what, n_psm=64 if what == "cfg2" else 24, seed=9100)
    gpu = _gpu(settings)
    n = int(batch["n_psm"])
    dev = torch.device("cuda", 0)
    plan = DevicePlan(gpu, synth.slice_batch(batch, 0, 2))
    res = gpu.score_batch(batch, ions=True, mz_profile={})
    params = res["mz_profile_params"]
    for n_slots in (1, 3, 65):
        run = None
        if n_slots > 1:
            run = (np.arange(n) * 7 % n_slots).astype(np.int32)
            run[run == 1] = 0                                             # slot 1 stays empty
        table = ru.mz_profile(res["ion_off"], res["ions"], res["n_sig"], run, n_slots, params)
        if n_slots == 1:
            assert table.tobytes() == res["mz_profile"].tobytes()
        assert table["n_ions"].sum() > 0
        for min_ions in (1, 20):
            want = ru.fit_mz_calibration(table, params, min_ions=min_ions)
            _same_cal(gpu.fit_mz_calibration(table, params, min_ions=min_ions), want, "%s, %d slots, host form" % (what, n_slots))
            d_table = torch.from_numpy(table.view(np.uint8).reshape(n_slots, -1)).to(dev)
            d_cal = plan.fit_mz_calibration(d_table, params, min_ions=min_ions)
            _same_cal(mz_calibration_records(d_cal.cpu().numpy()), want, "%s, %d slots, device form" % (what, n_slots))
            assert mz_profile_records(d_table.cpu().numpy()).tobytes() == table.tobytes()      # the table is only read
        if n_slots > 1:
            assert want[1].tobytes() == bytes(128)
        assert (ru.fit_mz_calibration(table, params, min_ions=1)["n_signal"] > 0).any()


def test_fit_refusals_and_the_empty_table():
    import torch
    gpu = _any_gpu()
    lib, h = gpu._lib, gpu._h
    assert gpu.fit_mz_calibration(np.zeros(0, ru.MZ_PROFILE_DTYPE), P).shape == (0,)
    t = _hand_made_tables()[:3]
    out = np.zeros(3, ru.MZ_CALIBRATION_DTYPE)
    dev = torch.device("cuda", 0)
    d_t = torch.from_numpy(t.view(np.uint8).reshape(3, -1)).to(dev)
    d_out = torch.full((3, 128), 0x5A, dtype=torch.uint8, device=dev)
    host = lambda table, n, p, m, o: lib.pya_mz_profile_fit_host(h, vp(table), n, p, m, vp(o))  # noqa: E731
    devc = lambda table, n, p, m, o: lib.pya_mz_profile_fit(h, None if table is None else table.data_ptr(), n, p, m, None,  # noqa: E731
                                                            None if o is None else o.data_ptr())
    assert host(None, 0, _cparams(P), 20, None) == 0 and devc(None, 0, _cparams(P), 20, None) == 0      # n_slots == 0: a no-op
    bads = [dict(P, max_rank=16), dict(P, inv_da=0.0), dict(P, inv_ppm=float("nan")), dict(P, inv_ppm=-1.0), dict(P, inv_band=float("inf"))]
    for bad in bads:
        assert host(t, 3, _cparams(bad), 20, out) == _lib.PYA_ERR_ARG, bad
        assert devc(d_t, 3, _cparams(bad), 20, d_out) == _lib.PYA_ERR_ARG, bad
    for args in ((None, 3, _cparams(P), 20, "out"), ("t", 3, _cparams(P), 20, None), ("t", 3, None, 20, "out"), ("t", 3, _cparams(P), 0, "out"),
                 ("t", 1 << 31, _cparams(P), 20, "out")):
        pick = lambda x, a, b: a if x == "t" else (b if x == "out" else x)  # noqa: E731
        assert host(pick(args[0], t, out), args[1], args[2], args[3], pick(args[4], t, out)) == _lib.PYA_ERR_ARG, args
        assert devc(pick(args[0], d_t, d_out), args[1], args[2], args[3], pick(args[4], d_t, d_out)) == _lib.PYA_ERR_ARG, args
    assert lib.pya_mz_profile_fit(None, d_t.data_ptr(), 3, _cparams(P), 20, None, d_out.data_ptr()) == _lib.PYA_ERR_ARG
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 0x5A).all() and out.tobytes() == bytes(3 * 128)             # nothing was launched
    with pytest.raises(ValueError):
        gpu.fit_mz_calibration(t, P, min_ions=0)


# ---- the apply ----

SIZES = [0, 1, 63, 64, 65, 129, 1000, 0, 5]


def _spectra(dtype, seed=5):
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    mz = np.concatenate([np.sort(rng.uniform(40.0, 2600.0, k)) for k in SIZES]).astype(dtype)
    mz[off[6] + 10:off[6] + 16] = [np.nan, np.inf, 0.0, -0.0, -3.0, -np.inf]                  # (inside the 1 000-peak spectrum)
    return mz, off


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_apply_equals_the_restatement(dtype):
    """spectra of 0, 1, 63, 64, 65, 129 and 1 000 peaks in one call, in place and out of place, run NULL, negative and mixed"""
    import torch
    from pyascore_amd.device import DevicePlan
    gpu = _any_gpu()
    plan = DevicePlan(gpu, synth.slice_batch(synth.make_batch("cfg2", n_psm=2, seed=1)[0], 0, 2))
    dev = torch.device("cuda", 0)
    mz, off = _spectra(dtype)
    n_spec = len(SIZES)
    cal = _cal(n=3)
    cal["ppm"][1] = np.random.default_rng(6).uniform(-1000.0, 1000.0, 8)
    cal["ppm"][2] = 0.0
    d_off, d_cal = torch.from_numpy(off).to(dev), torch.from_numpy(cal.view(np.uint8).reshape(3, -1)).to(dev)
    runs = {"NULL": None, "negative": np.full(n_spec, -1, np.int32), "mixed": np.array([0, 1, -1, 2, 1, 0, 1, 0, -1], np.int32),
            "zero record": np.full(n_spec, 2, np.int32)}
    for name, run in runs.items():
        want = ru.recalibrate(mz, off, run, cal)
        if name in ("negative", "zero record"):
            assert want.tobytes() == mz.tobytes()
        else:
            assert want.tobytes() != mz.tobytes()
        d_run = None if run is None else torch.from_numpy(run).to(dev)
        # out of place, into an array with guard words behind it
        d_mz = torch.from_numpy(mz).to(dev)
        buf = torch.full((mz.size + 64,), 7.0, dtype=d_mz.dtype, device=dev)
        out = plan.recalibrate(d_mz, d_off, d_cal, run=d_run, out=buf[:mz.size])
        host = buf.cpu().numpy()
        assert host[:mz.size].tobytes() == want.tobytes(), (name, "out of place")
        assert (host[mz.size:] == 7.0).all() and d_mz.cpu().numpy().tobytes() == mz.tobytes()
        assert plan.last_recalibrate_over.cpu().numpy().tolist() == [0, 0]
        # in place
        both = torch.full((mz.size + 64,), 7.0, dtype=d_mz.dtype, device=dev)
        both[:mz.size] = d_mz
        view = both[:mz.size]
        assert plan.recalibrate(view, d_off, d_cal, run=d_run, out=view) is view
        host = both.cpu().numpy()
        assert host[:mz.size].tobytes() == want.tobytes(), (name, "in place")
        assert (host[mz.size:] == 7.0).all()
        assert out.dtype == d_mz.dtype
    fresh = plan.recalibrate(torch.from_numpy(mz).to(dev), d_off, d_cal)                       # out=None: a new tensor
    assert fresh.cpu().numpy().tobytes() == ru.recalibrate(mz, off, None, cal).tobytes()
    other = plan.recalibrate(torch.from_numpy(mz).to(dev), d_off, d_cal, band_width=300.0)
    assert other.cpu().numpy().tobytes() == ru.recalibrate(mz, off, None, cal, band_width=300.0).tobytes()


def test_apply_many_spectra_and_a_part_of_an_array():
    """more spectra than the grid has wavefronts; offsets that do not start at 0"""
    import torch
    from pyascore_amd.device import DevicePlan
    gpu = _any_gpu()
    plan = DevicePlan(gpu, synth.slice_batch(synth.make_batch("cfg2", n_psm=2, seed=1)[0], 0, 2))
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(8)
    sizes = rng.integers(0, 9, 20_000)
    off = (3 + np.concatenate([[0], np.cumsum(sizes)])).astype(np.int64)
    mz = rng.uniform(40.0, 2600.0, int(off[-1])).astype(np.float32)
    run = rng.integers(-1, 4, sizes.size).astype(np.int32)
    cal = _cal(n=4)
    cal["ppm"][1:] = rng.uniform(-200.0, 200.0, (3, 8))
    want = ru.recalibrate(mz, off, run, cal)
    assert want[:3].tobytes() == mz[:3].tobytes()
    got = plan.recalibrate(torch.from_numpy(mz).to(dev), torch.from_numpy(off).to(dev), torch.from_numpy(cal.view(np.uint8).reshape(4, -1)).to(dev),
                           run=torch.from_numpy(run).to(dev))
    host = got.cpu().numpy()
    assert host[3:].tobytes() == want[3:].tobytes()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_apply_reports_slots_out_of_range_and_bad_records(dtype):
    import torch
    from pyascore_amd.device import DevicePlan
    gpu = _any_gpu()
    plan = DevicePlan(gpu, synth.slice_batch(synth.make_batch("cfg2", n_psm=2, seed=1)[0], 0, 2))
    dev = torch.device("cuda", 0)
    mz, off = _spectra(dtype)
    cal = _cal(n=4)
    cal["ppm"][1, 3] = np.nan
    cal["ppm"][2, 7] = 1000.5
    cal["ppm"][3, 0] = -np.inf
    run = np.array([0, 0, 1, 0, 4, 2, 0, 3, 9], np.int32)                 # spectra 2, 5, 7: bad records; 4, 8: out of range
    ok = np.where(np.isin(np.arange(len(SIZES)), [2, 4, 5, 7, 8]), -1, run)
    want = ru.recalibrate(mz, off, ok, _cal(n=1))
    d_off, d_cal, d_run = torch.from_numpy(off).to(dev), torch.from_numpy(cal.view(np.uint8).reshape(4, -1)).to(dev), torch.from_numpy(run).to(dev)
    for in_place in (False, True):
        buf = torch.full((mz.size + 64,), 7.0, dtype=torch.from_numpy(mz).dtype, device=dev)
        src = torch.from_numpy(mz).to(dev)
        if in_place:
            buf[:mz.size] = src
            src = buf[:mz.size]
        plan.recalibrate(src, d_off, d_cal, run=d_run, out=buf[:mz.size])
        host = buf.cpu().numpy()
        assert host[:mz.size].tobytes() == want.tobytes(), in_place      # the reported spectra keep their bytes
        assert (host[mz.size:] == 7.0).all()
        over = plan.last_recalibrate_over.cpu().numpy().view(np.uint32)
        assert over[0] == 5 and 0xFFFFFFFF - int(over[1]) == 2
    with pytest.raises(ValueError):
        ru.recalibrate(mz, off, run, cal)
    # the refusals of the call, with nothing launched
    lib, h = gpu._lib, gpu._h
    d_mz = torch.from_numpy(mz).to(dev)
    d_over = torch.zeros(2, dtype=torch.int32, device=dev)
    n_spec = len(SIZES)

    def call(mz_ptr=d_mz.data_ptr(), mz_type=_lib.spectrum_type(d_mz.dtype), off_ptr=d_off.data_ptr(), n=n_spec, cal_ptr=d_cal.data_ptr(),
             n_slots=4, inv_band=1.0 / 250.0, out_ptr=d_mz.data_ptr(), over_ptr=d_over.data_ptr(), sp=True):
        spec = _lib.TypedSpectra(mz_ptr, None, mz_type, _lib.PYA_F64)
        return lib.pya_recalibrate_spectra(h, C.byref(spec) if sp else None, off_ptr, n, None, cal_ptr, n_slots, inv_band, None, out_ptr, over_ptr)

    for kw in (dict(mz_ptr=None), dict(off_ptr=None), dict(cal_ptr=None), dict(out_ptr=None), dict(over_ptr=None), dict(sp=False), dict(mz_type=2),
               dict(n=0xFFFFFFFF), dict(n_slots=1 << 31), dict(inv_band=0.0), dict(inv_band=float("nan")), dict(inv_band=-1.0),
               dict(inv_band=float("inf"))):
        assert call(**kw) == _lib.PYA_ERR_ARG, kw
    assert call(n=0, off_ptr=None, mz_ptr=None, out_ptr=None, over_ptr=None) == 0             # no spectra: a no-op
    torch.cuda.synchronize()
    assert d_mz.cpu().numpy().tobytes() == mz.tobytes() and d_over.cpu().numpy().tolist() == [0, 0]


# ---- the batch path ----

def _drift_cal(n=1, seed=0):
    cal = _cal(n=n)
    if n > 1:
        cal["ppm"][1:] = np.random.default_rng(seed).uniform(-60.0, 60.0, (n - 1, 8))
    return cal


def _corrected(batch, run, cal, band_width=250.0):
    """the batch with its m/z corrected by the restatement; run per PSM (private spectra) or per spectrum (shared)"""
    return dict(batch, mz=ru.recalibrate(batch["mz"], batch["peak_off"], run, cal, band_width))


def _flagged_equals_corrected(settings, batch, what, **stages):
    gpu = _gpu(settings)
    n = int(batch["n_psm"])
    cal = _drift_cal(3, seed=n)
    run = (np.arange(n) % 4 - 1).astype(np.int32)                          # -1, 0, 1, 2
    mz_before = batch["mz"].copy()
    got = gpu.score_batch(batch, recalibrate=dict(calibration=cal, run=run), **stages)
    assert batch["mz"].tobytes() == mz_before.tobytes(), what            # the caller's arrays are never written
    want = gpu.score_batch(_corrected(batch, run, cal), **stages)
    plain = gpu.score_batch(batch, **stages)
    for key in want:
        if isinstance(want[key], np.ndarray):
            assert got[key].tobytes() == want[key].tobytes(), (what, key)
    zero = gpu.score_batch(batch, recalibrate=dict(calibration=np.zeros(3, ru.MZ_CALIBRATION_DTYPE), run=run), **stages)
    for key in plain:
        if isinstance(plain[key], np.ndarray):
            assert zero[key].tobytes() == plain[key].tobytes(), (what, key, "zero calibration")
    return got, plain


@pytest.mark.parametrize("cfg,n", [("cfg2", 64), ("cfg3", 48), ("cfg4", 24), ("cfg5", 16)])
def test_flagged_synth_batches_equal_corrected_arrays(cfg, n):
    batch, settings = synth.make_batch(cfg, n_psm=n, seed=9100)
    _flagged_equals_corrected(settings, batch, cfg)


def test_flagged_realistic_batch_equals_corrected_arrays():
    batch, settings = synth.make_realistic(40, seed=9201, general=True)
    _flagged_equals_corrected(settings, batch, "realistic general")


@pytest.mark.parametrize("case", ["edge_nl", "velos_z1"])
def test_flagged_goldens_equal_corrected_arrays(case):
    settings, batch, _ = harness.load_case(os.path.join(GOLDEN, case + ".npz"))
    _flagged_equals_corrected(settings, batch, case)


def test_cuts_and_forms(monkeypatch):
    """uncut, chunked by size, float32 and mixed spectra, a 5-hit shared batch: the same bytes as on corrected arrays"""
    big = synth.make_slice(synth.describe("cfg2", 12_000, seed=9500))
    settings = synth.describe("cfg2", 1, seed=9500)["settings"]
    gpu = _gpu(settings)
    cal = _drift_cal(4, seed=3)
    run = (np.arange(12_000) // 700 % 5 - 1).astype(np.int32)
    req = dict(calibration=cal, run=run)
    monkeypatch.setenv("PYA_NO_CHUNKS", "1")
    switches.from_env(gpu)
    want = gpu.score_batch(_corrected(big, run, cal))
    whole = gpu.score_batch(big, recalibrate=req)
    assert gpu._lib.pya_debug_last_chunks(gpu._h) == 1
    monkeypatch.delenv("PYA_NO_CHUNKS")
    monkeypatch.setenv("PYA_CHUNK_MB", "2")
    switches.from_env(gpu)
    cut = gpu.score_batch(big, recalibrate=req)
    assert gpu._lib.pya_debug_last_chunks(gpu._h) > 8
    monkeypatch.delenv("PYA_CHUNK_MB")
    switches.from_env(gpu)
    for res, what in ((whole, "uncut"), (cut, "chunk size")):
        for key in KEYS:
            assert res[key].tobytes() == want[key].tobytes(), (what, key)
    # (up to 60 ppm is up to a third of the 0.05 Da window: among 12 000 PSMs some match leaves it, the test is not vacuous)
    assert want["best_score"].tobytes() != gpu.score_batch(big)["best_score"].tobytes()
    part = synth.slice_batch(big, 0, 1500)
    for form, what in ((synth.narrow_batch(part), "float32"), (synth.narrow_batch(part, mz=np.float64), "float64 m/z, float32 intensities")):
        got = gpu.score_batch(form, recalibrate=dict(calibration=cal, run=run[:1500]))
        ref = gpu.score_batch(_corrected(form, run[:1500], cal))
        assert form["mz"].dtype == _corrected(form, run[:1500], cal)["mz"].dtype
        for key in KEYS:
            assert got[key].tobytes() == ref[key].tobytes(), (what, key)
    # five hits per spectrum; the slot is the spectrum's
    small_b, _ = synth.make_batch("cfg2", n_psm=100, seed=9501)
    spectra, psms = [], []
    for i in range(0, 100, 5):
        kw = synth.unpack_psm(small_b, i)
        spectra.append(dict(mz=kw["mz_arr"], intensity=kw["int_arr"]))
        for j in range(5):
            kj = synth.unpack_psm(small_b, i + j)
            psms.append(dict(peptide=kj["peptide"], n_of_mod=kj["n_of_mod"], max_charge=1, aux_pos=np.zeros(0, np.uint32),
                             aux_mass=np.zeros(0, np.float32), spectrum=len(spectra) - 1))
    spec_run = (np.arange(20) % 5 - 1).astype(np.int32)
    for order, what in ((np.arange(100), "shared"), (np.random.default_rng(3).permutation(100), "shuffled shared")):
        chosen = [psms[p] for p in order]
        shared = synth.pack_shared_batch(spectra, chosen)
        psm_run = spec_run[[p["spectrum"] for p in chosen]].copy()
        first = {}
        for k, p in enumerate(chosen):                                        # some PSMs of a corrected spectrum name no slot
            if p["spectrum"] in first and k % 3 == 0:
                psm_run[k] = -1
            first.setdefault(p["spectrum"], k)
        got = gpu.score_batch(shared, recalibrate=dict(calibration=cal, run=psm_run))
        ref = gpu.score_batch(_corrected(shared, spec_run, cal))
        for key in KEYS:
            assert got[key].tobytes() == ref[key].tobytes(), (what, key)
        clash = psm_run.copy()
        k = next(k for k, p in enumerate(chosen) if spec_run[p["spectrum"]] == 1 and first[p["spectrum"]] != k)
        clash[k] = 2
        with pytest.raises(ValueError, match="PSM %d" % k):
            gpu.score_batch(shared, recalibrate=dict(calibration=cal, run=clash))


def test_with_the_profile_and_beside_the_other_stages():
    batch, settings = synth.make_batch("cfg3", n_psm=120, seed=9996)
    gpu = _gpu(settings)
    cal = _drift_cal(2, seed=1)
    run = (np.arange(120) % 2).astype(np.int32)
    stages = dict(evidence=True, ions=True, sites=True, probs=True, ranked=5, mz_profile=dict(run=run, n_slots=2))
    got = gpu.score_batch(batch, recalibrate=dict(calibration=cal, run=run), **stages)
    want = gpu.score_batch(_corrected(batch, run, cal), **stages)
    for key in KEYS + ("evidence", "ion_off", "ions", "site_off", "sites", "site_probs", "psm_probs", "ranked", "mz_profile"):
        assert got[key].tobytes() == want[key].tobytes(), key
    # ... and the profile is the yardstick's over the ions of the corrected arrays: the residual errors
    yard = ru.mz_profile(want["ion_off"], want["ions"], want["n_sig"], run, 2, got["mz_profile_params"])
    assert got["mz_profile"].tobytes() == yard.tobytes() and yard["n_ions"].all()
    assert got["mz_profile"].tobytes() != gpu.score_batch(batch, mz_profile=dict(run=run, n_slots=2))["mz_profile"].tobytes()
    one = synth.slice_batch(batch, 7, 8)                                      # a batch of one takes the plan's launches
    a = gpu.score_batch(one, recalibrate=dict(calibration=cal, run=run[7:8]))
    b = gpu.score_batch(_corrected(one, run[7:8], cal))
    for key in KEYS:
        assert a[key].tobytes() == b[key].tobytes(), key


def test_batch_refusals():
    batch, settings = synth.make_batch("cfg2", n_psm=50, seed=9990)
    gpu = _gpu(settings)
    lib, h = gpu._lib, gpu._h
    cal = _drift_cal(2)
    run = (np.arange(50) % 2).astype(np.int32)
    with pytest.raises(ValueError, match="keep"):                             # documented: refused together with keep=True
        gpu.score_batch(batch, keep=True, recalibrate=dict(calibration=cal, run=run))
    with pytest.raises(ValueError, match="slot 2"):                           # PYA_ERR_LIMIT
        gpu.score_batch(batch, recalibrate=dict(calibration=cal, run=run * 2))
    arrs = [np.ascontiguousarray(batch[k], t) for k, t in (("peak_off", np.int64), ("pep", np.uint8), ("pep_off", np.int64), ("n_of_mod", np.int32),
                                                           ("max_charge", np.int32), ("aux_pos", np.uint32), ("aux_mass", np.float32),
                                                           ("aux_off", np.int64))]
    b = _lib.Batch(50, *[vp(a) for a in arrs])
    res = gpu.score_batch(batch)
    outs = [np.zeros_like(res[k]) for k in KEYS]
    rs = _lib.Results(res["ascores"].shape[1], *[vp(a) for a in outs])
    mz, it = np.ascontiguousarray(batch["mz"], np.float64), np.ascontiguousarray(batch["intensity"], np.float64)
    flag = _lib.PYA_FLAG_RECALIBRATE
    assert lib.pya_score_batch(h, C.byref(b), vp(mz), vp(it), flag, C.byref(rs)) == _lib.PYA_ERR_ARG       # the flag without a loan
    assert b"pya_set_recalibration" in lib.pya_last_error(h)
    assert lib.pya_set_recalibration(h, vp(run), 49, vp(cal), 2, 1.0 / 250.0) == 0                          # a loan of another size
    assert lib.pya_score_batch(h, C.byref(b), vp(mz), vp(it), flag, C.byref(rs)) == _lib.PYA_ERR_ARG
    assert lib.pya_score_batch(h, C.byref(b), vp(mz), vp(it), flag, C.byref(rs)) == _lib.PYA_ERR_ARG       # ... which ended with that call
    assert lib.pya_set_recalibration(h, vp(run), 50, vp(cal), 2, 1.0 / 250.0) == 0
    assert lib.pya_score_batch(h, C.byref(b), vp(mz), vp(it), flag | _lib.PYA_FLAG_KEEP, C.byref(rs)) == _lib.PYA_ERR_ARG
    assert b"PYA_FLAG_KEEP" in lib.pya_last_error(h)
    assert lib.pya_set_recalibration(h, vp(run * 2), 50, vp(cal), 2, 1.0 / 250.0) == 0
    assert lib.pya_score_batch(h, C.byref(b), vp(mz), vp(it), flag, C.byref(rs)) == _lib.PYA_ERR_LIMIT and lib.pya_error_index(h) == 1
    assert lib.pya_set_recalibration(h, vp(run), 50, vp(cal), 2, 1.0 / 250.0) == 0                          # and a good one
    assert lib.pya_score_batch(h, C.byref(b), vp(mz), vp(it), flag, C.byref(rs)) == 0
    want = gpu.score_batch(_corrected(batch, run, cal))
    for a, key in zip(outs, KEYS):
        assert a.tobytes() == want[key].tobytes(), key
    bad = cal.copy()
    bad["ppm"][1, 2] = np.nan
    far = cal.copy()
    far["ppm"][0, 0] = -1000.5
    for args in ((vp(run), 50, vp(bad), 2, 0.004), (vp(run), 50, vp(far), 2, 0.004), (vp(run), 50, None, 2, 0.004), (vp(run), 1 << 31, vp(cal), 2, 0.004),
                 (vp(run), 50, vp(cal), 1 << 31, 0.004), (vp(run), 50, vp(cal), 2, 0.0), (vp(run), 50, vp(cal), 2, float("nan"))):
        assert lib.pya_set_recalibration(h, *args) == _lib.PYA_ERR_ARG, args
    assert lib.pya_set_recalibration(None, vp(run), 50, vp(cal), 2, 0.004) == _lib.PYA_ERR_ARG
    # pya_score_one and pya_plan_create* refuse the flag
    kw = synth.unpack_psm(batch, 0)
    m, i = np.ascontiguousarray(kw["mz_arr"], np.float64), np.ascontiguousarray(kw["int_arr"], np.float64)
    pep = np.frombuffer(kw["peptide"].encode(), np.uint8)
    one = (np.zeros(1, np.float32), np.zeros(1, np.uint64), np.zeros(1, np.int32), np.zeros((1, 4), np.float32), np.zeros((1, 4), np.uint64))
    r1 = _lib.Results(4, *[vp(x) for x in one])
    rc = lib.pya_score_one(h, vp(m), vp(i), m.size, vp(pep), pep.size, int(kw["n_of_mod"]), int(kw["max_fragment_charge"]), None, None, 0,
                           flag, C.byref(r1))
    assert rc == _lib.PYA_ERR_ARG and b"PYA_FLAG_RECALIBRATE" in lib.pya_last_error(h)
    plan = C.c_void_p()
    assert lib.pya_plan_create(h, C.byref(b), flag, C.byref(plan)) == _lib.PYA_ERR_ARG and not plan.value
    assert b"pya_recalibrate_spectra" in lib.pya_last_error(h)
    spec_of = np.arange(50, dtype=np.uint32)
    assert lib.pya_plan_create_shared(h, C.byref(b), vp(spec_of), 50, flag, C.byref(plan)) == _lib.PYA_ERR_ARG and not plan.value


def test_plan_path_without_a_host_copy():
    """DevicePlan.run -> mz_profile -> fit_mz_calibration -> recalibrate -> run again on device tensors; the results equal
    the batch path's with the calibration the host form fits.  The batch and the drift are those of the host loop in
    tests/test_recalibrate_host.py, so the fitted knots are the ones measured there with the reference core (1.06 ppm off at
    most).  (With 300 PSMs of the same seed band 0 is 3.90 ppm off, on the device and with the reference core alike: at m/z
    below 250 a 32 ppm drift plus the scatter of a 0.01 Da generator reaches past the +50 ppm edge of the axis, the band's
    histogram is cut off there and its median is pulled down -- a limit of the definition)"""
    import torch
    from pyascore_amd.device import DevicePlan, mz_calibration_records
    batch, settings = synth.make_batch("cfg2", n_psm=120, seed=3, mz_error=0.01)
    drift = _cal()
    e = (batch["mz"] - ru.recalibrate(batch["mz"], batch["peak_off"], None, drift)) / batch["mz"] * 1e6
    drifted = dict(batch, mz=batch["mz"] * (1.0 + e * 1e-6))
    wide = _gpu(dict(settings, mz_error=0.05))
    narrow = _gpu(settings)
    params = ru.mz_profile_params(0.05, ppm_half_width=50.0, max_rank=9)
    dev = torch.device("cuda", 0)
    d_mz, d_it = torch.from_numpy(drifted["mz"]).to(dev), torch.from_numpy(drifted["intensity"]).to(dev)
    d_off = torch.from_numpy(np.ascontiguousarray(drifted["peak_off"], np.int64)).to(dev)
    p_wide = DevicePlan(wide, drifted, mz_profile=True)
    p_wide.run(d_mz, d_it)
    table = p_wide.mz_profile(params)
    d_cal = p_wide.fit_mz_calibration(table, params, min_ions=20)
    d_fixed = p_wide.recalibrate(d_mz, d_off, d_cal)
    p_narrow = DevicePlan(narrow, drifted)
    p_narrow.run(d_fixed, d_it)
    p_narrow.check()
    p_wide.check()
    cal = mz_calibration_records(d_cal.cpu().numpy())
    host_table = wide.score_batch(drifted, mz_profile=dict(da_half_width=0.05, ppm_half_width=50.0, max_rank=9))["mz_profile"]
    _same_cal(cal, wide.fit_mz_calibration(host_table, params, min_ions=20), "plan and batch calibration")
    fitted = cal["n_signal"][0] >= 20
    assert fitted.sum() >= 6 and np.abs(cal["ppm"][0] - np.array(KNOTS))[fitted].max() <= 2 * 50.0 / HALF   # two profile bins
    want = narrow.score_batch(drifted, recalibrate=dict(calibration=cal))
    assert p_narrow.best_score.cpu().numpy().tobytes() == want["best_score"].tobytes()
    assert p_narrow.best_sig.cpu().numpy().view(np.uint64).tobytes() == want["best_sig"].tobytes()
    assert p_narrow.ascores.cpu().numpy().tobytes() == want["ascores"].tobytes()
    clean = narrow.score_batch(batch)
    before = narrow.score_batch(drifted)
    agree = lambda r: int((r["best_sig"] == clean["best_sig"]).sum())  # noqa: E731
    assert agree(want) > agree(before)


def test_command_line_files(tmp_path):
    from pyascore_amd import PyAscore, __main__ as cli, batch_cli, ingest
    spec, ident = os.path.join(DATA, "test_spectra.mzML"), os.path.join(DATA, "test_psms.pep.xml")
    quiet = lambda *_: None  # noqa: E731
    first, cal_file = tmp_path / "first.tsv", tmp_path / "cal.tsv"
    rows = cli.run(cli.parse_args(["--mz_error", "0.05", "--hit_depth", "2", "--mz_calibration_out", str(cal_file), spec, ident, str(first)]), log=quiet)
    plain = cli.run(cli.parse_args(["--mz_error", "0.05", "--hit_depth", "2", spec, ident, str(tmp_path / "plain.tsv")]), log=quiet)
    assert rows == plain                                                      # fitting changes nothing of the run
    cal, width = ru.read_mz_calibration(str(cal_file))
    assert cal.shape == (1,) and width == 250.0
    # the file holds what the device fits to the profile of that run
    gpu = PyAscore(100.0, 10, "STY", 79.966331, 0.05, "by")
    spectra = ingest.SpectraParser(spec, "mzML", native_precision=True).to_dict()
    psms = sorted(ingest.IdentificationParser(ident, "pepXML").to_list(), key=lambda p: p["scan"])
    prof = []
    assert batch_cli.localize(gpu, psms, spectra, "STY", 79.966331, hit_depth=2, mz_profile=prof) == plain
    _same_cal(cal, ru.fit_mz_calibration(prof[0], prof[1], min_ions=20), "the calibration file")
    # the fixtures are well calibrated: use a calibration that moves something
    cal["ppm"][0] = [40.0, 35.0, 30.0, 25.0, 20.0, 15.0, 10.0, 5.0]
    batch_cli.write_mz_calibration_tsv(cal, width, str(cal_file))
    second, prof_file = tmp_path / "second.tsv", tmp_path / "residual.tsv"
    got = cli.run(cli.parse_args(["--mz_error", "0.05", "--hit_depth", "2", "--mz_calibration", str(cal_file), "--mz_profile", str(prof_file),
                                  spec, ident, str(second)]), log=quiet)
    fixed = {}
    for scan, rec in spectra.items():
        mz = rec["mz_values"]
        fixed[scan] = dict(rec, mz_values=ru.recalibrate(mz, [0, mz.size], None, cal, width))
    want_prof = []
    want = batch_cli.localize(gpu, psms, fixed, "STY", 79.966331, hit_depth=2, mz_profile=want_prof)
    assert got == want
    lines = [line.split("\t") for line in prof_file.read_text().splitlines()[1:]]
    counts = np.array([int(c[6]) for c in lines if c[2] == "ppm" and c[1] != "-1"]).reshape(BANDS, BINS)
    assert np.array_equal(counts, want_prof[0]["ppm"][0])                     # with --mz_profile: the residuals
    assert not np.array_equal(counts, prof[0]["ppm"][0])                      # (5 .. 40 ppm is 3 .. 25 bins: the profile has moved)
