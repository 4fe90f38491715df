"""Fragment mass-error profile on the GPU (pya_mz_profile: the m/z errors of the matched fragments of the reported localisations,
binned per run slot).  Yardstick: pyascore_amd.rollup.mz_profile over the ion records score_batch(ions=True) returns for the
same batch -- every comparison is on the raw bytes of the 4 128-byte records: every word is an integer count."""
import ctypes as C
import os

import numpy as np
import pytest

import fuzzcase
import switches
from conftest import GOLDEN
from oracle import harness
from pyascore_amd import _lib, rollup as ru, synth

pytestmark = pytest.mark.gpu

KEYS = ("best_score", "best_sig", "n_sig", "ascores", "alt_mask")
CHUNK = _lib.PYA_MZP_CHUNK
DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ingest")


def _gpu(settings):
    from pyascore_amd import PyAscore
    return harness.make_scorer(PyAscore, settings)


def _params(settings, **kw):
    kw.setdefault("max_rank", settings["n_top"] - 1)
    return ru.mz_profile_params(kw.pop("da_half_width", float(np.float32(settings["mz_error"]))), **kw)


def _same_bytes(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == ru.MZ_PROFILE_DTYPE, what
    a, b = got.view(np.uint32).reshape(got.size, -1), want.view(np.uint32).reshape(want.size, -1)
    bad = np.argwhere(a != b)
    assert bad.size == 0, "%s: %d words differ, first (slot, word) %s: got %d, want %d" % (
        what, len(bad), bad[0].tolist(), a[tuple(bad[0])], b[tuple(bad[0])])


def _want(res, settings, run, n_slots, **kw):
    return ru.mz_profile(res["ion_off"], res["ions"], res["n_sig"], run, n_slots, _params(settings, **kw))


def _against_yardstick(settings, batch, what, skip_invalid=False, need_ions=True):
    """one slot for everything, then three slots (one empty) with every fifth PSM left out and a narrow axis"""
    gpu = _gpu(settings)
    plain = gpu.score_batch(batch, skip_invalid=skip_invalid, ions=True)
    got = gpu.score_batch(batch, skip_invalid=skip_invalid, mz_profile={})
    for key in KEYS + (("status",) if skip_invalid else ()):                           # the flag changes nothing of the run
        assert got[key].tobytes() == plain[key].tobytes(), (what, key)
    want = _want(plain, settings, None, 1)
    if need_ions:
        assert want["n_ions"][0] > 0, what
    _same_bytes(got["mz_profile"], want, what)
    assert got["mz_profile_params"] == _params(settings)
    n = int(batch["n_psm"])
    run = (np.arange(n) % 2 * 2).astype(np.int32)
    run[::5] = -1
    err = float(np.float32(settings["mz_error"]))
    req = dict(run=run, n_slots=3, da_half_width=err / 4, ppm_half_width=5.0, band_width=300.0, max_rank=4)
    three = gpu.score_batch(batch, skip_invalid=skip_invalid, mz_profile=req, ions=True)
    assert three["ions"].tobytes() == plain["ions"].tobytes(), what
    want3 = _want(plain, settings, run, 3, da_half_width=err / 4, ppm_half_width=5.0, band_width=300.0, max_rank=4)
    _same_bytes(three["mz_profile"], want3, what + ", three slots")
    assert three["mz_profile"][1].tobytes() == bytes(4128)
    for t in three["mz_profile"]:
        assert int(t["da"].sum()) + int(t["out_da"].sum()) == t["n_ions"] == int(t["ppm"].sum()) + int(t["out_ppm"].sum())
    return plain, got


@pytest.mark.parametrize("case", ["edge_err05", "edge_nl", "edge_Zc", "velos_z1", "ties_cfg2"])
def test_goldens_equal_the_yardstick(case):
    settings, batch, _ = harness.load_case(os.path.join(GOLDEN, case + ".npz"))
    _against_yardstick(settings, batch, case)


@pytest.mark.parametrize("cfg,n", [("cfg1", 48), ("cfg2", 64), ("cfg3", 48), ("cfg4", 24), ("cfg5", 16)])
def test_synth_slices_equal_the_yardstick(cfg, n):
    batch, settings = synth.make_batch(cfg, n_psm=n, seed=9100)
    _against_yardstick(settings, batch, cfg)


@pytest.mark.parametrize("general", [False, True])
def test_realistic_batches_equal_the_yardstick(general):
    """general: charges up to 4, two neutral losses, four ion types"""
    batch, settings = synth.make_realistic(40, seed=9200 + general, general=general)
    plain, _ = _against_yardstick(settings, batch, "realistic general=%s" % general)
    if general:
        first = plain["ions"][plain["ions"]["site"] == 255]
        assert first["charge"].max() >= 3 and len(set(first["type"].tolist())) == 4 and (first["flags"] & 1).any()


def test_fuzz_cases_equal_the_yardstick():
    rng = np.random.default_rng(9300)
    done = 0
    for _ in range(60):                                                          # (a case without PSMs or without a matched ion is passed over)
        settings, batch = fuzzcase.random_case(rng)[:2]
        if batch["n_psm"] == 0:
            continue
        plain = _gpu(settings).score_batch(batch, skip_invalid=True, ions=True)
        if not (plain["ions"]["site"] == 255).any():
            continue
        _against_yardstick(settings, batch, "fuzz %d" % done, skip_invalid=True)
        done += 1
        if done == 6:
            break
    assert done == 6


def test_long_and_short_peptides():
    """a second block of 64 prefixes on the general route; a peptide of two residues"""
    long_b, settings = synth.make_batch("cfg2", n_psm=4, seed=9700, L=100, n_sites=5, n_mod=2)
    plain, _ = _against_yardstick(settings, long_b, "100 residues")
    assert plain["ions"]["size"][plain["ions"]["site"] == 255].max() > 64
    few, _ = synth.make_batch("cfg2", n_psm=3, seed=9701)
    psms = []
    for i in range(3):
        kw = synth.unpack_psm(few, i)
        psms.append(dict(mz=kw["mz_arr"], intensity=kw["int_arr"], peptide=kw["peptide"], n_of_mod=kw["n_of_mod"], max_charge=1))
    # b1 of S+phospho (168.0056 + ...), y1 of K (147.1128): peaks near both, and noise
    mz = np.sort(np.concatenate([[147.113, 168.006, 88.04, 227.08], np.linspace(100.0, 400.0, 40)]))
    psms.insert(1, dict(mz=mz, intensity=np.linspace(10.0, 500.0, mz.size), peptide="SK", n_of_mod=1, max_charge=1))
    batch = synth.pack_batch(psms)
    plain, _ = _against_yardstick(settings, batch, "two residues")
    assert plain["n_sig"][1] > 0


@pytest.mark.parametrize("n", [0, 1, CHUNK - 1, CHUNK, CHUNK + 1])
def test_chunk_boundaries(n):
    batch, settings = synth.make_batch("cfg2", n_psm=max(n, 1), seed=9710)
    batch = synth.slice_batch(batch, 0, n)
    gpu = _gpu(settings)
    plain = gpu.score_batch(batch, ions=True)
    # slots that change inside a chunk and exactly at its boundary; runs of one slot in between
    run = np.zeros(n, np.int32)
    run[n // 3:] = 2
    run[CHUNK - 2:CHUNK - 1] = 0
    run[CHUNK:] = 1
    for r, what in ((None, "one slot"), (run, "changing slots")):
        got = gpu.score_batch(batch, mz_profile=dict(run=r, n_slots=3))
        _same_bytes(got["mz_profile"], _want(plain, settings, r, 3), "%d PSMs, %s" % (n, what))
        for key in KEYS:
            assert got[key].tobytes() == plain[key].tobytes(), key
    if n:
        assert _want(plain, settings, None, 3)["n_ions"][0] > 0
        out = gpu.score_batch(batch, mz_profile=dict(run=np.full(n, -1, np.int32), n_slots=2))["mz_profile"]   # all PSMs left out
        assert out.tobytes() == bytes(2 * 4128)


def test_2000_copies_into_one_slot():
    """every flush of every workgroup hits the same cells"""
    one, settings = synth.make_batch("cfg2", n_psm=1, seed=9720)
    kw = synth.unpack_psm(one, 0)
    psm = dict(mz=kw["mz_arr"], intensity=kw["int_arr"], peptide=kw["peptide"], n_of_mod=kw["n_of_mod"], max_charge=1)
    gpu = _gpu(settings)
    single = gpu.score_batch(synth.pack_batch([psm]), mz_profile={})["mz_profile"]
    assert single["n_ions"][0] > 0 and single["n_psm"][0] == 1
    got = gpu.score_batch(synth.pack_batch([psm] * 2000), mz_profile={})["mz_profile"]
    want = (single.view(np.uint32) * np.uint32(2000)).view(ru.MZ_PROFILE_DTYPE)
    _same_bytes(got, want, "2 000 copies")


def test_every_route_and_cut_gives_the_same_bytes(monkeypatch):
    routes = {"default": {}, "no_fused": {"PYA_NO_FUSED": "1"}, "no_plain": {"PYA_NO_PLAIN": "1"}, "no_big": {"PYA_NO_BIG": "1"},
              "no_cnt": {"PYA_NO_CNT": "1"}, "no_loc_hash": {"PYA_NO_LOC_HASH": "1"}, "no_nodes": {"PYA_NO_NODES": "1"},
              "no_fork": {"PYA_NO_FORK": "1"}, "plain_all": {"PYA_PLAIN_MIN": "0"}, "no_tiny": {"PYA_NO_TINY": "1"}}
    for cfg, n in (("cfg3", 300), ("cfg4", 48)):
        batch, settings = synth.make_batch(cfg, n_psm=n, seed=9400)
        run = (np.arange(n) % 3).astype(np.int32)
        want = None
        for name, env in routes.items():
            with monkeypatch.context() as m:
                for k, v in env.items():
                    m.setenv(k, v)
                gpu = _gpu(settings)
                got = gpu.score_batch(batch, mz_profile=dict(run=run, n_slots=3))["mz_profile"]
                if want is None:
                    want = _want(gpu.score_batch(batch, ions=True), settings, run, 3)
                    assert want["n_ions"].all()
            _same_bytes(got, want, "%s %s" % (cfg, name))


def test_cuts_and_forms(monkeypatch):
    """chunked by size and by the workspace budget against uncut, float32 against widened, shared against expanded"""
    big = synth.make_slice(synth.describe("cfg2", 12_000, seed=9500))
    settings = synth.describe("cfg2", 1, seed=9500)["settings"]
    gpu = _gpu(settings)
    run = (np.arange(12_000) // 700 % 4).astype(np.int32)
    req = dict(run=run, n_slots=4)
    monkeypatch.setenv("PYA_NO_CHUNKS", "1")
    switches.from_env(gpu)
    plain = gpu.score_batch(big, ions=True)
    whole = gpu.score_batch(big, mz_profile=req)
    assert gpu._lib.pya_debug_last_chunks(gpu._h) == 1
    want = _want(plain, settings, run, 4)
    assert want["n_ions"].all()
    _same_bytes(whole["mz_profile"], want, "uncut")
    monkeypatch.delenv("PYA_NO_CHUNKS")
    monkeypatch.setenv("PYA_CHUNK_MB", "2")
    switches.from_env(gpu)
    cut = gpu.score_batch(big, mz_profile=req)
    assert gpu._lib.pya_debug_last_chunks(gpu._h) > 8
    monkeypatch.delenv("PYA_CHUNK_MB")
    switches.from_env(gpu)
    gpu.set_workspace_budget(48 << 20)
    small = gpu.score_batch(big, mz_profile=req)
    assert gpu._lib.pya_debug_last_chunks(gpu._h) > 1
    gpu.set_workspace_budget(0)
    for res, what in ((cut, "chunk size"), (small, "budget")):
        _same_bytes(res["mz_profile"], want, "chunked by " + what)
        for key in KEYS:
            assert res[key].tobytes() == plain[key].tobytes(), (what, key)
    part = synth.slice_batch(big, 0, 1500)
    p_req = dict(run=run[:1500], n_slots=4)
    narrow = gpu.score_batch(synth.narrow_batch(part), mz_profile=p_req, ions=True)
    wide = gpu.score_batch(synth.widen_batch(synth.narrow_batch(part)), mz_profile=p_req)
    _same_bytes(narrow["mz_profile"], _want(narrow, settings, run[:1500], 4), "float32")
    _same_bytes(wide["mz_profile"], narrow["mz_profile"], "widened")
    small_b, _ = synth.make_batch("cfg2", n_psm=60, seed=9501)
    spectra, psms = [], []
    for i in range(0, 60, 3):
        kw = synth.unpack_psm(small_b, i)
        spectra.append(dict(mz=kw["mz_arr"], intensity=kw["int_arr"]))
        for j in range(3):
            kj = synth.unpack_psm(small_b, i + j)
            psms.append(dict(peptide=kj["peptide"], n_of_mod=kj["n_of_mod"], max_charge=1, aux_pos=np.zeros(0, np.uint32),
                             aux_mass=np.zeros(0, np.float32), spectrum=len(spectra) - 1))
    s_run = (np.arange(60) % 2).astype(np.int32)
    for order, what in ((np.arange(60), "shared"), (np.random.default_rng(3).permutation(60), "shuffled shared")):
        shared = synth.pack_shared_batch(spectra, [psms[p] for p in order])
        flat = gpu.score_batch(synth.expand_shared_batch(shared), ions=True)
        s_want = _want(flat, settings, s_run, 2)
        assert s_want["n_ions"].all()
        _same_bytes(gpu.score_batch(shared, mz_profile=dict(run=s_run, n_slots=2))["mz_profile"], s_want, what)
        _same_bytes(gpu.score_batch(shared, mz_profile=dict(run=s_run, n_slots=2), keep=True)["mz_profile"], s_want, what + ", keep")


def _plan(gpu, batch, dev, **kw):
    import torch
    from pyascore_amd.device import DevicePlan
    plan = DevicePlan(gpu, batch, mz_profile=True, **kw)
    plan.run(torch.from_numpy(batch["mz"]).to(dev), torch.from_numpy(batch["intensity"]).to(dev))
    return plan


def test_accumulation():
    import torch
    from pyascore_amd.device import mz_profile_records
    batch, settings = synth.make_batch("cfg3", n_psm=600, seed=9980)
    gpu = _gpu(settings)
    run = (np.arange(600) % 3).astype(np.int32)
    res = gpu.score_batch(batch, ions=True)
    want = _want(res, settings, run, 3)
    assert want["n_ions"].all()
    _same_bytes(gpu.score_batch(batch, mz_profile=dict(run=run, n_slots=3))["mz_profile"], want, "one call")
    p = _params(settings)
    dev = torch.device("cuda", 0)
    plan = _plan(gpu, batch, dev)
    d_run = torch.from_numpy(run).to(dev)
    table = plan.mz_profile(p, d_run, n_slots=3)
    plan.check()
    _same_bytes(mz_profile_records(table.cpu().numpy()), want, "plan")
    other = torch.cuda.Stream(dev)
    with torch.cuda.stream(other):                                               # the same plan again, on another stream
        plan.mz_profile(p, d_run, table=table)
    torch.cuda.synchronize()
    plan.check()
    twice = (want.view(np.uint32) * np.uint32(2)).view(ru.MZ_PROFILE_DTYPE)
    _same_bytes(mz_profile_records(table.cpu().numpy()), twice, "two calls into one table")
    cut = 250
    for order in ((0, 1), (1, 0)):
        halves = [(synth.slice_batch(batch, 0, cut), run[:cut]), (synth.slice_batch(batch, cut, 600), run[cut:])]
        shared = None
        apart = []
        for h in order:
            pl = _plan(gpu, halves[h][0], dev)
            r = torch.from_numpy(halves[h][1]).to(dev)
            shared = pl.mz_profile(p, r, n_slots=3, table=shared)
            apart.append(mz_profile_records(pl.mz_profile(p, r, n_slots=3).cpu().numpy()))
            pl.check()
        _same_bytes(mz_profile_records(shared.cpu().numpy()), want, "two plans, order %s" % (order,))
        _same_bytes(ru.merge_mz_profiles(*apart), want, "merged on the host")
    slot0 = plan.mz_profile(p)                                                   # run None: everything is slot 0
    _same_bytes(mz_profile_records(slot0.cpu().numpy()), _want(res, settings, None, 1), "no run array")
    few = synth.slice_batch(batch, 0, 5)                                         # a handful of PSMs: created with the flag
    t5 = _plan(gpu, few, dev).mz_profile(p)
    _same_bytes(mz_profile_records(t5.cpu().numpy()), _want(gpu.score_batch(few, ions=True), settings, None, 1), "plan of five")
    for lo, hi in ((0, 1), (7, 8)):                                              # a batch of one takes the plan's launches
        part = synth.slice_batch(batch, lo, hi)
        _same_bytes(gpu.score_batch(part, mz_profile={})["mz_profile"], _want(gpu.score_batch(part, ions=True), settings, None, 1), "batch of one")


def test_refusals():
    import torch
    from pyascore_amd.device import DevicePlan, mz_profile_records
    batch, settings = synth.make_batch("cfg2", n_psm=200, seed=9990)
    gpu = _gpu(settings)
    lib = gpu._lib
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    out = np.zeros(3, ru.MZ_PROFILE_DTYPE)
    assert lib.pya_last_batch_mz_profile(None, vp(out), 3) == _lib.PYA_ERR_ARG
    assert lib.pya_last_batch_mz_profile(gpu._h, vp(out), 3) == _lib.PYA_ERR_STATE and b"PYA_FLAG_MZ_PROFILE" in lib.pya_last_error(gpu._h)
    res = gpu.score_batch(batch, ions=True)
    assert lib.pya_last_batch_mz_profile(gpu._h, vp(out), 3) == _lib.PYA_ERR_STATE
    run = (np.arange(200) % 3).astype(np.int32)
    want = _want(res, settings, run, 3)
    got = gpu.score_batch(batch, mz_profile=dict(run=run, n_slots=3))["mz_profile"]
    _same_bytes(got, want, "batch")
    assert lib.pya_last_batch_mz_profile(gpu._h, vp(out), 3) == 0 and out.tobytes() == got.tobytes()
    assert lib.pya_last_batch_mz_profile(gpu._h, vp(out), 2) == _lib.PYA_ERR_ARG
    assert lib.pya_last_batch_mz_profile(gpu._h, None, 3) == _lib.PYA_ERR_ARG
    # the flag without a loan (the loan of the call above ended with it), and a loan of another size
    arrs = [np.ascontiguousarray(batch[k], t) for k, t in (("peak_off", np.int64), ("pep", np.uint8), ("pep_off", np.int64), ("n_of_mod", np.int32),
                                                           ("max_charge", np.int32), ("aux_pos", np.uint32), ("aux_mass", np.float32),
                                                           ("aux_off", np.int64))]
    b = _lib.Batch(200, *[vp(a) for a in arrs])
    outs = [np.zeros_like(res[k]) for k in KEYS]
    rs = _lib.Results(res["ascores"].shape[1], *[vp(a) for a in outs])
    mz, it = np.ascontiguousarray(batch["mz"], np.float64), np.ascontiguousarray(batch["intensity"], np.float64)
    good = _params(settings)
    cp = lambda p: C.byref(_lib.MzProfileParams(p["inv_da"], p["inv_ppm"], p["inv_band"], p["max_rank"], 0))  # noqa: E731
    assert lib.pya_score_batch(gpu._h, C.byref(b), vp(mz), vp(it), _lib.PYA_FLAG_MZ_PROFILE, C.byref(rs)) == _lib.PYA_ERR_ARG
    assert b"pya_set_mz_profile" in lib.pya_last_error(gpu._h)
    assert lib.pya_set_mz_profile(gpu._h, vp(run), 199, 3, cp(good)) == 0
    assert lib.pya_score_batch(gpu._h, C.byref(b), vp(mz), vp(it), _lib.PYA_FLAG_MZ_PROFILE, C.byref(rs)) == _lib.PYA_ERR_ARG
    assert lib.pya_last_batch_mz_profile(gpu._h, vp(out), 3) == _lib.PYA_ERR_STATE
    # what pya_set_mz_profile and pya_plan_mz_profile refuse, with nothing launched
    bads = [dict(good, max_rank=16), dict(good, inv_da=0.0), dict(good, inv_da=-1.0), dict(good, inv_ppm=float("nan")),
            dict(good, inv_band=float("inf")), dict(good, inv_band=-0.0)]
    dev = torch.device("cuda", 0)
    plan = _plan(gpu, batch, dev)
    d_run = torch.from_numpy(run).to(dev)
    table = torch.zeros((3, 4128), dtype=torch.uint8, device=dev)
    call = lambda pl, p, n_slots, t=table, r=d_run: lib.pya_plan_mz_profile(  # noqa: E731
        pl._plan, C.byref(pl._res), None, None if r is None else r.data_ptr(), n_slots, p, None if t is None else t.data_ptr())
    for bad in bads:
        assert lib.pya_set_mz_profile(gpu._h, vp(run), 200, 3, cp(bad)) == _lib.PYA_ERR_ARG, bad
        assert call(plan, cp(bad), 3) == _lib.PYA_ERR_ARG, bad
    assert lib.pya_set_mz_profile(gpu._h, vp(run), 200, 1 << 31, cp(good)) == _lib.PYA_ERR_ARG
    assert lib.pya_set_mz_profile(gpu._h, vp(run), 200, 3, None) == _lib.PYA_ERR_ARG
    assert call(plan, cp(good), 1 << 31) == _lib.PYA_ERR_ARG
    assert call(plan, None, 3) == _lib.PYA_ERR_ARG
    assert call(plan, cp(good), 3, t=None) == _lib.PYA_ERR_ARG
    assert lib.pya_plan_mz_profile(None, None, None, None, 0, cp(good), None) == _lib.PYA_ERR_ARG
    torch.cuda.synchronize()
    assert table.cpu().numpy().tobytes() == bytes(3 * 4128)                      # nothing was launched
    fresh = DevicePlan(gpu, batch, mz_profile=True)
    assert call(fresh, cp(good), 3) == _lib.PYA_ERR_STATE                        # before the first run
    with pytest.raises(ValueError):
        plan.mz_profile(good, d_run[:-1], table=table)
    # a slot at or above n_slots: nothing of it is written, nothing lies behind the table, pya_plan_check reports it
    with pytest.raises(ValueError, match="n_slots"):
        gpu.score_batch(batch, mz_profile=dict(run=run, n_slots=2))
    guard = torch.full((5, 4128), 0x5A, dtype=torch.uint8, device=dev)
    guard[:2] = 0
    assert call(plan, cp(good), 2, t=guard) == 0
    with pytest.raises(ValueError, match="n_slots"):
        plan.check()
    assert lib.pya_plan_check(plan._plan) == _lib.PYA_ERR_LIMIT and lib.pya_error_index(gpu._h) == 2
    host = guard.cpu().numpy()
    assert (host[2:] == 0x5A).all()
    _same_bytes(mz_profile_records(host[:2]), want[:2], "the slots inside the table")
    assert call(plan, cp(good), 3) == 0                                          # the call repeated with room: the report is gone
    plan.check()
    _same_bytes(mz_profile_records(table.cpu().numpy()), want, "plan")
    assert call(plan, cp(good), 2, t=guard) == 0                                 # ... and a report does not outlive the run it belongs to
    assert lib.pya_plan_check(plan._plan) == _lib.PYA_ERR_LIMIT
    plan.run(torch.from_numpy(batch["mz"]).to(dev), torch.from_numpy(batch["intensity"]).to(dev))
    plan.check()
    assert (guard.cpu().numpy()[2:] == 0x5A).all()
    # pya_score_one refuses the flag
    kw = synth.unpack_psm(batch, 0)
    m, i = np.ascontiguousarray(kw["mz_arr"], np.float64), np.ascontiguousarray(kw["int_arr"], np.float64)
    pep = np.frombuffer(kw["peptide"].encode(), np.uint8)
    one = (np.zeros(1, np.float32), np.zeros(1, np.uint64), np.zeros(1, np.int32), np.zeros((1, 4), np.float32), np.zeros((1, 4), np.uint64))
    r1 = _lib.Results(4, *[vp(x) for x in one])
    rc = lib.pya_score_one(gpu._h, vp(m), vp(i), m.size, vp(pep), pep.size, int(kw["n_of_mod"]), int(kw["max_fragment_charge"]), None, None, 0,
                           _lib.PYA_FLAG_MZ_PROFILE, C.byref(r1))
    assert rc == _lib.PYA_ERR_ARG and b"PYA_FLAG_MZ_PROFILE" in lib.pya_last_error(gpu._h)


def test_beside_the_other_stages():
    batch, settings = synth.make_batch("cfg3", n_psm=200, seed=9996)
    gpu = _gpu(settings)
    plain = gpu.score_batch(batch, evidence=True, ions=True, sites=True, probs=True, ranked=5)
    got = gpu.score_batch(batch, evidence=True, ions=True, sites=True, probs=True, ranked=5, mz_profile={})
    for key in KEYS + ("evidence", "ion_off", "ions", "site_off", "sites", "site_probs", "psm_probs", "ranked"):
        assert got[key].tobytes() == plain[key].tobytes(), key
    _same_bytes(got["mz_profile"], _want(plain, settings, None, 1), "beside the other stages")


def test_command_line_file(tmp_path):
    from pyascore_amd import PyAscore, __main__ as cli, batch_cli, ingest
    out, prof = tmp_path / "ascores.tsv", tmp_path / "profile.tsv"
    spec, ident = os.path.join(DATA, "test_spectra.mzML"), os.path.join(DATA, "test_psms.pep.xml")
    logged = []
    rows = cli.run(cli.parse_args(["--mz_error", "0.05", "--hit_depth", "2", "--mz_profile", str(prof), spec, ident, str(out)]), log=logged.append)
    plain = cli.run(cli.parse_args(["--mz_error", "0.05", "--hit_depth", "2", spec, ident, str(tmp_path / "plain.tsv")]), log=lambda *_: None)
    assert rows == plain                                                         # the main table is unchanged
    assert any("mass-error profile, slot 0" in line for line in logged)
    gpu = PyAscore(100.0, 10, "STY", 79.966331, 0.05, "by")
    spectra = ingest.SpectraParser(spec, "mzML", native_precision=True).to_dict()
    psms = sorted(ingest.IdentificationParser(ident, "pepXML").to_list(), key=lambda p: p["scan"])
    picked, scans = batch_cli.select_psms(psms, spectra, "STY", 79.966331, 2, 5)
    res = gpu.score_batch(batch_cli.pack_hits(picked, scans), skip_invalid=True, ions=True)
    settings = dict(mz_error=0.05, n_top=10)
    want = _want(res, settings, None, 1)[0]
    assert want["n_ions"] > 0
    lines = prof.read_text().splitlines()
    assert lines[0].split("\t") == list(batch_cli.MZ_PROFILE_COLUMNS)
    cells = [line.split("\t") for line in lines[1:]]
    assert len(cells) == 2 * (ru.MZP_BANDS * ru.MZP_BINS + 2)
    table = np.zeros(1, ru.MZ_PROFILE_DTYPE)
    for slot, band, unit, q, lo, hi, count in cells:
        assert slot == "0" and unit in ("da", "ppm")
        if band == "-1":
            table["out_" + unit][0, 0 if q == "-1" else 1] = int(count)
        else:
            table[unit][0, int(band), int(q)] = int(count)
            assert float(lo) < float(hi)
    for f in ("da", "ppm", "out_da", "out_ppm"):
        assert np.array_equal(table[f][0], want[f]), f
    # the bin edges of the file are those of the parameters the batch was binned with
    p = _params(settings)
    da = [c for c in cells if c[2] == "da" and c[1] == "0"]
    assert [float(c[4]) for c in da] == [(q - 32) / p["inv_da"] for q in range(64)]
    # no PSM at all: the empty table, file and summary all the same
    got = []
    assert batch_cli.localize(gpu, [], spectra, "STY", 79.966331, hit_depth=2, mz_profile=got) == []
    assert got[0].tobytes() == bytes(4128) and got[1] == p
    none = tmp_path / "none.tsv"
    batch_cli.write_mz_profile_tsv(got[0], got[1], str(none))
    assert len(none.read_text().splitlines()) == len(lines) and batch_cli.mz_profile_report(got[0], got[1])
