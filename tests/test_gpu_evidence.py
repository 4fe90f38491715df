"""Evidence records on the GPU (pya_evidence: the depth an Ascore was taken at, the site-determining ions possible and
matched on both sides, the competitor and its PepScore; cpp/Ascore.cpp:157-254).  The yardstick is tests/evidence_ref.py,
which builds the rows on the CPU from the reference-pinned scripting classes and is itself held to the golden vectors
(tests/test_evidence_ref.py).  Everything here goes through the C ABI or the Python on top of it."""
import ctypes as C
import os

import numpy as np
import pytest

import evidence_ref
import fuzzcase
import switches
from conftest import GOLDEN
from oracle import harness
from pyascore_amd import _lib, batch_cli, synth

pytestmark = pytest.mark.gpu

KEYS = ("best_score", "best_sig", "n_sig", "ascores", "alt_mask")
PHOSPHO = 79.966331


def _gpu(settings):
    from pyascore_amd import PyAscore
    return harness.make_scorer(PyAscore, settings)


def _same_rows(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = np.argwhere(got.view("V16") != want.view("V16"))
    assert bad.size == 0, "%s: evidence differs at (PSM, site) %s: got %s, want %s" % (
        what, bad[:5].tolist(), [got[tuple(b)] for b in bad[:5]], [want[tuple(b)] for b in bad[:5]])


def _check_invariant(settings, res, what):
    """kind against ascores, comp_pos in alt_mask, and the two scores of every counted row against the Ascore's bits"""
    ev, asc = res["evidence"], res["ascores"]
    none, tied, counted = (ev["kind"] == k for k in (evidence_ref.NONE, evidence_ref.TIED, evidence_ref.COUNTED))
    scored = (res["n_sig"] > 0)[:, None] & np.isfinite(asc)
    assert not (none & scored & (res["alt_mask"] != 0)).any(), what
    assert (asc[tied] == 0.).all(), what
    zero = np.zeros((), ev.dtype)
    assert (ev[none] == zero).all(), what
    cache = {}
    for i, a in np.argwhere(counted):
        e = ev[i, a]
        key = (int(e["depth"]), int(e["ref_possible"]), int(e["ref_matched"]), int(e["comp_possible"]), int(e["comp_matched"]))
        if key not in cache:
            cache[key] = np.float32(evidence_ref.score(settings, key[0], key[1], key[2]) - evidence_ref.score(settings, key[0], key[3], key[4]))
        assert cache[key].tobytes() == np.float32(asc[i, a]).tobytes(), (what, i, a, e, asc[i, a])


def _against_yardstick(settings, batch, what, skip_invalid=False):
    gpu = _gpu(settings)
    plain = gpu.score_batch(batch, skip_invalid=skip_invalid)
    got = gpu.score_batch(batch, skip_invalid=skip_invalid, evidence=True)
    for key in KEYS + (("status",) if skip_invalid else ()):                  # asking for evidence changes nothing else
        assert np.array_equal(got[key].view(np.uint8), plain[key].view(np.uint8)), (what, key)
    assert got["evidence"].shape == got["ascores"].shape and got["evidence"].dtype.itemsize == 16
    kept = gpu.score_batch(batch, keep=True, skip_invalid=skip_invalid, evidence=True)
    _same_rows(kept["evidence"], got["evidence"], what + " (keep)")
    ps = gpu.batch_pep_scores()
    want, _ = evidence_ref.batch_rows(settings, batch, got, ps, synth.unpack_psm)
    _same_rows(got["evidence"], want, what)
    _check_invariant(settings, got, what)
    return got


@pytest.mark.parametrize("case", ["velos_z1", "velos_nl", "velos_zprec", "ties_cfg2", "edge_default", "edge_nl", "edge_Zc",
                                  "edge_nKc", "edge_highres", "edge_err05", "edge_yb"])
def test_goldens_equal_the_yardstick(case):
    settings, batch, exp = harness.load_case(os.path.join(GOLDEN, case + ".npz"))
    got = _against_yardstick(settings, batch, case)
    if case == "ties_cfg2":
        assert (got["evidence"]["kind"] == evidence_ref.TIED).any()


@pytest.mark.parametrize("cfg,n", [("cfg1", 48), ("cfg2", 64), ("cfg3", 48), ("cfg4", 24), ("cfg5", 16)])
def test_synth_slices_equal_the_yardstick(cfg, n):
    batch, settings = synth.make_batch(cfg, n_psm=n, seed=9100)
    _against_yardstick(settings, batch, cfg)


@pytest.mark.parametrize("general", [False, True])
def test_realistic_batches_equal_the_yardstick(general):
    """isotope doublets inside the tolerance: the greedy cancellation and the two-partner cases"""
    batch, settings = synth.make_realistic(40, seed=9200 + general, general=general)
    got = _against_yardstick(settings, batch, "realistic general=%s" % general)
    assert (got["evidence"]["kind"] == evidence_ref.COUNTED).any()


def test_fuzz_cases_equal_the_yardstick():
    rng = np.random.default_rng(9300)
    done = 0
    while done < 6:
        settings, batch = fuzzcase.random_case(rng)[:2]
        if batch["n_psm"] == 0:
            continue
        _against_yardstick(settings, batch, "fuzz %d" % done, skip_invalid=True)
        done += 1


ROUTES = {"default": {}, "no_fused": {"PYA_NO_FUSED": "1"}, "no_plain": {"PYA_NO_PLAIN": "1"}, "no_big": {"PYA_NO_BIG": "1"},
          "no_cnt": {"PYA_NO_CNT": "1"}, "no_loc_hash": {"PYA_NO_LOC_HASH": "1"}, "no_nodes": {"PYA_NO_NODES": "1"},
          "hash_declines": {"PYA_NO_PLAIN": "1", "PYA_DEBUG": "8192"}, "no_fork": {"PYA_NO_FORK": "1"},
          "plain_all": {"PYA_PLAIN_MIN": "0"}, "no_tiny": {"PYA_NO_TINY": "1"}}


@pytest.mark.parametrize("cfg,n", [("cfg3", 700), ("cfg4", 96), ("cfg5", 48)])
def test_every_route_writes_the_same_rows(monkeypatch, cfg, n):
    """the invariant against what each route wrote, and identical rows whoever scored and localised the PSM"""
    batch, settings = synth.make_batch(cfg, n_psm=n, seed=9400)
    first = None
    for name, env in ROUTES.items():
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            got = _gpu(settings).score_batch(batch, evidence=True)
        _check_invariant(settings, got, "%s %s" % (cfg, name))
        in_alt = [int(p) in evidence_ref.alt_positions(got["alt_mask"][i, a], "x" * 8, []) for i, a in np.argwhere(got["evidence"]["kind"] != 0)
                  for p in [got["evidence"]["comp_pos"][i, a]]]
        assert all(in_alt), name
        if first is None:
            first = got
        else:
            _same_rows(got["evidence"], first["evidence"], "%s %s" % (cfg, name))
            for key in KEYS:
                assert np.array_equal(got[key], first[key]), (name, key)


def test_cuts_and_forms(monkeypatch):
    big = synth.make_slice(synth.describe("cfg2", 12_000, seed=9500))         # > 32 MB of spectra: worth cutting
    settings = synth.describe("cfg2", 1, seed=9500)["settings"]
    gpu = _gpu(settings)
    monkeypatch.setenv("PYA_NO_CHUNKS", "1")
    switches.from_env(gpu)
    whole = gpu.score_batch(big, evidence=True)
    assert gpu._lib.pya_debug_last_chunks(gpu._h) == 1
    monkeypatch.delenv("PYA_NO_CHUNKS")
    monkeypatch.setenv("PYA_CHUNK_MB", "2")                                    # many chunks
    switches.from_env(gpu)
    got = gpu.score_batch(big, evidence=True)
    assert gpu._lib.pya_debug_last_chunks(gpu._h) > 8
    monkeypatch.delenv("PYA_CHUNK_MB")
    switches.from_env(gpu)
    _same_rows(got["evidence"], whole["evidence"], "chunked")
    for key in KEYS:
        assert np.array_equal(got[key], whole[key]), key
    assert (whole["evidence"]["kind"] == evidence_ref.COUNTED).any()
    batch = synth.slice_batch(big, 0, 2000)
    narrow = gpu.score_batch(synth.narrow_batch(batch), evidence=True)           # float32 spectra against their widened form
    wide = gpu.score_batch(synth.widen_batch(synth.narrow_batch(batch)), evidence=True)
    _same_rows(narrow["evidence"], wide["evidence"], "float32")
    # a shared batch against its expanded form, and in shuffled PSM order
    small, _ = synth.make_batch("cfg2", n_psm=60, seed=9501)
    spectra, psms = [], []
    for i in range(0, 60, 3):
        kw = synth.unpack_psm(small, i)
        spectra.append(dict(mz=kw["mz_arr"], intensity=kw["int_arr"]))
        for j in range(3):
            kj = synth.unpack_psm(small, i + j)
            psms.append(dict(peptide=kj["peptide"], n_of_mod=kj["n_of_mod"], max_charge=1, aux_pos=np.zeros(0, np.uint32),
                             aux_mass=np.zeros(0, np.float32), spectrum=len(spectra) - 1))
    shared = synth.pack_shared_batch(spectra, psms)
    flat = gpu.score_batch(synth.expand_shared_batch(shared), evidence=True)
    sh = gpu.score_batch(shared, evidence=True)
    _same_rows(sh["evidence"], flat["evidence"], "shared")
    assert (sh["evidence"]["kind"] != 0).any()
    perm = np.random.default_rng(3).permutation(len(psms))
    shuffled = synth.pack_shared_batch(spectra, [psms[p] for p in perm])
    back = gpu.score_batch(shuffled, evidence=True)
    _same_rows(back["evidence"], flat["evidence"][perm], "shuffled shared")


def test_plan_api():
    import torch
    from pyascore_amd.device import DevicePlan, evidence_rows
    batch, settings = synth.make_batch("cfg3", n_psm=3000, seed=9600)          # fused PSMs beside others: the run forks
    gpu = _gpu(settings)
    want = gpu.score_batch(batch, evidence=True)
    dev = torch.device("cuda", 0)
    mz, it = torch.from_numpy(batch["mz"]).to(dev), torch.from_numpy(batch["intensity"]).to(dev)
    plan = DevicePlan(gpu, batch)
    raw = torch.zeros((plan.n_psm, plan.max_k, 16), dtype=torch.uint8, device=dev)
    rc = gpu._lib.pya_plan_evidence(plan._plan, C.byref(plan._res), None, raw.data_ptr())
    assert rc == _lib.PYA_ERR_STATE                                           # before the first run
    st = torch.cuda.Stream(dev)
    with torch.cuda.stream(st):                                                # a caller stream, twice in a row
        plan.run(mz, it)
        a = plan.evidence()
        b = plan.evidence()
    other = torch.cuda.Stream(dev)
    with torch.cuda.stream(other):                                             # another stream than the run's waits for it
        c = plan.evidence()
    torch.cuda.synchronize()
    plan.check()
    for t, what in ((a, "first"), (b, "second"), (c, "other stream")):
        _same_rows(evidence_rows(t.cpu().numpy()), want["evidence"], "plan " + what)
    assert np.array_equal(plan.ascores.cpu().numpy(), want["ascores"])
    few = synth.slice_batch(batch, 0, 5)                                       # a handful of PSMs: the one-launch kernel, or not
    for flag in (False, True):
        p = DevicePlan(gpu, few, evidence=flag)
        mz5, it5 = torch.from_numpy(few["mz"]).to(dev), torch.from_numpy(few["intensity"]).to(dev)
        p.run(mz5, it5)
        rows = evidence_rows(p.evidence().cpu().numpy())
        p.check()
        assert not want["evidence"][:5, p.max_k:]["kind"].any()
        _same_rows(rows, np.ascontiguousarray(want["evidence"][:5, :p.max_k]), "plan of five, evidence=%s" % flag)


def _general_case(settings, batch, what):
    got = _against_yardstick(settings, batch, what)
    assert (got["evidence"]["kind"] == evidence_ref.COUNTED).any(), what
    return got


def test_general_route_long_peptide():
    batch, settings = synth.make_batch("cfg2", n_psm=4, seed=9700, L=80, n_sites=5, n_mod=2)
    got = _general_case(settings, batch, "80 residues")
    for i in range(batch["n_psm"]):                                           # comp_pos is a peptide position, not a site bit
        pep = synth.unpack_psm(batch, i)["peptide"]
        sites = evidence_ref.modifiable_positions(pep, settings["mod_group"])
        for e in got["evidence"][i]:
            if e["kind"]:
                assert int(e["comp_pos"]) - 1 in sites


def test_general_route_n_top_12():
    batch, settings = synth.make_batch("cfg2", n_psm=12, seed=9701)
    _general_case(dict(settings, n_top=12), batch, "n_top 12")


def test_general_route_big_spectrum():
    rng = np.random.default_rng(9702)
    small, settings = synth.make_batch("cfg2", n_psm=4, seed=9702)
    psms = []
    for i in range(small["n_psm"]):
        kw = synth.unpack_psm(small, i)
        mz, it = kw["mz_arr"], kw["int_arr"]
        if i == 1:
            mz = np.concatenate([mz, rng.uniform(100.0, 2500.0, 9000 - mz.size)])
            it = np.concatenate([it, rng.lognormal(4.0, 1.0, 9000 - it.size)])
            o = np.argsort(mz, kind="stable")
            mz, it = mz[o], it[o]
        psms.append(dict(mz=mz, intensity=it, peptide=kw["peptide"], n_of_mod=kw["n_of_mod"], max_charge=1))
    _general_case(settings, synth.pack_batch(psms), "9 000 peaks")


def test_general_route_six_loss_masses():
    batch, settings = synth.make_batch("cfg2", n_psm=8, seed=9703)
    nls = [["s", 97.9769], ["t", 97.0], ["y", 79.9], ["S", 18.01528], ["T", 17.0265], ["Y", 63.998]]
    _general_case(dict(settings, neutral_losses=nls), batch, "six loss masses")


def test_set_aside_psms_have_zero_rows():
    good, settings = synth.make_batch("cfg2", n_psm=6, seed=9800)
    psms = []
    for i in range(good["n_psm"]):
        kw = synth.unpack_psm(good, i)
        psms.append(dict(mz=kw["mz_arr"], intensity=kw["int_arr"], peptide=kw["peptide"], n_of_mod=kw["n_of_mod"], max_charge=1))
    psms[1] = dict(psms[1], peptide="PEPTXIDESK")                              # unknown residue
    psms[3] = dict(psms[3], mz=np.zeros(0), intensity=np.zeros(0))             # empty spectrum
    psms[4] = dict(psms[4], peptide="S" * 40 + "K", n_of_mod=20)              # C(40, 20) site assignments: over a limit
    batch = synth.pack_batch(psms)
    gpu = _gpu(settings)
    got = gpu.score_batch(batch, skip_invalid=True, evidence=True)
    assert got["status"][[1, 3, 4]].all() and not got["status"][[0, 2, 5]].any()
    assert (got["evidence"][[1, 3, 4]] == np.zeros((), got["evidence"].dtype)).all()
    clean = gpu.score_batch(synth.pack_batch([psms[i] for i in (0, 2, 5)]), evidence=True)
    k = clean["evidence"].shape[1]
    _same_rows(np.ascontiguousarray(got["evidence"][[0, 2, 5]][:, :k]), clean["evidence"], "neighbours of set-aside PSMs")
    assert (clean["evidence"]["kind"] != 0).any()
    gpu.score_batch(batch, skip_invalid=True)                                  # ... and without the flag there is nothing to read
    buf = np.zeros((6, got["evidence"].shape[1]), got["evidence"].dtype)
    assert gpu._lib.pya_last_batch_evidence(gpu._h, buf.ctypes.data_as(C.c_void_p), 6, buf.shape[1]) == _lib.PYA_ERR_STATE
    gpu.score_batch(batch, skip_invalid=True, evidence=True)
    assert gpu._lib.pya_last_batch_evidence(gpu._h, buf.ctypes.data_as(C.c_void_p), 5, buf.shape[1]) == _lib.PYA_ERR_ARG
    assert gpu._lib.pya_last_batch_evidence(gpu._h, buf.ctypes.data_as(C.c_void_p), 6, buf.shape[1]) == _lib.PYA_OK
    _same_rows(buf, got["evidence"], "pya_last_batch_evidence")


def test_score_one_refuses_the_flag():
    batch, settings = synth.make_batch("cfg2", n_psm=1, seed=9801)
    gpu = _gpu(settings)
    kw = synth.unpack_psm(batch, 0)
    pep = np.frombuffer(kw["peptide"].encode(), np.uint8)
    res = [np.zeros(1, np.float32), np.zeros(1, np.uint64), np.zeros(1, np.int32), np.zeros(3, np.float32), np.zeros(3, np.uint64)]
    r = _lib.Results(3, *[a.ctypes.data_as(C.c_void_p) for a in res])
    rc = gpu._lib.pya_score_one(gpu._h, kw["mz_arr"].ctypes.data, kw["int_arr"].ctypes.data, kw["mz_arr"].size, pep.ctypes.data,
                                pep.size, kw["n_of_mod"], 1, None, None, 0, _lib.PYA_FLAG_EVIDENCE, C.byref(r))
    assert rc == _lib.PYA_ERR_ARG and b"PYA_FLAG_EVIDENCE" in gpu._lib.pya_last_error(gpu._h)


def test_score_then_evidence_property():
    batch, settings = synth.make_batch("cfg3", n_psm=24, seed=9900)
    gpu = _gpu(settings)
    want = gpu.score_batch(batch, evidence=True)
    for i in (3, 17):
        kw = synth.unpack_psm(batch, i)
        gpu.score(**kw)
        k = kw["n_of_mod"]
        _same_rows(gpu.evidence.reshape(1, -1), want["evidence"][i:i + 1, :k].copy(), "score(%d).evidence" % i)
        assert np.array_equal(gpu.ascores, want["ascores"][i, :k])
    # the lazy-records guard: an intervening score_batch must not make the property answer for another PSM
    gpu.score(**synth.unpack_psm(batch, 3))
    gpu.score_batch(synth.slice_batch(batch, 17, 18))
    gpu.score_batch(synth.slice_batch(batch, 5, 12), evidence=True)
    k = int(batch["n_of_mod"][3])
    _same_rows(gpu.evidence.reshape(1, -1), want["evidence"][3:4, :k].copy(), "evidence after an intervening score_batch")
    assert len(gpu.pep_scores) == int(want["n_sig"][3])


def test_batch_cli_columns():
    from test_batch_cli import _toy_inputs
    from pyascore_amd import PyAscore
    spectra, psms = _toy_inputs()
    gpu = PyAscore(100.0, 10, "STY", PHOSPHO, 0.05, "by")
    plain = batch_cli.localize(gpu, psms, spectra, "STY", PHOSPHO, hit_depth=2, max_fragment_charge=3)
    wide = batch_cli.localize(gpu, psms, spectra, "STY", PHOSPHO, hit_depth=2, max_fragment_charge=3, evidence=True)
    assert len(plain) == len(wide) and all(len(r) == 5 for r in plain) and all(len(r) == 8 for r in wide)
    assert [r[:5] for r in wide] == plain or all(str(a) == str(b) for ra, rb in zip(wide, plain) for a, b in zip(ra[:5], rb))
    picked, scans = batch_cli.select_psms(psms, spectra, "STY", PHOSPHO, 2, 3)
    res = gpu.score_batch(batch_cli.pack_hits(picked, scans), skip_invalid=True, evidence=True)
    seen = set()
    for i, row in enumerate(wide):
        k = picked[i]["n_of_mod"]
        assert row[5:] == batch_cli.evidence_fields(res["evidence"][i, :k])
        depth, ions, comp = (f.split(";") for f in row[5:])
        assert len(depth) == len(ions) == len(comp) == k
        for a in range(k):
            e = res["evidence"][i, a]
            seen.add(int(e["kind"]))
            if e["kind"] == evidence_ref.COUNTED:
                assert depth[a] == str(int(e["depth"]) + 1) and float(comp[a]) == float(e["comp_score"])
                assert ions[a] == "%d/%d|%d/%d" % (e["ref_matched"], e["ref_possible"], e["comp_matched"], e["comp_possible"])
            elif e["kind"] == evidence_ref.TIED:
                assert ions[a] == "tie" and depth[a] == ""
            else:
                assert depth[a] == ions[a] == comp[a] == ""
    assert evidence_ref.COUNTED in seen
