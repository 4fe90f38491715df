"""Site tables on the GPU (pya_site: per modifiable residue the best PepScore among the site assignments that modify it and
among those that do not).  Yardstick: tests/sites_ref.py fed with the batch_pep_scores() of a keep=True run -- pep_scores is
pinned to the reference by the parity suites, and tests/test_sites_ref.py holds the helper to the golden vectors.  Every
comparison is on raw bytes; everything goes through the C ABI or the Python on top of it."""
import ctypes as C
import os

import numpy as np
import pytest

import sites_ref
import switches
from conftest import GOLDEN, golden_cases
from oracle import harness
from pyascore_amd import _lib, sites as st, synth

pytestmark = pytest.mark.gpu

KEYS = ("best_score", "best_sig", "n_sig", "ascores", "alt_mask")


def _gpu(settings):
    from pyascore_amd import PyAscore
    return harness.make_scorer(PyAscore, settings)


def _same_sites(got, want, what):
    assert np.array_equal(got["site_off"], want["site_off"]), what
    assert got["sites"].dtype.itemsize == 32 and got["sites"].shape == want["sites"].shape, what
    bad = np.flatnonzero(got["sites"].view("V32") != want["sites"].view("V32"))
    assert bad.size == 0, "%s: records differ at %s: got %s, want %s" % (what, bad[:5].tolist(), got["sites"][bad[:5]], want["sites"][bad[:5]])


def _yardstick(gpu, settings, batch, res, sig_cap=0, status=None):
    """sites_ref over the pep_scores of a keep=True run of the same scorer"""
    kept = gpu.score_batch(batch, keep=True, skip_invalid=status is not None)
    for key in KEYS:
        assert kept[key].tobytes() == res[key].tobytes(), key
    off, rec = sites_ref.batch_records(settings, batch, res, gpu.batch_pep_scores(), synth.unpack_psm, sig_cap, status)
    return dict(site_off=off, sites=rec)


def _check_consequences(batch, got, what):
    """what the header promises of a record, against the results of the same call (and its evidence rows where present)"""
    rec, off = got["sites"], got["site_off"]
    psm = np.repeat(np.arange(int(batch["n_psm"])), np.diff(off))
    sc = rec["kind"] == st.SCORED
    inb = (rec["flags"] & st.IN_BEST) != 0
    assert not rec["reserved"].any(), what
    w = sc & inb
    assert np.array_equal(rec["with_score"][w].view(np.uint32), got["best_score"][psm[w]].view(np.uint32)), what
    assert np.array_equal(rec["with_sig"][w], got["best_sig"][psm[w]]), what
    o = sc & ~inb
    assert np.array_equal(rec["without_score"][o].view(np.uint32), got["best_score"][psm[o]].view(np.uint32)), what
    assert np.array_equal(rec["without_sig"][o], got["best_sig"][psm[o]]), what
    none = rec["kind"] == st.NONE
    assert all(r.tobytes()[:24] == b"\0" * 24 and r.tobytes()[26:] == b"\0" * 6 for r in rec[none]), what
    if "evidence" not in got:
        return 0
    tied_in = 0
    for i in range(int(batch["n_psm"])):
        r = rec[off[i]:off[i + 1]]
        if not r.size or r[0]["kind"] != st.SCORED:
            continue
        mods = np.flatnonzero((r["flags"] & st.IN_BEST) != 0)
        by_pos = {int(p): j for j, p in enumerate(r["pos"])}
        for a, e in enumerate(got["evidence"][i][: mods.size]):
            if not e["kind"]:
                continue
            assert e["comp_score"] <= r["without_score"][mods[a]], (what, i, a)
            assert e["comp_score"] <= r["with_score"][by_pos[int(e["comp_pos"])]], (what, i, a)
            if mods.size == 1:                                     # every alternative is a single move
                assert np.float32(e["comp_score"]).tobytes() == np.float32(r["without_score"][mods[0]]).tobytes(), (what, i)
                tied_in += 1
    return tied_in


def _against_yardstick(settings, batch, what, skip_invalid=False):
    gpu = _gpu(settings)
    plain = gpu.score_batch(batch, skip_invalid=skip_invalid, evidence=True, ions=True)
    got = gpu.score_batch(batch, skip_invalid=skip_invalid, evidence=True, ions=True, sites=True, site_sig_cap=0)
    for key in KEYS + ("evidence", "ion_off", "ions") + (("status",) if skip_invalid else ()):   # nothing else moves
        assert got[key].tobytes() == plain[key].tobytes(), (what, key)
    alone = gpu.score_batch(batch, skip_invalid=skip_invalid, sites=True, site_sig_cap=0)
    _same_sites(alone, got, what + " (sites alone)")
    _same_sites(got, _yardstick(gpu, settings, batch, got, 0, got["status"] if skip_invalid else None), what)
    kept = gpu.score_batch(batch, keep=True, skip_invalid=skip_invalid, sites=True, site_sig_cap=0)
    _same_sites(kept, got, what + " (keep)")
    return gpu, got, _check_consequences(batch, got, what)


@pytest.mark.parametrize("case", [c for c in golden_cases() if c.startswith(("velos_", "ties_", "edge_"))])
def test_golden_cases_equal_the_yardstick(case):
    settings, batch, exp = harness.load_case(os.path.join(GOLDEN, case + ".npz"))
    _, got, _ = _against_yardstick(settings, batch, case)
    assert (got["sites"]["kind"] == st.SCORED).any()
    if "ps_bits" in exp:                                            # ... and the golden file's own pep_scores
        off, rec = sites_ref.batch_records(settings, batch, exp, exp, synth.unpack_psm)
        _same_sites(got, dict(site_off=off, sites=rec), case + " (golden pep_scores)")


@pytest.mark.parametrize("cfg,n", [("cfg1", 300), ("cfg2", 300), ("cfg3", 200), ("cfg4", 60), ("cfg5", 24)])
def test_seeded_batches_equal_the_yardstick(cfg, n):
    batch, settings = synth.make_batch(cfg, n_psm=n, seed=9310)
    _, got, tied_in = _against_yardstick(settings, batch, cfg)
    assert (got["sites"]["kind"] == st.SCORED).all()
    if cfg in ("cfg1", "cfg2"):
        assert tied_in or int(batch["n_of_mod"].min()) > 1
    ru = st.runner_up(got["sites"], got["site_off"], got["best_sig"])
    multi = got["n_sig"] > 1
    assert ru["found"][multi].all() and (ru["sig"][multi] != got["best_sig"][multi]).all() and (ru["delta"][multi] >= 0).all()


@pytest.mark.parametrize("general", [False, True])
def test_realistic_batches_equal_the_yardstick(general):
    batch, settings = synth.make_realistic(40, seed=9320 + general, general=general)
    _, got, tied_in = _against_yardstick(settings, batch, "realistic general=%s" % general)
    assert tied_in > 0                                              # PSMs with one modification: without_score IS comp_score


ROUTES = {"default": {}, "no_fused": {"PYA_NO_FUSED": "1"}, "no_plain": {"PYA_NO_PLAIN": "1"}, "no_big": {"PYA_NO_BIG": "1"},
          "no_cnt": {"PYA_NO_CNT": "1"}, "no_loc_hash": {"PYA_NO_LOC_HASH": "1"}, "no_nodes": {"PYA_NO_NODES": "1"},
          "hash_declines": {"PYA_NO_PLAIN": "1", "PYA_DEBUG": "8192"}, "no_fork": {"PYA_NO_FORK": "1"},
          "plain_all": {"PYA_PLAIN_MIN": "0"}, "no_tiny": {"PYA_NO_TINY": "1"}}


@pytest.mark.parametrize("cfg,n", [("cfg1", 400), ("cfg2", 400), ("cfg3", 500), ("cfg4", 96), ("cfg5", 32)])
def test_every_route_leaves_the_same_records(monkeypatch, cfg, n):
    batch, settings = synth.make_batch(cfg, n_psm=n, seed=9330)
    first = None
    for name, env in ROUTES.items():
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            gpu = _gpu(settings)
            got = gpu.score_batch(batch, sites=True, site_sig_cap=0)
            if first is None:
                first = got
                _same_sites(got, _yardstick(gpu, settings, batch, got), "%s %s" % (cfg, name))
        _check_consequences(batch, got, "%s %s" % (cfg, name))
        _same_sites(got, first, "%s %s" % (cfg, name))


def test_general_kernel_psms():
    """beyond the fast kernels' limits: a peptide above 64 residues (pos beyond 64), n_top 12, five loss masses"""
    batch, settings = synth.make_batch("cfg2", n_psm=4, seed=9340, L=80, n_sites=5, n_mod=2)
    _, got, _ = _against_yardstick(settings, batch, "80 residues")
    assert (got["sites"]["pos"] > 64).any() and (got["sites"]["kind"] == st.SCORED).all()
    batch, settings = synth.make_batch("cfg2", n_psm=10, seed=9341)
    _against_yardstick(dict(settings, n_top=12), batch, "n_top 12")
    nls = [["s", 97.9769], ["t", 97.0], ["y", 79.9], ["S", 18.01528], ["T", 17.0265]]
    _against_yardstick(dict(settings, neutral_losses=nls), synth.slice_batch(batch, 0, 6), "five loss masses")


def test_sig_cap():
    """PSMs above the cap: pos and IN_BEST only; the others untouched; the default cap of a batch call is PYA_FAST_SIGNATURES"""
    batch, settings = synth.make_realistic(40, seed=9350, general=True)       # PSMs of many shapes
    gpu = _gpu(settings)
    assert gpu._lib.pya_get_site_sig_cap(gpu._h) == _lib.PYA_FAST_SIGNATURES
    full = gpu.score_batch(batch, sites=True, site_sig_cap=0)
    cap = int(np.median(full["n_sig"]))
    assert (full["n_sig"] > cap).any() and (full["n_sig"] <= cap).any()
    got = gpu.score_batch(batch, sites=True, site_sig_cap=cap)
    assert gpu._lib.pya_get_site_sig_cap(gpu._h) == _lib.PYA_FAST_SIGNATURES       # (the argument is for the call)
    _same_sites(got, _yardstick(gpu, settings, batch, got, cap), "cap %d" % cap)
    psm = np.repeat(np.arange(40), np.diff(got["site_off"]))
    over = got["n_sig"][psm] > cap
    assert (got["sites"]["kind"][over] == st.OVER).all() and got["sites"][~over].tobytes() == full["sites"][~over].tobytes()
    assert np.array_equal(got["sites"]["pos"], full["sites"]["pos"])
    assert np.array_equal(got["sites"]["flags"][over], full["sites"]["flags"][over] & st.IN_BEST)
    assert all(r.tobytes()[:24] == b"\0" * 24 for r in got["sites"][over])
    _same_sites(gpu.score_batch(batch, sites=True), full, "default cap above every PSM")


def test_unscored_and_set_aside_psms():
    good, settings = synth.make_batch("cfg2", n_psm=6, seed=9360)
    psms = []
    for i in range(good["n_psm"]):
        kw = synth.unpack_psm(good, i)
        psms.append(dict(mz=kw["mz_arr"], intensity=kw["int_arr"], peptide=kw["peptide"], n_of_mod=kw["n_of_mod"], max_charge=1))
    psms[0] = dict(psms[0], peptide="ASGTPEYIDEK", n_of_mod=3)                 # as many modifications as sites
    psms[1] = dict(psms[1], peptide="PEPTXIDESK")                              # unknown residue: set aside
    psms[2] = dict(psms[2], peptide="AGSPEPIDEK", n_of_mod=2)                  # more modifications than sites: n_sig 0
    psms[3] = dict(psms[3], mz=np.zeros(0), intensity=np.zeros(0))             # empty spectrum: set aside
    psms[4] = dict(psms[4], mz=np.array([350.0, 350.0 + 1e-9, 350.0 + 2e-9]), intensity=np.ones(3))   # one window: rejected by a kernel
    batch = synth.pack_batch(psms)
    gpu = _gpu(settings)
    plain = gpu.score_batch(batch, skip_invalid=True)
    got = gpu.score_batch(batch, skip_invalid=True, sites=True)
    for key in KEYS + ("status",):
        assert got[key].tobytes() == plain[key].tobytes(), key
    n_rec = np.diff(got["site_off"])
    assert got["status"][[1, 3]].all() and n_rec[1] == 0 and n_rec[3] == 0
    r0 = got["sites"][got["site_off"][0]:got["site_off"][1]]
    assert n_rec[0] == 3 and (r0["flags"] == (st.IN_BEST | st.NO_WITHOUT)).all() and (r0["without_score"] == -1).all()
    assert (r0["with_sig"] == 7).all() and not r0["without_sig"].any() and (r0["with_score"] == got["best_score"][0]).all()
    assert r0["pos"].tolist() == [2, 4, 7] and (r0["kind"] == st.SCORED).all()
    r2 = got["sites"][got["site_off"][2]:got["site_off"][3]]
    assert n_rec[2] == 1 and r2["kind"][0] == st.NONE and r2["pos"][0] == 3 and r2[0].tobytes()[:24] == b"\0" * 24
    if got["status"][4]:                                                       # kernel-rejected: records exist, PYA_SITE_NONE
        r4 = got["sites"][got["site_off"][4]:got["site_off"][5]]
        assert r4.size and (r4["kind"] == st.NONE).all() and r4["pos"].all()
    _same_sites(got, _yardstick(gpu, settings, batch, got, 0, got["status"]), "mixed batch")
    with pytest.raises(ValueError):                                            # without skip_invalid the call fails as before
        gpu.score_batch(batch, sites=True)
    off = np.zeros(7, np.int64)
    assert gpu._lib.pya_last_batch_sites(gpu._h, off.ctypes.data_as(C.c_void_p), None, 0) == _lib.PYA_ERR_STATE


def test_cuts_and_forms(monkeypatch):
    big = synth.make_slice(synth.describe("cfg2", 12_000, seed=9370))         # > 32 MB of spectra: worth cutting
    settings = synth.describe("cfg2", 1, seed=9370)["settings"]
    gpu = _gpu(settings)
    monkeypatch.setenv("PYA_NO_CHUNKS", "1")
    switches.from_env(gpu)
    plain = gpu.score_batch(big, evidence=True)
    whole = gpu.score_batch(big, sites=True)
    assert gpu._lib.pya_debug_last_chunks(gpu._h) == 1
    monkeypatch.delenv("PYA_NO_CHUNKS")
    monkeypatch.setenv("PYA_CHUNK_MB", "2")                                    # many chunks
    switches.from_env(gpu)
    got = gpu.score_batch(big, sites=True, evidence=True)
    assert gpu._lib.pya_debug_last_chunks(gpu._h) > 8
    monkeypatch.delenv("PYA_CHUNK_MB")
    switches.from_env(gpu)
    gpu.set_workspace_budget(48 << 20)                                         # ... and cut by the workspace budget
    small = gpu.score_batch(big, sites=True)
    assert gpu._lib.pya_debug_last_chunks(gpu._h) > 1
    gpu.set_workspace_budget(0)
    for res, what in ((got, "chunk size"), (small, "budget")):
        _same_sites(res, whole, "chunked by " + what)
        for key in KEYS:
            assert np.array_equal(res[key], plain[key]), key
    assert got["evidence"].tobytes() == plain["evidence"].tobytes()
    _check_consequences(big, got, "12 000 PSMs")                              # (the inequalities with the chunked evidence rows)
    batch = synth.slice_batch(big, 0, 1500)
    base = gpu.score_batch(batch, sites=True)
    _same_sites(base, _yardstick(gpu, settings, batch, base), "1500 PSMs")
    narrow = gpu.score_batch(synth.narrow_batch(batch), sites=True)            # float32 spectra against their widened form
    wide = gpu.score_batch(synth.widen_batch(synth.narrow_batch(batch)), sites=True)
    _same_sites(narrow, wide, "float32")
    # a shared batch against its expanded form, and in shuffled PSM order
    small_b, _ = synth.make_batch("cfg2", n_psm=60, seed=9371)
    spectra, psms = [], []
    for i in range(0, 60, 3):
        kw = synth.unpack_psm(small_b, i)
        spectra.append(dict(mz=kw["mz_arr"], intensity=kw["int_arr"]))
        for j in range(3):
            kj = synth.unpack_psm(small_b, i + j)
            psms.append(dict(peptide=kj["peptide"], n_of_mod=kj["n_of_mod"], max_charge=1, aux_pos=np.zeros(0, np.uint32),
                             aux_mass=np.zeros(0, np.float32), spectrum=len(spectra) - 1))
    shared = synth.pack_shared_batch(spectra, psms)
    flat_b = synth.expand_shared_batch(shared)
    flat = gpu.score_batch(flat_b, sites=True)
    _same_sites(flat, _yardstick(gpu, settings, flat_b, flat), "expanded")
    _same_sites(gpu.score_batch(shared, sites=True), flat, "shared")
    _same_sites(gpu.score_batch(synth.narrow_batch(shared), sites=True), gpu.score_batch(synth.narrow_batch(flat_b), sites=True), "shared float32")
    perm = np.random.default_rng(3).permutation(len(psms))
    shuffled = synth.pack_shared_batch(spectra, [psms[p] for p in perm])
    want = gpu.score_batch(synth.expand_shared_batch(shuffled), sites=True)
    _same_sites(gpu.score_batch(shuffled, sites=True), want, "shuffled shared")
    _same_sites(gpu.score_batch(shuffled, sites=True, keep=True), want, "shuffled shared, keep")
    # beside named queries: the named entry point takes the flag too
    q = [[int(b)] for b in flat["best_sig"]]
    both = gpu.score_batch(flat_b, sites=True, named=q)
    _same_sites(both, flat, "with named queries")
    assert both["named"].tobytes() == gpu.score_batch(flat_b, named=q)["named"].tobytes()


def test_plan_api():
    import torch
    from pyascore_amd.device import DevicePlan, site_records
    batch, settings = synth.make_batch("cfg3", n_psm=3000, seed=9380)          # fused PSMs beside others: the run forks
    gpu = _gpu(settings)
    want = gpu.score_batch(batch, sites=True, site_sig_cap=0)
    dev = torch.device("cuda", 0)
    mz, it = torch.from_numpy(batch["mz"]).to(dev), torch.from_numpy(batch["intensity"]).to(dev)
    plan = DevicePlan(gpu, batch)
    off = plan.site_offsets()                                                  # known before a run
    assert np.array_equal(off, want["site_off"])
    raw = torch.zeros((int(off[-1]), 32), dtype=torch.uint8, device=dev)
    assert gpu._lib.pya_plan_sites(plan._plan, C.byref(plan._res), None, 0, raw.data_ptr()) == _lib.PYA_ERR_STATE
    s1 = torch.cuda.Stream(dev)
    with torch.cuda.stream(s1):                                                # a caller stream: twice in a row
        plan.run(mz, it)
        _, a = plan.sites()
        _, b = plan.sites()
    other = torch.cuda.Stream(dev)
    with torch.cuda.stream(other):                                             # another stream than the run's waits for it
        _, c = plan.sites()
    torch.cuda.synchronize()
    plan.check()
    with torch.cuda.stream(s1):                                                # after a second run, with a cap
        plan.run(mz, it)
        _, d = plan.sites()
        cap = int(want["n_sig"].max()) - 1
        _, e = plan.sites(sig_cap=cap)
    torch.cuda.synchronize()
    plan.check()
    for t, what in ((a, "first"), (b, "again"), (c, "other stream"), (d, "second run")):
        assert site_records(t.cpu().numpy()).tobytes() == want["sites"].tobytes(), what
    capped = gpu.score_batch(batch, sites=True, site_sig_cap=cap)
    assert site_records(e.cpu().numpy()).tobytes() == capped["sites"].tobytes() and (capped["sites"]["kind"] == st.OVER).any()
    few = synth.slice_batch(batch, 0, 5)                                       # a handful of PSMs takes the per-stage launches
    p = DevicePlan(gpu, few, sites=True)
    p.run(torch.from_numpy(few["mz"]).to(dev), torch.from_numpy(few["intensity"]).to(dev))
    off5, r5 = p.sites()
    p.check()
    n5 = int(want["site_off"][5])
    assert np.array_equal(off5, want["site_off"][:6]) and site_records(r5.cpu().numpy()).tobytes() == want["sites"][:n5].tobytes()


def test_score_then_sites_and_score_one_refuses_the_flag():
    batch, settings = synth.make_batch("cfg3", n_psm=24, seed=9390)
    gpu = _gpu(settings)
    want = gpu.score_batch(batch, sites=True, site_sig_cap=0)
    for i in (3, 17):
        gpu.score(**synth.unpack_psm(batch, i))
        lo, hi = want["site_off"][i:i + 2]
        assert gpu.sites.tobytes() == want["sites"][lo:hi].tobytes()
        assert len(gpu.pep_scores) == want["n_sig"][i]                          # the PSM's own records are still there
        assert gpu.sites.tobytes() == want["sites"][lo:hi].tobytes()
    kw = synth.unpack_psm(batch, 0)
    mz, it = np.ascontiguousarray(kw["mz_arr"], np.float64), np.ascontiguousarray(kw["int_arr"], np.float64)
    pep = np.frombuffer(kw["peptide"].encode(), np.uint8)
    res = (np.zeros(1, np.float32), np.zeros(1, np.uint64), np.zeros(1, np.int32), np.zeros((1, 4), np.float32), np.zeros((1, 4), np.uint64))
    r = _lib.Results(4, *[a.ctypes.data_as(C.c_void_p) for a in res])
    rc = gpu._lib.pya_score_one(gpu._h, mz.ctypes.data_as(C.c_void_p), it.ctypes.data_as(C.c_void_p), mz.size,
                                pep.ctypes.data_as(C.c_void_p), pep.size, int(kw["n_of_mod"]), int(kw["max_fragment_charge"]), None, None, 0,
                                _lib.PYA_FLAG_SITES, C.byref(r))
    assert rc == _lib.PYA_ERR_ARG and b"PYA_FLAG_SITES" in gpu._lib.pya_last_error(gpu._h)


def test_batch_cli_site_table():
    from test_batch_cli import _toy_inputs
    from pyascore_amd import PyAscore, batch_cli
    spectra, psms = _toy_inputs()
    gpu = PyAscore(100.0, 10, "STY", 79.966331, 0.05, "by")
    plain = batch_cli.localize(gpu, psms, spectra, "STY", 79.966331, hit_depth=2, max_fragment_charge=3)
    table = []
    wide = batch_cli.localize(gpu, psms, spectra, "STY", 79.966331, hit_depth=2, max_fragment_charge=3, sites=table)
    assert len(plain) == len(wide) and all(len(r) == 7 for r in wide)
    assert all(str(a) == str(b) for ra, rb in zip(wide, plain) for a, b in zip(ra[:5], rb))     # the first five as they were
    assert table and all(len(r) == len(batch_cli.SITE_COLUMNS) for r in table)
    by_scan = {}
    for r in table:
        by_scan.setdefault(r[0], []).append(r)
    seen = 0
    for row in wide:
        if not row[1] or row[0] not in by_scan:
            continue
        mine = [r for r in by_scan[row[0]] if r[4] == "1" and r[8] == row[1]]       # the winner's residues of this hit
        if not mine:
            continue
        assert all(np.float32(r[5]) == np.float32(row[2]) for r in mine)                            # WithScore of a winner's residue: PepScore
        if row[5]:
            best_without = max(np.float32(r[6]) for r in mine if r[6])
            assert np.float32(row[2]) - np.float32(best_without) == np.float32(row[6]) and row[5] != row[1]
            seen += 1
    assert seen
