"""Named localisations on the GPU (pya_named: the score container of a signature the caller names and its ambiguity against
the winner; cpp/Ascore.cpp:53-210).  Yardsticks: the reference's own core (score, pep_scores, calculate_ambiguity) and
tests/named_ref.py, which tests/test_named_ref.py holds to the golden vectors and to that core.  Every comparison is on
bit patterns; everything goes through the C ABI or the Python on top of it."""
import ctypes as C
import os

import numpy as np
import pytest

import evidence_ref
import named_ref
import switches
from conftest import GOLDEN, checker_kind
from oracle import harness, orc
from pyascore_amd import _lib, named as nm, synth

pytestmark = pytest.mark.gpu

KEYS = ("best_score", "best_sig", "n_sig", "ascores", "alt_mask")


def _gpu(settings):
    from pyascore_amd import PyAscore
    return harness.make_scorer(PyAscore, settings)


def _same_named(got, want, what):
    """records as 32 raw bytes, the two optional arrays as their bits"""
    assert np.array_equal(got["named_off"], want["named_off"]), what
    assert got["named"].dtype.itemsize == 32 and got["named"].shape == want["named"].shape, what
    bad = np.flatnonzero(got["named"].view("V32") != want["named"].view("V32"))
    assert bad.size == 0, "%s: records differ at queries %s: got %s, want %s" % (what, bad[:5].tolist(), got["named"][bad[:5]], want["named"][bad[:5]])
    assert np.array_equal(got["named_counts"], want["named_counts"]), what
    assert np.array_equal(got["named_scores"].view(np.uint32), want["named_scores"].view(np.uint32)), what


def _n_sites(settings, batch, i):
    return len(nm.site_residues(synth.unpack_psm(batch, i)["peptide"], settings["mod_group"]))


def _queries(settings, batch, res, rng, mode):
    """one list of signatures per PSM.  mix: the winner, every single move, a multi-move, three malformed ones, a duplicate
    (every fifth PSM: no query); one: a random single move; moves: all k(n - k) single moves"""
    out = []
    for i in range(int(batch["n_psm"])):
        ns, k, best = _n_sites(settings, batch, i), int(batch["n_of_mod"][i]), int(res["best_sig"][i])
        moves = [q for _, _, q in named_ref.single_moves(best, ns)] if res["n_sig"][i] > 0 and bin(best).count("1") == k else []
        if mode == "one":
            out.append([moves[int(rng.integers(len(moves)))]] if moves else [best])
        elif mode == "moves":
            out.append(moves)
        elif i % 5 == 4:
            out.append([])
        else:
            q = [best] + moves
            if ns - k >= 2 and k >= 2:                                # two modifications moved at once
                free = [j for j in range(ns) if not best >> j & 1]
                mods = [j for j in range(ns) if best >> j & 1]
                q.append((best & ~(1 << mods[0]) & ~(1 << mods[-1])) | (1 << free[0]) | (1 << free[-1]))
            q += [0 if k else 1, best | (1 << ns) if ns < 64 else 0, (best | ((1 << ns) - 1)) if k < ns else best ^ 1]
            q += moves[:1]
            out.append(q)
    return out


def _against_yardstick(settings, batch, what, mode="mix", skip_invalid=False, seed=1):
    gpu = _gpu(settings)
    plain = gpu.score_batch(batch, skip_invalid=skip_invalid, evidence=True, ions=True)
    queries = _queries(settings, batch, plain, np.random.default_rng(seed), mode)
    got = gpu.score_batch(batch, skip_invalid=skip_invalid, evidence=True, ions=True, named=queries)
    for key in KEYS + ("evidence", "ion_off", "ions") + (("status",) if skip_invalid else ()):   # nothing else moves
        assert got[key].tobytes() == plain[key].tobytes(), (what, key)
    alone = gpu.score_batch(batch, skip_invalid=skip_invalid, named=queries)
    _same_named(alone, got, what + " (named alone)")
    kept = gpu.score_batch(batch, keep=True, skip_invalid=skip_invalid, named=queries)
    _same_named(kept, got, what + " (keep)")
    ps = gpu.batch_pep_scores()
    rec, counts, scores = named_ref.batch_records(settings, batch, got, ps, got["named_off"], np.concatenate(
        [np.asarray(q, np.uint64) for q in queries] + [np.zeros(0, np.uint64)]), synth.unpack_psm)
    _same_named(got, dict(named_off=got["named_off"], named=rec, named_counts=counts, named_scores=scores), what)
    _check_invariants(settings, batch, got, what)
    return gpu, got, queries


def _check_invariants(settings, batch, got, what):
    rec, off = got["named"], got["named_off"]
    psm = np.repeat(np.arange(int(batch["n_psm"])), np.diff(off))
    win = rec["kind"] == named_ref.WINNER
    assert np.array_equal(rec["pep_score"][win].view(np.uint32), got["best_score"][psm[win]].view(np.uint32)), what
    assert (rec["sig_bits"][win] == got["best_sig"][psm[win]]).all() and not rec["ambiguity"][win].any(), what
    low = rec["kind"] <= named_ref.INVALID
    assert not got["named_counts"][low].any() and not got["named_scores"][low].any(), what
    assert not rec["reserved"].any(), what
    for f in ("depth", "ref_matched", "ref_possible", "comp_matched", "comp_possible"):
        assert not rec[f][rec["kind"] != named_ref.COUNTED].any(), (what, f)
    cache = {}
    for r in rec[rec["kind"] == named_ref.COUNTED]:
        key = (int(r["depth"]), int(r["ref_possible"]), int(r["ref_matched"]), int(r["comp_possible"]), int(r["comp_matched"]))
        if key not in cache:
            cache[key] = np.float32(evidence_ref.score(settings, key[0], key[1], key[2]) - evidence_ref.score(settings, key[0], key[3], key[4]))
        assert cache[key].tobytes() == np.float32(r["ambiguity"]).tobytes(), (what, r)


def _evidence_tie_in(settings, batch, got, what):
    """the winner with site j moved to an evidence row's comp_pos: that row's depth and counts, ambiguity == ascores[j]"""
    seen = set()
    for i in range(int(batch["n_psm"])):
        pep = synth.unpack_psm(batch, i)["peptide"]
        sites = nm.site_residues(pep, settings["mod_group"])
        best = int(got["best_sig"][i])
        mods = [j for j in range(len(sites)) if best >> j & 1]
        recs = {int(r["sig_bits"]): r for r in got["named"][got["named_off"][i]:got["named_off"][i + 1]]}
        for a, e in enumerate(got["evidence"][i]):
            if not e["kind"] or a >= len(mods):
                continue
            q = (best & ~(1 << mods[a])) | (1 << sites.index(int(e["comp_pos"]) - 1))
            if q not in recs:
                continue
            r = recs[q]
            seen.add(int(e["kind"]))
            assert np.float32(r["pep_score"]).tobytes() == np.float32(e["comp_score"]).tobytes(), (what, i, a)
            if e["kind"] == evidence_ref.TIED:
                assert r["kind"] == named_ref.TIED, (what, i, a)
            else:
                assert r["kind"] == named_ref.COUNTED and np.float32(r["ambiguity"]).tobytes() == np.float32(got["ascores"][i, a]).tobytes()
                for f in ("depth", "ref_matched", "ref_possible", "comp_matched", "comp_possible"):
                    assert r[f] == e[f], (what, i, a, f)
    return seen


@pytest.mark.parametrize("case", ["velos_z1", "velos_nl", "velos_zprec", "ties_cfg2", "edge_default", "edge_nl", "edge_Zc",
                                  "edge_nKc", "edge_highres", "edge_err05", "edge_yb"])
def test_goldens_equal_the_yardstick(case):
    settings, batch, exp = harness.load_case(os.path.join(GOLDEN, case + ".npz"))
    _, got, _ = _against_yardstick(settings, batch, case)
    seen = _evidence_tie_in(settings, batch, got, case)
    kinds = set(got["named"]["kind"].tolist())
    assert {named_ref.INVALID, named_ref.WINNER} <= kinds
    if case == "ties_cfg2":
        assert named_ref.TIED in kinds and evidence_ref.TIED in seen
    if case == "velos_z1":
        assert named_ref.COUNTED in kinds and evidence_ref.COUNTED in seen and (got["named"]["n_moved"] > 1).any()


@pytest.mark.parametrize("cfg,n", [("cfg1", 48), ("cfg2", 64), ("cfg3", 48), ("cfg4", 24), ("cfg5", 16)])
def test_synth_slices_equal_the_yardstick(cfg, n):
    batch, settings = synth.make_batch(cfg, n_psm=n, seed=9100)
    _, got, _ = _against_yardstick(settings, batch, cfg)
    assert evidence_ref.COUNTED in _evidence_tie_in(settings, batch, got, cfg)


@pytest.mark.parametrize("general", [False, True])
def test_realistic_batches_equal_the_yardstick(general):
    batch, settings = synth.make_realistic(40, seed=9200 + general, general=general)
    _, got, _ = _against_yardstick(settings, batch, "realistic general=%s" % general)
    assert (got["named"]["kind"] == named_ref.COUNTED).any()


@pytest.mark.parametrize("case,n", [("velos_z1", 10), ("velos_nl", 8), ("cfg2", 10), ("cfg3", 6)])
def test_the_reference_core_itself(case, n):
    """score, pep_scores and calculate_ambiguity(pep_scores[0], rec) of the reference's own core for EVERY site assignment
    of small PSMs, in the reference's sorted order; the same records as batch_pep_scores() of a keep=True run"""
    if case.startswith("cfg"):
        batch, settings = synth.make_batch(case, n_psm=n, seed=9150)
    else:
        settings, batch, _ = harness.load_case(os.path.join(GOLDEN, case + ".npz"))
        batch = synth.slice_batch(batch, 0, min(n, int(batch["n_psm"])))
    ref = harness.make_scorer(orc.OracleAscore, settings, kind=checker_kind())
    gpu = _gpu(settings)
    kept = gpu.score_batch(batch, keep=True)
    ps = gpu.batch_pep_scores()
    queries = [ps["sig_bits"][ps["rec_off"][i]:ps["rec_off"][i + 1]] for i in range(int(batch["n_psm"]))]
    assert sum(q.size for q in queries) > 2 * batch["n_psm"]
    got = gpu.score_batch(batch, named=queries)
    assert np.array_equal(got["named_off"], ps["rec_off"]) and np.array_equal(got["named"]["sig_bits"], ps["sig_bits"])
    assert np.array_equal(got["named"]["pep_score"].view(np.uint32), ps["weighted_score"].view(np.uint32))
    assert np.array_equal(got["named"]["total_fragments"], ps["total_fragments"].astype(np.uint32))
    assert np.array_equal(got["named_counts"], ps["counts"])
    assert np.array_equal(got["named_scores"].view(np.uint32), ps["scores"].view(np.uint32))
    for i in range(int(batch["n_psm"])):
        ref.score(**synth.unpack_psm(batch, i))
        want = ref.pep_scores
        recs = got["named"][got["named_off"][i]:got["named_off"][i + 1]]
        assert len(want) == recs.size == kept["n_sig"][i]
        assert recs[0]["kind"] == named_ref.WINNER and np.float32(ref.best_score).tobytes() == np.float32(recs[0]["pep_score"]).tobytes()
        for r, w in zip(recs, want):
            assert int(r["sig_bits"]) == harness.sig_bits(w["signature"])
            assert np.float32(r["pep_score"]).tobytes() == np.float32(w["weighted_score"]).tobytes()
            amb = np.float32(ref.calculate_ambiguity(want[0], w)) if r["kind"] != named_ref.WINNER else np.float32(0)
            assert np.float32(r["ambiguity"]).tobytes() == amb.tobytes(), (i, r, amb)


ROUTES = {"default": {}, "no_fused": {"PYA_NO_FUSED": "1"}, "no_plain": {"PYA_NO_PLAIN": "1"}, "no_big": {"PYA_NO_BIG": "1"},
          "no_cnt": {"PYA_NO_CNT": "1"}, "no_loc_hash": {"PYA_NO_LOC_HASH": "1"}, "no_nodes": {"PYA_NO_NODES": "1"},
          "hash_declines": {"PYA_NO_PLAIN": "1", "PYA_DEBUG": "8192"}, "no_fork": {"PYA_NO_FORK": "1"},
          "plain_all": {"PYA_PLAIN_MIN": "0"}, "no_tiny": {"PYA_NO_TINY": "1"}}


@pytest.mark.parametrize("cfg,n", [("cfg3", 700), ("cfg4", 96), ("cfg5", 48)])
def test_every_route_leaves_the_same_records(monkeypatch, cfg, n):
    """fused, count-node, big, hash and general-instantiation PSMs: whoever scored and localised a PSM, the stage reads the
    same retained tables and winner"""
    batch, settings = synth.make_batch(cfg, n_psm=n, seed=9400)
    first = queries = None
    for name, env in ROUTES.items():
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            gpu = _gpu(settings)
            if queries is None:
                queries = _queries(settings, batch, gpu.score_batch(batch), np.random.default_rng(2), "mix")
            got = gpu.score_batch(batch, named=queries)
        _check_invariants(settings, batch, got, "%s %s" % (cfg, name))
        if first is None:
            first = got
        else:
            _same_named(got, first, "%s %s" % (cfg, name))
    assert (first["named"]["kind"] == named_ref.COUNTED).any()


def test_general_kernel_psms():
    """beyond the fast kernels' limits: a peptide above 64 residues, n_top 12, five loss masses"""
    batch, settings = synth.make_batch("cfg2", n_psm=4, seed=9700, L=80, n_sites=5, n_mod=2)
    _, got, _ = _against_yardstick(settings, batch, "80 residues")
    assert (got["named"]["kind"] == named_ref.COUNTED).any()
    batch, settings = synth.make_batch("cfg2", n_psm=10, seed=9701)
    _, got, _ = _against_yardstick(dict(settings, n_top=12), batch, "n_top 12")
    assert got["named_counts"].shape[1] == 12 and (got["named"]["kind"] == named_ref.COUNTED).any()
    nls = [["s", 97.9769], ["t", 97.0], ["y", 79.9], ["S", 18.01528], ["T", 17.0265]]
    _, got, _ = _against_yardstick(dict(settings, neutral_losses=nls), synth.slice_batch(batch, 0, 6), "five loss masses")
    assert (got["named"]["kind"] == named_ref.COUNTED).any()


@pytest.mark.parametrize("n_q", [62, 63, 64, 65, 127])
def test_slice_edges(n_q):
    """the winner + 63 queries go through together: a PSM with as many queries as a slice takes, one fewer, one more, two"""
    batch, settings = synth.make_batch("cfg4", n_psm=3, seed=9450)
    gpu = _gpu(settings)
    kept = gpu.score_batch(batch, keep=True)
    ps = gpu.batch_pep_scores()
    sigs = ps["sig_bits"][ps["rec_off"][1]:ps["rec_off"][2]]
    assert sigs.size >= 20
    q1 = np.resize(sigs[::-1], n_q)                              # (duplicates when the PSM has fewer site assignments)
    q1[n_q // 2] = np.uint64(0)                                  # a malformed one in the middle
    queries = [[], q1, [kept["best_sig"][2]]]
    got = gpu.score_batch(batch, named=queries)
    one = {int(b): gpu.score_batch(batch, named=[[], [b], []]) for b in set(q1.tolist())}
    for j, b in enumerate(q1.tolist()):
        assert got["named"][j].tobytes() == one[b]["named"][0].tobytes(), (n_q, j)
        assert np.array_equal(got["named_counts"][j], one[b]["named_counts"][0])
        assert got["named_scores"][j].tobytes() == one[b]["named_scores"][0].tobytes()
    assert got["named"][n_q]["kind"] == named_ref.WINNER and got["named"][n_q // 2]["kind"] == named_ref.INVALID
    rec, counts, scores = named_ref.batch_records(settings, batch, got, ps, got["named_off"], got["named"]["sig_bits"], synth.unpack_psm)
    _same_named(got, dict(named_off=got["named_off"], named=rec, named_counts=counts, named_scores=scores), "%d queries" % n_q)


def test_unambiguous_and_set_aside_psms():
    good, settings = synth.make_batch("cfg2", n_psm=6, seed=9800)
    psms = []
    for i in range(good["n_psm"]):
        kw = synth.unpack_psm(good, i)
        psms.append(dict(mz=kw["mz_arr"], intensity=kw["int_arr"], peptide=kw["peptide"], n_of_mod=kw["n_of_mod"], max_charge=1))
    psms[0] = dict(psms[0], peptide="ASGTPEYIDEK", n_of_mod=3)                 # as many modifications as sites
    psms[1] = dict(psms[1], peptide="PEPTXIDESK")                              # unknown residue
    psms[2] = dict(psms[2], peptide="AGSPEPIDEK", n_of_mod=2)                  # more modifications than sites: n_sig 0
    psms[3] = dict(psms[3], mz=np.zeros(0), intensity=np.zeros(0))             # empty spectrum
    batch = synth.pack_batch(psms)
    gpu = _gpu(settings)
    plain = gpu.score_batch(batch, skip_invalid=True)
    queries = [[7, 3, 0xf], [1, 2], [1, 3], [1], [plain["best_sig"][4], 1 << 62], []]
    got = gpu.score_batch(batch, skip_invalid=True, named=queries)
    for key in KEYS + ("status",):
        assert got[key].tobytes() == plain[key].tobytes(), key
    assert got["status"][[1, 3]].all() and got["n_sig"][2] <= 0 and got["n_sig"][0] == 1 and got["best_sig"][0] == 7
    assert got["named"]["kind"].tolist() == [named_ref.WINNER, named_ref.INVALID, named_ref.INVALID, 0, 0, 0, 0, 0, named_ref.WINNER,
                                             named_ref.INVALID]
    assert got["named"]["sig_bits"].tolist() == [7, 3, 0xf, 1, 2, 1, 3, 1, int(plain["best_sig"][4]), 1 << 62]
    assert all(got["named"][j].tobytes()[8:] == b"\0" * 24 for j in range(3, 8))
    assert got["named"][0]["pep_score"] == got["best_score"][0] and got["named"][0]["total_fragments"] > 0
    # malformed offsets are an error of the call that names the PSM, before anything is scored
    for off, psm in (([1, 3, 5, 7, 8, 10, 10], 0), ([0, 3, 5, 4, 8, 10, 10], 2)):
        with pytest.raises(ValueError, match="PSM %d" % psm):
            gpu.score_batch(batch, skip_invalid=True, named=(np.array(off, np.int64), got["named"]["sig_bits"]))
        assert gpu._lib.pya_error_index(gpu._h) == psm


def test_cuts_and_forms(monkeypatch):
    big = synth.make_slice(synth.describe("cfg2", 12_000, seed=9500))         # > 32 MB of spectra: worth cutting
    settings = synth.describe("cfg2", 1, seed=9500)["settings"]
    gpu = _gpu(settings)
    monkeypatch.setenv("PYA_NO_CHUNKS", "1")
    switches.from_env(gpu)
    plain = gpu.score_batch(big)
    queries = _queries(settings, big, plain, np.random.default_rng(5), "mix")
    whole = gpu.score_batch(big, named=queries)
    assert gpu._lib.pya_debug_last_chunks(gpu._h) == 1
    monkeypatch.delenv("PYA_NO_CHUNKS")
    monkeypatch.setenv("PYA_CHUNK_MB", "2")                                    # many chunks
    switches.from_env(gpu)
    got = gpu.score_batch(big, named=queries, evidence=True)
    assert gpu._lib.pya_debug_last_chunks(gpu._h) > 8
    monkeypatch.delenv("PYA_CHUNK_MB")
    switches.from_env(gpu)
    gpu.set_workspace_budget(48 << 20)                                         # ... and cut by the workspace budget
    small = gpu.score_batch(big, named=queries)
    assert gpu._lib.pya_debug_last_chunks(gpu._h) > 1
    gpu.set_workspace_budget(0)
    for res, what in ((got, "chunk size"), (small, "budget")):
        _same_named(res, whole, "chunked by " + what)
        for key in KEYS:
            assert np.array_equal(res[key], plain[key]), key
    assert (whole["named"]["kind"] == named_ref.COUNTED).any()
    _check_invariants(settings, big, whole, "12 000 PSMs")
    assert evidence_ref.COUNTED in _evidence_tie_in(settings, synth.slice_batch(big, 0, 400), dict(
        got, named_off=got["named_off"][:401]), "chunked")
    batch, q = synth.slice_batch(big, 0, 2000), queries[:2000]
    base = gpu.score_batch(batch, named=q)
    narrow = gpu.score_batch(synth.narrow_batch(batch), named=q)               # float32 spectra against their widened form
    wide = gpu.score_batch(synth.widen_batch(synth.narrow_batch(batch)), named=q)
    _same_named(narrow, wide, "float32")
    _same_named(gpu.score_batch(batch, named=(base["named_off"], base["named"]["sig_bits"])), base, "CSR pair against lists")
    # a shared batch against its expanded form, and in shuffled PSM order
    small_b, _ = synth.make_batch("cfg2", n_psm=60, seed=9501)
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
    q = _queries(settings, flat_b, gpu.score_batch(flat_b), np.random.default_rng(6), "mix")
    flat = gpu.score_batch(flat_b, named=q)
    _same_named(gpu.score_batch(shared, named=q), flat, "shared")
    _same_named(gpu.score_batch(synth.narrow_batch(shared), named=q), gpu.score_batch(synth.narrow_batch(flat_b), named=q), "shared float32")
    assert (flat["named"]["kind"] == named_ref.COUNTED).any()
    perm = np.random.default_rng(3).permutation(len(psms))
    shuffled = synth.pack_shared_batch(spectra, [psms[p] for p in perm])
    back = gpu.score_batch(shuffled, named=[q[p] for p in perm])
    want = gpu.score_batch(synth.expand_shared_batch(shuffled), named=[q[p] for p in perm])
    _same_named(back, want, "shuffled shared")
    kept = gpu.score_batch(shuffled, named=[q[p] for p in perm], keep=True)
    _same_named(kept, want, "shuffled shared, keep")


def _dev_queries(torch, dev, res):
    off = torch.from_numpy(np.ascontiguousarray(res["named_off"])).to(dev)
    bits = torch.from_numpy(np.ascontiguousarray(res["named"]["sig_bits"]).view(np.int64)).to(dev)
    return off, bits


def test_plan_api():
    import torch
    from pyascore_amd.device import DevicePlan, named_records
    batch, settings = synth.make_batch("cfg3", n_psm=3000, seed=9600)          # fused PSMs beside others: the run forks
    gpu = _gpu(settings)
    queries = _queries(settings, batch, gpu.score_batch(batch), np.random.default_rng(7), "mix")
    want = gpu.score_batch(batch, named=queries)
    want1 = gpu.score_batch(batch, named=_queries(settings, batch, want, np.random.default_rng(8), "one"))
    dev = torch.device("cuda", 0)
    mz, it = torch.from_numpy(batch["mz"]).to(dev), torch.from_numpy(batch["intensity"]).to(dev)
    off, bits = _dev_queries(torch, dev, want)
    off1, bits1 = _dev_queries(torch, dev, want1)
    plan = DevicePlan(gpu, batch)
    raw = torch.zeros((bits.numel(), 32), dtype=torch.uint8, device=dev)
    rc = gpu._lib.pya_plan_named(plan._plan, C.byref(plan._res), None, off.data_ptr(), bits.data_ptr(), bits.numel(), raw.data_ptr(),
                                 None, None)
    assert rc == _lib.PYA_ERR_STATE                                           # before the first run
    st = torch.cuda.Stream(dev)
    with torch.cuda.stream(st):                                                # a caller stream: twice, then another list
        plan.run(mz, it)
        a = plan.named(off, bits, counts=True, scores=True)
        b = plan.named(off, bits)
        c = plan.named(off1, bits1, counts=True)
    other = torch.cuda.Stream(dev)
    with torch.cuda.stream(other):                                             # another stream than the run's waits for it
        d = plan.named(off, bits, scores=True)
    torch.cuda.synchronize()
    plan.check()
    with torch.cuda.stream(st):                                                # after a second run
        plan.run(mz, it)
        e = plan.named(off, bits, counts=True, scores=True)
    torch.cuda.synchronize()
    plan.check()
    host = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
    for (r, cn, sc), w, what in ((a, want, "first"), ((b, None, None), want, "records alone"), (c, want1, "second list"),
                                 (d, want, "other stream"), (e, want, "second run")):
        assert named_records(host(r)).tobytes() == w["named"].tobytes(), what
        assert cn is None or np.array_equal(host(cn), w["named_counts"]), what
        assert sc is None or host(sc).tobytes() == w["named_scores"].tobytes(), what
    few = synth.slice_batch(batch, 0, 5)                                       # a handful of PSMs takes the per-stage launches
    p = DevicePlan(gpu, few, named=True)
    p.run(torch.from_numpy(few["mz"]).to(dev), torch.from_numpy(few["intensity"]).to(dev))
    n5 = int(want["named_off"][5])
    r5 = p.named(off[:6].contiguous(), bits[:n5].contiguous())
    p.check()
    assert named_records(r5.cpu().numpy()).tobytes() == want["named"][:n5].tobytes()


def test_no_write_at_or_past_n_q():
    """an output of n_q records followed by a sentinel region this test allocates; offsets that claim more than n_q: the
    PSMs whose range is inside [0, n_q] are written, the others write nothing, check() reports them"""
    import torch
    from pyascore_amd.device import DevicePlan, named_records
    batch, settings = synth.make_batch("cfg2", n_psm=40, seed=9650)
    gpu = _gpu(settings)
    want = gpu.score_batch(batch, named=_queries(settings, batch, gpu.score_batch(batch), np.random.default_rng(9), "moves"))
    dev = torch.device("cuda", 0)
    plan = DevicePlan(gpu, batch, named=True)
    plan.run(torch.from_numpy(batch["mz"]).to(dev), torch.from_numpy(batch["intensity"]).to(dev))
    off, bits = _dev_queries(torch, dev, want)
    n_top = settings["n_top"]
    n_q = int(want["named_off"][25])                                            # room for the queries of 25 PSMs only
    rec = torch.full((n_q + 64, 32), 0xA5, dtype=torch.uint8, device=dev)
    cnt = torch.full((n_q + 64, n_top), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    sco = torch.full((n_q + 64, n_top), -7.0, dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    rc = gpu._lib.pya_plan_named(plan._plan, C.byref(plan._res), stream, off.data_ptr(), bits.data_ptr(), n_q, rec.data_ptr(),
                                 cnt.data_ptr(), sco.data_ptr())
    assert rc == 0
    with pytest.raises(ValueError, match="PSM 25"):
        plan.check()
    assert (rec[n_q:] == 0xA5).all() and (cnt[n_q:] == 0x5A5A5A5A).all() and (sco[n_q:] == -7.0).all()
    assert named_records(rec[:n_q].cpu().numpy()).tobytes() == want["named"][:n_q].tobytes()
    assert np.array_equal(cnt[:n_q].cpu().numpy(), want["named_counts"][:n_q])
    full = plan.named(off, bits)                                                # repeated with room: the report is gone
    plan.check()
    assert named_records(full.cpu().numpy()).tobytes() == want["named"].tobytes()


def test_sig_bits_of_against_the_library():
    """the pure-Python site list against pya_count_sites, termini in the mod group included"""
    from pyascore_amd import PyAscore
    rng = np.random.default_rng(11)
    for group in ("STY", "nSTY", "STYc", "nKc"):
        gpu = PyAscore(100.0, 10, group, 79.966331, 0.05, "by")
        for _ in range(20):
            pep = "".join(rng.choice(list("ACDEFGHIKLMNPQRSTVWY"), int(rng.integers(2, 90))))
            raw = np.frombuffer(pep.encode(), np.uint8)
            ns, pos = C.c_int32(0), np.zeros(_lib.PYA_MAX_PEPTIDE_LEN, np.uint16)
            assert gpu._lib.pya_count_sites(gpu._h, raw.ctypes.data_as(C.c_void_p), raw.size, C.byref(ns), pos.ctypes.data_as(C.c_void_p)) == 0
            sites = nm.site_residues(pep, group)
            assert sites == pos[:ns.value].tolist(), (group, pep)
            for j, res in enumerate(sites[:64]):
                assert nm.sig_bits_of(pep, [res + 1], group) == 1 << j


def test_score_then_named():
    batch, settings = synth.make_batch("cfg3", n_psm=24, seed=9900)
    gpu = _gpu(settings)
    queries = _queries(settings, batch, gpu.score_batch(batch), np.random.default_rng(12), "mix")
    want = gpu.score_batch(batch, named=queries)
    for i in (3, 17):
        gpu.score(**synth.unpack_psm(batch, i))
        lo, hi = want["named_off"][i:i + 2]
        got = gpu.named(queries[i])
        assert got["named"].tobytes() == want["named"][lo:hi].tobytes()
        assert np.array_equal(got["counts"], want["named_counts"][lo:hi]) and got["scores"].tobytes() == want["named_scores"][lo:hi].tobytes()
        ps = gpu.pep_scores                                                     # the PSM's own records are still there
        assert len(ps) == want["n_sig"][i]
        by_sig = gpu.named([p["signature"] for p in ps[:4]])
        for p, r in zip(ps, by_sig["named"]):
            assert np.float32(p["weighted_score"]).tobytes() == np.float32(r["pep_score"]).tobytes()
            if r["kind"] == named_ref.COUNTED:
                assert np.float32(gpu.calculate_ambiguity(ps[0], p)).tobytes() == np.float32(r["ambiguity"]).tobytes()


def test_batch_cli_reported_columns():
    from test_batch_cli import _toy_inputs
    from pyascore_amd import PyAscore, batch_cli
    spectra, psms = _toy_inputs()
    gpu = PyAscore(100.0, 10, "STY", 79.966331, 0.05, "by")
    plain = batch_cli.localize(gpu, psms, spectra, "STY", 79.966331, hit_depth=2, max_fragment_charge=3)
    wide = batch_cli.localize(gpu, psms, spectra, "STY", 79.966331, hit_depth=2, max_fragment_charge=3, reported=True)
    assert len(plain) == len(wide) and all(len(r) == 8 for r in wide)
    assert all(str(a) == str(b) for ra, rb in zip(wide, plain) for a, b in zip(ra[:5], rb))
    assert any(r[5] for r in wide)
    for r in wide:
        if r[5] == r[1] and r[1]:
            assert r[7] == "0" and float(r[6]) == r[2]
