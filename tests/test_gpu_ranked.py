"""Ranked localisations on the GPU (pya_ranked: the K best site assignments of a PSM by PepScore, the reported localisation
first).  Yardstick: tests/ranked_ref.py fed with the pep_scores of the reference checker and with the batch_pep_scores() of a
keep=True run -- bytewise, the records hold no float the device computes but the PepScores themselves.  The two front ends of
csrc/ranked.hip, every list length and every context a PSM can be scored in are compared on raw bytes."""
import ctypes as C
import os

import numpy as np
import pytest

import ranked_ref
import switches
from conftest import GOLDEN, checker_kind, golden_cases
from oracle import harness, orc
from pyascore_amd import _lib, probs as pb, ranked as rk, sites as st, synth
from test_gpu_count_nodes import CASES, _edge_spectra

pytestmark = pytest.mark.gpu

KEYS = ("best_score", "best_sig", "n_sig", "ascores", "alt_mask")
K = 16


def _gpu(settings, **debug):
    from pyascore_amd import PyAscore
    gpu = harness.make_scorer(PyAscore, settings)
    for k, v in debug.items():
        gpu.set_debug(k, v)
    return gpu


def _same_bytes(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype.itemsize == 16, what
    bad = np.argwhere(got.view("V16") != want.view("V16"))
    assert bad.size == 0, "%s: rows differ at %s: got %s, want %s" % (what, bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def _yardstick(gpu, batch, res, top_k, sig_cap=0, status=None):
    """the restatement from the records of the same batch scored with keep=True"""
    kept = gpu.score_batch(batch, keep=True, skip_invalid=status is not None)
    for key in KEYS:
        assert kept[key].tobytes() == res[key].tobytes(), key
    return ranked_ref.batch_rows(top_k, res, gpu.batch_pep_scores(), sig_cap, status)


def _checker_rows(settings, batch, res, top_k):
    """the restatement from the reference checker's own pep_scores, PSM by PSM"""
    chk = harness.make_scorer(orc.OracleAscore, settings, kind=checker_kind())
    out = np.zeros((int(batch["n_psm"]), top_k), ranked_ref.DTYPE)
    for i in range(int(batch["n_psm"])):
        chk.score(**synth.unpack_psm(batch, i))
        raw = chk.raw_pep_scores()
        n_sites = raw["signature"].shape[1]
        bits = (raw["signature"].astype(np.uint64) << np.arange(n_sites, dtype=np.uint64)).sum(axis=1).astype(np.uint64)
        out[i] = ranked_ref.psm_rows(top_k, res["best_sig"][i], res["best_score"][i], bits, raw["weighted_score"].astype(np.float32),
                                     scored=res["n_sig"][i] > 0)
    return out


def _check_definition(got, what):
    rows, n = got["ranked"], got["ranked"].shape[0]
    sc = rows["kind"][:, 0] == rk.SCORED
    assert np.array_equal(rows["sig_bits"][sc, 0], got["best_sig"][sc]), what
    assert rows["pep_score"][sc, 0].tobytes() == got["best_score"][sc].tobytes(), what
    listed = rows["kind"] == rk.SCORED
    assert (rows["pep_score"][listed] <= np.broadcast_to(got["best_score"][:, None], rows.shape)[listed]).all(), what   # none above best_score
    assert np.array_equal(rk.lengths(rows)[sc], np.minimum(got["n_sig"][sc], rows.shape[1])), what
    assert (rows["rank"][listed] == np.broadcast_to(np.arange(rows.shape[1]), rows.shape)[listed]).all(), what
    assert not rows[~listed & (rows["kind"] != rk.OVER)].view("u1").any(), what
    s, b = rows["pep_score"], rows["sig_bits"]
    both = listed[:, 1:] & listed[:, :-1]
    later = both.copy()
    later[:, 0] = False                                                          # (row 1 against row 0: the winner is pinned)
    assert ((s[:, 1:] < s[:, :-1]) | ((s[:, 1:] == s[:, :-1]) & (b[:, 1:] > b[:, :-1])))[later].all(), what
    assert (((rows["flags"][:, 1:] & rk.TIED_PREV) != 0) == (s[:, 1:] == s[:, :-1]))[both].all(), what
    assert ((rows["flags"] & rk.IN_BEST_TIE) != 0)[listed].tolist() == (s == got["best_score"][:, None])[listed].tolist(), what
    assert n == got["best_sig"].size


def _front_ends(gpu):
    sw, lds = (C.c_uint32 * 2)(), (C.c_uint64 * 2)()
    assert gpu._lib.pya_debug_last_ranked_launch(gpu._h, sw, lds) == 0
    return (int(sw[0]), int(sw[1])), (int(lds[0]), int(lds[1]))


def _against_yardstick(settings, batch, what, skip_invalid=False, checker=True, top_k=K, **debug):
    gpu = _gpu(settings, **debug)
    plain = gpu.score_batch(batch, skip_invalid=skip_invalid, evidence=True, ions=True, sites=True, probs=True, site_sig_cap=0)
    got = gpu.score_batch(batch, skip_invalid=skip_invalid, evidence=True, ions=True, sites=True, probs=True, ranked=top_k, site_sig_cap=0)
    for key in KEYS + ("evidence", "ion_off", "ions", "site_off", "sites", "site_probs", "psm_probs") + (("status",) if skip_invalid else ()):
        assert got[key].tobytes() == plain[key].tobytes(), (what, key)          # nothing else moves
    alone = gpu.score_batch(batch, skip_invalid=skip_invalid, ranked=top_k, site_sig_cap=0)
    _same_bytes(alone["ranked"], got["ranked"], what + " (ranked alone)")
    _same_bytes(got["ranked"], _yardstick(gpu, batch, got, top_k, 0, got["status"] if skip_invalid else None), what + " (keep=True records)")
    if checker:
        _same_bytes(got["ranked"], _checker_rows(settings, batch, got, top_k), what + " (reference checker)")
    _check_definition(got, what)
    general = _gpu(settings, PYA_NO_PROB_CNT="1", **debug).score_batch(batch, skip_invalid=skip_invalid, ranked=top_k, site_sig_cap=0)
    _same_bytes(general["ranked"], got["ranked"], what + " (general front end)")
    return gpu, got


@pytest.mark.parametrize("case", [c for c in golden_cases() if c.startswith(("velos_", "ties_", "edge_"))])
def test_golden_cases_equal_the_yardstick(case):
    settings, batch, exp = harness.load_case(os.path.join(GOLDEN, case + ".npz"))
    _, got = _against_yardstick(settings, batch, case)
    assert (got["ranked"]["kind"][:, 0] == rk.SCORED).any()
    if "ps_bits" in exp:                                            # ... and the golden file's own pep_scores
        _same_bytes(got["ranked"], ranked_ref.batch_rows(K, exp, exp), case + " (golden pep_scores)")


@pytest.mark.parametrize("cfg,n", [("cfg1", 300), ("cfg2", 300), ("cfg3", 200), ("cfg4", 60), ("cfg5", 24)])
def test_seeded_batches_equal_the_yardstick(cfg, n):
    batch, settings = synth.make_batch(cfg, n_psm=n, seed=9710)
    _, got = _against_yardstick(settings, batch, cfg)
    assert (got["ranked"]["kind"][:, 0] == rk.SCORED).all()


@pytest.mark.parametrize("general", [False, True])
def test_realistic_batches_equal_the_yardstick(general):
    batch, settings = synth.make_realistic(40, seed=9720 + general, general=general)
    _against_yardstick(settings, batch, "realistic general=%s" % general)


def test_general_kernel_psms():
    """beyond the fast kernels' limits: a peptide above 64 residues, more than 15 000 site assignments, n_top 12"""
    batch, settings = synth.make_batch("cfg2", n_psm=4, seed=9740, L=80, n_sites=5, n_mod=2)
    _, got = _against_yardstick(settings, batch, "80 residues")
    assert (got["ranked"]["kind"][:, 0] == rk.SCORED).all()
    batch, settings = synth.make_batch("cfg5", n_psm=2, seed=9742, L=40, n_sites=18, n_mod=8)       # C(18, 8) = 43 758
    gpu, got = _against_yardstick(settings, batch, "43 758 assignments", checker=False, top_k=64)
    assert (got["n_sig"] == 43758).all() and (rk.lengths(got["ranked"]) == 64).all() and _front_ends(gpu)[0][1] != 0
    batch, settings = synth.make_batch("cfg2", n_psm=10, seed=9741)
    _against_yardstick(dict(settings, n_top=12), batch, "n_top 12")


@pytest.mark.parametrize("case", range(len(CASES)))
def test_count_node_front_end_equals_the_general_one(case, monkeypatch):
    over, st_over = CASES[case]
    monkeypatch.setenv("PYA_NO_TINY", "1")
    batch, settings = synth.make_batch("cfg5", n_psm=6, seed=60 + case, **over)
    settings = dict(settings, **st_over)
    rng = np.random.default_rng(case)
    for label, b2 in (("plain", batch), ("edges", _edge_spectra(batch, settings, rng, 0.5)), ("edges_wide", _edge_spectra(batch, settings, rng, 0.0))):
        table = _gpu(settings).score_batch(b2, ranked=64, site_sig_cap=0)
        general = _gpu(settings, PYA_NO_PROB_CNT="1").score_batch(b2, ranked=64, site_sig_cap=0)
        marked = _gpu(settings, PYA_DEBUG=str(0x40000000)).score_batch(b2, ranked=64, site_sig_cap=0)
        assert (table["ranked"]["kind"][:, 0] == rk.SCORED).all(), label
        _same_bytes(general["ranked"], table["ranked"], "%d %s: general front end" % (case, label))
        _same_bytes(marked["ranked"], table["ranked"], "%d %s: every node marked" % (case, label))
    gpu = _gpu(settings)
    got = gpu.score_batch(batch, ranked=64, site_sig_cap=0)
    _same_bytes(got["ranked"], _yardstick(gpu, batch, got, 64), "case %d" % case)


@pytest.mark.parametrize("cfg,n,want", [("cfg2", 300, 1), ("cfg3", 200, 1), ("cfg5", 24, 1), ("cfg4", 60, 2)])
def test_the_front_end_a_launch_takes(cfg, n, want):
    batch, settings = synth.make_batch(cfg, n_psm=n, seed=9730)
    gpu = _gpu(settings)
    got = gpu.score_batch(batch, ranked=5, site_sig_cap=0)
    assert (got["ranked"]["kind"][:, 0] == rk.SCORED).all()
    sw, lds = _front_ends(gpu)
    assert sw == (want, 0), (cfg, sw)
    assert 1024 < lds[0] <= 160 * 1024 and lds[1] == 0
    if want == 1:
        assert lds[0] <= 64 * 1024
        forced = _gpu(settings, PYA_NO_PROB_CNT="1")
        _same_bytes(forced.score_batch(batch, ranked=5, site_sig_cap=0)["ranked"], got["ranked"], cfg)
        assert _front_ends(forced)[0] == (2, 0)


def _dense_psms(seed, sizes):
    rng = np.random.default_rng(seed)
    small, settings = synth.make_batch("cfg2", n_psm=8, seed=seed)
    psms = []
    for i in range(small["n_psm"]):
        kw = synth.unpack_psm(small, i)
        psms.append(dict(mz=kw["mz_arr"], intensity=kw["int_arr"], peptide=kw["peptide"], n_of_mod=kw["n_of_mod"], max_charge=1))
    dense = []
    for j, P in enumerate(sizes):
        base = psms[j]
        mz = np.concatenate([base["mz"], rng.uniform(100.0, 2500.0, P - base["mz"].size)])
        it = np.concatenate([base["intensity"], rng.lognormal(4.0, 1.0, P - base["intensity"].size)])
        o = np.argsort(mz, kind="stable")
        dense.append(dict(base, mz=mz[o], intensity=it[o]))
    return settings, psms, dense


def test_spectra_of_more_than_8192_peaks():
    settings, sparse, dense = _dense_psms(9745, (10_000, 8193))
    gpu, forced = _gpu(settings), _gpu(settings, PYA_NO_PROB_CNT="1")
    for what, psms, want_sw in (("alone", dense[:1], (0, 2)), ("beside sparse PSMs", sparse + dense, (1, 2))):
        batch = synth.pack_batch(psms)
        got = gpu.score_batch(batch, ranked=K, site_sig_cap=0)
        assert _front_ends(gpu)[0] == want_sw, what
        assert (got["ranked"]["kind"][:, 0] == rk.SCORED).all(), what
        _same_bytes(got["ranked"], _yardstick(gpu, batch, got, K), what)
        _check_definition(got, what)
        _same_bytes(forced.score_batch(batch, ranked=K, site_sig_cap=0)["ranked"], got["ranked"], what + " (general front end)")


def test_prefix_property_and_complete_lists():
    """K = 1, 2, 5, 16, 64 on one plan: each list is the bytewise prefix of the longer one; K >= n_sig lists every signature
    of the PSM's signature list exactly once"""
    import torch
    from pyascore_amd.device import DevicePlan, ranked_records
    for cfg, n, over in (("cfg2", 200, {}), ("cfg4", 40, {}), ("cfg5", 8, dict(L=20, n_sites=8, n_mod=4)), ("cfg5", 6, {})):
        batch, settings = synth.make_batch(cfg, n_psm=n, seed=9750, **over)
        gpu = _gpu(settings)
        kept = gpu.score_batch(batch, keep=True)
        dev = torch.device("cuda", 0)
        plan = DevicePlan(gpu, batch)
        plan.run(torch.from_numpy(batch["mz"]).to(dev), torch.from_numpy(batch["intensity"]).to(dev))
        lists = {k: ranked_records(plan.ranked(k).cpu().numpy()) for k in (64, 16, 5, 2, 1)}
        plan.check()
        for k in (1, 2, 5, 16):
            _same_bytes(lists[k], np.ascontiguousarray(lists[64][:, :k]), "%s: K = %d is the prefix of K = 64" % (cfg, k))
        _same_bytes(lists[5], gpu.score_batch(batch, ranked=5, site_sig_cap=0)["ranked"], cfg + ": plan against batch")
        gpu.score_batch(batch, keep=True)
        full = lists[64]
        seen = 0
        for i in range(n):
            if kept["n_sig"][i] > 64:
                continue
            cnt = C.c_uint64()
            assert gpu._lib.pya_debug_signature_list(gpu._h, i, None, 0, C.byref(cnt)) == 0 and cnt.value == kept["n_sig"][i]
            order = np.zeros(cnt.value, np.uint64)
            assert gpu._lib.pya_debug_signature_list(gpu._h, i, order.ctypes.data_as(C.c_void_p), order.size, C.byref(cnt)) == 0
            assert sorted(full["sig_bits"][i, :cnt.value].tolist()) == sorted(order.tolist()) and len(set(order.tolist())) == cnt.value
            assert not full[i, cnt.value:].view("u1").any()
            seen += 1
        assert seen or cfg == "cfg5"


def test_against_the_other_stages():
    """row 1 has the PepScore bits of the site stage's runner-up; the weights of a complete list sum to the probability
    stage's z; rows fed to named() come back WINNER / TIED where they are flagged IN_BEST_TIE, with bit-equal PepScores"""
    for cfg, n, over in (("cfg2", 200, {}), ("cfg3", 100, {}), ("cfg5", 8, dict(L=20, n_sites=7, n_mod=3))):
        batch, settings = synth.make_batch(cfg, n_psm=n, seed=9760, **over)
        gpu = _gpu(settings)
        got = gpu.score_batch(batch, sites=True, probs=True, ranked=64, site_sig_cap=0)
        rows = got["ranked"]
        runner = st.runner_up(got["sites"], got["site_off"], got["best_sig"])
        has = runner["found"] & (got["n_sig"] > 1)
        assert has.any()
        assert rows["pep_score"][has, 1].tobytes() == runner["score"][has].tobytes(), cfg
        alone = has & ((rows["flags"][:, 2] & rk.TIED_PREV) == 0)                # (no tie behind the runner-up: the same assignment too)
        assert alone.any() and np.array_equal(rows["sig_bits"][alone, 1], runner["sig"][alone]), cfg
        assert (rows["kind"][~has, 1] == rk.NONE).all(), cfg
        full = got["n_sig"] <= 64
        assert full.any()
        w = np.exp2((rows["pep_score"].astype(np.float64) - got["best_score"].astype(np.float64)[:, None]) * 0.33219280948873623)
        z = np.where(rows["kind"] == rk.SCORED, w, 0.0).sum(axis=1)
        np.testing.assert_allclose(z[full], got["psm_probs"]["z"][full], rtol=64 * 2.0 ** -53, atol=0, err_msg=cfg)
        q = [[int(b) for b in rows["sig_bits"][i, :rk.lengths(rows[i])[0]]] for i in range(n)]
        named = gpu.score_batch(batch, named=q)
        off = named["named_off"]
        for i in range(n):
            rec, mine = named["named"][off[i]:off[i + 1]], rows[i, :off[i + 1] - off[i]]
            assert rec["pep_score"].tobytes() == mine["pep_score"].tobytes(), (cfg, i)
            tie = (mine["flags"] & rk.IN_BEST_TIE) != 0
            assert ((rec["kind"] == 2) | (rec["kind"] == 3))[tie].all() and (rec["kind"][~tie] >= 3).all(), (cfg, i)   # (TIED: within 1e-6)
            assert rec["kind"][0] == 2


def test_sig_cap():
    batch, settings = synth.make_realistic(40, seed=9770, general=True)
    gpu = _gpu(settings)
    full = gpu.score_batch(batch, ranked=K, site_sig_cap=0)
    cap = int(np.median(full["n_sig"]))
    assert (full["n_sig"] > cap).any() and (full["n_sig"] <= cap).any()
    got = gpu.score_batch(batch, ranked=K, sites=True, site_sig_cap=cap)
    _same_bytes(got["ranked"], _yardstick(gpu, batch, got, K, cap), "cap %d" % cap)
    over = got["n_sig"] > cap
    rows = got["ranked"]
    assert (rows["kind"][over, 0] == rk.OVER).all() and not rows[over, 1:].view("u1").any()
    assert np.array_equal(rows["sig_bits"][over, 0], got["best_sig"][over]) and rows["pep_score"][over, 0].tobytes() == got["best_score"][over].tobytes()
    _same_bytes(rows[~over], full["ranked"][~over], "under the cap")
    assert rk.lengths(rows)[over].tolist() == [1] * int(over.sum()) and not rk.best_tie_size(rows)[over].any()
    _same_bytes(gpu.score_batch(batch, ranked=K)["ranked"], full["ranked"], "default cap above every PSM")


def test_unscored_and_set_aside_psms():
    good, settings = synth.make_batch("cfg2", n_psm=6, seed=9780)
    psms = []
    for i in range(good["n_psm"]):
        kw = synth.unpack_psm(good, i)
        psms.append(dict(mz=kw["mz_arr"], intensity=kw["int_arr"], peptide=kw["peptide"], n_of_mod=kw["n_of_mod"], max_charge=1))
    psms[0] = dict(psms[0], peptide="ASGTPEYIDEK", n_of_mod=3)                 # as many modifications as sites
    psms[1] = dict(psms[1], peptide="PEPTXIDESK")                              # unknown residue: set aside
    psms[2] = dict(psms[2], peptide="AGSPEPIDEK", n_of_mod=2)                  # more modifications than sites: n_sig 0
    psms[3] = dict(psms[3], mz=np.zeros(0), intensity=np.zeros(0))             # empty spectrum: set aside
    psms[5] = dict(psms[5], peptide="ASGTPEYIDEK", n_of_mod=0)                 # no modification
    batch = synth.pack_batch(psms)
    gpu = _gpu(settings)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    out = np.zeros((6, 5), rk.RANKED_DTYPE)
    assert gpu._lib.pya_last_batch_ranked(None, vp(out), 6, 5) == _lib.PYA_ERR_ARG
    assert gpu._lib.pya_last_batch_ranked(gpu._h, vp(out), 6, 5) == _lib.PYA_ERR_STATE     # no batch with the flag yet
    assert b"PYA_FLAG_RANKED" in gpu._lib.pya_last_error(gpu._h)
    assert gpu._lib.pya_get_ranked_k(gpu._h) == 5
    assert gpu._lib.pya_set_ranked_k(gpu._h, 0) == _lib.PYA_ERR_ARG and gpu._lib.pya_set_ranked_k(gpu._h, 65) == _lib.PYA_ERR_ARG
    assert gpu._lib.pya_get_ranked_k(gpu._h) == 5
    plain = gpu.score_batch(batch, skip_invalid=True)
    got = gpu.score_batch(batch, skip_invalid=True, ranked=5)
    assert gpu._lib.pya_get_ranked_k(gpu._h) == 5                              # the handle's own setting came back
    for key in KEYS + ("status",):
        assert got[key].tobytes() == plain[key].tobytes(), key
    rows = got["ranked"]
    assert got["status"][[1, 3]].all() and not rows[[1, 2, 3]].view("u1").any()
    assert rows["kind"][0].tolist() == [1, 0, 0, 0, 0] and rows["sig_bits"][0, 0] == 7 and not rows[0, 1:].view("u1").any()
    assert rows["kind"][5].tolist() == [1, 0, 0, 0, 0] and rows["sig_bits"][5, 0] == 0 and rows["pep_score"][5, 0] == got["best_score"][5]
    assert rows["kind"][4].tolist() == [1] * 5
    _same_bytes(rows, _yardstick(gpu, batch, got, 5, 0, got["status"]), "mixed batch")
    general = _gpu(settings, PYA_NO_PROB_CNT="1").score_batch(batch, skip_invalid=True, ranked=5)
    _same_bytes(general["ranked"], rows, "mixed batch, general front end")
    with pytest.raises(ValueError):                                            # without skip_invalid the call fails as before
        gpu.score_batch(batch, ranked=5)
    assert gpu._lib.pya_last_batch_ranked(gpu._h, vp(out), 6, 5) == _lib.PYA_ERR_STATE
    gpu.score_batch(batch, skip_invalid=True, ranked=5)
    assert gpu._lib.pya_last_batch_ranked(gpu._h, vp(out), 6, 5) == 0 and out.tobytes() == rows.tobytes()
    assert gpu._lib.pya_last_batch_ranked(gpu._h, vp(out), 6, 4) == _lib.PYA_ERR_ARG
    assert gpu._lib.pya_last_batch_ranked(gpu._h, vp(out), 5, 5) == _lib.PYA_ERR_ARG
    assert gpu._lib.pya_last_batch_ranked(gpu._h, None, 6, 5) == _lib.PYA_ERR_ARG
    for bad in (0, 65, 2.5, True):
        with pytest.raises(ValueError):
            gpu.score_batch(batch, skip_invalid=True, ranked=bad)
    with pytest.raises(ValueError):
        gpu.ranked(0)


def test_bytes_do_not_depend_on_the_context(monkeypatch):
    """a PSM alone, inside a 100 000-PSM batch, in a chunked call, shared against expanded, float32 against widened, two runs"""
    big = synth.make_slice(synth.describe("cfg2", 100_000, seed=9790))
    settings = synth.describe("cfg2", 1, seed=9790)["settings"]
    gpu = _gpu(settings)
    whole = gpu.score_batch(big, ranked=5)["ranked"]
    assert (whole["kind"][:, 0] == rk.SCORED).all()
    _same_bytes(gpu.score_batch(big, ranked=5)["ranked"], whole, "again")
    for i in (0, 1, 49_999, 99_999):
        one = gpu.score_batch(synth.slice_batch(big, i, i + 1), ranked=5)["ranked"]
        assert one[0].tobytes() == whole[i].tobytes(), i
        gpu.score(**synth.unpack_psm(big, i))                                 # PyAscore.ranked: a batch of one
        assert gpu.ranked(5).tobytes() == whole[i].tobytes() and gpu.ranked(2).tobytes() == whole[i, :2].tobytes(), i
    few = gpu.score_batch(synth.slice_batch(big, 10, 15), ranked=5)["ranked"]
    _same_bytes(few, whole[10:15], "a handful")
    part = synth.slice_batch(big, 0, 12_000)
    monkeypatch.setenv("PYA_NO_CHUNKS", "1")
    switches.from_env(gpu)
    uncut = gpu.score_batch(part, ranked=5)["ranked"]
    assert gpu._lib.pya_debug_last_chunks(gpu._h) == 1
    monkeypatch.delenv("PYA_NO_CHUNKS")
    monkeypatch.setenv("PYA_CHUNK_MB", "2")
    switches.from_env(gpu)
    cut = gpu.score_batch(part, ranked=5, evidence=True)["ranked"]
    assert gpu._lib.pya_debug_last_chunks(gpu._h) > 8
    monkeypatch.delenv("PYA_CHUNK_MB")
    switches.from_env(gpu)
    _same_bytes(cut, uncut, "chunked")
    _same_bytes(uncut, whole[:12_000], "a part")
    batch = synth.slice_batch(big, 0, 1500)
    narrow = gpu.score_batch(synth.narrow_batch(batch), ranked=5)["ranked"]
    wide = gpu.score_batch(synth.widen_batch(synth.narrow_batch(batch)), ranked=5)["ranked"]
    _same_bytes(narrow, wide, "float32")
    small_b, _ = synth.make_batch("cfg2", n_psm=60, seed=9791)
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
    flat = gpu.score_batch(flat_b, ranked=5)
    _same_bytes(flat["ranked"], _yardstick(gpu, flat_b, flat, 5), "expanded")
    _same_bytes(gpu.score_batch(shared, ranked=5)["ranked"], flat["ranked"], "shared")
    perm = np.random.default_rng(3).permutation(len(psms))
    shuffled = synth.pack_shared_batch(spectra, [psms[p] for p in perm])
    want = gpu.score_batch(synth.expand_shared_batch(shuffled), ranked=5)["ranked"]
    _same_bytes(gpu.score_batch(shuffled, ranked=5)["ranked"], want, "shuffled shared")
    _same_bytes(gpu.score_batch(shuffled, ranked=5, keep=True)["ranked"], want, "shuffled shared, keep")


def test_every_route_switch_leaves_the_same_bytes(monkeypatch):
    """the on / off switches of tests/switches.py, one at a time: whatever route scores a PSM, the rows are the same"""
    flags = [n for n in switches.SWITCHES if n.startswith(("PYA_NO_", "PYA_ONE_")) or n in ("PYA_PEAK_CLASSES", "PYA_SORT_ROOM")]
    assert len(flags) >= 15
    batch, settings = synth.make_batch("cfg3", n_psm=300, seed=9795)
    few = synth.slice_batch(batch, 0, 6)
    plain = _gpu(settings)
    want, want_few = plain.score_batch(batch, ranked=K, site_sig_cap=0)["ranked"], plain.score_batch(few, ranked=K, site_sig_cap=0)["ranked"]
    _same_bytes(want_few, want[:6], "a handful")
    for name in flags:
        monkeypatch.setenv(name, "1")
        gpu = _gpu(settings)
        switches.from_env(gpu)
        _same_bytes(gpu.score_batch(batch, ranked=K, site_sig_cap=0)["ranked"], want, name)
        _same_bytes(gpu.score_batch(few, ranked=K, site_sig_cap=0)["ranked"], want_few, name + " (a handful)")
        monkeypatch.delenv(name)


def test_all_stage_flags_together():
    """with all six stage flags set, every other record is what it is without PYA_FLAG_RANKED"""
    batch, settings = synth.make_batch("cfg3", n_psm=400, seed=9800)
    gpu = _gpu(settings)
    q = [[int(b)] for b in gpu.score_batch(batch)["best_sig"]]
    plain = gpu.score_batch(batch, evidence=True, ions=True, named=q, sites=True, probs=True)
    got = gpu.score_batch(batch, evidence=True, ions=True, named=q, sites=True, probs=True, ranked=K)
    for key in KEYS + ("evidence", "ion_off", "ions", "named", "site_off", "sites", "site_probs", "psm_probs"):
        assert got[key].tobytes() == plain[key].tobytes(), key
    _same_bytes(got["ranked"], gpu.score_batch(batch, ranked=K)["ranked"], "beside the other stages")
    _check_definition(got, "cfg3")


def test_plan_api_and_score_one():
    import torch
    from pyascore_amd.device import DevicePlan, ranked_records
    batch, settings = synth.make_batch("cfg3", n_psm=3000, seed=9810)          # fused PSMs beside others: the run forks
    gpu = _gpu(settings)
    want = gpu.score_batch(batch, ranked=5, site_sig_cap=0)["ranked"]
    dev = torch.device("cuda", 0)
    mz, it = torch.from_numpy(batch["mz"]).to(dev), torch.from_numpy(batch["intensity"]).to(dev)
    plan = DevicePlan(gpu, batch)
    raw = torch.zeros((3000, 5, 16), dtype=torch.uint8, device=dev)
    assert gpu._lib.pya_plan_ranked(plan._plan, C.byref(plan._res), None, 5, 0, raw.data_ptr()) == _lib.PYA_ERR_STATE   # not yet run
    s1 = torch.cuda.Stream(dev)
    with torch.cuda.stream(s1):
        plan.run(mz, it)
        a = plan.ranked(5)
        b = plan.ranked(5)
        b2 = plan.ranked(5, out=torch.full_like(b, 7))                         # into the caller's tensor
    other = torch.cuda.Stream(dev)
    with torch.cuda.stream(other):                                             # another stream than the run's waits for it
        c = plan.ranked(5)
        _, sites = plan.sites()                                                # ... and shares the uploaded offsets
    torch.cuda.synchronize()
    plan.check()
    assert gpu._lib.pya_plan_ranked(plan._plan, C.byref(plan._res), None, 5, 0, None) == _lib.PYA_ERR_ARG
    assert gpu._lib.pya_plan_ranked(plan._plan, C.byref(plan._res), None, 0, 0, raw.data_ptr()) == _lib.PYA_ERR_ARG
    assert gpu._lib.pya_plan_ranked(plan._plan, C.byref(plan._res), None, 65, 0, raw.data_ptr()) == _lib.PYA_ERR_ARG
    assert gpu._lib.pya_plan_ranked(None, None, None, 5, 0, None) == _lib.PYA_ERR_ARG
    with pytest.raises(ValueError):
        plan.ranked(5, out=torch.zeros((3000, 4, 16), dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError):
        plan.ranked(65)
    for t, what in ((a, "first"), (b, "again"), (b2, "out="), (c, "other stream")):
        _same_bytes(ranked_records(t.cpu().numpy()), want, what)
    plan.run(mz, it)                                                           # two runs of one plan
    _same_bytes(ranked_records(plan.ranked(5).cpu().numpy()), want, "second run")
    few = synth.slice_batch(batch, 0, 5)                                       # a handful of PSMs takes the per-stage launches
    p = DevicePlan(gpu, few, ranked=True)
    p.run(torch.from_numpy(few["mz"]).to(dev), torch.from_numpy(few["intensity"]).to(dev))
    r5 = p.ranked(5)
    p.check()
    _same_bytes(ranked_records(r5.cpu().numpy()), want[:5], "a handful")
    kw = synth.unpack_psm(batch, 0)
    m, i = np.ascontiguousarray(kw["mz_arr"], np.float64), np.ascontiguousarray(kw["int_arr"], np.float64)
    pep = np.frombuffer(kw["peptide"].encode(), np.uint8)
    res = (np.zeros(1, np.float32), np.zeros(1, np.uint64), np.zeros(1, np.int32), np.zeros((1, 4), np.float32), np.zeros((1, 4), np.uint64))
    r = _lib.Results(4, *[x.ctypes.data_as(C.c_void_p) for x in res])
    rc = gpu._lib.pya_score_one(gpu._h, m.ctypes.data_as(C.c_void_p), i.ctypes.data_as(C.c_void_p), m.size,
                                pep.ctypes.data_as(C.c_void_p), pep.size, int(kw["n_of_mod"]), int(kw["max_fragment_charge"]), None, None, 0,
                                _lib.PYA_FLAG_RANKED, C.byref(r))
    assert rc == _lib.PYA_ERR_ARG and b"PYA_FLAG_RANKED" in gpu._lib.pya_last_error(gpu._h)
    gpu.score(**kw)
    assert gpu.ranked(5).tobytes() == want[0].tobytes()


def test_command_line_file(tmp_path):
    from test_batch_cli import _toy_inputs
    from pyascore_amd import PyAscore, batch_cli
    spectra, psms = _toy_inputs()
    gpu = PyAscore(100.0, 10, "STY", 79.966331, 0.05, "by")
    plain = batch_cli.localize(gpu, psms, spectra, "STY", 79.966331, hit_depth=2, max_fragment_charge=3)
    ranked_rows = []
    wide = batch_cli.localize(gpu, psms, spectra, "STY", 79.966331, hit_depth=2, max_fragment_charge=3, ranked=ranked_rows, ranked_depth=3)
    assert [[str(f) for f in r] for r in wide] == [[str(f) for f in r] for r in plain]      # the main table is unchanged
    assert ranked_rows and all(len(r) == len(batch_cli.RANKED_COLUMNS) for r in ranked_rows)
    by_psm = {}
    for r in ranked_rows:
        by_psm.setdefault((r[0], r[1]), []).append(r)
    main = {}
    hit = 0
    for j, row in enumerate(plain):
        hit = hit + 1 if j and row[0] == plain[j - 1][0] else 1
        main[(row[0], hit)] = row
    for key, rows in by_psm.items():
        assert [r[2] for r in rows] == [str(x + 1) for x in range(len(rows))] and len(rows) <= 3
        assert rows[0][3] == main[key][1] and float(rows[0][4]) == float(main[key][2]) and float(rows[0][5]) == 0.0
        scores = [float(r[4]) for r in rows]
        assert scores[1:] == sorted(scores[1:], reverse=True) and all(s <= scores[0] for s in scores)
        assert all(r[3] for r in rows) and len({r[3] for r in rows}) == len(rows)
    path = str(tmp_path / "ranked.tsv")
    batch_cli.write_ranked_tsv(ranked_rows, path)
    lines = open(path).read().splitlines()
    assert lines[0].split("\t") == list(batch_cli.RANKED_COLUMNS) and len(lines) == 1 + len(ranked_rows)
