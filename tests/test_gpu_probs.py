"""Site probabilities on the GPU (pya_site_prob / pya_psm_prob: the posterior over a PSM's site assignments that their
PepScores imply, summed per modifiable residue).  Yardstick: tests/probs_ref.py fed with the batch_pep_scores() of a
keep=True run -- floats at rtol 1e-12 (only exp2 and the order of the sums separate the two), everything else exactly.  The
two front ends of csrc/probs.hip, and every context a PSM can be scored in, are compared on raw bytes."""
import ctypes as C
import os

import numpy as np
import pytest

import probs_ref
import switches
from conftest import GOLDEN, golden_cases
from oracle import harness
from pyascore_amd import _lib, probs as pb, sites as st, synth
from test_gpu_count_nodes import CASES, _edge_spectra

pytestmark = pytest.mark.gpu

KEYS = ("best_score", "best_sig", "n_sig", "ascores", "alt_mask")
RTOL = probs_ref.RTOL


def _gpu(settings, **debug):
    from pyascore_amd import PyAscore
    gpu = harness.make_scorer(PyAscore, settings)
    for k, v in debug.items():
        gpu.set_debug(k, v)
    return gpu


def _same_bytes(got, want, what):
    assert np.array_equal(got["site_off"], want["site_off"]), what
    for key in ("site_probs", "psm_probs"):
        assert got[key].shape == want[key].shape and got[key].dtype.itemsize == 16, (what, key)
        bad = np.flatnonzero(got[key].view("V16") != want[key].view("V16"))
        assert bad.size == 0, "%s: %s differ at %s: got %s, want %s" % (what, key, bad[:5].tolist(), got[key][bad[:5]], want[key][bad[:5]])


def _close(got, want, what):
    assert np.array_equal(got["site_off"], want["site_off"]), what
    assert np.array_equal(got["psm_probs"]["kind"], want["psm_probs"]["kind"]), what
    assert np.array_equal(got["psm_probs"]["n_summed"], want["psm_probs"]["n_summed"]) and not got["psm_probs"]["pad"].any(), what
    np.testing.assert_allclose(got["psm_probs"]["z"], want["psm_probs"]["z"], rtol=RTOL, atol=0, err_msg=what)
    for f in ("with_prob", "without_prob"):
        np.testing.assert_allclose(got["site_probs"][f], want["site_probs"][f], rtol=RTOL, atol=1e-300, err_msg=what + " " + f)


def _yardstick(gpu, settings, batch, res, sig_cap=0, status=None):
    kept = gpu.score_batch(batch, keep=True, skip_invalid=status is not None)
    for key in KEYS:
        assert kept[key].tobytes() == res[key].tobytes(), key
    off, sites, psms = probs_ref.batch_records(settings, batch, res, gpu.batch_pep_scores(), synth.unpack_psm, sig_cap, status)
    return dict(site_off=off, site_probs=sites, psm_probs=psms)


def _check_definition(batch, got, what):
    """what the header promises of the records, against the results and the site table of the same call"""
    sp, pp, off = got["site_probs"], got["psm_probs"], got["site_off"]
    psm = np.repeat(np.arange(int(batch["n_psm"])), np.diff(off))
    sc = pp["kind"] == pb.SCORED
    assert np.array_equal(pp["n_summed"][sc], got["n_sig"][sc].astype(np.uint32)) and (pp["z"][sc] >= 1.0).all(), what
    s = sc[psm]
    np.testing.assert_allclose(sp["with_prob"][s] + sp["without_prob"][s], 1.0, rtol=1e-12, err_msg=what)
    sums = np.bincount(psm[s], sp["with_prob"][s], int(batch["n_psm"]))
    np.testing.assert_allclose(sums[sc], batch["n_of_mod"][sc], rtol=1e-12, atol=1e-12, err_msg=what)
    if "sites" in got:            # with_prob >= 1 / z, bitwise: the sum of a winner's residue contains the winner's exact 1
        inb = s & ((got["sites"]["flags"] & st.IN_BEST) != 0) & (got["sites"]["kind"] == st.SCORED)
        assert inb.any() or not sc.any(), what
        assert (sp["with_prob"][inb] >= 1.0 / pp["z"][psm[inb]]).all(), what
    none = pp["kind"] == pb.NONE
    assert not pp["z"][none].any() and not pp["n_summed"][none].any() and not sp["with_prob"][none[psm]].any(), what


def _front_ends(gpu):
    """what the last probability launches of the scorer carved: (PSMs inside the fast limits, general list); 1 the count-node
    tables alone, 2 the general front end alone, 3 both, 0 no launch -- and their LDS bytes"""
    sw, lds = (C.c_uint32 * 2)(), (C.c_uint64 * 2)()
    assert gpu._lib.pya_debug_last_probs_launch(gpu._h, sw, lds) == 0
    return (int(sw[0]), int(sw[1])), (int(lds[0]), int(lds[1]))


def _list_order_records(gpu, settings, batch, res):
    """probs_ref with every PSM's sums replayed in the order of its signature list (a keep=True run of the same batch)"""
    gpu.score_batch(batch, keep=True)
    ps = gpu.batch_pep_scores()
    n = int(batch["n_psm"])
    sites, psms, off = [], np.zeros(n, probs_ref.PSM_DTYPE), [0]
    for i in range(n):
        cnt = C.c_uint64()
        assert gpu._lib.pya_debug_signature_list(gpu._h, i, None, 0, C.byref(cnt)) == 0 and cnt.value == res["n_sig"][i]
        order = np.zeros(cnt.value, np.uint64)
        assert gpu._lib.pya_debug_signature_list(gpu._h, i, order.ctypes.data_as(C.c_void_p), order.size, C.byref(cnt)) == 0
        lo, hi = int(ps["rec_off"][i]), int(ps["rec_off"][i + 1])
        n_sites = int(res["site_off"][i + 1] - res["site_off"][i])
        s, psms[i] = probs_ref.psm_records(n_sites, res["best_score"][i], ps["sig_bits"][lo:hi], ps["weighted_score"][lo:hi], order=order)
        sites.append(s)
        off.append(off[-1] + n_sites)
    return dict(site_off=np.asarray(off, np.int64), site_probs=np.concatenate(sites), psm_probs=psms)


def _against_yardstick(settings, batch, what, skip_invalid=False, **debug):
    gpu = _gpu(settings, **debug)
    plain = gpu.score_batch(batch, skip_invalid=skip_invalid, evidence=True, ions=True, sites=True, site_sig_cap=0)
    got = gpu.score_batch(batch, skip_invalid=skip_invalid, evidence=True, ions=True, sites=True, probs=True, site_sig_cap=0)
    for key in KEYS + ("evidence", "ion_off", "ions", "site_off", "sites") + (("status",) if skip_invalid else ()):   # nothing else moves
        assert got[key].tobytes() == plain[key].tobytes(), (what, key)
    alone = gpu.score_batch(batch, skip_invalid=skip_invalid, probs=True, site_sig_cap=0)
    _same_bytes(alone, got, what + " (probs alone)")
    _close(got, _yardstick(gpu, settings, batch, got, 0, got["status"] if skip_invalid else None), what)
    _check_definition(batch, got, what)
    general = _gpu(settings, PYA_NO_PROB_CNT="1", **debug).score_batch(batch, skip_invalid=skip_invalid, probs=True, site_sig_cap=0)
    _same_bytes(general, got, what + " (general front end)")
    return gpu, got


@pytest.mark.parametrize("case", [c for c in golden_cases() if c.startswith(("velos_", "ties_", "edge_"))])
def test_golden_cases_equal_the_yardstick(case):
    settings, batch, exp = harness.load_case(os.path.join(GOLDEN, case + ".npz"))
    _, got = _against_yardstick(settings, batch, case)
    assert (got["psm_probs"]["kind"] == pb.SCORED).any()
    if "ps_bits" in exp:                                            # ... and the golden file's own pep_scores
        off, sites, psms = probs_ref.batch_records(settings, batch, exp, exp, synth.unpack_psm)
        _close(got, dict(site_off=off, site_probs=sites, psm_probs=psms), case + " (golden pep_scores)")


@pytest.mark.parametrize("cfg,n", [("cfg1", 300), ("cfg2", 300), ("cfg3", 200), ("cfg4", 60), ("cfg5", 24)])
def test_seeded_batches_equal_the_yardstick(cfg, n):
    """every kernel family: fused (cfg1-3), score_cnt (cfg3's 495), score_cntg / nodes (cfg4: losses, charges), score_big (cfg5)"""
    batch, settings = synth.make_batch(cfg, n_psm=n, seed=9510)
    _, got = _against_yardstick(settings, batch, cfg)
    assert (got["psm_probs"]["kind"] == pb.SCORED).all()
    best = pb.best_prob(got["psm_probs"])
    assert ((best > 0) & (best <= 1)).all()


@pytest.mark.parametrize("general", [False, True])
def test_realistic_batches_equal_the_yardstick(general):
    batch, settings = synth.make_realistic(40, seed=9520 + general, general=general)
    _against_yardstick(settings, batch, "realistic general=%s" % general)


def test_general_kernel_psms():
    """beyond the fast kernels' limits: a peptide above 64 residues, n_top 12, five loss masses"""
    batch, settings = synth.make_batch("cfg2", n_psm=4, seed=9540, L=80, n_sites=5, n_mod=2)
    _, got = _against_yardstick(settings, batch, "80 residues")
    assert (got["psm_probs"]["kind"] == pb.SCORED).all()
    batch, settings = synth.make_batch("cfg2", n_psm=10, seed=9541)
    _against_yardstick(dict(settings, n_top=12), batch, "n_top 12")
    nls = [["s", 97.9769], ["t", 97.0], ["y", 79.9], ["S", 18.01528], ["T", 17.0265]]
    _against_yardstick(dict(settings, neutral_losses=nls), synth.slice_batch(batch, 0, 6), "five loss masses")


@pytest.mark.parametrize("case", range(len(CASES)))
def test_count_node_front_end_equals_the_general_one(case, monkeypatch):
    """the shapes of tests/test_gpu_count_nodes.py, with peaks AT the window ends of fragments so that marked nodes occur:
    the tables, the general front end and the tables with every node marked leave the same bytes"""
    over, st_over = CASES[case]
    monkeypatch.setenv("PYA_NO_TINY", "1")
    batch, settings = synth.make_batch("cfg5", n_psm=6, seed=40 + case, **over)
    settings = dict(settings, **st_over)
    rng = np.random.default_rng(case)
    for label, b2 in (("plain", batch), ("edges", _edge_spectra(batch, settings, rng, 0.5)), ("edges_wide", _edge_spectra(batch, settings, rng, 0.0))):
        table = _gpu(settings).score_batch(b2, probs=True, site_sig_cap=0)
        general = _gpu(settings, PYA_NO_PROB_CNT="1").score_batch(b2, probs=True, site_sig_cap=0)
        marked = _gpu(settings, PYA_DEBUG=str(0x40000000)).score_batch(b2, probs=True, site_sig_cap=0)
        assert (table["psm_probs"]["kind"] == pb.SCORED).all(), label
        _same_bytes(general, table, "%d %s: general front end" % (case, label))
        _same_bytes(marked, table, "%d %s: every node marked" % (case, label))
    gpu = _gpu(settings)
    got = gpu.score_batch(batch, probs=True, site_sig_cap=0)
    _close(got, _yardstick(gpu, settings, batch, got), "case %d" % case)


@pytest.mark.parametrize("cfg,n,want", [("cfg2", 300, 1), ("cfg3", 200, 1), ("cfg5", 24, 1), ("cfg4", 60, 2)])
def test_the_front_end_a_launch_takes(cfg, n, want):
    """plain settings: the count-node tables alone, so every SCORED record below came through them; losses and charges
    (cfg4), PYA_NO_PROB_CNT, a tolerance above 0.49: the general front end alone"""
    batch, settings = synth.make_batch(cfg, n_psm=n, seed=9530)
    gpu = _gpu(settings)
    got = gpu.score_batch(batch, probs=True, site_sig_cap=0)
    assert (got["psm_probs"]["kind"] == pb.SCORED).all()
    sw, lds = _front_ends(gpu)
    assert sw == (want, 0), (cfg, sw)
    assert 1024 < lds[0] <= 160 * 1024 and lds[1] == 0
    if want == 1:
        assert lds[0] <= 64 * 1024                                  # the tables are held to what a score_cnt bucket may take
        forced = _gpu(settings, PYA_NO_PROB_CNT="1")
        _same_bytes(forced.score_batch(batch, probs=True, site_sig_cap=0), got, cfg)
        assert _front_ends(forced)[0] == (2, 0)
        wide = _gpu(dict(settings, mz_error=0.5))
        assert (wide.score_batch(batch, probs=True, site_sig_cap=0)["psm_probs"]["kind"] == pb.SCORED).all()
        assert _front_ends(wide)[0] == (2, 0)
    # a PSM with more modifications than sites is not scored: it neither sets the caps nor forces the general front end
    if cfg == "cfg2":
        psms = []
        for i in range(8):
            kw = synth.unpack_psm(batch, i)
            psms.append(dict(mz=kw["mz_arr"], intensity=kw["int_arr"], peptide=kw["peptide"], n_of_mod=kw["n_of_mod"], max_charge=1))
        base = gpu.score_batch(synth.pack_batch(psms), skip_invalid=True, probs=True, site_sig_cap=0)
        lds_base = _front_ends(gpu)[1][0]
        psms.append(dict(psms[0], peptide="AGSPEPIDEK", n_of_mod=25))
        more = gpu.score_batch(synth.pack_batch(psms), skip_invalid=True, probs=True, site_sig_cap=0)
        assert _front_ends(gpu) == ((1, 0), (lds_base, 0)) and more["psm_probs"]["kind"][8] == pb.NONE
        assert more["psm_probs"][:8].tobytes() == base["psm_probs"].tobytes()


def test_sums_are_sequential_in_list_order():
    """the header's promise: given the weights, a host loop in the order of the signature list reproduces the sums -- here up
    to exp2 (an ulp or two per weight), where the yardstick in another order is only held to 1e-12"""
    for cfg, n, over in (("cfg2", 40, {}), ("cfg3", 40, {}), ("cfg5", 6, {}), ("cfg5", 4, dict(L=30, n_sites=16, n_mod=6))):
        batch, settings = synth.make_batch(cfg, n_psm=n, seed=9535, **over)
        gpu = _gpu(settings)
        got = gpu.score_batch(batch, probs=True, site_sig_cap=0)
        want = _list_order_records(gpu, settings, batch, got)
        assert np.array_equal(got["psm_probs"]["kind"], want["psm_probs"]["kind"]) and np.array_equal(got["psm_probs"]["n_summed"], want["psm_probs"]["n_summed"])
        tol = probs_ref.RTOL_ORDERED
        np.testing.assert_allclose(got["psm_probs"]["z"], want["psm_probs"]["z"], rtol=tol, atol=0, err_msg=cfg)
        for f in ("with_prob", "without_prob"):
            np.testing.assert_allclose(got["site_probs"][f], want["site_probs"][f], rtol=tol, atol=1e-300, err_msg=cfg + " " + f)


def _dense_psms(seed, sizes):
    """ordinary cfg2 PSMs (plain settings: charge 1, no loss) and, behind them, copies of the first ones whose spectra are
    padded to `sizes` peaks -- above PYA_FAST_PEAKS such a PSM goes to the general kernel"""
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
    """a PSM of the general list under plain settings: short peptide, charge 1, a retained table far above what the plan's
    peak classes are sized for.  Alone, as a handful, beside sparse PSMs, through score(): SCORED, equal to the yardstick and
    to the general front end bytewise -- and the sparse PSMs beside it keep the count-node tables"""
    settings, sparse, dense = _dense_psms(9545, (10_000, 8193, 20_000))
    gpu, forced = _gpu(settings), _gpu(settings, PYA_NO_PROB_CNT="1")
    for what, psms, want_sw in (("alone", dense[:1], (0, 2)), ("a handful", dense, (0, 2)), ("beside sparse PSMs", sparse + dense[:2], (1, 2)),
                                ("one sparse PSM first", sparse[:1] + dense[:1], (1, 2))):
        batch = synth.pack_batch(psms)
        got = gpu.score_batch(batch, probs=True, sites=True, site_sig_cap=0)
        assert _front_ends(gpu)[0] == want_sw, what
        assert (got["psm_probs"]["kind"] == pb.SCORED).all() and (got["psm_probs"]["z"] >= 1).all(), what
        _close(got, _yardstick(gpu, settings, batch, got), what)
        _check_definition(batch, got, what)
        _same_bytes(forced.score_batch(batch, probs=True, site_sig_cap=0), got, what + " (general front end)")
    kw = synth.unpack_psm(synth.pack_batch(dense[:1]), 0)                      # PyAscore.probs: a batch of one
    gpu.score(**kw)
    mine = gpu.probs
    one = gpu.score_batch(synth.pack_batch(dense[:1]), probs=True, site_sig_cap=0)
    assert mine["psm_prob"]["kind"] == pb.SCORED and mine["site_probs"].tobytes() == one["site_probs"].tobytes()
    # a spectrum inside the fast limits whose table does not fit the 64 KiB of the tables: the general front end for that PSM,
    # the tables for its neighbours
    settings, sparse, dense = _dense_psms(9546, (8000,))
    batch = synth.pack_batch(sparse + dense)
    got = gpu.score_batch(batch, probs=True, site_sig_cap=0)
    sw, lds = _front_ends(gpu)
    assert sw == (3, 0) and (got["psm_probs"]["kind"] == pb.SCORED).all()
    _close(got, _yardstick(gpu, settings, batch, got), "8000 peaks")
    _same_bytes(forced.score_batch(batch, probs=True, site_sig_cap=0), got, "8000 peaks (general front end)")
    alone = gpu.score_batch(synth.pack_batch(sparse), probs=True, site_sig_cap=0)
    assert _front_ends(gpu)[0] == (1, 0) and alone["psm_probs"].tobytes() == got["psm_probs"][:len(sparse)].tobytes()


def test_sig_cap():
    batch, settings = synth.make_realistic(40, seed=9550, general=True)
    gpu = _gpu(settings)
    full = gpu.score_batch(batch, probs=True, site_sig_cap=0)
    cap = int(np.median(full["n_sig"]))
    assert (full["n_sig"] > cap).any() and (full["n_sig"] <= cap).any()
    got = gpu.score_batch(batch, probs=True, sites=True, site_sig_cap=cap)
    _close(got, _yardstick(gpu, settings, batch, got, cap), "cap %d" % cap)
    over = got["n_sig"] > cap
    psm = np.repeat(np.arange(40), np.diff(got["site_off"]))
    assert (got["psm_probs"]["kind"][over] == pb.OVER).all() and not got["psm_probs"]["z"][over].any()
    assert (got["site_probs"]["with_prob"][over[psm]] == -1).all() and (got["site_probs"]["without_prob"][over[psm]] == -1).all()
    assert got["psm_probs"][~over].tobytes() == full["psm_probs"][~over].tobytes()
    assert got["site_probs"][~over[psm]].tobytes() == full["site_probs"][~over[psm]].tobytes()
    assert ((got["sites"]["kind"] == st.OVER) == over[psm]).all()              # the site table of the call takes the same cap
    assert np.isnan(pb.best_prob(got["psm_probs"])[over]).all()
    _same_bytes(gpu.score_batch(batch, probs=True), full, "default cap above every PSM")


def test_unscored_and_set_aside_psms():
    good, settings = synth.make_batch("cfg2", n_psm=6, seed=9560)
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
    off = np.zeros(7, np.int64)
    assert gpu._lib.pya_last_batch_probs(gpu._h, None, None, None, 0) == _lib.PYA_ERR_ARG
    assert gpu._lib.pya_last_batch_probs(gpu._h, off.ctypes.data_as(C.c_void_p), None, None, 0) == _lib.PYA_ERR_STATE   # no batch with the flag yet
    assert b"PYA_FLAG_PROBS" in gpu._lib.pya_last_error(gpu._h)
    assert gpu._lib.pya_set_debug(gpu._h, b"PYA_NO_PROB_CNT", b"1") == 0 and gpu._lib.pya_set_debug(gpu._h, b"PYA_NO_PROB_CNT", None) == 0
    plain = gpu.score_batch(batch, skip_invalid=True)
    got = gpu.score_batch(batch, skip_invalid=True, probs=True)
    for key in KEYS + ("status",):
        assert got[key].tobytes() == plain[key].tobytes(), key
    n_rec = np.diff(got["site_off"])
    pp, sp = got["psm_probs"], got["site_probs"]
    assert got["status"][[1, 3]].all() and n_rec[1] == 0 and n_rec[3] == 0 and pp[[1, 3]].tobytes() == b"\0" * 32
    r0 = sp[got["site_off"][0]:got["site_off"][1]]
    assert n_rec[0] == 3 and pp["kind"][0] == pb.SCORED and pp["z"][0] == 1.0 and pp["n_summed"][0] == 1
    assert (r0["with_prob"] == 1).all() and (r0["without_prob"] == 0).all()
    assert n_rec[2] == 1 and pp["kind"][2] == pb.NONE and sp[got["site_off"][2]].tobytes() == b"\0" * 16
    r5 = sp[got["site_off"][5]:got["site_off"][6]]
    assert n_rec[5] == 3 and pp["kind"][5] == pb.SCORED and pp["z"][5] == 1.0 and (r5["with_prob"] == 0).all() and (r5["without_prob"] == 1).all()
    _close(got, _yardstick(gpu, settings, batch, got, 0, got["status"]), "mixed batch")
    general = _gpu(settings, PYA_NO_PROB_CNT="1").score_batch(batch, skip_invalid=True, probs=True)
    _same_bytes(general, got, "mixed batch, general front end")
    with pytest.raises(ValueError):                                            # without skip_invalid the call fails as before
        gpu.score_batch(batch, probs=True)
    assert gpu._lib.pya_last_batch_probs(gpu._h, off.ctypes.data_as(C.c_void_p), None, None, 0) == _lib.PYA_ERR_STATE
    gpu.score_batch(batch, skip_invalid=True, probs=True)
    assert gpu._lib.pya_last_batch_probs(gpu._h, off.ctypes.data_as(C.c_void_p), None, None, 0) == 0 and off[-1] == sp.size
    out = np.zeros(sp.size, pb.SITE_PROB_DTYPE)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert gpu._lib.pya_last_batch_probs(gpu._h, vp(off), vp(out), vp(np.zeros(6, pb.PSM_PROB_DTYPE)), sp.size - 1) == _lib.PYA_ERR_ARG
    assert gpu._lib.pya_last_batch_probs(gpu._h, vp(off), vp(out), None, sp.size) == _lib.PYA_ERR_ARG
    assert gpu._lib.pya_last_batch_probs(gpu._h, vp(off), None, vp(np.zeros(6, pb.PSM_PROB_DTYPE)), sp.size) == _lib.PYA_ERR_ARG


def _records_of(res, i):
    lo, hi = res["site_off"][i:i + 2]
    return res["site_probs"][lo:hi].tobytes() + res["psm_probs"][i].tobytes()


def test_bytes_do_not_depend_on_the_context(monkeypatch):
    """a PSM alone, inside a 100 000-PSM batch, in a chunked call, shared against expanded, float32 against widened"""
    big = synth.make_slice(synth.describe("cfg2", 100_000, seed=9570))
    settings = synth.describe("cfg2", 1, seed=9570)["settings"]
    gpu = _gpu(settings)
    whole = gpu.score_batch(big, probs=True)
    n_chunks = gpu._lib.pya_debug_last_chunks(gpu._h)
    assert (whole["psm_probs"]["kind"] == pb.SCORED).all()
    for i in (0, 1, 49_999, 99_999):
        one = gpu.score_batch(synth.slice_batch(big, i, i + 1), probs=True)
        assert _records_of(one, 0) == _records_of(whole, i), i
        gpu.score(**synth.unpack_psm(big, i))                                 # PyAscore.probs: a batch of one, produced when read
        mine = gpu.probs
        assert mine["site_probs"].tobytes() + mine["psm_prob"].tobytes() == _records_of(whole, i), i
    few = gpu.score_batch(synth.slice_batch(big, 10, 15), probs=True)           # a handful
    assert all(_records_of(few, j) == _records_of(whole, 10 + j) for j in range(5))
    part = synth.slice_batch(big, 0, 12_000)
    monkeypatch.setenv("PYA_NO_CHUNKS", "1")
    switches.from_env(gpu)
    uncut = gpu.score_batch(part, probs=True)
    assert gpu._lib.pya_debug_last_chunks(gpu._h) == 1
    monkeypatch.delenv("PYA_NO_CHUNKS")
    monkeypatch.setenv("PYA_CHUNK_MB", "2")
    switches.from_env(gpu)
    cut = gpu.score_batch(part, probs=True, evidence=True)
    assert gpu._lib.pya_debug_last_chunks(gpu._h) > 8
    monkeypatch.delenv("PYA_CHUNK_MB")
    switches.from_env(gpu)
    _same_bytes(cut, uncut, "chunked")
    assert uncut["site_probs"].tobytes() == whole["site_probs"][:uncut["site_probs"].size].tobytes() and n_chunks >= 1
    assert uncut["psm_probs"].tobytes() == whole["psm_probs"][:12_000].tobytes()
    batch = synth.slice_batch(big, 0, 1500)
    narrow = gpu.score_batch(synth.narrow_batch(batch), probs=True)            # float32 spectra against their widened form
    wide = gpu.score_batch(synth.widen_batch(synth.narrow_batch(batch)), probs=True)
    _same_bytes(narrow, wide, "float32")
    small_b, _ = synth.make_batch("cfg2", n_psm=60, seed=9571)
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
    flat = gpu.score_batch(flat_b, probs=True)
    _close(flat, _yardstick(gpu, settings, flat_b, flat), "expanded")
    _same_bytes(gpu.score_batch(shared, probs=True), flat, "shared")
    perm = np.random.default_rng(3).permutation(len(psms))
    shuffled = synth.pack_shared_batch(spectra, [psms[p] for p in perm])
    want = gpu.score_batch(synth.expand_shared_batch(shuffled), probs=True)
    _same_bytes(gpu.score_batch(shuffled, probs=True), want, "shuffled shared")
    _same_bytes(gpu.score_batch(shuffled, probs=True, keep=True), want, "shuffled shared, keep")


def test_all_stage_flags_together():
    """with all five stage flags set, every other record is what it is without PYA_FLAG_PROBS"""
    batch, settings = synth.make_batch("cfg3", n_psm=400, seed=9580)
    gpu = _gpu(settings)
    q = [[int(b)] for b in gpu.score_batch(batch)["best_sig"]]
    plain = gpu.score_batch(batch, evidence=True, ions=True, named=q, sites=True)
    got = gpu.score_batch(batch, evidence=True, ions=True, named=q, sites=True, probs=True)
    for key in KEYS + ("evidence", "ion_off", "ions", "named", "site_off", "sites"):
        assert got[key].tobytes() == plain[key].tobytes(), key
    _same_bytes(got, gpu.score_batch(batch, probs=True), "beside the other stages")
    _check_definition(batch, got, "cfg3")


def test_plan_api_and_score_one():
    import torch
    from pyascore_amd.device import DevicePlan, psm_prob_records
    batch, settings = synth.make_batch("cfg3", n_psm=3000, seed=9590)          # fused PSMs beside others: the run forks
    gpu = _gpu(settings)
    want = gpu.score_batch(batch, probs=True, site_sig_cap=0)
    dev = torch.device("cuda", 0)
    mz, it = torch.from_numpy(batch["mz"]).to(dev), torch.from_numpy(batch["intensity"]).to(dev)
    plan = DevicePlan(gpu, batch)
    raw = torch.zeros((int(want["site_off"][-1]), 2), dtype=torch.float64, device=dev)
    rawp = torch.zeros((3000, 16), dtype=torch.uint8, device=dev)
    assert gpu._lib.pya_plan_probs(plan._plan, C.byref(plan._res), None, 0, raw.data_ptr(), rawp.data_ptr()) == _lib.PYA_ERR_STATE
    s1 = torch.cuda.Stream(dev)
    with torch.cuda.stream(s1):
        plan.run(mz, it)
        off, a, ap = plan.probs()
        _, b, bp = plan.probs()
        _, b2, bp2 = plan.probs(out=(torch.full_like(b, 7.0), torch.full_like(bp, 7)))     # into the caller's tensors
    other = torch.cuda.Stream(dev)
    with torch.cuda.stream(other):                                             # another stream than the run's waits for it
        _, c, cp = plan.probs()
        _, sites = plan.sites()                                                # ... and shares the uploaded offsets
    torch.cuda.synchronize()
    plan.check()
    assert gpu._lib.pya_plan_probs(plan._plan, C.byref(plan._res), None, 0, raw.data_ptr(), None) == _lib.PYA_ERR_ARG
    assert np.array_equal(off, want["site_off"])
    with pytest.raises(ValueError):
        plan.probs(out=(b.float(), bp))
    for t, tp, what in ((a, ap, "first"), (b, bp, "again"), (b2, bp2, "out="), (c, cp, "other stream")):
        assert t.cpu().numpy().tobytes() == want["site_probs"].tobytes(), what
        assert psm_prob_records(tp.cpu().numpy()).tobytes() == want["psm_probs"].tobytes(), what
    few = synth.slice_batch(batch, 0, 5)                                       # a handful of PSMs takes the per-stage launches
    p = DevicePlan(gpu, few, probs=True)
    p.run(torch.from_numpy(few["mz"]).to(dev), torch.from_numpy(few["intensity"]).to(dev))
    off5, r5, p5 = p.probs()
    p.check()
    n5 = int(want["site_off"][5])
    assert np.array_equal(off5, want["site_off"][:6]) and r5.cpu().numpy().tobytes() == want["site_probs"][:n5].tobytes()
    assert psm_prob_records(p5.cpu().numpy()).tobytes() == want["psm_probs"][:5].tobytes()
    kw = synth.unpack_psm(batch, 0)
    m, i = np.ascontiguousarray(kw["mz_arr"], np.float64), np.ascontiguousarray(kw["int_arr"], np.float64)
    pep = np.frombuffer(kw["peptide"].encode(), np.uint8)
    res = (np.zeros(1, np.float32), np.zeros(1, np.uint64), np.zeros(1, np.int32), np.zeros((1, 4), np.float32), np.zeros((1, 4), np.uint64))
    r = _lib.Results(4, *[x.ctypes.data_as(C.c_void_p) for x in res])
    rc = gpu._lib.pya_score_one(gpu._h, m.ctypes.data_as(C.c_void_p), i.ctypes.data_as(C.c_void_p), m.size,
                                pep.ctypes.data_as(C.c_void_p), pep.size, int(kw["n_of_mod"]), int(kw["max_fragment_charge"]), None, None, 0,
                                _lib.PYA_FLAG_PROBS, C.byref(r))
    assert rc == _lib.PYA_ERR_ARG and b"PYA_FLAG_PROBS" in gpu._lib.pya_last_error(gpu._h)


def test_batch_cli_columns():
    from test_batch_cli import _toy_inputs
    from pyascore_amd import PyAscore, batch_cli
    spectra, psms = _toy_inputs()
    gpu = PyAscore(100.0, 10, "STY", 79.966331, 0.05, "by")
    plain = batch_cli.localize(gpu, psms, spectra, "STY", 79.966331, hit_depth=2, max_fragment_charge=3)
    wide = batch_cli.localize(gpu, psms, spectra, "STY", 79.966331, hit_depth=2, max_fragment_charge=3, probs=True)
    assert len(plain) == len(wide) and all(len(r) == 7 for r in wide)
    assert all(str(a) == str(b) for ra, rb in zip(wide, plain) for a, b in zip(ra[:5], rb))     # the first five as they were
    seen = 0
    for row in wide:
        if not row[1]:
            continue
        assert 0 < float(row[6]) <= 1 and "(" in row[5]
        seen += 1
    assert seen
