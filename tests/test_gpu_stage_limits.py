"""The stages behind a run at the general route's limits (tests/limitcases.py) on the device: evidence, ion records, named
localisations, site tables, site probabilities, ranked localisations, explained ion current and the mass-error profile of PSMs
with 511 residues, fragment charge 255, n_top 16, eight loss masses, 65 535 peaks, 4 096 theoretical fragments per site
assignment and more than 15 000 site assignments.

THE ANCHOR (test_the_run_equals_the_checker): the run's results and its retained per-assignment records are held to the
checker, PSM by PSM.  Every stage is then held to its CPU yardstick computed from the CHECKER's answers -- nothing a stage is
compared with comes from the library.  tests/test_limitcases_host.py proves on the CPU that those yardsticks carry positions and
sizes above 255, charge 255, depth and rank up to 15: only therefore do the field checks here say anything.

One scorer per settings and module (the score table up to row 4 096 is built once), one run per case."""
import ctypes as C

import numpy as np
import pytest

import ions_ref
import limitcases as lc
import probs_ref
import switches
import test_gpu_coverage as t_coverage
import test_gpu_evidence as t_evidence
import test_gpu_ions as t_ions
import test_gpu_mz_profile as t_mz_profile
import test_gpu_named as t_named
import test_gpu_ranked as t_ranked
import test_gpu_sites as t_sites
from conftest import checker_kind
from oracle import harness
from pyascore_amd import _lib, rollup as ru, synth

pytestmark = pytest.mark.gpu

STAGES = dict(evidence=True, ions=True, sites=True, probs=True, ranked=lc.RANKED_K, coverage=True, mz_profile={})
OUTPUTS = ("evidence", "ion_off", "ions", "named_off", "named", "named_counts", "named_scores", "site_off", "sites", "site_probs",
           "psm_probs", "ranked", "coverage", "mz_profile")
SCORED_CASES = [n for n in lc.NAMES if n != "past_last_row"]
_scorers, _runs = {}, {}


def _new_scorer(settings):
    from pyascore_amd import PyAscore
    return harness.make_scorer(PyAscore, settings)


def _scorer(settings):
    key = repr(sorted(settings.items()))
    if key not in _scorers:
        _scorers[key] = _new_scorer(settings)
    return _scorers[key]


def _want(name, sig_cap=0):
    """the checker's answers and every stage's yardstick over them"""
    res, ps = lc.answer(name, checker_kind())
    return res, ps, lc.yardsticks(name, res, ps, sig_cap=sig_cap, key=checker_kind())


def _all_stages(gpu, name, **kw):
    _, batch, _ = lc.case(name)
    res, ps = lc.answer(name, checker_kind())
    return gpu.score_batch(batch, named=lc.queries(name, res, ps), **dict(STAGES, **kw))


def _run(name):
    """(scorer, plain results, results with every stage) of a case; made once"""
    if name not in _runs:
        settings, batch, info = lc.case(name)
        gpu = _scorer(settings)
        skip = dict(skip_invalid=True) if info["refused"] else {}
        _runs[name] = (gpu, gpu.score_batch(batch, **skip), _all_stages(gpu, name, site_sig_cap=0, **skip))
    return _runs[name]


def _same_outputs(a, b, what, keys=lc.KEYS + OUTPUTS):
    for key in keys:
        x, y = np.ascontiguousarray(a[key]), np.ascontiguousarray(b[key])
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), (what, key)


def _device_order(gpu, i, n):
    cnt = C.c_uint64()
    order = np.zeros(n, np.uint64)
    assert gpu._lib.pya_debug_signature_list(gpu._h, i, order.ctypes.data_as(C.c_void_p), order.size, C.byref(cnt)) == 0 and cnt.value == n
    return order


def _probs_in_device_order(gpu, name, res, ps, status=None):
    """probs_ref over the CHECKER's records, every PSM's sums replayed in the order of the device's signature list (read back
    after a keep=True run of the same batch on the same scorer)"""
    settings, batch, info = lc.case(name)
    gpu.score_batch(batch, keep=True, skip_invalid=status is not None)
    n = int(batch["n_psm"])
    sites, psms, off = [np.zeros(0, probs_ref.SITE_DTYPE)], np.zeros(n, probs_ref.PSM_DTYPE), [0]
    for i in range(n):
        if status is not None and status[i]:
            off.append(off[-1])
            continue
        lo, hi = int(ps["rec_off"][i]), int(ps["rec_off"][i + 1])
        ns = len(lc.sites_of(settings, synth.unpack_psm(batch, i)["peptide"]))
        s, psms[i] = probs_ref.psm_records(ns, res["best_score"][i], ps["sig_bits"][lo:hi], ps["weighted_score"][lo:hi],
                                           order=_device_order(gpu, i, hi - lo))
        sites.append(s)
        off.append(off[-1] + ns)
    return dict(site_off=np.asarray(off, np.int64), site_probs=np.concatenate(sites), psm_probs=psms)


def _close_ordered(got, want, what):
    tol = probs_ref.RTOL_ORDERED
    assert np.array_equal(got["site_off"], want["site_off"]), what
    assert np.array_equal(got["psm_probs"]["kind"], want["psm_probs"]["kind"]) and np.array_equal(got["psm_probs"]["n_summed"], want["psm_probs"]["n_summed"]), what
    np.testing.assert_allclose(got["psm_probs"]["z"], want["psm_probs"]["z"], rtol=tol, atol=0, err_msg=what)
    for f in ("with_prob", "without_prob"):
        np.testing.assert_allclose(got["site_probs"][f], want["site_probs"][f], rtol=tol, atol=1e-300, err_msg=what + " " + f)


def _no_stray_bytes(got, what):
    """reserved and pad bytes of every record are zero"""
    for key in ("evidence", "ions", "named", "sites", "psm_probs", "ranked", "coverage"):
        for f in got[key].dtype.names:
            if f.startswith(("reserved", "pad")):
                assert not np.asarray(got[key][f]).any(), (what, key, f)


def _against_yardsticks(name, gpu, plain, got, y, status=None):
    res, ps = lc.answer(name, checker_kind())
    for key in lc.KEYS:                                                          # asking for the stages changes no byte of the run
        assert got[key].tobytes() == plain[key].tobytes(), (name, key)
    t_evidence._same_rows(got["evidence"], y["evidence"], name)
    t_ions._same_records(got["ion_off"], ions_ref.canonical_batch(got["ion_off"], got["ions"]), y["ion_off"], y["ions"], name)
    t_named._same_named(got, y, name)
    t_sites._same_sites(got, y, name)
    _close_ordered(got, _probs_in_device_order(gpu, name, y["res"], ps, status), name)
    assert not got["psm_probs"]["pad"].any()
    t_ranked._same_bytes(got["ranked"], y["ranked"], name)
    t_coverage._same_bytes(got["coverage"], y["coverage"], name)
    t_mz_profile._same_bytes(got["mz_profile"], y["mz_profile"], name)
    _no_stray_bytes(got, name)


# ---- the anchor ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(lc.NAMES))
def test_the_run_equals_the_checker(name):
    """best_sig, best_score, n_sig, Ascores, the alternative sites (as bits of the library's layout, made from the checker's
    positions) and every field of batch_pep_scores() in the checker's sorted order, PSM by PSM"""
    settings, batch, info = lc.case(name)
    res, ps = lc.answer(name, checker_kind())
    gpu, plain, _ = _run(name)
    ok = [i for i in range(int(batch["n_psm"])) if i not in info["refused"]]
    for key in lc.KEYS:
        assert plain[key].dtype == res[key].dtype and plain[key][ok].tobytes() == res[key][ok].tobytes(), (name, key)
    kept = gpu.score_batch(batch, keep=True, skip_invalid=bool(info["refused"]))
    for key in lc.KEYS:
        assert kept[key].tobytes() == plain[key].tobytes(), (name, key)
    mine = gpu.batch_pep_scores()
    for i in ok:
        lo, hi = int(ps["rec_off"][i]), int(ps["rec_off"][i + 1])
        a = int(mine["rec_off"][i])
        assert int(mine["rec_off"][i + 1]) - a == hi - lo, (name, i)
        for key in ("sig_bits", "counts", "scores", "weighted_score", "total_fragments"):
            assert np.array_equal(mine[key][a:a + hi - lo], ps[key][lo:hi]), (name, i, key)
        assert mine["scores"][a:a + hi - lo].tobytes() == ps["scores"][lo:hi].astype(mine["scores"].dtype).tobytes(), (name, i)
    for i in info["refused"]:
        assert mine["rec_off"][i + 1] == mine["rec_off"][i]


# ---- every stage, every case -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCORED_CASES)
def test_every_stage_equals_its_yardstick(name):
    gpu, plain, got = _run(name)
    _, _, y = _want(name)
    _against_yardsticks(name, gpu, plain, got, y)


def _matched(ions):
    return ions[ions["rank"] != ions_ref.NO_MATCH]


def test_fields_wider_than_a_byte_survive():
    """on the library's records: comp_pos, pos and size above 255; a 16-bit position on either side of 256"""
    for name in ("far_positions", "long_list", "big_retained"):
        got = _run(name)[2]
        assert (got["evidence"]["comp_pos"] > 256).any() and (got["sites"]["pos"] > 256).any() and (_matched(got["ions"])["size"] > 255).any(), name
        assert (got["ranked"]["kind"][:, 0] == 1).all() and (got["named"]["kind"] >= 3).any(), name
    got = _run("byte_edge")[2]
    assert {255, 256, 257} <= set(got["sites"]["pos"].tolist()) and {255, 256} <= set(_matched(got["ions"])["size"].tolist())
    got = _run("long_list")[2]
    m = _matched(got["ions"])
    assert ((m["charge"] == 8) & (m["size"] > 255)).any()


def test_fields_as_wide_as_a_byte_survive():
    """charge 255; depth and rank up to 15"""
    m = _matched(_run("charge_255")[2]["ions"])
    assert (m["charge"] == 255).any() and (m["charge"] >= 128).any()
    assert (_matched(_run("charge_40")[2]["ions"])["charge"] > 16).any()
    for name in ("ntop16", "ntop16_cfg4", "eight_losses_ntop16", "big_retained"):
        got = _run(name)[2]
        m = _matched(got["ions"])
        assert (m["rank"] == 15).any() and (got["evidence"]["depth"] >= 10).any(), name
        assert ((got["named"]["kind"] == 4) & (got["named"]["depth"] >= 10)).any() or name == "big_retained", name
    ev = _run("ntop16_cfg4")[2]["evidence"]
    assert (ev["depth"] == 15).any()
    cov = _run("most_peaks")[2]["coverage"]
    assert cov["n_peaks"].max() == 65535
    assert _run("big_retained")[2]["coverage"]["n_retained"].min() > 8192


# ---- more than 15 000 site assignments -------------------------------------------------------------------------------------
def test_many_assignments_and_the_cap():
    """sig_cap 0 is test_every_stage_equals_its_yardstick's run: sites, probabilities and ranked rows over all 15 504 / 24 310
    assignments.  With a cap of n_sig - 1 of either limit PSM: exactly the OVER records of the header, byte for byte the
    yardstick's, and every PSM at or under the cap keeps the bytes of the uncapped run"""
    name = "many_assignments"
    settings, batch, info = lc.case(name)
    gpu, plain, full = _run(name)
    assert tuple(full["n_sig"][info["limit"]].tolist()) == info["n_sig"]
    assert (full["psm_probs"]["n_summed"][info["limit"]] == np.array(info["n_sig"])).all() and (full["sites"]["kind"] == 1).all()
    before = int(gpu._lib.pya_get_site_sig_cap(gpu._h))
    try:
        for cap in info["sig_caps"]:
            y = _want(name, sig_cap=cap)[2]
            assert gpu._lib.pya_set_site_sig_cap(gpu._h, cap) == 0
            got = gpu.score_batch(batch, sites=True, probs=True, ranked=lc.RANKED_K)
            t_sites._same_sites(got, y, "cap %d" % cap)
            t_ranked._same_bytes(got["ranked"], y["ranked"], "cap %d" % cap)
            over = full["n_sig"] > cap
            assert over.sum() == (2 if cap == info["sig_caps"][0] else 1)
            assert got["psm_probs"][over].tobytes() == y["psm_probs"][over].tobytes() and (got["psm_probs"]["kind"][over] == 2).all()
            assert got["psm_probs"][~over].tobytes() == full["psm_probs"][~over].tobytes()
            per_site = np.repeat(over, np.diff(got["site_off"]))
            assert got["site_probs"][per_site].tobytes() == y["site_probs"][per_site].tobytes() and (got["site_probs"]["with_prob"][per_site] == -1.0).all()
            assert got["site_probs"][~per_site].tobytes() == full["site_probs"][~per_site].tobytes()
            assert got["sites"][~per_site].tobytes() == full["sites"][~per_site].tobytes() and (got["sites"]["kind"][per_site] == 2).all()
            assert got["ranked"][~over].tobytes() == full["ranked"][~over].tobytes() and (got["ranked"]["kind"][over, 0] == 2).all()
            assert not got["ranked"][over][:, 1:].view(np.uint8).any()
    finally:
        gpu._lib.pya_set_site_sig_cap(gpu._h, before)


# ---- the score table's last row --------------------------------------------------------------------------------------------
def test_a_psm_past_the_last_row_is_refused_and_set_aside():
    name = "past_last_row"
    settings, batch, info = lc.case(name)
    bad = info["refused"][0]
    gpu = _new_scorer(settings)                                                  # its first call is the refused one
    with pytest.raises(ValueError, match=r"PSM %d: up to 4112 theoretical fragments per site assignment; the score table covers 4096" % bad):
        _all_stages(gpu, name, site_sig_cap=0)
    assert gpu._lib.pya_error_index(gpu._h) == bad
    plain = gpu.score_batch(batch, skip_invalid=True)
    got = _all_stages(gpu, name, site_sig_cap=0, skip_invalid=True)
    status = lc.status_of(name)
    assert got["status"].tolist() == status.tolist() and "score table" in got["status_message"]
    assert got["n_sig"][bad] == -1 and got["best_score"][bad] == -1.0 and got["best_sig"][bad] == 0
    y = _want(name)[2]
    _against_yardsticks(name, gpu, plain, got, y, status)
    assert not got["evidence"][bad].view(np.uint8).any() and got["ion_off"][bad] == got["ion_off"][bad + 1]
    assert got["site_off"][bad] == got["site_off"][bad + 1] and not got["psm_probs"][bad:bad + 1].view(np.uint8).any()
    assert not got["ranked"][bad].view(np.uint8).any() and not got["coverage"][bad:bad + 1].view(np.uint8).any()
    a, e = int(got["named_off"][bad]), int(got["named_off"][bad + 1])
    assert e - a == 1 and got["named"][a].tobytes()[8:] == bytes(24)
    # ... and the scorer that refused scores last_row to the bytes of one that never did
    _same_outputs(_all_stages(gpu, "last_row", site_sig_cap=0), _run("last_row")[2], "last_row after the refusal")
    gpu.score_batch(lc.case("last_row")[1], keep=True)
    assert (gpu.batch_pep_scores()["total_fragments"] == 4096).any()                  # (row 4 096 of the table was read)


# ---- one call, chunks, a resident plan -------------------------------------------------------------------------------------
def _forms_among_7000():
    """the limit PSMs of `forms` at four places among 7 000 cfg2 PSMs (36 MB of spectra: a batch call cuts nothing smaller)"""
    _, forms, info = lc.case("forms")
    big = synth.make_slice(synth.describe("cfg2", 7000, seed=8790))
    lim = info["limit"]
    parts = [synth.slice_batch(big, 0, 2500), lc.take(forms, [lim[0], lim[2]]), synth.slice_batch(big, 2500, 5000),
             lc.take(forms, [lim[1], lim[3]]), synth.slice_batch(big, 5000, 7000)]
    where = {lim[0]: 2500, lim[2]: 2501, lim[1]: 5002, lim[3]: 5003}
    return synth.concat_batches(parts), where


def test_one_call_and_chunks_give_the_same_bytes(monkeypatch):
    settings, forms, info = lc.case("forms")
    small = _run("forms")[2]
    batch, where = _forms_among_7000()
    for i, at in where.items():
        assert synth.unpack_psm(batch, at)["peptide"] == synth.unpack_psm(forms, i)["peptide"]
    gpu = _scorer(settings)
    stages = dict(STAGES, site_sig_cap=0)
    monkeypatch.setenv("PYA_NO_CHUNKS", "1")
    switches.from_env(gpu)
    whole = gpu.score_batch(batch, **stages)
    assert gpu._lib.pya_debug_last_chunks(gpu._h) == 1
    monkeypatch.delenv("PYA_NO_CHUNKS")
    monkeypatch.setenv("PYA_CHUNK_MB", "2")
    switches.from_env(gpu)
    cut = gpu.score_batch(batch, **stages)
    assert gpu._lib.pya_debug_last_chunks(gpu._h) > 8
    monkeypatch.delenv("PYA_CHUNK_MB")
    switches.from_env(gpu)
    keys = tuple(k for k in lc.KEYS + OUTPUTS if not k.startswith("named"))
    _same_outputs(cut, whole, "chunked", keys)
    for i, at in where.items():                                                  # the limit PSMs: the bytes of the small batch
        for key in lc.KEYS + ("evidence", "ranked", "coverage", "psm_probs"):
            assert whole[key][at].tobytes() == small[key][i].tobytes(), (key, i)
        for off, key in (("ion_off", "ions"), ("site_off", "sites"), ("site_off", "site_probs")):
            assert whole[key][whole[off][at]:whole[off][at + 1]].tobytes() == small[key][small[off][i]:small[off][i + 1]].tobytes(), (key, i)


def test_a_resident_plan_on_a_second_stream_gives_the_same_bytes():
    import torch
    from pyascore_amd import device as dv
    name = "forms"
    settings, batch, info = lc.case(name)
    gpu, _, want = _run(name)
    res, ps = lc.answer(name, checker_kind())
    q = lc.queries(name, res, ps)
    dev = torch.device("cuda", 0)
    mz, it = torch.from_numpy(batch["mz"]).to(dev), torch.from_numpy(batch["intensity"]).to(dev)
    q_off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(x) for x in q])]).astype(np.int64)).to(dev)
    q_bits = torch.from_numpy(np.concatenate([np.asarray(x, np.uint64) for x in q]).view(np.int64)).to(dev)
    plan = dv.DevicePlan(gpu, batch, evidence=True, ions=True, named=True, sites=True, probs=True, ranked=True, mz_profile=True, coverage=True)
    first, second = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    with torch.cuda.stream(first):
        plan.run(mz, it)
    with torch.cuda.stream(second):                                              # another stream than the run's waits for it
        ev = plan.evidence()
        ion_off, ions = plan.ions()
        named, counts, scores = plan.named(q_off, q_bits, counts=True, scores=True)
        site_off, sites = plan.sites(sig_cap=0)
        _, site_probs, psm_probs = plan.probs(sig_cap=0)
        ranked = plan.ranked(lc.RANKED_K, sig_cap=0)
        cov = plan.coverage(mz, it)
        prof = plan.mz_profile(ru.mz_profile_params(float(np.float32(settings["mz_error"])), max_rank=settings["n_top"] - 1))
    torch.cuda.synchronize()
    plan.check()
    host = lambda t: t.cpu().numpy()  # noqa: E731
    got = dict(best_score=host(plan.best_score), best_sig=host(plan.best_sig).view(np.uint64), n_sig=host(plan.n_sig), ascores=host(plan.ascores),
               alt_mask=host(plan.alt_mask).view(np.uint64), evidence=dv.evidence_rows(host(ev)), ion_off=host(ion_off),
               ions=dv.ion_records(host(ions)), named_off=host(q_off), named=dv.named_records(host(named)), named_counts=host(counts),
               named_scores=host(scores), site_off=site_off, sites=dv.site_records(host(sites)),
               site_probs=host(site_probs).view(want["site_probs"].dtype).reshape(-1), psm_probs=dv.psm_prob_records(host(psm_probs)),
               ranked=dv.ranked_records(host(ranked)), coverage=dv.coverage_records(host(cov)), mz_profile=dv.mz_profile_records(host(prof)))
    for key in lc.KEYS + OUTPUTS:
        x, y = np.ascontiguousarray(got[key]), np.ascontiguousarray(want[key])
        assert x.size == y.size and x.tobytes() == y.tobytes(), key
    plan.close()


# ---- guard regions behind the largest LDS launches -------------------------------------------------------------------------
def test_nothing_is_written_behind_the_payload_of_the_longest_lists():
    """long_list (general launches of 102 640 and 146 352 bytes of LDS): pya_plan_evidence and pya_plan_ions fill buffers
    with a 256-byte guard of 0xA5 behind the payload; the payload is the batch call's, the guards keep their fill"""
    import torch
    from pyascore_amd import device as dv
    name = "long_list"
    settings, batch, info = lc.case(name)
    gpu, _, want = _run(name)
    dev = torch.device("cuda", 0)
    mz, it = torch.from_numpy(batch["mz"]).to(dev), torch.from_numpy(batch["intensity"]).to(dev)
    plan = dv.DevicePlan(gpu, batch, evidence=True, ions=True)
    plan.run(mz, it)
    stream = torch.cuda.current_stream(dev).cuda_stream
    n_ev = plan.n_psm * plan.max_k * 16
    ev = torch.full((n_ev + 256,), 0xA5, dtype=torch.uint8, device=dev)
    assert gpu._lib.pya_plan_evidence(plan._plan, C.byref(plan._res), stream, ev.data_ptr()) == 0
    off = torch.empty(plan.n_psm + 1, dtype=torch.int64, device=dev)
    assert gpu._lib.pya_plan_ions_count(plan._plan, C.byref(plan._res), stream, off.data_ptr()) == 0
    total = int(off[-1].item())
    assert total == want["ions"].size > 4080
    ions = torch.full((total * 16 + 256,), 0xA5, dtype=torch.uint8, device=dev)
    assert gpu._lib.pya_plan_ions(plan._plan, C.byref(plan._res), stream, off.data_ptr(), ions.data_ptr(), total) == 0
    torch.cuda.synchronize()
    plan.check()
    ev, ions = ev.cpu().numpy(), ions.cpu().numpy()
    assert (ev[n_ev:] == 0xA5).all() and (ions[total * 16:] == 0xA5).all()
    assert ev[:n_ev].tobytes() == np.ascontiguousarray(want["evidence"]).tobytes()
    assert ions[:total * 16].tobytes() == np.ascontiguousarray(want["ions"]).tobytes()
    plan.close()
