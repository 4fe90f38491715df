"""Site roll-up on the GPU (pya_site_rollup: the probability records of many PSMs collapsed onto caller-keyed slots).
Yardstick: tests/rollup_ref.py fed with the arrays score_batch(probs=True) returns for the same batch -- every comparison is on
the raw bytes of the 32-byte records; no field is a float the stage computes.  Slots are keyed by peptide, and the batches
repeat their peptides against other spectra so that many PSMs share a slot."""
import ctypes as C
import os

import numpy as np
import pytest

import rollup_ref
import switches
from conftest import GOLDEN, golden_cases
from oracle import harness
from pyascore_amd import _lib, probs as pb, rollup as ru, synth

pytestmark = pytest.mark.gpu

KEYS = ("best_score", "best_sig", "n_sig", "ascores", "alt_mask")
THR = 0.75


def _gpu(settings, **debug):
    from pyascore_amd import PyAscore
    gpu = harness.make_scorer(PyAscore, settings)
    for k, v in debug.items():
        gpu.set_debug(k, v)
    return gpu


def _same_bytes(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype.itemsize == 32, what
    bad = np.flatnonzero(got.view("V32") != want.view("V32"))
    assert bad.size == 0, "%s: %d slots differ, first %d: got %s, want %s" % (what, bad.size, bad[0], got[bad[0]], want[bad[0]])


def _repeats(batch, share=3):
    """the batch with the peptides of its first n / share PSMs repeated against the spectra of the others"""
    n = int(batch["n_psm"])
    m = max(1, n // share)
    kws = [synth.unpack_psm(batch, i) for i in range(n)]
    psms = [dict(mz=kws[i]["mz_arr"], intensity=kws[i]["int_arr"], peptide=kws[i % m]["peptide"], n_of_mod=kws[i % m]["n_of_mod"],
                 max_charge=kws[i % m]["max_fragment_charge"]) for i in range(n)]
    return synth.pack_batch(psms), [p["peptide"] for p in psms]


def _peptides(batch):
    return [synth.unpack_psm(batch, i)["peptide"] for i in range(int(batch["n_psm"]))]


def _ref(res, slot, n_slots, thr=THR, psm_id=None, psm_base=0, into=None):
    return rollup_ref.table(res["site_probs"], res["psm_probs"], res["site_off"], res["best_sig"], res["ascores"], slot, n_slots, thr,
                            psm_id=psm_id, psm_base=psm_base, into=into)


def _against_yardstick(settings, batch, peptides, what, skip_invalid=False, cap=0, **debug):
    gpu = _gpu(settings, **debug)
    plain = gpu.score_batch(batch, skip_invalid=skip_invalid, probs=True, site_sig_cap=cap)
    slot, n_slots, keys = ru.peptide_slots(peptides, plain["site_off"], residues=settings["mod_group"])
    req = dict(slot=slot, n_slots=n_slots, threshold=THR)
    got = gpu.score_batch(batch, skip_invalid=skip_invalid, probs=True, rollup=req, site_sig_cap=cap)
    for key in KEYS + ("site_off", "site_probs", "psm_probs") + (("status",) if skip_invalid else ()):
        assert got[key].tobytes() == plain[key].tobytes(), (what, key)          # nothing of the run moves
    want = _ref(plain, slot, n_slots)
    _same_bytes(got["rollup"], want, what)
    alone = gpu.score_batch(batch, skip_invalid=skip_invalid, rollup=req, site_sig_cap=cap)
    for key in KEYS:
        assert alone[key].tobytes() == plain[key].tobytes(), (what, key)
    assert "site_probs" not in alone
    _same_bytes(alone["rollup"], want, what + " (the library's own probability stage)")
    general = _gpu(settings, PYA_NO_PROB_CNT="1", **debug).score_batch(batch, skip_invalid=skip_invalid, rollup=req, site_sig_cap=cap)
    _same_bytes(general["rollup"], want, what + " (general front end)")
    assert not want["reserved"].any() and (want["n_confident"] <= want["n_psm"]).all() and (want["n_in_best"] <= want["n_psm"]).all()
    rows = ru.table(got["rollup"], keys)
    assert len(rows) == int((want["n_psm"] != 0).sum())
    return gpu, got, plain, (slot, n_slots, keys)


@pytest.mark.parametrize("case", [c for c in golden_cases() if c.startswith(("velos_", "ties_", "edge_"))])
def test_golden_cases_equal_the_yardstick(case):
    settings, batch, _ = harness.load_case(os.path.join(GOLDEN, case + ".npz"))
    _, got, _, _ = _against_yardstick(settings, batch, _peptides(batch), case)
    assert got["rollup"]["n_psm"].any()


@pytest.mark.parametrize("cfg,n", [("cfg1", 300), ("cfg2", 300), ("cfg3", 200), ("cfg4", 60), ("cfg5", 24)])
def test_seeded_batches_equal_the_yardstick(cfg, n):
    batch, settings = synth.make_batch(cfg, n_psm=n, seed=9910)
    batch, peptides = _repeats(batch)
    _, got, _, _ = _against_yardstick(settings, batch, peptides, cfg)
    t = got["rollup"]
    assert (t["n_psm"] >= 3).any() and t["n_in_best"].any() and (t["best_psm"] != ru.NO_PSM).all()


@pytest.mark.parametrize("general", [False, True])
def test_realistic_batches_equal_the_yardstick(general):
    batch, settings = synth.make_realistic(60, seed=9920 + general, general=general)
    batch, peptides = _repeats(batch, share=2)
    _against_yardstick(settings, batch, peptides, "realistic general=%s" % general)


def test_set_aside_and_unscored_psms():
    good, settings = synth.make_batch("cfg2", n_psm=12, seed=9930)
    psms = []
    for i in range(good["n_psm"]):
        kw = synth.unpack_psm(good, i)
        psms.append(dict(mz=kw["mz_arr"], intensity=kw["int_arr"], peptide=kw["peptide"], n_of_mod=kw["n_of_mod"], max_charge=1))
    for i in range(6, 12):                                                     # every peptide twice
        psms[i] = dict(psms[i], peptide=psms[i - 6]["peptide"], n_of_mod=psms[i - 6]["n_of_mod"])
    psms[0] = dict(psms[0], peptide="ASGTPEYIDEK", n_of_mod=3)                 # as many modifications as sites
    psms[1] = dict(psms[1], peptide="PEPTXIDESK")                              # unknown residue: set aside, no records
    psms[2] = dict(psms[2], peptide="AGSPEPIDEK", n_of_mod=2)                  # more modifications than sites: not scored
    psms[3] = dict(psms[3], mz=np.zeros(0), intensity=np.zeros(0))             # empty spectrum: set aside
    psms[5] = dict(psms[5], peptide="ASGTPEYIDEK", n_of_mod=0)                 # no modification: covers, reports nothing
    batch = synth.pack_batch(psms)
    peptides = [p["peptide"] for p in psms]
    gpu, got, plain, (slot, n_slots, keys) = _against_yardstick(settings, batch, peptides, "mixed batch", skip_invalid=True)
    assert got["status"][[1, 3]].all() and np.diff(plain["site_off"])[[1, 3]].tolist() == [0, 0]
    t = got["rollup"]
    first = keys.index(("ASGTPEYIDEK", 2))
    assert t["n_psm"][first] == 2 and t["n_in_best"][first] == 1 and t["best_prob"][first] == 1.0 and t["best_psm"][first] == 0
    unscored = keys.index(("AGSPEPIDEK", 3))
    assert t[unscored].tobytes() == ru.empty(1)[0].tobytes()
    with pytest.raises(ValueError):                                            # without skip_invalid the call fails as before
        gpu.score_batch(batch, rollup=dict(slot=slot, n_slots=n_slots))


def test_sig_cap_leaves_psms_out():
    batch, settings = synth.make_realistic(60, seed=9940, general=True)
    batch, peptides = _repeats(batch, share=2)
    n_sig = _gpu(settings).score_batch(batch)["n_sig"]
    cap = int(np.median(n_sig))
    assert (n_sig > cap).any() and (n_sig <= cap).any()
    _, got, plain, (slot, n_slots, _) = _against_yardstick(settings, batch, peptides, "cap %d" % cap, cap=cap)
    over = plain["psm_probs"]["kind"] == pb.OVER
    assert over.any() and got["rollup"]["n_psm"].sum() == int(np.diff(plain["site_off"])[plain["psm_probs"]["kind"] == pb.SCORED].sum())


def test_bytes_do_not_depend_on_the_context(monkeypatch):
    """chunked against uncut, float32 against widened, shared against expanded, a shuffled shared batch in the caller's numbering"""
    big = synth.make_slice(synth.describe("cfg2", 12_000, seed=9950))
    settings = synth.describe("cfg2", 1, seed=9950)["settings"]
    big, peptides = _repeats(big, share=5)
    gpu = _gpu(settings)
    monkeypatch.setenv("PYA_NO_CHUNKS", "1")
    switches.from_env(gpu)
    plain = gpu.score_batch(big, probs=True)
    slot, n_slots, _ = ru.peptide_slots(peptides, plain["site_off"], residues=settings["mod_group"])
    req = dict(slot=slot, n_slots=n_slots, threshold=THR)
    uncut = gpu.score_batch(big, rollup=req)["rollup"]
    assert gpu._lib.pya_debug_last_chunks(gpu._h) == 1
    grid, n_rec = (C.c_uint32 * 2)(), C.c_uint64()
    assert gpu._lib.pya_debug_last_rollup_launch(gpu._h, grid, C.byref(n_rec)) == 0
    assert n_rec.value == slot.size and list(grid) == [(slot.size + 255) // 256] * 2
    monkeypatch.delenv("PYA_NO_CHUNKS")
    monkeypatch.setenv("PYA_CHUNK_MB", "2")
    switches.from_env(gpu)
    cut = gpu.score_batch(big, rollup=req, evidence=True)["rollup"]
    assert gpu._lib.pya_debug_last_chunks(gpu._h) > 8
    cut_probs = gpu.score_batch(big, rollup=req, probs=True)
    monkeypatch.delenv("PYA_CHUNK_MB")
    switches.from_env(gpu)
    want = _ref(plain, slot, n_slots)
    assert (want["n_psm"] >= 5).any()
    _same_bytes(uncut, want, "uncut")
    _same_bytes(cut, want, "chunked")
    _same_bytes(cut_probs["rollup"], want, "chunked, beside PYA_FLAG_PROBS")
    assert cut_probs["site_probs"].tobytes() == plain["site_probs"].tobytes()
    part = synth.slice_batch(big, 0, 1500)
    p_slot = slot[:int(plain["site_off"][1500])]
    p_req = dict(slot=p_slot, n_slots=n_slots, threshold=THR)
    wide = gpu.score_batch(synth.widen_batch(synth.narrow_batch(part)), rollup=p_req, probs=True)
    _same_bytes(wide["rollup"], _ref(wide, p_slot, n_slots), "widened")
    _same_bytes(gpu.score_batch(synth.narrow_batch(part), rollup=p_req)["rollup"], wide["rollup"], "float32")
    small_b, _ = synth.make_batch("cfg2", n_psm=60, seed=9951)
    spectra, psms = [], []
    for i in range(0, 60, 3):
        kw = synth.unpack_psm(small_b, i)
        spectra.append(dict(mz=kw["mz_arr"], intensity=kw["int_arr"]))
        for j in range(3):
            kj = synth.unpack_psm(small_b, (i + j) % 12)
            psms.append(dict(peptide=kj["peptide"], n_of_mod=kj["n_of_mod"], max_charge=1, aux_pos=np.zeros(0, np.uint32),
                             aux_mass=np.zeros(0, np.float32), spectrum=len(spectra) - 1))
    for order, what in ((np.arange(60), "shared"), (np.random.default_rng(3).permutation(60), "shuffled shared")):
        mine = [psms[p] for p in order]
        shared = synth.pack_shared_batch(spectra, mine)
        flat = gpu.score_batch(synth.expand_shared_batch(shared), probs=True)
        s_slot, s_n, _ = ru.peptide_slots([p["peptide"] for p in mine], flat["site_off"], residues=settings["mod_group"])
        s_req = dict(slot=s_slot, n_slots=s_n, threshold=THR)
        want = _ref(flat, s_slot, s_n)                                         # best_psm: the caller's numbering
        assert (want["n_psm"] >= 4).any()
        _same_bytes(gpu.score_batch(synth.expand_shared_batch(shared), rollup=s_req)["rollup"], want, what + ", expanded")
        _same_bytes(gpu.score_batch(shared, rollup=s_req)["rollup"], want, what)
        _same_bytes(gpu.score_batch(shared, rollup=s_req, keep=True)["rollup"], want, what + ", keep")
        ids = (1000 - np.arange(60)).astype(np.uint32)
        _same_bytes(gpu.score_batch(shared, rollup=dict(s_req, psm_id=ids))["rollup"], _ref(flat, s_slot, s_n, psm_id=ids), what + ", psm_id")


def test_mixed_peptide_lengths_keep_the_callers_numbering():
    """the library orders PSMs by shape internally; best_psm names the PSM of the caller's batch"""
    a, settings = synth.make_batch("cfg2", n_psm=40, seed=9960)
    b, _ = synth.make_batch("cfg2", n_psm=40, seed=9961, L=30, n_sites=6, n_mod=2)
    c, _ = synth.make_batch("cfg2", n_psm=4, seed=9962, L=80, n_sites=5, n_mod=2)      # the general kernel's
    psms = []
    for src in (a, b, c):
        for i in range(int(src["n_psm"])):
            kw = synth.unpack_psm(src, i)
            psms.append(dict(mz=kw["mz_arr"], intensity=kw["int_arr"], peptide=kw["peptide"], n_of_mod=kw["n_of_mod"], max_charge=1))
    order = np.random.default_rng(11).permutation(len(psms))
    psms = [psms[j] for j in order] + [psms[j] for j in order[::-1]]            # every PSM twice: ties on every slot
    batch = synth.pack_batch(psms)
    _, got, _, _ = _against_yardstick(settings, batch, [p["peptide"] for p in psms], "mixed lengths")
    t = got["rollup"]
    assert (t["n_psm"] == 2).all() and (t["best_psm"] < len(order)).all() and len(set(t["best_psm"].tolist())) > 40


def test_reversed_ids_move_best_psm_only():
    batch, settings = synth.make_batch("cfg2", n_psm=300, seed=9970)
    batch, peptides = _repeats(batch)
    gpu = _gpu(settings)
    res = gpu.score_batch(batch, probs=True)
    slot, n_slots, _ = ru.peptide_slots(peptides, res["site_off"], residues=settings["mod_group"])
    fwd = gpu.score_batch(batch, rollup=dict(slot=slot, n_slots=n_slots))["rollup"]
    ids = (299 - np.arange(300)).astype(np.uint32)
    rev = gpu.score_batch(batch, rollup=dict(slot=slot, n_slots=n_slots, psm_id=ids))["rollup"]
    _same_bytes(rev, _ref(res, slot, n_slots, psm_id=ids), "reversed ids")
    moved = rev.copy()
    moved["best_psm"] = fwd["best_psm"]
    _same_bytes(moved, fwd, "everything but best_psm")
    bits = res["site_probs"]["with_prob"].view(np.uint64)
    owner = np.repeat(np.arange(300), np.diff(res["site_off"]))
    ties = 0
    for s in range(n_slots):
        at = np.flatnonzero((slot == s) & (bits == fwd["best_prob"][s:s + 1].view(np.uint64)[0]))
        assert fwd["best_psm"][s] == owner[at].min() and rev["best_psm"][s] == ids[owner[at]].min() == 299 - owner[at].max()
        ties += at.size > 1
    assert ties > 10


def _plan(gpu, batch, dev):
    import torch
    from pyascore_amd.device import DevicePlan
    plan = DevicePlan(gpu, batch, rollup=True)
    plan.run(torch.from_numpy(batch["mz"]).to(dev), torch.from_numpy(batch["intensity"]).to(dev))
    return plan


def test_accumulation_over_plans_equals_one_call():
    import torch
    from pyascore_amd.device import rollup_records
    batch, settings = synth.make_batch("cfg3", n_psm=600, seed=9980)
    batch, peptides = _repeats(batch, share=4)
    gpu = _gpu(settings)
    res = gpu.score_batch(batch, probs=True, site_sig_cap=0)
    slot, n_slots, _ = ru.peptide_slots(peptides, res["site_off"], residues=settings["mod_group"])
    whole = gpu.score_batch(batch, rollup=dict(slot=slot, n_slots=n_slots), site_sig_cap=0)["rollup"]
    _same_bytes(whole, _ref(res, slot, n_slots), "one call")
    dev = torch.device("cuda", 0)
    cut, rec = 250, int(res["site_off"][250])
    halves = [(synth.slice_batch(batch, 0, cut), slot[:rec], 0), (synth.slice_batch(batch, cut, 600), slot[rec:], cut)]
    ids = np.random.default_rng(5).permutation(600).astype(np.uint32) + 7
    want_ids = _ref(res, slot, n_slots, psm_id=ids)
    for order in ((0, 1), (1, 0)):
        plans = [_plan(gpu, halves[h][0], dev) for h in order]
        table = plans[0].rollup_clear(n_slots)
        table_ids = plans[0].rollup_clear(n_slots)
        for plan, h in zip(plans, order):
            _, sp, pp = plan.probs()
            d_slot = torch.from_numpy(halves[h][1]).to(dev)
            plan.rollup(sp, pp, d_slot, table, psm_base=halves[h][2])
            lo = halves[h][2]
            d_ids = torch.from_numpy(ids[lo:lo + plan.n_psm].astype(np.int64)).to(dev).to(torch.int32)
            plan.rollup(sp, pp, d_slot, table_ids, psm_id=d_ids)               # the same plan again, another table
            plan.check()
        _same_bytes(rollup_records(table.cpu().numpy()), whole, "two plans, order %s" % (order,))
        _same_bytes(rollup_records(table_ids.cpu().numpy()), want_ids, "two plans with psm_id, order %s" % (order,))
        a = plans[0].rollup_clear(n_slots)
        b = plans[0].rollup_clear(n_slots)
        for plan, h, t in zip(plans, order, (a, b)):                           # a table per half, merged on the host
            _, sp, pp = plan.probs()
            plan.rollup(sp, pp, torch.from_numpy(halves[h][1]).to(dev), t, psm_base=halves[h][2])
        _same_bytes(ru.merge(rollup_records(a.cpu().numpy()), rollup_records(b.cpu().numpy())), whole, "merged on the host")
        again = plans[0].rollup_clear(table=table)                             # emptied again
        assert rollup_records(again.cpu().numpy()).tobytes() == ru.empty(n_slots).tobytes()


def test_guards():
    import torch
    from pyascore_amd.device import rollup_records
    batch, settings = synth.make_batch("cfg2", n_psm=200, seed=9990)
    batch, peptides = _repeats(batch)
    gpu = _gpu(settings)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    out = np.zeros(4, ru.ROLLUP_DTYPE)
    assert gpu._lib.pya_last_batch_rollup(None, vp(out), 4) == _lib.PYA_ERR_ARG
    assert gpu._lib.pya_last_batch_rollup(gpu._h, vp(out), 4) == _lib.PYA_ERR_STATE      # no batch with the flag yet
    assert b"PYA_FLAG_ROLLUP" in gpu._lib.pya_last_error(gpu._h)
    res = gpu.score_batch(batch, probs=True)
    assert gpu._lib.pya_last_batch_rollup(gpu._h, vp(out), 4) == _lib.PYA_ERR_STATE
    slot, n_slots, _ = ru.peptide_slots(peptides, res["site_off"], residues=settings["mod_group"])
    want = _ref(res, slot, n_slots)
    for bad in (slot[:-1], np.concatenate([slot, [0]]).astype(np.int32), slot[:5]):             # wrong n_records
        with pytest.raises(ValueError, match="pya_set_rollup"):
            gpu.score_batch(batch, rollup=dict(slot=bad, n_slots=n_slots))
        assert gpu._lib.pya_last_batch_rollup(gpu._h, vp(out), 4) == _lib.PYA_ERR_STATE
    got = gpu.score_batch(batch, rollup=dict(slot=slot, n_slots=n_slots))["rollup"]
    _same_bytes(got, want, "after the refused calls")
    back = np.zeros(n_slots, ru.ROLLUP_DTYPE)
    assert gpu._lib.pya_last_batch_rollup(gpu._h, vp(back), n_slots) == 0 and back.tobytes() == got.tobytes()
    assert gpu._lib.pya_last_batch_rollup(gpu._h, vp(back), n_slots - 1) == _lib.PYA_ERR_ARG
    assert gpu._lib.pya_last_batch_rollup(gpu._h, None, n_slots) == _lib.PYA_ERR_ARG
    # the flag without a loan (the loan of the call above ended with it)
    r = gpu.score_batch(batch)
    arrs = [np.ascontiguousarray(batch[k], t) for k, t in (("peak_off", np.int64), ("pep", np.uint8), ("pep_off", np.int64), ("n_of_mod", np.int32),
                                                           ("max_charge", np.int32), ("aux_pos", np.uint32), ("aux_mass", np.float32),
                                                           ("aux_off", np.int64))]
    b = _lib.Batch(200, *[vp(a) for a in arrs])
    outs = [np.zeros_like(r[k]) for k in KEYS]
    rs = _lib.Results(r["ascores"].shape[1], *[vp(a) for a in outs])
    mz, it = np.ascontiguousarray(batch["mz"], np.float64), np.ascontiguousarray(batch["intensity"], np.float64)
    assert gpu._lib.pya_score_batch(gpu._h, C.byref(b), vp(mz), vp(it), _lib.PYA_FLAG_ROLLUP, C.byref(rs)) == _lib.PYA_ERR_ARG
    assert b"pya_set_rollup" in gpu._lib.pya_last_error(gpu._h)
    assert gpu._lib.pya_set_rollup(gpu._h, None, 5, 4, 0.75, None) == _lib.PYA_ERR_ARG
    assert gpu._lib.pya_set_rollup(gpu._h, vp(slot), slot.size, 1 << 31, 0.75, None) == _lib.PYA_ERR_ARG
    # a slot at or above n_slots: PYA_ERR_LIMIT, and nothing of it is written
    with pytest.raises(ValueError, match="n_slots"):
        gpu.score_batch(batch, rollup=dict(slot=slot, n_slots=n_slots - 3))
    dev = torch.device("cuda", 0)
    plan = _plan(gpu, batch, dev)
    _, sp, pp = plan.probs()
    small = n_slots - 3
    table = torch.full((n_slots + 5, 32), 0x5A, dtype=torch.uint8, device=dev)     # guard words behind the table
    assert gpu._lib.pya_rollup_clear(gpu._h, table.data_ptr(), small, None) == 0
    d_slot = torch.from_numpy(slot).to(dev)
    assert gpu._lib.pya_plan_rollup(plan._plan, C.byref(plan._res), None, sp.data_ptr(), pp.data_ptr(), d_slot.data_ptr(), small, THR, None, 0,
                                    table.data_ptr()) == 0
    with pytest.raises(ValueError, match="n_slots"):
        plan.check()
    assert gpu._lib.pya_plan_check(plan._plan) == _lib.PYA_ERR_LIMIT
    host = table.cpu().numpy()
    assert (host[small:] == 0x5A).all()
    _same_bytes(rollup_records(host[:small]), _ref(res, slot, small), "the slots inside the table")
    _same_bytes(rollup_records(host[:small]), want[:small], "... are what they are in the full table")
    full = plan.rollup_clear(n_slots)
    plan.rollup(sp, pp, d_slot, full)                                          # the call repeated with room: the report is gone
    plan.check()
    _same_bytes(rollup_records(full.cpu().numpy()), want, "plan")
    assert gpu._lib.pya_plan_rollup(plan._plan, C.byref(plan._res), None, sp.data_ptr(), None, d_slot.data_ptr(), n_slots, THR, None, 0,
                                    full.data_ptr()) == _lib.PYA_ERR_ARG
    assert gpu._lib.pya_plan_rollup(None, None, None, None, None, None, 0, THR, None, 0, None) == _lib.PYA_ERR_ARG
    with pytest.raises(ValueError):
        plan.rollup(sp, pp, d_slot[:-1], full)
    fresh = DevicePlanNotRun(gpu, batch)
    assert gpu._lib.pya_plan_rollup(fresh._plan, C.byref(fresh._res), None, sp.data_ptr(), pp.data_ptr(), d_slot.data_ptr(), n_slots, THR, None, 0,
                                    full.data_ptr()) == _lib.PYA_ERR_STATE
    # pya_score_one refuses the flag
    kw = synth.unpack_psm(batch, 0)
    m, i = np.ascontiguousarray(kw["mz_arr"], np.float64), np.ascontiguousarray(kw["int_arr"], np.float64)
    pep = np.frombuffer(kw["peptide"].encode(), np.uint8)
    one = (np.zeros(1, np.float32), np.zeros(1, np.uint64), np.zeros(1, np.int32), np.zeros((1, 4), np.float32), np.zeros((1, 4), np.uint64))
    r1 = _lib.Results(4, *[vp(x) for x in one])
    rc = gpu._lib.pya_score_one(gpu._h, vp(m), vp(i), m.size, vp(pep), pep.size, int(kw["n_of_mod"]), int(kw["max_fragment_charge"]), None, None, 0,
                                _lib.PYA_FLAG_ROLLUP, C.byref(r1))
    assert rc == _lib.PYA_ERR_ARG and b"PYA_FLAG_ROLLUP" in gpu._lib.pya_last_error(gpu._h)


def DevicePlanNotRun(gpu, batch):
    from pyascore_amd.device import DevicePlan
    return DevicePlan(gpu, batch, rollup=True)


def test_the_report_is_the_last_call_s_on_whatever_stream():
    """one plan asked on two streams in turn, with nothing between them that orders the streams: the second call waits for the
    first call's report event before it clears the two words, so check() sees the words of the LAST call -- nothing to report
    after (outside, inside), the roll-up's error after (inside, outside) -- and the tables are what the calls give alone"""
    import torch
    from pyascore_amd.device import rollup_records
    batch, settings = synth.make_batch("cfg2", n_psm=200, seed=9990)
    batch, peptides = _repeats(batch)
    gpu = _gpu(settings)
    res = gpu.score_batch(batch, probs=True)
    slot, n_slots, _ = ru.peptide_slots(peptides, res["site_off"], residues=settings["mod_group"])
    want = _ref(res, slot, n_slots)
    dev = torch.device("cuda", 0)
    plan = _plan(gpu, batch, dev)
    _, sp, pp = plan.probs()
    d_slot = torch.from_numpy(slot).to(dev)
    outside = torch.full_like(d_slot, n_slots)
    streams = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    for calls, fails in (((outside, d_slot), False), ((d_slot, outside), True)):
        tables = plan.rollup_clear(n_slots), plan.rollup_clear(n_slots)
        torch.cuda.synchronize()                                               # (the inputs are there; from here on only the library orders)
        for st, d, table in zip(streams, calls, tables):
            with torch.cuda.stream(st):
                plan.rollup(sp, pp, d, table)
        if fails:
            with pytest.raises(ValueError, match="pya_plan_rollup"):
                plan.check()
        else:
            plan.check()
        torch.cuda.synchronize()
        for d, table in zip(calls, tables):
            _same_bytes(rollup_records(table.cpu().numpy()), ru.empty(n_slots) if d is outside else want, "outside" if d is outside else "inside")


def test_a_handful_and_a_batch_of_one():
    batch, settings = synth.make_batch("cfg2", n_psm=300, seed=9995)
    batch, peptides = _repeats(batch)
    gpu = _gpu(settings)
    res = gpu.score_batch(batch, probs=True)
    slot, n_slots, _ = ru.peptide_slots(peptides, res["site_off"], residues=settings["mod_group"])
    for lo, hi in ((0, 1), (7, 8), (10, 15)):
        r0, r1 = int(res["site_off"][lo]), int(res["site_off"][hi])
        part = gpu.score_batch(synth.slice_batch(batch, lo, hi), probs=True, rollup=dict(slot=slot[r0:r1], n_slots=n_slots))
        _same_bytes(part["rollup"], _ref(part, slot[r0:r1], n_slots), "PSMs %d..%d" % (lo, hi))
        assert part["rollup"]["n_psm"].sum() == r1 - r0
    empty = gpu.score_batch(synth.slice_batch(batch, 0, 0), rollup=dict(slot=np.zeros(0, np.int32), n_slots=3))
    assert empty["rollup"].tobytes() == ru.empty(3).tobytes()


def test_all_stage_flags_together():
    batch, settings = synth.make_batch("cfg3", n_psm=400, seed=9996)
    batch, peptides = _repeats(batch)
    gpu = _gpu(settings)
    q = [[int(b)] for b in gpu.score_batch(batch)["best_sig"]]
    plain = gpu.score_batch(batch, evidence=True, ions=True, named=q, sites=True, probs=True, ranked=5)
    slot, n_slots, _ = ru.peptide_slots(peptides, plain["site_off"], residues=settings["mod_group"])
    got = gpu.score_batch(batch, evidence=True, ions=True, named=q, sites=True, probs=True, ranked=5, rollup=dict(slot=slot, n_slots=n_slots))
    for key in KEYS + ("evidence", "ion_off", "ions", "named", "site_off", "sites", "site_probs", "psm_probs", "ranked"):
        assert got[key].tobytes() == plain[key].tobytes(), key
    _same_bytes(got["rollup"], _ref(plain, slot, n_slots), "beside the other stages")


def test_command_line_file(tmp_path):
    from test_batch_cli import _toy_inputs
    from pyascore_amd import PyAscore, batch_cli
    spectra, psms = _toy_inputs()
    gpu = PyAscore(100.0, 10, "STY", 79.966331, 0.05, "by")
    plain = batch_cli.localize(gpu, psms, spectra, "STY", 79.966331, hit_depth=2, max_fragment_charge=3, probs=True)
    rows = []
    wide = batch_cli.localize(gpu, psms, spectra, "STY", 79.966331, hit_depth=2, max_fragment_charge=3, probs=True, site_table=rows,
                              site_table_threshold=0.5)
    assert [[str(f) for f in r] for r in wide] == [[str(f) for f in r] for r in plain]      # the main table is unchanged
    assert rows and all(len(r) == len(batch_cli.SITE_TABLE_COLUMNS) for r in rows)
    assert len({(r[0], r[1]) for r in rows}) == len(rows)
    scans = {r[0] for r in plain}
    for r in rows:
        assert r[2] in "STY" and r[0][int(r[1]) - 1] == r[2] and r[4] in scans
        assert 0.0 <= float(r[3]) <= 1.0 and int(r[5]) >= int(r[6]) and int(r[5]) >= int(r[7]) >= 0
        assert (r[8] == "") == (int(r[7]) == 0)
    assert sum(int(r[7]) for r in rows) > 0
    path = str(tmp_path / "site_table.tsv")
    batch_cli.write_site_table_tsv(rows, path)
    lines = open(path).read().splitlines()
    assert lines[0].split("\t") == list(batch_cli.SITE_TABLE_COLUMNS) and len(lines) == 1 + len(rows)


def test_crafted_records_on_the_device():
    """pya_plan_rollup takes the caller's probability records and results: negative, -0, +0, +-inf Ascores on one slot, a slot
    that only ever sees negative ones, slot -1, with_prob exactly at the threshold, and two calls per table so that a slot's
    first Ascore arrives in the first call, in the second, or in both"""
    import torch
    from pyascore_amd.device import rollup_records
    batch, settings = synth.make_batch("cfg2", n_psm=64, seed=9998)
    gpu = _gpu(settings)
    dev = torch.device("cuda", 0)
    plan = _plan(gpu, batch, dev)
    off = plan.site_offsets()
    n, n_rec, k = 64, int(off[-1]), max(8, plan.max_k)
    ns = np.diff(off)
    assert ns.min() >= 1
    rng = np.random.default_rng(42)
    owner = np.repeat(np.arange(n), ns)
    sp = np.zeros(n_rec, np.dtype(_lib.SITE_PROB_DTYPE))
    sp["with_prob"] = rng.choice([0.0, 0.25, THR, 1.0], n_rec)
    sp["without_prob"] = 1.0 - sp["with_prob"]
    pp = np.zeros(n, np.dtype(_lib.PSM_PROB_DTYPE))
    pp["kind"] = pb.SCORED
    pp["kind"][[5, 40]] = [pb.OVER, pb.NONE]
    sig = np.array([int(rng.integers(1, 1 << min(int(s), 8))) for s in ns], np.uint64)
    asc = rng.choice(np.array([-3.0, -0.0, 0.0, 2.5, np.inf, -np.inf, -1e-30], np.float32), (n, k))
    asc[:16] = rng.choice(np.array([-3.0, -7.5, -np.inf, -1e-30], np.float32), (16, k))       # PSMs 0..15: negative only
    slot = np.where(owner < 16, 3, rng.integers(0, 3, n_rec)).astype(np.int32)                 # ... alone on slot 3
    slot[rng.random(n_rec) < 0.1] = -1
    ids = rng.permutation(n).astype(np.uint32) + 100
    res = dict(site_probs=sp, psm_probs=pp, site_off=off, best_sig=sig, ascores=asc)
    want = _ref(res, slot, 5, psm_id=ids)
    assert want["best_ascore"][3] < 0 and want["n_in_best"][3] > 3 and (want["n_in_best"][:3] > 3).all()
    assert want[4].tobytes() == ru.empty(1)[0].tobytes() and (want["n_confident"][:4] > 0).all()
    assert ((sp["with_prob"] == THR) & (slot >= 0) & (pp["kind"][owner] == pb.SCORED)).any() and (slot < 0).any()
    d_sp = torch.from_numpy(sp.view(np.float64).reshape(n_rec, 2).copy()).to(dev)
    d_pp = torch.from_numpy(pp.view(np.uint8).reshape(n, 16).copy()).to(dev)
    d_sig = torch.from_numpy(sig.view(np.int64).copy()).to(dev)
    d_asc = torch.from_numpy(asc.copy()).to(dev)
    d_ids = torch.from_numpy(ids.astype(np.int64)).to(dev).to(torch.int32)
    r = _lib.Results(k, plan.best_score.data_ptr(), d_sig.data_ptr(), plan.n_sig.data_ptr(), d_asc.data_ptr(), plan.alt_mask.data_ptr())

    def roll(table, s):
        d_slot = torch.from_numpy(np.ascontiguousarray(s, np.int32)).to(dev)
        assert gpu._lib.pya_plan_rollup(plan._plan, C.byref(r), None, d_sp.data_ptr(), d_pp.data_ptr(), d_slot.data_ptr(), 5, THR,
                                        d_ids.data_ptr(), 0, table.data_ptr()) == 0
        torch.cuda.synchronize()
        assert gpu._lib.pya_plan_check(plan._plan) == 0

    one = plan.rollup_clear(5)
    roll(one, slot)
    _same_bytes(rollup_records(one.cpu().numpy()), want, "one call")
    for trial in range(6):
        first = rng.random(n_rec) < (0.5, 0.1, 0.9)[trial % 3]
        parts = (np.where(first, slot, -1), np.where(first, -1, slot))
        table = plan.rollup_clear(5)
        for s in parts[::-1] if trial & 1 else parts:
            roll(table, s)
        _same_bytes(rollup_records(table.cpu().numpy()), want, "two calls, split %d" % trial)
    table = plan.rollup_clear(5)
    for s in range(4):                                                         # slot by slot: a call per slot
        roll(table, np.where(slot == s, slot, -1))
    _same_bytes(rollup_records(table.cpu().numpy()), want, "a call per slot")
