"""One scorer's life (tests/lifecases.py): live plans while the handle's device tables grow and move, settings changed under
a live plan, and long sequences of calls on ONE handle.  Bytes only: a plan's results and the records of its seven stages
before and after the tables moved; every step of a sequence against the same call on a fresh scorer; the five result arrays
of every pool entry against the reference checker once, so that "fresh" stands on the reference.

The settings tests are refusals only: after ``add_neutral_loss`` nothing is launched over a plan made before it (a plan's
routes, caps and LDS carves belong to the settings it was made under; include/pyascore_hip.h at pya_plan_create)."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import lifecases as lc
import named_ref
from conftest import checker_kind
from oracle import harness, orc
from pyascore_amd import PyAscore, _lib, synth
from pyascore_amd.device import DevicePlan

pytestmark = pytest.mark.gpu

KEYS = ("best_score", "best_sig", "n_sig", "ascores", "alt_mask")
STAGES = ("evidence", "ions", "named", "sites", "probs", "ranked", "coverage")
ALL_STAGES = dict(evidence=True, ions=True, named=True, sites=True, probs=True, ranked=True, coverage=True)
STALE = "settings changed since the plan was made"
DEV = torch.device("cuda", 0)


def _gpu(settings=lc.SETTINGS):
    return harness.make_scorer(PyAscore, settings)


def _tables(gpu):
    out = (C.c_uint64 * 4)()
    assert gpu._lib.pya_debug_table_sizes(gpu._h, out) == _lib.PYA_OK
    return dict(order=int(out[0]), rows=int(out[1]), cfg=int(out[2]), lut_ptr=int(out[3]))


def _upload(batch, dtype=None):
    mz, it = batch["mz"], batch["intensity"]
    if dtype is not None:
        mz, it = mz.astype(dtype), it.astype(dtype)
    return torch.from_numpy(np.ascontiguousarray(mz)).to(DEV), torch.from_numpy(np.ascontiguousarray(it)).to(DEV)


def _results(plan):
    """the plan's five result tensors on the host (waits for the device)"""
    torch.cuda.synchronize()
    return dict(best_score=plan.best_score.cpu().numpy(), best_sig=plan.best_sig.cpu().numpy().view(np.uint64),
                n_sig=plan.n_sig.cpu().numpy(), ascores=plan.ascores.cpu().numpy(), alt_mask=plan.alt_mask.cpu().numpy().view(np.uint64))


def _fill(plan, byte=0xA5):
    """every byte of the plan's result tensors set to a sentinel"""
    for t in (plan.best_score, plan.best_sig, plan.n_sig, plan.ascores, plan.alt_mask):
        t.view(torch.uint8).fill_(byte)


def _untouched(plan, byte=0xA5):
    torch.cuda.synchronize()
    return all(bool((t.view(torch.uint8) == byte).all()) for t in (plan.best_score, plan.best_sig, plan.n_sig, plan.ascores, plan.alt_mask))


def _want(names, with_loss=False):
    """the checker's answers for the PSMs of the entries, one after the other, rows padded to the widest"""
    parts = [lc.answer(n, checker_kind(), with_loss) for n in names]
    k = max(p["ascores"].shape[1] for p in parts)
    pad = lambda a: np.concatenate([a, np.zeros((a.shape[0], k - a.shape[1]), a.dtype)], axis=1)      # noqa: E731
    return {key: np.concatenate([pad(p[key]) if p[key].ndim == 2 else p[key] for p in parts]) for key in KEYS}


def _is_the_checkers(got, want, n_of_mod, what):
    """the columns of a PSM's modifications (the reference has no others; a plan's tensors are not cleared beyond them)"""
    for key in KEYS:
        g, w = np.asarray(got[key]), np.asarray(want[key])
        if g.ndim == 2:
            live = np.arange(g.shape[1])[None, :] < np.asarray(n_of_mod)[:, None]
            g, w = np.where(live, g, 0), np.where(live[:, :w.shape[1]], w, 0)
            g = g[:, :w.shape[1]]
        bad = np.flatnonzero((g != w).reshape(g.shape[0], -1).any(axis=1))
        assert bad.size == 0, "%s: %s differs from the checker for PSMs %s" % (what, key, bad[:10].tolist())


def _same_bytes(got, want, what):
    assert set(got) == set(want), (what, sorted(set(got) ^ set(want)))
    for key in want:
        g, w = got[key], want[key]
        if isinstance(w, np.ndarray):
            assert isinstance(g, np.ndarray) and g.dtype == w.dtype and g.shape == w.shape, (what, key, getattr(g, "shape", None), w.shape)
            if g.tobytes() != w.tobytes():
                rows = np.flatnonzero((g.reshape(g.shape[0], -1).view(np.uint8) != w.reshape(w.shape[0], -1).view(np.uint8)).any(axis=1)) \
                    if g.ndim and g.shape[0] else []
                raise AssertionError("%s: %s differs in rows %s" % (what, key, list(rows[:10])))
        else:
            assert g == w, (what, key, g, w)


def _queries(batch, best_sig):
    """the single moves of every PSM's reported localisation as device tensors (q_off, sig_bits)"""
    per_psm = [[m[2] for m in named_ref.single_moves(int(b), ns)] for b, (ns, _) in zip(best_sig, lc.shapes(batch))]
    q_off = np.concatenate([[0], np.cumsum([len(q) for q in per_psm])]).astype(np.int64)
    bits = np.array([b for q in per_psm for b in q], np.uint64).view(np.int64)
    return torch.from_numpy(q_off).to(DEV), torch.from_numpy(bits).to(DEV)


def _stages(plan, mz, it, queries, ion_cap=None):
    """the seven stages behind the plan's last run, each once, on torch's current stream: name -> list of device tensors.
    ``ion_cap``: the number of ion records, where it is known (``ions()`` then waits for nothing on the host)"""
    out = dict(evidence=[plan.evidence()], ions=list(plan.ions(cap=ion_cap)), named=list(plan.named(queries[0], queries[1], counts=True, scores=True)))
    out["sites"] = [plan.sites()[1]]
    out["probs"] = list(plan.probs()[1:])
    out["ranked"] = [plan.ranked(5)]
    out["coverage"] = [plan.coverage(mz, it)]
    return out


def _host(stages):
    torch.cuda.synchronize()
    return {"%s.%d" % (name, i): t.cpu().numpy() for name, ts in stages.items() for i, t in enumerate(ts)}


def _plan_a(gpu, **flags):
    """plan A over a_small, run once and checked against the checker: (plan, mz, it, first results)"""
    a = lc.entry("a_small")
    mz, it = _upload(a)
    plan = DevicePlan(gpu, a, **flags)
    plan.run(mz, it)
    plan.check()
    first = _results(plan)
    _is_the_checkers(first, _want(["a_small"]), a["n_of_mod"], "plan A")
    return plan, mz, it, first


def _grow(gpu, before, what):
    """plan B over b_shapes + b_lut on the same scorer: BOTH handle tables must grow, and the score table must move"""
    b = lc.concat("b_shapes", "b_lut")
    plan = DevicePlan(gpu, b)
    after, exp = _tables(gpu), lc.expected_growth("a_small", ["b_shapes", "b_lut"])
    assert exp["lut"] and exp["order"]
    assert (before["rows"], after["rows"]) == exp["lut_rows"] == (129, 601), (what, before, after)
    assert (before["order"], after["order"]) == exp["order_entries"], (what, before, after)
    assert after["lut_ptr"] != before["lut_ptr"] and before["lut_ptr"] and after["lut_ptr"], (what, before, after)
    assert after["cfg"] == before["cfg"] == 1
    print("%s: score table %d -> %d rows at %#x -> %#x, order table %d -> %d entries" %
          (what, before["rows"], after["rows"], before["lut_ptr"], after["lut_ptr"], before["order"], after["order"]))
    return plan, b, _upload(b)


# ---- growth under live plans ---------------------------------------------------------------------------------------------------
def test_a_plan_outlives_the_growth_of_both_tables():
    gpu = _gpu()
    a = lc.entry("a_small")
    plan_a, mz, it, first = _plan_a(gpu, **ALL_STAGES)
    queries = _queries(a, first["best_sig"])
    stages = _host(_stages(plan_a, mz, it, queries))
    plan_a.check()
    plan_b, b, (bmz, bit) = _grow(gpu, _tables(gpu), "growth under plan A")
    plan_b.run(bmz, bit)
    plan_b.check()
    _is_the_checkers(_results(plan_b), _want(["b_shapes", "b_lut"]), b["n_of_mod"], "plan B")
    _fill(plan_a)
    plan_a.run(mz, it)
    plan_a.check()
    _same_bytes(_results(plan_a), first, "plan A after the growth")
    _same_bytes(_host(_stages(plan_a, mz, it, queries)), stages, "plan A's stages after the growth")
    plan_a.check()


def test_growth_while_a_run_is_in_flight():
    """plan A's runs and stages are ENQUEUED on a side stream and nobody has waited for them when plan B makes the tables move"""
    gpu = _gpu()
    a = lc.entry("a_small")
    plan_a, mz, it, first = _plan_a(gpu, **ALL_STAGES)
    queries = _queries(a, first["best_sig"])
    stages = _host(_stages(plan_a, mz, it, queries))
    before = _tables(gpu)
    _fill(plan_a)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        for _ in range(8):
            plan_a.run(mz, it)
        in_flight = _stages(plan_a, mz, it, queries, ion_cap=stages["ions.1"].shape[0])
    plan_b, b, (bmz, bit) = _grow(gpu, before, "growth under an enqueued run")          # (no synchronise in between)
    plan_b.run(bmz, bit)
    torch.cuda.synchronize()
    plan_a.check()
    plan_b.check()
    _same_bytes(_results(plan_a), first, "plan A, enqueued before the growth")
    _same_bytes(_host(in_flight), stages, "plan A's stages, enqueued before the growth")
    _is_the_checkers(_results(plan_b), _want(["b_shapes", "b_lut"]), b["n_of_mod"], "plan B")


def test_two_plans_on_two_streams_then_one_then_none():
    gpu = _gpu()
    plan_a, mz, it, first = _plan_a(gpu)
    plan_b, b, (bmz, bit) = _grow(gpu, _tables(gpu), "growth before the alternating runs")
    streams = [torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)]
    for s in streams:
        s.wait_stream(torch.cuda.current_stream(DEV))
    _fill(plan_a)
    for _ in range(6):
        for plan, st, sp in ((plan_a, streams[0], (mz, it)), (plan_b, streams[1], (bmz, bit))):
            with torch.cuda.stream(st):
                plan.run(*sp)
    torch.cuda.synchronize()
    plan_a.check()
    plan_b.check()
    _same_bytes(_results(plan_a), first, "plan A beside plan B")
    _is_the_checkers(_results(plan_b), _want(["b_shapes", "b_lut"]), b["n_of_mod"], "plan B beside plan A")
    plan_b.close()
    _fill(plan_a)
    plan_a.run(mz, it)
    plan_a.check()
    _same_bytes(_results(plan_a), first, "plan A after plan B was destroyed")
    plan_a.close()
    got = gpu.score_batch(lc.entry("a_small"))
    _same_bytes({k: got[k] for k in KEYS}, first, "score_batch after both plans were destroyed")


def test_a_plan_outlives_the_growth_by_the_one_psm_path():
    """``score()`` extends the score table and uploads the order tables as well (host_one.cpp)"""
    gpu = _gpu()
    plan_a, mz, it, first = _plan_a(gpu)
    before = _tables(gpu)
    kw = synth.unpack_psm(lc.entry("b_lut"), 4)                                 # the 51-mer at charge 6: 600 trials
    gpu.score(**kw)
    records = gpu.pep_scores
    after, exp = _tables(gpu), lc.expected_growth("a_small", "b_lut")
    assert (before["rows"], after["rows"]) == exp["lut_rows"] and after["lut_ptr"] != before["lut_ptr"] and after["order"] > before["order"]
    print("growth by score(): score table %d -> %d rows, order table %d -> %d entries" % (before["rows"], after["rows"], before["order"], after["order"]))
    chk = harness.make_scorer(orc.OracleAscore, lc.SETTINGS, kind=checker_kind())
    chk.score(**kw)
    assert gpu.best_sequence == chk.best_sequence and np.array_equal(gpu.ascores, chk.ascores)
    assert [r["weighted_score"] for r in records] == [r["weighted_score"] for r in chk.pep_scores]
    _fill(plan_a)
    plan_a.run(mz, it)
    plan_a.check()
    _same_bytes(_results(plan_a), first, "plan A after score() of a b_lut PSM")


def test_a_shared_and_a_plain_plan_typed_after_the_growth():
    gpu = _gpu()
    shared = lc.entry("shared")
    plain = synth.expand_shared_batch(shared)
    p_shared, p_plain = DevicePlan(gpu, shared), DevicePlan(gpu, plain)
    want64 = _want(["shared"])
    for plan, batch, what in ((p_shared, shared, "shared"), (p_plain, plain, "plain")):
        plan.run(*_upload(batch))
        plan.check()
        _is_the_checkers(_results(plan), want64, shared["n_of_mod"], what + " plan, float64")
    _grow(gpu, _tables(gpu), "growth before the typed runs")
    narrow = synth.widen_batch(synth.narrow_batch(plain))                      # the float32 values, as the checker takes them
    want32 = harness.make_scorer(orc.OracleAscore, lc.SETTINGS, kind=checker_kind()).score_batch(narrow, want64["ascores"].shape[1])
    got = {}
    for plan, batch, what in ((p_shared, shared, "shared"), (p_plain, plain, "plain")):
        _fill(plan)
        plan.run(*_upload(batch, np.float32))
        plan.check()
        got[what] = _results(plan)
        _is_the_checkers(got[what], want32, shared["n_of_mod"], what + " plan, float32 after the growth")
    _same_bytes(got["shared"], got["plain"], "shared against plain")


# ---- settings changes: refusals only ---------------------------------------------------------------------------------------------
def _refused(call, *args, **kw):
    with pytest.raises(RuntimeError, match=STALE):
        call(*args, **kw)


def test_a_settings_change_ends_the_launching_life_of_a_plan():
    gpu = _gpu()
    a = lc.entry("a_small")
    plan, mz, it, first = _plan_a(gpu, **ALL_STAGES)
    queries = _queries(a, first["best_sig"])
    stages = _host(_stages(plan, mz, it, queries))
    kept = gpu.score_batch(a, keep=True)
    records = gpu.batch_pep_scores()
    gpu.add_neutral_loss(*lc.LOSS)
    before = _tables(gpu)
    _fill(plan)
    _refused(plan.run, mz, it)
    assert _untouched(plan), "a refused run wrote results"
    mz32, it32 = _upload(a, np.float32)
    _refused(plan.run, mz32, it32)                                              # (pya_plan_run_typed)
    canary = torch.full((1 << 16,), 0x5A, dtype=torch.uint8, device=DEV)
    _refused(plan.evidence, out=canary[:64 * 3 * 16].view(64, 3, 16))
    _refused(plan.ions)
    _refused(plan.named, queries[0], queries[1])
    _refused(plan.sites)
    _refused(plan.probs)
    _refused(plan.ranked, 5)
    _refused(plan.coverage, mz, it, out=canary[:64 * 64].view(64, 64))
    lib, res = gpu._lib, C.byref(plan._res)
    off = torch.zeros(65, dtype=torch.int64, device=DEV)
    assert lib.pya_plan_ions(plan._plan, res, None, off.data_ptr(), canary.data_ptr(), 1 << 12) == _lib.PYA_ERR_STATE
    assert STALE.encode() in lib.pya_last_error(gpu._h)
    # the stages this suite drives through other files refuse the same way, before they look at their arguments
    for name, args in (("pya_plan_rollup", (None, None, None, 0, 0.75, None, 0, None)),
                       ("pya_plan_peptidoforms", (None, None, None, 0.75, None, 0, None, 0, None, 0, None, 0, None)),
                       ("pya_plan_mz_profile", (None, 0, None, None))):
        assert getattr(lib, name)(plan._plan, res, None, *args) == _lib.PYA_ERR_STATE, name
        assert STALE.encode() in lib.pya_last_error(gpu._h), name
    # the retained batch is a plan too
    ps = np.ascontiguousarray(records["scores"][:2]), records["weighted_score"][:2], records["sig_bits"][:2]
    out = C.c_float(-1.0)
    rc = lib.pya_calculate_ambiguity(gpu._h, 0, int(ps[2][0]), ps[0][0].ctypes.data, float(ps[1][0]), int(ps[2][1]), ps[0][1].ctypes.data,
                                     float(ps[1][1]), C.byref(out))
    assert rc == _lib.PYA_ERR_STATE and STALE.encode() in lib.pya_last_error(gpu._h) and out.value == -1.0
    torch.cuda.synchronize()
    assert _untouched(plan) and bool((canary == 0x5A).all()), "a refused call wrote something"
    assert _tables(gpu) == before, "a refused call uploaded a table"
    # what only reads back stays valid: the status of the old run, the offsets, the sizes
    plan.check()
    assert plan.site_offsets()[-1] == 64 * 6 and plan.workspace_bytes > 0
    assert {k: kept[k].tobytes() for k in KEYS} == {k: first[k].tobytes() for k in KEYS}
    assert sorted(stages) == sorted("%s.%d" % (s, i) for s, n in zip(STAGES, (1, 2, 3, 1, 2, 1, 1)) for i in range(n))


def test_score_refuses_ambiguity_of_a_psm_scored_under_the_old_settings():
    gpu = _gpu()
    gpu.score(**synth.unpack_psm(lc.entry("a_small"), 5))
    ps = gpu.pep_scores
    assert gpu.calculate_ambiguity(ps[0], ps[0]) == 0.0
    gpu.add_neutral_loss(*lc.LOSS)
    _refused(gpu.calculate_ambiguity, ps[0], ps[1])
    assert [r["weighted_score"] for r in gpu.pep_scores] == [r["weighted_score"] for r in ps]       # the records stay readable
    gpu.score(**synth.unpack_psm(lc.entry("a_small"), 5))                      # scored again: under the new settings
    ps2 = gpu.pep_scores
    assert gpu.calculate_ambiguity(ps2[0], ps2[0]) == 0.0 and ps2[0]["total_fragments"] != ps[0]["total_fragments"]


def test_after_the_change_new_plans_and_batch_calls_score_under_the_new_settings():
    gpu = _gpu()
    a = lc.entry("a_small")
    old_plan, mz, it, old = _plan_a(gpu)
    gpu.add_neutral_loss(*lc.LOSS)
    want = _want(["a_small"], with_loss=True)
    got = gpu.score_batch(a)                                                  # score_batch makes its own plan per call
    assert _tables(gpu)["cfg"] == 2
    _is_the_checkers(got, want, a["n_of_mod"], "score_batch after the change")
    new_plan = DevicePlan(gpu, a)
    new_plan.run(mz, it)
    new_plan.check()
    new = _results(new_plan)
    _is_the_checkers(new, want, a["n_of_mod"], "a new plan after the change")
    assert (new["best_score"] != old["best_score"]).any(), "the loss does not matter on this batch"
    _refused(old_plan.run, mz, it)                                             # (a new plan does not revive the old one)


def test_retained_records_read_after_the_change_are_those_of_the_old_settings():
    gpu = _gpu()
    a = lc.entry("a_small")
    gpu.score_batch(a, keep=True)
    gpu.add_neutral_loss(*lc.LOSS)
    got = gpu.batch_pep_scores()
    chk = harness.make_scorer(orc.OracleAscore, lc.SETTINGS, kind=checker_kind())          # WITHOUT the loss
    for i in range(0, 64, 7):
        chk.score(**synth.unpack_psm(a, i))
        raw = chk.raw_pep_scores()
        lo, hi = got["rec_off"][i:i + 2]
        bits = (raw["signature"].astype(np.uint64) << np.arange(raw["signature"].shape[1], dtype=np.uint64)).sum(axis=1)
        assert np.array_equal(got["sig_bits"][lo:hi], bits), i
        for key in ("counts", "scores", "weighted_score"):
            assert got[key][lo:hi].tobytes() == raw[key].tobytes(), (i, key)
        assert np.array_equal(got["total_fragments"][lo:hi], raw["total_fragments"]), i


def test_an_identical_second_change_ends_a_plans_life_too():
    """the setter does not compare: EVERY call bumps the generation"""
    gpu = _gpu()
    a = lc.entry("a_small")
    gpu.add_neutral_loss(*lc.LOSS)
    mz, it = _upload(a)
    plan = DevicePlan(gpu, a)
    plan.run(mz, it)
    plan.check()
    _is_the_checkers(_results(plan), _want(["a_small"], with_loss=True), a["n_of_mod"], "a plan under the loss")
    gpu.add_neutral_loss(*lc.LOSS)
    _fill(plan)
    _refused(plan.run, mz, it)
    assert _untouched(plan)
    _is_the_checkers(gpu.score_batch(a), _want(["a_small"], with_loss=True), a["n_of_mod"], "score_batch after the second call")


# ---- one scorer, many calls --------------------------------------------------------------------------------------------------------
def _do(gpu, step):
    """one step of a sequence: everything the caller gets back, as a dict of arrays and plain values"""
    if step[0] == "score":
        _, name, i, read = step
        gpu.score(**synth.unpack_psm(lc.entry(name), i))
        out = dict(best_score=gpu.best_score, best_sequence=gpu.best_sequence, ascores=np.asarray(gpu.ascores),
                   alt_sites=[s.tolist() for s in gpu.alt_sites])
        if read:
            out["pep_scores"] = [(r["signature"].tolist(), r["counts"].tolist(), r["scores"].tobytes(), r["weighted_score"],
                                  r["total_fragments"], r["sequence"]) for r in gpu.pep_scores]
        return out
    _, name, flags, budget = step
    batch = lc.entry(name)
    gpu.set_workspace_budget(budget)
    try:
        out = dict(gpu.score_batch(batch, **flags))
        # (a retained batch is one plan and leaves the count alone -- unless its records do not fit the budget: such a call is
        # scored without them, in chunks like any other)
        counted = name == "chunked" and (not flags.get("keep") or budget)
        out["chunks"] = int(gpu._lib.pya_debug_last_chunks(gpu._h)) if counted else -1
    finally:
        gpu.set_workspace_budget(0)
    if flags.get("keep") and int(batch["n_psm"]):
        n = min(int(batch["n_psm"]), 16)
        out.update({"records." + k: v for k, v in gpu.batch_pep_scores(0, n).items()})
    return out


_fresh = {}


def _fresh_answer(step):
    key = lc.step_key(step)
    if key not in _fresh:
        _fresh[key] = _do(_gpu(), step)
    return _fresh[key]


_checked = set()


def _alt_by_position(batch, alt_mask):
    """``alt_mask`` as the checker writes it.  For a peptide of more than 64 residues the library's bit j is the j-th modifiable
    residue (include/pyascore_hip.h: pya_results.alt_mask); the checker's bit p - 1 is peptide position p, positions above 64
    dropped (oracle/oracle_abi.h)."""
    out = alt_mask.copy()
    for i in np.flatnonzero(np.diff(batch["pep_off"]) > 64):
        pep = bytes(batch["pep"][batch["pep_off"][i]:batch["pep_off"][i + 1]]).decode()
        sites = [p for p, c in enumerate(pep) if c in lc.SETTINGS["mod_group"]]
        for j in range(out.shape[1]):
            m = int(alt_mask[i, j])
            out[i, j] = sum(1 << sites[b] for b in range(len(sites)) if m >> b & 1 and sites[b] < 64)
    return out


def _fresh_is_the_checkers(name):
    if name in _checked or not int(lc.entry(name)["n_psm"]):
        return
    got = _fresh_answer(("batch", name, {"skip_invalid": True} if name in lc.MUST_SKIP_INVALID else {}, 0))
    ok = lc.valid(name)
    got = dict(got, alt_mask=_alt_by_position(lc.entry(name), got["alt_mask"]))
    _is_the_checkers({k: got[k][ok] for k in KEYS}, _want([name]), lc.entry(name)["n_of_mod"][ok], "fresh " + name)
    _checked.add(name)


@pytest.mark.parametrize("seed", lc.SEEDS)
def test_a_long_sequence_on_one_scorer_equals_fresh_scorers(seed):
    for name in lc.NAMES:
        _fresh_is_the_checkers(name)
    gpu = _gpu()
    t0, chunked = time.time(), set()
    for i, step in enumerate(lc.sequence(seed, lc.N_STEPS)):
        got = _do(gpu, step)                                                   # (a step that raises fails the test)
        _same_bytes(got, _fresh_answer(step), "seed %d step %d %r" % (seed, i, step))
        if step[0] == "batch" and got["chunks"] >= 0:
            assert (got["chunks"] > 1) == (step[3] == lc.SMALL_BUDGET), (i, step, got["chunks"])
            chunked.add(got["chunks"] > 1)
    print("seed %d: %d steps on one scorer and their fresh answers in %.1f s; tables at the end %r" %
          (seed, lc.N_STEPS, time.time() - t0, _tables(gpu)))
    assert True in chunked, "no call of this sequence was cut into chunks"
    # shrink, then grow back: every flag at once
    every = dict(evidence=True, ions=True, sites=True, probs=True, ranked=5, coverage=True, keep=True, skip_invalid=True)
    first = _do(gpu, ("batch", "wide", every, 0))
    _same_bytes(_do(gpu, ("batch", "one", every, 0)), _fresh_answer(("batch", "one", every, 0)), "one after wide")
    _same_bytes(_do(gpu, ("batch", "wide", every, 0)), first, "wide, one, wide")
    _same_bytes(first, _fresh_answer(("batch", "wide", every, 0)), "wide after the sequence")


def test_status_and_over_reports_do_not_leak_into_the_next_call():
    gpu = _gpu()
    a, inv = lc.entry("a_small"), lc.entry("invalid")
    got = gpu.score_batch(inv, skip_invalid=True)
    assert np.flatnonzero(got["status"]).tolist() == list(lc.INVALID_PSMS) and got["status_message"]
    clean = gpu.score_batch(a, skip_invalid=True)
    assert not clean["status"].any() and clean["status_message"] == ""
    _is_the_checkers(clean, _want(["a_small"]), a["n_of_mod"], "a clean call after one with PSMs set aside")
    # a site cap that reports PSMs, then none
    b = lc.entry("b_shapes")
    over = 2                                                                   # pya_site.kind: PYA_SITE_OVER
    assert _lib.PYA_SITE_OVER == over
    capped = gpu.score_batch(b, sites=True, site_sig_cap=10)
    psm = np.repeat(np.arange(int(b["n_psm"])), np.diff(capped["site_off"]))
    assert ((capped["sites"]["kind"] == over) == (capped["n_sig"][psm] > 10)).all() and (capped["sites"]["kind"] == over).any()
    free = gpu.score_batch(b, sites=True, site_sig_cap=0)
    assert not (free["sites"]["kind"] == over).any()
    _same_bytes(free, _gpu().score_batch(b, sites=True, site_sig_cap=0), "an uncapped call after a capped one")
    assert gpu._lib.pya_get_site_sig_cap(gpu._h) == _lib.PYA_FAST_SIGNATURES


def test_an_ion_room_report_does_not_leak_into_the_next_fill():
    from pyascore_amd.device import ion_records
    gpu = _gpu()
    a = lc.entry("a_small")
    want = gpu.score_batch(a, ions=True)
    total = int(want["ion_off"][-1])
    plan, mz, it, _ = _plan_a(gpu, ions=True)
    lib, res = gpu._lib, C.byref(plan._res)
    off = torch.zeros(plan.n_psm + 1, dtype=torch.int64, device=DEV)
    raw = torch.full((total + 8, 16), 0xEE, dtype=torch.uint8, device=DEV)
    s1, s2 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    with torch.cuda.stream(s1):                                                # room for all but one record
        assert lib.pya_plan_ions_count(plan._plan, res, s1.cuda_stream, off.data_ptr()) == _lib.PYA_OK
        assert lib.pya_plan_ions(plan._plan, res, s1.cuda_stream, off.data_ptr(), raw.data_ptr(), total - 1) == _lib.PYA_OK
    torch.cuda.synchronize()
    assert lib.pya_plan_check(plan._plan) == _lib.PYA_ERR_LIMIT and b"pya_plan_ions" in lib.pya_last_error(gpu._h)
    last = int(np.flatnonzero(np.diff(want["ion_off"]) > 0)[-1])
    assert bool((raw[int(want["ion_off"][last]):] == 0xEE).all())               # nothing of the PSM that did not fit, nothing behind the room
    with torch.cuda.stream(s2):                                                # with room, on ANOTHER stream
        assert lib.pya_plan_ions(plan._plan, res, s2.cuda_stream, off.data_ptr(), raw.data_ptr(), total) == _lib.PYA_OK
    torch.cuda.synchronize()
    plan.check()
    assert np.array_equal(off.cpu().numpy(), want["ion_off"])
    assert ion_records(raw.cpu().numpy()[:total]).tobytes() == want["ions"].tobytes()
    assert bool((raw[total:] == 0xEE).all())
