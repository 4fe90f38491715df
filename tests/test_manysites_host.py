"""The many-site family of tests/manysites.py, without a GPU: the CPU restatement against the reference's own core on every
case, the conditions on the INPUTS that keep tests/test_gpu_many_sites.py from being vacuous (asserted on the reference's
answers, never on the library's), and the numpy yardsticks of the later stages held to their reference-derived checks on a
33-site and a 63-site case -- a yardstick that is itself wrong above bit 31 would hide a kernel that is wrong the same way."""
import os
from math import comb

import numpy as np
import pytest

import manysites as ms
import rollup_ref
import test_evidence_ref
import test_ions_ref
import test_named_ref
import test_probs_ref
import test_ranked_ref
import test_sites_ref
from oracle import harness, orc
from pyascore_amd import _lib, synth

needs_ref = pytest.mark.skipif(not orc.available("ref"), reason="oracle/_ref not built")
KIND = "ref" if orc.available("ref") else "oracle"
ALL = list(ms.CASES) + list(ms.MIXED)


@needs_ref
@pytest.mark.parametrize("name", ALL)
def test_restatement_equals_the_reference(name):
    """every field of score_batch, and for three PSMs every per-assignment record and property, both kinds of checker"""
    settings, batch, _ = ms.case(name)
    bad = ms.changed(ms.answer(name, "ref"), ms.answer(name, "oracle"))
    assert bad.size == 0, (name, bad[:10].tolist())
    ref, port = ms.checker(settings, "ref"), ms.checker(settings, "oracle")
    for i in range(min(3, int(batch["n_psm"]))):
        kw = synth.unpack_psm(batch, i)
        ref.score(**kw)
        port.score(**kw)
        a, b = ref.raw_pep_scores(), port.raw_pep_scores()
        for key in a:
            assert a[key].tobytes() == b[key].tobytes(), (name, i, key)
        assert ref.best_sequence == port.best_sequence and ref.ascores.tobytes() == port.ascores.tobytes(), (name, i)
        assert [s.tolist() for s in ref.alt_sites] == [s.tolist() for s in port.alt_sites], (name, i)


@pytest.mark.parametrize("name", ALL)
def test_the_cases_are_what_they_say(name):
    """shapes, assignment counts, and for the planted PSMs that the truth went where its kind says"""
    settings, batch, shape = ms.case(name)
    want = ms.answer(name, KIND)
    assert int(batch["n_psm"]) == len(shape) <= 24
    for i, (L, s, k) in enumerate(shape):
        kw = synth.unpack_psm(batch, i)
        assert len(kw["peptide"]) == L and sum(c in "STY" for c in kw["peptide"]) == s and kw["n_of_mod"] == k
        assert want["n_sig"][i] == comb(s, k)
    if name in ms.CASES:
        L, s, k, n, _ = ms.CASES[name]
        psms = ms.planted(L, s, k, n, ms._seed(name), settings["mz_error"], ms.max_charge_of(settings))
        for i, p in enumerate(psms):
            t = p["truth"]
            assert t.size == k and np.all(np.diff(t) > 0) and (t.size == 0 or t[-1] < s)
            if s > 32 and 0 < k < s:
                marked = t if k <= 32 else np.setdiff1d(np.arange(s), t)
                n_high = int((marked >= 32).sum())
                assert n_high == {"straddle": 1, "low": 0, "high": min(marked.size, s - 32)}[ms.KINDS[i % 3]], (name, i)


def _localises(name):
    _, _, shape = ms.case(name)
    return [i for i, (_, s, k) in enumerate(shape) if 0 < k < s]


@pytest.mark.parametrize("name", ALL)
def test_the_winners_use_the_high_sites(name):
    """on the reference's answers.  Of the PSMs with more than 32 sites (and something to localise): at least a third have a
    winner with a bit of index >= 32 set, at least one has none; for k >= 2 at least two winners have modified sites on both
    sides of bit 32.  (k > 32: the same of the unmodified sites, see manysites.winner_masks.)  At least a quarter of all
    Ascores of the case are neither 0 nor infinite."""
    _, batch, shape = ms.case(name)
    want = ms.answer(name, KIND)
    loc = _localises(name)
    masks = ms.winner_masks(name, want)
    many = [i for i in loc if shape[i][1] > 32]
    if many:
        high = np.array([bool(masks[i] & ms.HIGH) for i in many])
        both = np.array([bool(masks[i] & ms.HIGH) and bool(masks[i] & ~ms.HIGH) for i in many])
        print("%s: %d of %d winners use a site >= 32, %d straddle" % (name, high.sum(), len(many), both.sum()))
        assert 3 * int(high.sum()) >= len(many) and not high.all(), (name, high.tolist())
        if any(min(shape[i][2], shape[i][1] - shape[i][2]) >= 2 for i in many):
            assert int(both.sum()) >= 2, (name, both.tolist())
        if all(shape[i][1] == 33 for i in many):
            assert all(bool(int(masks[i]) >> 32 & 1) == bool(masks[i] & ms.HIGH) for i in many)
    if loc:
        a = np.concatenate([want["ascores"][i, :shape[i][2]] for i in loc])
        share = float(np.mean((a != 0) & np.isfinite(a)))
        print("%s: %.2f of %d Ascores are neither 0 nor infinite" % (name, share, a.size))
        assert share >= 0.25, (name, share)
    else:
        assert name in ("p_64_63_0", "p_64_63_63")                  # one assignment: nothing to localise


def test_the_mixed_batches_share_a_class():
    """the pairs of manysites.MIXED fall into one C(n,k) class of host_internal.h's kBucketLimits, and C(32,2) / C(33,2),
    the pair one would pick first, do not"""
    limits = (64, 512, 4096, 15000)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "kBucketLimits[] = {64, 512, 4096, PYA_FAST_SIGNATURES}" in open(os.path.join(root, "pyascore_amd", "csrc", "host_internal.h")).read()
    assert "#define PYA_FAST_SIGNATURES 15000" in open(os.path.join(root, "include", "pyascore_hip.h")).read()

    def cls(s, k):
        return next(j for j, lim in enumerate(limits) if comb(s, k) <= lim)

    assert cls(32, 2) != cls(33, 2)
    assert cls(32, 3) == cls(33, 3) == 3 and cls(33, 2) == cls(16, 3) == cls(12, 6) == 2
    for name, (_, groups) in ms.MIXED.items():
        _, batch, shape = ms.case(name)
        assert {sh for sh in shape} == {g[:3] for g in groups}
        assert shape[0] != shape[1]                                   # interleaved


# ---- the yardsticks of the later stages above bit 31 ---------------------------------------------------------------------
YARDSTICK_CASES = ["p_40_33_2", "p_64_63_2"]
_exp = {}


def _as_golden(name):
    """the first PSMs of a case (five; one where a PSM has 1 953 records for the checker to list, seven seconds each time) with the reference's answers in the layout
    of a golden file (harness.collect)"""
    if name not in _exp:
        settings, batch, _ = ms.case(name)
        n = 5 if ms.CASES[name][1] == 33 else 1
        sub = synth.slice_batch(batch, 0, n)
        sub = {k: (np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v) for k, v in sub.items()}
        exp = harness.collect(ms.checker(settings, "ref"), sub, synth.unpack_psm)
        assert (exp["best_sig"] >> np.uint64(32)).any(), name                   # the winners above bit 31 are among them
        _exp[name] = (settings, sub, exp)
    return _exp[name]


@needs_ref
@pytest.mark.parametrize("name", YARDSTICK_CASES)
@pytest.mark.parametrize("check", [
    test_evidence_ref.test_yardstick_reproduces_golden_ascores,
    test_ions_ref.test_yardstick_adds_up_to_the_golden_counts,
    test_named_ref.test_single_moves_reproduce_golden_ascores_and_evidence,
    test_named_ref.test_any_pair_equals_the_reference,
    test_sites_ref.test_golden_cases_satisfy_the_consequences,
    test_sites_ref.test_the_reference_pep_scores_give_the_same_records,
    test_probs_ref.test_golden_cases_agree_with_the_brute_force,
    test_ranked_ref.test_golden_cases_agree_with_the_brute_force,
], ids=lambda f: f.__module__[5:] + "." + f.__name__[5:30])
def test_yardsticks_pass_their_own_checks(name, check, monkeypatch):
    """evidence_ref, ions_ref, named_ref, sites_ref, probs_ref, ranked_ref: the checks their test_*_ref.py files run on the
    golden files (the reference's Ascores, counts, pep_scores and calculate_ambiguity; a brute force), run on PSMs with 33
    and 63 sites -- the golden file is replaced by the reference's answers of now, the checks are those files' own"""
    monkeypatch.setattr(harness, "load_case", lambda path: _as_golden(name))
    check(name)


def test_rollup_yardstick_above_bit_31():
    """rollup_ref by hand, in the way of tests/test_rollup_ref.py: two 63-residue PSMs whose winners differ only above bit 31"""
    SP, PP = np.dtype(_lib.SITE_PROB_DTYPE), np.dtype(_lib.PSM_PROB_DTYPE)
    sig = np.array([(1 << 3) | (1 << 32) | (1 << 62), (1 << 3) | (1 << 33) | (1 << 62)], np.uint64)
    off = np.array([0, 63, 126], np.int64)
    sp = np.zeros(126, SP)
    for i in range(2):
        for r in range(63):
            sp["with_prob"][63 * i + r] = 0.875 if int(sig[i]) >> r & 1 else 0.03125
    sp["without_prob"] = 1.0 - sp["with_prob"]
    pp = np.zeros(2, PP)
    pp["kind"] = 1
    asc = np.array([[5.0, 11.0, 17.0], [6.0, 12.0, 3.0]], np.float32)
    slot = np.concatenate([np.arange(63), np.arange(63)]).astype(np.int32)      # one slot per site
    t = rollup_ref.table(sp, pp, off, sig, asc, slot, 63, 0.5)
    assert t["n_psm"].tolist() == [2] * 63
    want_in_best = np.zeros(63, int)
    want_in_best[[3, 62]] = 2
    want_in_best[[32, 33]] = 1
    assert t["n_in_best"].tolist() == want_in_best.tolist() and t["n_confident"].tolist() == want_in_best.tolist()
    assert t["best_ascore"][[3, 32, 33, 62]].tolist() == [6.0, 11.0, 12.0, 17.0]       # the column is the popcount BELOW the site
    assert not t["best_ascore"][want_in_best == 0].any()
    assert t["best_psm"][32] == 0 and t["best_psm"][33] == 1 and t["best_psm"][62] == 0 and t["best_prob"][32] == 0.875
