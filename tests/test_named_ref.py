"""The named-localisation yardstick (tests/named_ref.py) held to the golden vectors, to the evidence yardstick and, where
oracle/_ref is built, to the reference's own calculate_ambiguity on pairs that differ in more than one site.  No GPU."""
import os

import numpy as np
import pytest

import evidence_ref
import named_ref
from conftest import GOLDEN, golden_cases
from oracle import harness, orc
from pyascore_amd import synth


def _cases_with_containers():
    return [c for c in golden_cases() if "exp_ps_bits" in np.load(os.path.join(GOLDEN, c + ".npz"), allow_pickle=True)]


@pytest.mark.parametrize("case", _cases_with_containers())
def test_single_moves_reproduce_golden_ascores_and_evidence(case):
    """For every modified site of every golden PSM: the minimum of the yardstick's ambiguity over the competitors in
    alt_mask IS the golden Ascore, bit for bit, and the record of the evidence row's competitor carries that row's depth
    and counts."""
    settings, batch, exp = harness.load_case(os.path.join(GOLDEN, case + ".npz"))
    res = dict(best_sig=exp["best_sig"], alt_mask=exp["alt_mask"], ascores=exp["ascores"], n_sig=exp["n_sig"])
    ev, _ = evidence_ref.batch_rows(settings, batch, res, exp, synth.unpack_psm)
    kinds = set()
    for i in range(batch["n_psm"]):
        if exp["n_sig"][i] <= 0:
            continue
        kw = synth.unpack_psm(batch, i)
        k, best = int(kw["n_of_mod"]), int(exp["best_sig"][i])
        sites = evidence_ref.modifiable_positions(kw["peptide"], settings["mod_group"])
        cont = named_ref.containers_of(exp, int(exp["ps_off"][i]), int(exp["ps_off"][i + 1]))
        win, (counts, scores) = named_ref.record(settings, kw, best, cont, best)
        assert win["kind"] == named_ref.WINNER and win["ambiguity"] == 0 and win["n_moved"] == 0
        assert np.float32(win["pep_score"]).tobytes() == np.float32(exp["best_score"][i]).tobytes()
        assert np.array_equal(scores, cont[best][1]) and np.array_equal(counts, cont[best][0])
        if k >= len(sites):
            continue
        mp = evidence_ref.matcher(settings, kw)
        mods = [j for j in range(len(sites)) if best >> j & 1]
        for a in range(k):
            if np.isinf(exp["ascores"][i, a]):
                continue
            recs = {}
            for pos in evidence_ref.alt_positions(exp["alt_mask"][i, a], kw["peptide"], sites):
                q = (best & ~(1 << mods[a])) | (1 << sites.index(pos - 1))
                recs[pos] = named_ref.record(settings, kw, best, cont, q, mp)[0]
                assert recs[pos]["n_moved"] == 1 and recs[pos]["kind"] in (named_ref.TIED, named_ref.COUNTED)
                kinds.add(int(recs[pos]["kind"]))
            if not recs:
                continue
            low = min(np.float32(r["ambiguity"]) for r in recs.values())
            assert np.float32(low).tobytes() == np.float32(exp["ascores"][i, a]).tobytes(), (i, a)
            row = ev[i, a]
            mine = recs[int(row["comp_pos"])]
            assert np.float32(mine["pep_score"]).tobytes() == np.float32(row["comp_score"]).tobytes()
            if row["kind"] == evidence_ref.TIED:
                assert mine["kind"] == named_ref.TIED and mine["depth"] == 0 and mine["ref_possible"] == 0
            else:
                assert mine["kind"] == named_ref.COUNTED
                assert np.float32(mine["ambiguity"]).tobytes() == np.float32(exp["ascores"][i, a]).tobytes()
                for f in ("depth", "ref_matched", "ref_possible", "comp_matched", "comp_possible"):
                    assert mine[f] == row[f], (i, a, f)
    assert named_ref.COUNTED in kinds


def test_invalid_and_not_scored():
    settings, batch, exp = harness.load_case(os.path.join(GOLDEN, "velos_z1.npz"))
    i = int(np.flatnonzero(exp["n_sig"] > 1)[0])
    kw = synth.unpack_psm(batch, i)
    cont = named_ref.containers_of(exp, int(exp["ps_off"][i]), int(exp["ps_off"][i + 1]))
    n_sites = len(evidence_ref.modifiable_positions(kw["peptide"], settings["mod_group"]))
    for bad in (0, (1 << n_sites) | 1, (1 << (kw["n_of_mod"] + 1)) - 1):
        rec, (c, s) = named_ref.record(settings, kw, exp["best_sig"][i], cont, bad)
        assert rec["kind"] == named_ref.INVALID and rec["sig_bits"] == bad and not c.any() and not s.any()
        assert rec.tobytes()[8:20] == b"\0" * 12 and rec.tobytes()[21:] == b"\0" * 11
    rec, _ = named_ref.record(settings, kw, 0, {}, 5)
    assert rec["kind"] == named_ref.NONE and rec.tobytes()[8:] == b"\0" * 24 and rec["sig_bits"] == 5


@pytest.mark.parametrize("case", ["velos_z1", "velos_nl", "edge_default"])
def test_any_pair_equals_the_reference(case):
    """the reference's calculate_ambiguity(pep_scores[0], rec) for every site assignment of the PSM -- pairs that differ
    in several sites included -- against the yardstick's ambiguity"""
    settings, batch, exp = harness.load_case(os.path.join(GOLDEN, case + ".npz"))
    ref = harness.make_scorer(orc.OracleAscore, settings, kind="ref")
    multi = 0
    for i in range(min(int(batch["n_psm"]), 12)):
        kw = synth.unpack_psm(batch, i)
        ref.score(**kw)
        ps = ref.pep_scores
        if len(ps) < 2:
            continue
        cont = named_ref.containers_of(exp, int(exp["ps_off"][i]), int(exp["ps_off"][i + 1]))
        mp = evidence_ref.matcher(settings, kw)
        for rec in ps[1:40]:
            bits = harness.sig_bits(rec["signature"])
            got = named_ref.record(settings, kw, exp["best_sig"][i], cont, bits, mp)[0]
            want = np.float32(ref.calculate_ambiguity(ps[0], rec))
            assert np.float32(got["ambiguity"]).tobytes() == want.tobytes(), (i, bits, got, want)
            assert np.float32(got["pep_score"]).tobytes() == np.float32(rec["weighted_score"]).tobytes()
            assert got["total_fragments"] == rec["total_fragments"]
            multi += int(got["n_moved"] > 1)
    assert multi > 0
