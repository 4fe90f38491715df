"""The site-table yardstick (tests/sites_ref.py) held to the golden vectors: every consequence include/pyascore_hip.h lists
for a pya_site record, against the golden best_score / best_sig / pep_scores and the evidence yardstick, and, where
oracle/_ref is built, against the reference's own pep_scores.  Hand-made known answers for the tie rule.  No GPU."""
import os

import numpy as np
import pytest

import evidence_ref
import sites_ref
from conftest import GOLDEN, golden_cases
from oracle import harness, orc
from pyascore_amd import synth


def _cases_with_containers():
    return [c for c in golden_cases() if "exp_ps_bits" in np.load(os.path.join(GOLDEN, c + ".npz"), allow_pickle=True)]


def _bits(x):
    return np.float32(x).tobytes()


def _check_psm(rec, best_sig, best_score, bits, ws):
    """the consequences of the definition for the records of one scored PSM"""
    best = int(best_sig)
    assert (rec["kind"] == sites_ref.SCORED).all() and not rec["reserved"].any()
    for s, r in enumerate(rec):
        has = (bits >> np.uint64(s)) & np.uint64(1) == 1
        in_best = bool(best >> s & 1)
        assert bool(r["flags"] & sites_ref.IN_BEST) == in_best
        if in_best:
            assert _bits(r["with_score"]) == _bits(best_score) and int(r["with_sig"]) == best
        else:
            assert _bits(r["without_score"]) == _bits(best_score) and int(r["without_sig"]) == best
        for score, sig, pick, tied in ((r["with_score"], r["with_sig"], has, sites_ref.WITH_TIED),
                                       (r["without_score"], r["without_sig"], ~has, sites_ref.WITHOUT_TIED)):
            if not pick.any():
                assert score == -1 and sig == 0
                continue
            assert _bits(score) == _bits(ws[pick].max())                       # bit for bit the maximum of the set
            at = bits[pick & (ws == ws[pick].max())]
            assert int(sig) in at.tolist() and bool(r["flags"] & tied) == (at.size > 1)
            assert int(sig) == best or best not in at.tolist()
            assert int(sig) == best or int(sig) == int(at.min())
        assert bool(r["flags"] & sites_ref.NO_WITHOUT) == (not (~has).any())


@pytest.mark.parametrize("case", _cases_with_containers())
def test_golden_cases_satisfy_the_consequences(case):
    settings, batch, exp = harness.load_case(os.path.join(GOLDEN, case + ".npz"))
    off, rec = sites_ref.batch_records(settings, batch, exp, exp, synth.unpack_psm)
    assert off.size == batch["n_psm"] + 1 and off[-1] == rec.size
    res = dict(best_sig=exp["best_sig"], alt_mask=exp["alt_mask"], ascores=exp["ascores"], n_sig=exp["n_sig"])
    ev, _ = evidence_ref.batch_rows(settings, batch, res, exp, synth.unpack_psm)
    scored = k1 = 0
    for i in range(batch["n_psm"]):
        r = rec[off[i]:off[i + 1]]
        kw = synth.unpack_psm(batch, i)
        positions = sites_ref.modifiable_positions(kw["peptide"], settings["mod_group"])
        assert r["pos"].tolist() == [p + 1 for p in positions]
        if exp["n_sig"][i] <= 0:
            assert (r["kind"] == sites_ref.NONE).all() and all(x.tobytes()[:24] == b"\0" * 24 for x in r)
            continue
        lo, hi = int(exp["ps_off"][i]), int(exp["ps_off"][i + 1])
        _check_psm(r, exp["best_sig"][i], exp["best_score"][i], exp["ps_bits"][lo:hi], exp["ps_ws"][lo:hi])
        scored += 1
        mods = np.flatnonzero((r["flags"] & sites_ref.IN_BEST) != 0)
        by_pos = {int(p): j for j, p in enumerate(r["pos"])}
        for a, e in enumerate(ev[i][: mods.size]):
            if not e["kind"]:
                continue
            assert e["comp_score"] <= r["without_score"][mods[a]] and e["comp_score"] <= r["with_score"][by_pos[int(e["comp_pos"])]]
            if mods.size == 1:                                                 # every alternative is a single move
                assert _bits(e["comp_score"]) == _bits(r["without_score"][mods[0]])
                k1 += 1
    assert scored
    if int(np.min(batch["n_of_mod"])) == 1:
        assert k1


@pytest.mark.parametrize("case", ["velos_z1", "velos_nl", "edge_default"])
def test_the_reference_pep_scores_give_the_same_records(case):
    if not orc.available("ref"):
        pytest.skip("oracle/_ref is not built here")
    settings, batch, exp = harness.load_case(os.path.join(GOLDEN, case + ".npz"))
    ref = harness.make_scorer(orc.OracleAscore, settings, kind="ref")
    off, rec = sites_ref.batch_records(settings, batch, exp, exp, synth.unpack_psm)
    for i in range(min(int(batch["n_psm"]), 12)):
        kw = synth.unpack_psm(batch, i)
        ref.score(**kw)
        ps = ref.pep_scores
        if not ps:
            continue
        bits = np.array([harness.sig_bits(p["signature"]) for p in ps], np.uint64)
        ws = np.array([p["weighted_score"] for p in ps], np.float32)
        positions = sites_ref.modifiable_positions(kw["peptide"], settings["mod_group"])
        mine = sites_ref.psm_records(positions, harness.sig_bits(ps[0]["signature"]), bits[::-1], ws[::-1])    # any order
        assert mine.tobytes() == rec[off[i]:off[i + 1]].tobytes(), (case, i)


def test_known_answers():
    # k = 1, three sites at residues 1, 3, 4 (0-based): every residue's "with" set is one assignment
    r = sites_ref.psm_records([1, 3, 4], 2, [1, 2, 4], [5.0, 9.0, 7.5])
    assert r["pos"].tolist() == [2, 4, 5] and (r["kind"] == 1).all()
    assert r["with_score"].tolist() == [5.0, 9.0, 7.5] and r["with_sig"].tolist() == [1, 2, 4]
    assert r["without_score"].tolist() == [9.0, 7.5, 9.0] and r["without_sig"].tolist() == [2, 4, 2]
    assert r["flags"].tolist() == [0, sites_ref.IN_BEST, 0]
    # n_of_mod == n_sites: nothing leaves a residue unmodified
    r = sites_ref.psm_records([0, 5], 3, [3], [12.5])
    assert (r["flags"] == (sites_ref.IN_BEST | sites_ref.NO_WITHOUT)).all() and (r["without_score"] == -1).all()
    assert not r["without_sig"].any() and (r["with_sig"] == 3).all() and (r["with_score"] == 12.5).all()
    # a top tie where best_sig is not the smallest bits: k = 2 of 3 sites, 0b110 (the winner) ties 0b011
    r = sites_ref.psm_records([0, 1, 2], 0b110, [0b011, 0b101, 0b110], [8.0, 3.0, 8.0])
    assert r["with_sig"].tolist() == [0b011, 0b110, 0b110] and r["with_score"].tolist() == [8.0, 8.0, 8.0]
    assert r["without_sig"].tolist() == [0b110, 0b101, 0b011] and r["without_score"].tolist() == [8.0, 3.0, 8.0]
    assert r["flags"].tolist() == [0, sites_ref.IN_BEST | sites_ref.WITH_TIED, sites_ref.IN_BEST]
    # ... and a tie that best_sig is no part of: the smallest bits
    r = sites_ref.psm_records([0, 1, 2, 3], 0b1000, [1, 2, 4, 8], [6.0, 6.0, 6.0, 9.0])
    assert r["without_sig"].tolist() == [8, 8, 8, 1] and r["flags"].tolist() == [0, 0, 0, sites_ref.IN_BEST | sites_ref.WITHOUT_TIED]
    # not scored, and over the cap
    r = sites_ref.psm_records([2, 7], 0, [], [], scored=False)
    assert r["pos"].tolist() == [3, 8] and all(x.tobytes()[:24] == b"\0" * 24 and x.tobytes()[26:] == b"\0" * 6 for x in r)
    r = sites_ref.psm_records([0, 1, 2], 0b110, [0b011, 0b101, 0b110], [8.0, 3.0, 8.0], sig_cap=2)
    assert (r["kind"] == sites_ref.OVER).all() and r["flags"].tolist() == [0, 1, 1] and not r["with_score"].any() and not r["with_sig"].any()
    # n_of_mod 0: one assignment, nothing modified
    r = sites_ref.psm_records([1, 2], 0, [0], [4.0])
    assert (r["with_score"] == -1).all() and (r["without_score"] == 4.0).all() and not r["flags"].any()
