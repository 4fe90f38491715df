"""The ranked yardstick (tests/ranked_ref.py) held to its definition (include/pyascore_hip.h: pya_ranked): on the golden
pep_scores and on the oracle's pep_scores of seeded PSMs it agrees with an independent brute force (python tuples, sorted),
row 0 is the golden winner, row 1 the runner-up the site yardstick derives, and hand-made cases have their known answers.
No GPU."""
import os

import numpy as np
import pytest

import ranked_ref
import sites_ref
from conftest import GOLDEN, checker_kind, golden_cases
from oracle import harness, orc
from pyascore_amd import ranked as rk, synth


def _cases_with_containers():
    return [c for c in golden_cases() if "exp_ps_bits" in np.load(os.path.join(GOLDEN, c + ".npz"), allow_pickle=True)]


def _check_psm(rows, best_sig, best_score, bits, ws, n_sites):
    K = rows.size
    want = ranked_ref.brute_force(best_sig, bits, ws)
    n = min(len(want), K)
    assert (rows["kind"][:n] == ranked_ref.SCORED).all() and rows[n:].tobytes() == b"\0" * 16 * (K - n)
    assert [(int(b), float(s)) for b, s in zip(rows["sig_bits"][:n], rows["pep_score"][:n])] == want[:n]
    assert rows["rank"][:n].tolist() == list(range(n))
    assert rows["sig_bits"][0] == best_sig and rows["pep_score"][0].tobytes() == np.float32(best_score).tobytes()
    assert (rows["pep_score"][:n] <= np.float32(best_score)).all()               # no assignment scores above best_score
    assert len(set(rows["sig_bits"][:n].tolist())) == n
    for r in range(n):
        tied = r > 0 and rows["pep_score"][r] == rows["pep_score"][r - 1]
        assert bool(rows["flags"][r] & ranked_ref.TIED_PREV) == tied
        assert bool(rows["flags"][r] & ranked_ref.IN_BEST_TIE) == (rows["pep_score"][r] == np.float32(best_score))
    if n >= 2:
        # row 1 is the runner-up the site table gives: the largest without_score among the winner's residues
        site = sites_ref.psm_records(list(range(n_sites)), best_sig, bits, ws)
        inb = (site["flags"] & sites_ref.IN_BEST) != 0
        assert inb.any() and rows["pep_score"][1] == site["without_score"][inb].max()
    return n


@pytest.mark.parametrize("case", _cases_with_containers())
def test_golden_cases_agree_with_the_brute_force(case):
    settings, batch, exp = harness.load_case(os.path.join(GOLDEN, case + ".npz"))
    for K in (1, 5, 64):
        rows = ranked_ref.batch_rows(K, exp, exp)
        assert rows.shape == (batch["n_psm"], K)
        seen = 0
        for i in range(batch["n_psm"]):
            lo, hi = int(exp["ps_off"][i]), int(exp["ps_off"][i + 1])
            if exp["n_sig"][i] <= 0:
                assert rows[i].tobytes() == b"\0" * 16 * K
                continue
            n_sites = len(sites_ref.modifiable_positions(synth.unpack_psm(batch, i)["peptide"], settings["mod_group"]))
            n = _check_psm(rows[i], exp["best_sig"][i], exp["best_score"][i], exp["ps_bits"][lo:hi], exp["ps_ws"][lo:hi], n_sites)
            assert n == min(hi - lo, K) == rk.lengths(rows[i])[0]
            seen += 1
        assert seen
        if K > 1:                                                               # the shorter list is the prefix of the longer
            assert ranked_ref.batch_rows(K - 1, exp, exp).tobytes() == np.ascontiguousarray(rows[:, :K - 1]).tobytes()


@pytest.mark.parametrize("cfg,over", [("cfg1", {}), ("cfg2", {}), ("cfg3", {}), ("cfg4", {}), ("cfg5", dict(L=24, n_sites=9, n_mod=4))])
def test_seeded_psms_agree_with_the_brute_force(cfg, over):
    batch, settings = synth.make_batch(cfg, n_psm=4, seed=9610, **over)
    chk = harness.make_scorer(orc.OracleAscore, settings, kind=checker_kind())
    for i in range(batch["n_psm"]):
        kw = synth.unpack_psm(batch, i)
        chk.score(**kw)
        raw = chk.raw_pep_scores()
        n_sites = raw["signature"].shape[1]
        bits = (raw["signature"].astype(np.uint64) << np.arange(n_sites, dtype=np.uint64)).sum(axis=1).astype(np.uint64)
        ws = raw["weighted_score"].astype(np.float32)
        best = bits[0]                                                         # the reference's winner: first of its sorted records
        assert ws[0] == ws.max()
        for K in (2, 16, 64):
            rows = ranked_ref.psm_rows(K, best, ws[0], bits, ws)
            _check_psm(rows, best, ws[0], bits, ws, n_sites)
            again = ranked_ref.psm_rows(K, best, ws[0], bits[::-1], ws[::-1])   # the order of the records does not matter
            assert again.tobytes() == rows.tobytes()


def test_known_answers():
    f = np.float32
    # one modification on three sites; the winner is sig 2 although sig 1 ties it: the reference's tie-break stands
    rows = ranked_ref.psm_rows(5, 2, f(30), [1, 2, 4], f([30, 30, 20]))
    assert rows["sig_bits"].tolist() == [2, 1, 4, 0, 0] and rows["pep_score"].tolist() == [30, 30, 20, 0, 0]
    assert rows["rank"].tolist() == [0, 1, 2, 0, 0] and rows["kind"].tolist() == [1, 1, 1, 0, 0]
    assert rows["flags"].tolist() == [ranked_ref.IN_BEST_TIE, ranked_ref.TIED_PREV | ranked_ref.IN_BEST_TIE, 0, 0, 0]
    assert rk.best_tie_size(rows).tolist() == [2] and rk.lengths(rows).tolist() == [3]
    # equal floats behind the winner: ascending sig bits, whatever order the records come in
    rows = ranked_ref.psm_rows(4, 8, f(40), [4, 8, 1, 2], f([10, 40, 10, 10]))
    assert rows["sig_bits"].tolist() == [8, 1, 2, 4] and rows["flags"].tolist() == [2, 0, 1, 1]
    assert ranked_ref.psm_rows(2, 8, f(40), [4, 8, 1, 2], f([10, 40, 10, 10])).tobytes() == rows[:2].tobytes()   # the prefix
    # no modification: one assignment that modifies nothing; as many modifications as sites: one that modifies everything
    rows = ranked_ref.psm_rows(3, 0, f(12.5), [0], f([12.5]))
    assert rows["kind"].tolist() == [1, 0, 0] and rows["sig_bits"][0] == 0 and rows["pep_score"][0] == f(12.5) and rows[1:].tobytes() == b"\0" * 32
    rows = ranked_ref.psm_rows(3, 7, f(7), [7], f([7]))
    assert rows["kind"].tolist() == [1, 0, 0] and rows["sig_bits"][0] == 7 and rows["flags"][0] == ranked_ref.IN_BEST_TIE
    # more modifications than sites: no assignment, not scored
    assert ranked_ref.psm_rows(3, 0, 0, [], [], scored=False).tobytes() == b"\0" * 48
    assert ranked_ref.psm_rows(3, 0, 0, [], []).tobytes() == b"\0" * 48
    # over the cap: row 0 alone
    rows = ranked_ref.psm_rows(3, 2, f(30), [1, 2, 4], f([30, 30, 20]), sig_cap=2)
    assert rows["kind"].tolist() == [ranked_ref.OVER, 0, 0] and rows["sig_bits"][0] == 2 and rows["pep_score"][0] == 30 and rows["flags"][0] == 0
    assert rows[1:].tobytes() == b"\0" * 32 and rk.lengths(rows).tolist() == [1] and rk.best_tie_size(rows).tolist() == [0]
    with pytest.raises(AssertionError):
        ranked_ref.psm_rows(0, 2, f(30), [1, 2], f([30, 30]))
    with pytest.raises(AssertionError):
        ranked_ref.psm_rows(65, 2, f(30), [1, 2], f([30, 30]))
