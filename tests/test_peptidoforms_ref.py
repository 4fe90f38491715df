"""The peptidoform yardstick (tests/peptidoforms_ref.py) against answers worked out by hand, and the numpy host form
(pyascore_amd.rollup.merge_peptidoforms) against the yardstick, on the list kinds the GPU tests use.  No GPU."""
import numpy as np
import pytest

import peptidoform_lists as pl
import peptidoforms_ref as ref
from pyascore_amd import probs as pb, rollup as ru

DT = ref.DTYPE


def _rec(rows):
    return np.array(rows, DT)


def test_reduce_known_answer():
    a = _rec([(6, 2, 1, 1, 9, 0.9, 2.0, 5.0, 0), (5, 2, 2, 0, 4, 0.5, 1.5, -1.0, 7), (6, 2, 3, 2, 3, 0.9, 1.25, np.inf, 0),
              (1, 7, 1, 1, 1, 1.0, 1.0, 0.0, 0), (9, 2, 0, 5, 0, 1.0, 0.5, 99.0, 0)])
    want = _rec([(5, 2, 2, 0, 4, 0.5, 1.5, -1.0, 2), (6, 2, 4, 3, 3, 0.9, 1.25, np.inf, 2), (1, 7, 1, 1, 1, 1.0, 1.0, 0.0, 1)])
    assert ref.reduce(a).tobytes() == want.tobytes()
    assert ref.reduce(a[:2], a[2:]).tobytes() == want.tobytes()
    assert ref.reduce(np.zeros(0, DT)).size == 0 and ref.reduce(a[4:]).size == 0


def test_ascore_order_and_prob_bits():
    vals = np.array([0xFFC00000, 0xFF800000, 0xBF800000, 0x80000000, 0x00000000, 0x3F800000, 0x7F800000, 0x7FC00000], np.uint32)
    assert [ref.akey(int(v)) for v in vals] == sorted(ref.akey(int(v)) for v in vals)
    for i in range(len(vals) - 1):
        a = _rec([(1, 1, 1, 0, 0, 0.5, 1.0, 0.0, 0)] * 2)
        a["best_min_ascore"] = vals[i:i + 2].view(np.float32)
        assert ref.reduce(a)["best_min_ascore"].view(np.uint32)[0] == vals[i + 1]
    a = _rec([(1, 1, 1, 0, 8, 0.0, 1.0, 0.0, 0), (1, 1, 1, 0, 7, 5e-324, 3.0, 0.0, 0)])
    got = ref.reduce(a)[0]
    assert got["best_min_prob"] == 5e-324 and got["best_psm"] == 7 and got["best_z"] == 1.0


def test_psms_known_answer():
    # three PSMs of group 4: residues with probabilities, best_sig 0b101 / 0b101 / 0b010; one OVER, one negative group, one unmodified
    site_off = np.array([0, 3, 6, 9, 12, 15, 17], np.int64)
    sp = np.zeros(17, pb.SITE_PROB_DTYPE)
    sp["with_prob"] = [0.9, 0.1, 0.8, 0.7, 0.2, 0.95, 0.3, 0.6, 0.1, -1, -1, -1, 1, 1, 1, 0.0, 0.0]
    pp = np.zeros(6, pb.PSM_PROB_DTYPE)
    pp["kind"] = [pb.SCORED, pb.SCORED, pb.SCORED, pb.OVER, pb.SCORED, pb.SCORED]
    pp["z"] = [1.5, 1.25, 2.0, 0.0, 1.0, 1.0]
    best_sig = np.array([0b101, 0b101, 0b010, 0b011, 0b111, 0], np.uint64)
    asc = np.array([[3.0, 7.0, 0.0], [np.inf, -2.0, 0.0], [1.0, 99.0, 99.0], [5, 5, 5], [1, 2, 3], [42, 42, 42]], np.float32)
    group = np.array([4, 4, 4, 4, -1, 2], np.int32)
    got = ref.from_psms(best_sig, asc, site_off, sp, pp, group, threshold=0.75, psm_base=100)
    want = _rec([(0, 2, 1, 1, 105, 1.0, 1.0, np.inf, 1), (0b010, 4, 1, 0, 102, 0.6, 2.0, 1.0, 2), (0b101, 4, 2, 1, 100, 0.8, 1.25, 3.0, 2)])
    assert got.tobytes() == want.tobytes()
    ids = np.array([9, 8, 7, 6, 5, 4], np.uint32)
    again = ref.from_psms(best_sig, asc, site_off, sp, pp, group, psm_id=ids, prev=got)
    assert again["n_psm"].tolist() == [2, 2, 4] and again["best_psm"].tolist() == [4, 7, 9] and again["n_isomers"].tolist() == [1, 2, 2]
    halves = ref.from_psms(best_sig[3:], asc[3:], site_off[3:] - 9, sp[9:], pp[3:], group[3:], psm_base=103,
                           prev=ref.from_psms(best_sig[:3], asc[:3], site_off[:4], sp[:9], pp[:3], group[:3], psm_base=100))
    assert halves.tobytes() == want.tobytes()


@pytest.mark.parametrize("kind", pl.KINDS)
def test_host_merge_equals_the_yardstick(kind):
    for n in pl.SIZES:
        r = pl.make(n, kind)
        want = ref.reduce(r)
        assert ru.merge_peptidoforms(r).tobytes() == want.tobytes(), (kind, n)
        assert ru.merge_peptidoforms(r[: n // 3], r[n // 3:]).tobytes() == want.tobytes(), (kind, n)
        assert (want["n_isomers"] >= 1).all() and (np.diff(want["group"].astype(np.int64)) >= 0).all()


@pytest.mark.parametrize("kind", pl.KINDS)
def test_merge_is_associative_and_commutative(kind):
    n = 2 * pl.T + 1
    r = pl.make(n, kind)
    a, b, c = r[:700], r[700:1500], r[1500:]
    m = ru.merge_peptidoforms
    whole = m(r)
    assert m(a, b).tobytes() == m(b, a).tobytes()
    assert m(m(a, b), c).tobytes() == m(a, m(b, c)).tobytes() == whole.tobytes()
    assert m(whole).tobytes() == whole.tobytes() and m(whole, np.zeros(0, DT)).tobytes() == whole.tobytes()
    assert m(r[np.random.default_rng(1).permutation(n)]).tobytes() == whole.tobytes()
