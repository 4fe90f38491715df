"""Peptidoform quantification on the host (include/pyascore_hip.h): the numpy restatement pyascore_amd.rollup.peptidoform_quant
against the plain-Python yardstick tests/peptidoform_quant_ref.py on the raw bytes of list, head and cell; the multiset
property; the cap prefix; the value rule; what is refused; and planted reporter intensities recovered per peptidoform through the
reference core's PepScores.  No GPU.  In every test the quant threshold is the median min_prob of the PSMs that contribute to
the list (peptidoform_quant_cases.threshold asserts the coverage conditions)."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import markers_cases as mc
import peptidoform_quant_cases as pc
import peptidoform_quant_ref as ref
import probs_ref
from conftest import GOLDEN, ROOT, checker_kind, golden_cases
from oracle import harness, orc
from pyascore_amd import _lib, rollup as ru, synth

NAN, INF = pc.NAN, pc.INF
SCALE = pc.SCALE


def _both(r, values, row, p, list_thr=0.75, psm_id=None, psm_base=0, prev=None, cap=None):
    got = ru.peptidoform_quant(r["site_probs"], r["psm_probs"], r["site_off"], r["best_sig"], r["ascores"], r["group"], values, row, p,
                               threshold=list_thr, psm_id=psm_id, psm_base=psm_base, prev=prev, cap=cap)
    want = ref.pair(r["best_sig"], r["ascores"], r["site_off"], r["site_probs"], r["psm_probs"], r["group"], values, row, list_thr,
                    p["threshold"], p["scale_log2"], p["complete_only"], psm_id=psm_id, psm_base=psm_base, prev=prev, cap=cap)
    return got, want


def _rescored(settings, batch):
    """the arrays score_batch(probs=True) returns for `batch`, through the reference core and tests/probs_ref.py"""
    chk = harness.make_scorer(orc.OracleAscore, settings, kind=checker_kind())
    exp = harness.collect(chk, batch, synth.unpack_psm)
    site_off, site_probs, psm_probs = probs_ref.batch_records(settings, batch, exp, exp, synth.unpack_psm)
    return dict(site_probs=site_probs, psm_probs=psm_probs, site_off=site_off, best_sig=exp["best_sig"], ascores=exp["ascores"])


def _golden(case):
    """a golden with its peptides repeated against its other spectra, as the GPU test feeds it, rescored through the reference core"""
    settings, batch, _ = harness.load_case(os.path.join(GOLDEN, case + ".npz"))
    batch, names = pc.repeats(batch, share=pc.GOLDEN_SHARE)
    group, _, _ = ru.peptide_groups(names)
    return dict(_rescored(settings, batch), group=group)


@pytest.mark.parametrize("case", [c for c in golden_cases() if c.startswith(("velos_", "ties_", "edge_"))])
def test_golden_cases_equal_the_yardstick(case):
    """the goldens with repeated peptides; the coverage conditions hold for all but six edge goldens, whose listed PSMs have
    min_prob 1.0 throughout (peptidoform_quant_cases.EDGE_WITHOUT_SPREAD says why they cannot hold; that is asserted here)"""
    r = _golden(case)
    n = len(r["best_sig"])
    mp = [p for _, p, _ in pc.min_probs(r, r["group"])]
    assert mp
    if case in pc.EDGE_WITHOUT_SPREAD:
        assert all(q == 1.0 for q in mp)                                             # the median is 1.0 and everything reaches it
        with pytest.raises(AssertionError, match="contribute at the median"):
            pc.threshold(r, r["group"])
        thr = 1.0
    else:
        thr = pc.threshold(r, r["group"])
    for n_ch in (1, 18):
        p = ru.site_quant_params(threshold=thr, scale_log2=SCALE, n_channels=n_ch)
        got, want = _both(r, pc.matrix(n + n_ch, n, n_ch), None, p)
        pc.same(got, want, "%s, %d channels" % (case, n_ch))
        assert int(got[1]["n_records"].sum()) == sum(1 for q in mp if q >= thr) >= 1
        assert got[0].tobytes() == ru.merge_peptidoforms(got[0]).tobytes()


@pytest.mark.parametrize("n_ch", [1, 18, 63, 64])
@pytest.mark.parametrize("complete_only", [False, True])
def test_restatement_equals_the_yardstick_on_random_records(n_ch, complete_only):
    r = pc.records(200 + n_ch, 700)
    n_rows = 300
    row = (np.arange(700) % (n_rows + 1) - 1).astype(np.int32)                        # fewer rows than PSMs, some PSMs without
    thr = pc.threshold(r, r["group"], row, n_rows)
    values = pc.matrix(n_ch, n_rows, n_ch, wide=True)
    p = ru.site_quant_params(threshold=thr, scale_log2=7, n_channels=n_ch, complete_only=complete_only)
    got, want = _both(r, values, row, p, list_thr=0.6, psm_base=1000)
    pc.same(got, want, "%d channels" % n_ch)
    records, head, cell = got
    assert (head["n_records"] <= records["n_psm"]).all() and (head["n_records"] == 0).any() and (head["n_records"] >= 3).any()
    assert (head["n_complete"] <= head["n_records"]).all() and (cell["n"] <= head["n_records"][:, None]).all()
    assert (cell["n_saturated"] <= cell["n"]).all()
    if complete_only:                                                                # (the matrix has no saturating reading in a row without a gap)
        assert (cell["n"] == head["n_complete"][:, None]).all()
    else:
        assert cell["n_saturated"].any()
    sums = ru.site_quant_sums(head, cell, p)                                         # (the table's records are the site quantification's)
    assert sums.shape == (records.size, n_ch) and np.isnan(sums[cell["n"] == 0]).all() and (sums[cell["n"] != 0] >= 0).all()


def test_known_answer_of_four_psms():
    """four PSMs of group 4, two channels, scale 2^2, list threshold 0.75, quant threshold 0.5 -- worked by hand:
    PSM 0 best_sig 0b101, min_prob min(0.9, 0.8) = 0.8, row 1 (1.3, NaN): contributes, not complete: channel 0 int(5.2) = 5.
    PSM 1 best_sig 0b101, min_prob min(0.7, 0.95) = 0.7, row 0 (2.5, 0.26): contributes, complete: 10 and int(1.04) = 1.
    PSM 2 best_sig 0b010, min_prob 0.4: in the list, not in the table.
    PSM 3 best_sig 0b010, min_prob 0.6, row -1: in the list, not in the table.
    list: (4, 0b010) n_psm 2, (4, 0b101) n_psm 2; table: row 0 all zero; row 1 n_records 2, n_complete 1, (15, 2, 0), (1, 1, 0)."""
    site_off = np.array([0, 3, 6, 9, 12], np.int64)
    sp = np.zeros(12, probs_ref.SITE_DTYPE)
    sp["with_prob"] = [0.9, 0.1, 0.8, 0.7, 0.2, 0.95, 0.3, 0.4, 0.1, 0.2, 0.6, 0.2]
    pp = np.zeros(4, probs_ref.PSM_DTYPE)
    pp["kind"], pp["z"] = pc.SCORED, [1.5, 1.25, 2.0, 1.0]
    r = dict(site_probs=sp, psm_probs=pp, site_off=site_off, best_sig=np.array([0b101, 0b101, 0b010, 0b010], np.uint64),
             ascores=np.array([[3.0, 7.0], [9.0, 2.0], [1.0, 0.0], [4.0, 0.0]], np.float32), group=np.array([4, 4, 4, 4], np.int32))
    values = np.array([[2.5, 0.26], [1.3, NAN]])
    row = np.array([1, 0, 0, -1], np.int32)
    p = ru.site_quant_params(threshold=0.5, scale_log2=2, n_channels=2)
    got, want = _both(r, values, row, p)
    pc.same(got, want, "known answer")
    records, head, cell = got
    assert records[["sig_bits", "group", "n_psm", "n_confident", "best_psm", "n_isomers"]].tolist() == [(0b010, 4, 2, 0, 3, 2), (0b101, 4, 2, 1, 0, 2)]
    assert head.tolist() == [(0, 0), (2, 1)] and cell.tolist() == [[(0, 0, 0), (0, 0, 0)], [(15, 2, 0), (1, 1, 0)]]
    only = _both(r, values, row, dict(p, complete_only=True))
    pc.same(*only, "known answer, complete only")
    assert only[0][1].tolist() == head.tolist() and only[0][2].tolist() == [[(0, 0, 0), (0, 0, 0)], [(10, 1, 0), (1, 1, 0)]]
    assert ru.site_quant_sums(head, cell, p)[1].tolist() == [3.75, 0.25]


def test_the_pair_is_a_function_of_the_multiset():
    n, n_ch, n_rows = 600, 18, 250
    r = pc.records(11, n)
    row = (np.arange(n) * 7 % (n_rows + 1) - 1).astype(np.int32)
    ids = (np.arange(n) * 3 + 5).astype(np.uint32)
    thr = pc.threshold(r, r["group"], row, n_rows)
    values = pc.matrix(5, n_rows, n_ch)
    p = ru.site_quant_params(threshold=thr, scale_log2=SCALE, n_channels=n_ch)
    whole, want = _both(r, values, row, p, psm_id=ids)
    pc.same(whole, want, "whole")
    perm = np.random.default_rng(1).permutation(n)
    pc.same(_both(pc.take(r, perm), values, row[perm], p, psm_id=ids[perm])[0], whole, "permuted")
    for n_chunks in (2, 7):                                                           # the pair fed forward as prev
        got = refd = None
        for part in np.array_split(perm, n_chunks):
            got, refd = _both(pc.take(r, part), values, row[part], p, psm_id=ids[part], prev=got)
        pc.same(got, whole, "%d chunks" % n_chunks)
        pc.same(refd, whole, "%d chunks, the yardstick" % n_chunks)
    a, b = perm[:260], perm[260:]
    first = _both(pc.take(r, a), values, row[a], p, psm_id=ids[a])[0]
    second = _both(pc.take(r, b), values, row[b], p, psm_id=ids[b])[0]
    assert first[1].tobytes() != whole[1].tobytes()[:first[1].nbytes]
    pc.same(ru.merge_peptidoform_quant(first, second), whole, "merged halves")
    pc.same(ru.merge_peptidoform_quant(second, first), whole, "merged halves, the other way round")
    pc.same(ref.reduce(first, second, n_ch), whole, "merged halves, the yardstick")
    pc.same(ru.merge_peptidoform_quant(whole), whole, "merge of one")
    # a NULL earlier table is an all-zero one; a record with n_psm == 0 is skipped and its row with it
    zero = (first[0], np.zeros_like(first[1]), np.zeros_like(first[2]))
    bare = _both(pc.take(r, b), values, row[b], p, psm_id=ids[b], prev=(first[0], None, None))
    pc.same(*bare, "prev without a table")
    pc.same(bare[0], _both(pc.take(r, b), values, row[b], p, psm_id=ids[b], prev=zero)[0], "prev with an all-zero table")
    dropped = tuple(x.copy() for x in first)
    dropped[0]["n_psm"][::3] = 0
    kept = tuple(x[dropped[0]["n_psm"] != 0] for x in dropped)
    pc.same(ru.merge_peptidoform_quant(dropped, second), ru.merge_peptidoform_quant(kept, second), "records without PSMs")
    pc.same(ru.merge_peptidoform_quant(dropped, second), ref.reduce(dropped, second, n_ch), "records without PSMs, the yardstick")
    for bad in ((), (whole, (whole[0], whole[1], whole[2][:, :17])), ((whole[0], None, None),), (whole, (whole[0], whole[1], None)),
                (whole, (whole[0][:-1], whole[1], whole[2]))):
        with pytest.raises(ValueError):
            ru.merge_peptidoform_quant(*bad)


def test_cap_gives_the_byte_prefix():
    n, n_ch = 400, 3
    r = pc.records(12, n)
    thr = pc.threshold(r, r["group"])
    values = pc.matrix(6, n, n_ch)
    p = ru.site_quant_params(threshold=thr, scale_log2=SCALE, n_channels=n_ch)
    whole, _ = _both(r, values, None, p)
    half = _both(pc.take(r, np.arange(200)), values, None, p)[0]
    m = whole[0].size
    for cap in (0, 1, m // 2, m - 1, m, m + 5):
        got, want = _both(r, values, None, p, cap=cap)
        pc.same(got, want, "cap %d" % cap)
        pc.same(got, tuple(x[:cap] for x in whole), "cap %d is a prefix" % cap)
        fed = _both(pc.take(r, np.arange(200, n)), values, np.arange(200, n), p, psm_base=200, prev=half, cap=cap)
        pc.same(*fed, "cap %d with prev" % cap)
        pc.same(fed[0], tuple(x[:cap] for x in whole), "cap %d with prev is a prefix" % cap)
        pc.same(ru.merge_peptidoform_quant(half, whole, cap=cap), ref.reduce(half, whole, n_ch, cap=cap), "merge, cap %d" % cap)


def _one_value(v, scale_log2, complete_only=False, other=1.0):
    """the cells of one contributing PSM whose row is (v, other)"""
    sp = np.zeros(1, probs_ref.SITE_DTYPE)
    sp["with_prob"] = 1.0
    pp = np.zeros(1, probs_ref.PSM_DTYPE)
    pp["kind"], pp["z"] = pc.SCORED, 1.0
    r = dict(site_probs=sp, psm_probs=pp, site_off=np.array([0, 1], np.int64), best_sig=np.array([1], np.uint64),
             ascores=np.array([[5.0]], np.float32), group=np.array([0], np.int32))
    p = ru.site_quant_params(threshold=0.75, scale_log2=scale_log2, n_channels=2, complete_only=complete_only)
    got, want = _both(r, np.array([[v, other]]), None, p)
    pc.same(got, want, "value %r" % v)
    return got[1].tolist()[0], got[2].tolist()[0]


@pytest.mark.parametrize("scale_log2", [-64, -3, 0, 10, 64])
def test_value_rule(scale_log2):
    """site quantification's, word for word: the same expectations as its own test"""
    other = (1 << 48, 1, 1) if scale_log2 >= 48 else (1 << scale_log2, 1, 0) if scale_log2 >= 0 else (0, 1, 0)
    for v in (NAN, 0.0, -0.0, -1.0, -INF, -5e-324):                                 # no reading
        assert _one_value(v, scale_log2) == ((1, 0), [(0, 0, 0), other])
        assert _one_value(v, scale_log2, complete_only=True) == ((1, 0), [(0, 0, 0), (0, 0, 0)])
    assert _one_value(INF, scale_log2) == ((1, 1), [(1 << 48, 1, 1), other])
    edge = 2.0 ** (48 - scale_log2)
    assert _one_value(edge, scale_log2) == ((1, 1), [(1 << 48, 1, 1), other])
    assert _one_value(np.nextafter(edge, 0.0), scale_log2) == ((1, 1), [((1 << 48) - 1, 1, 0), other])
    small = np.nextafter(2.0 ** -scale_log2, 0.0)                                   # below one quantum: q = 0, n counted
    assert _one_value(small, scale_log2) == ((1, 1), [(0, 1, 0), other])
    assert _one_value(7.75 * 2.0 ** -scale_log2, scale_log2, complete_only=True) == ((1, 1), [(7, 1, 0), other])


def test_a_row_out_of_range_is_reported_and_nothing_is_written():
    r = pc.records(13, 300)
    thr = pc.threshold(r, r["group"])
    values = pc.matrix(7, 300, 3)
    p = ru.site_quant_params(threshold=thr, scale_log2=SCALE, n_channels=3)
    who = [i for i, q, _ in pc.min_probs(r, r["group"]) if q >= thr]
    with pytest.raises(ValueError, match="row"):                                    # the library answers PYA_ERR_LIMIT
        _both(r, values[:who[-1]], None, p)
    with pytest.raises(ref.Outside):
        ref.pair(r["best_sig"], r["ascores"], r["site_off"], r["site_probs"], r["psm_probs"], r["group"], values[:who[-1]], None, 0.75, thr, SCALE)
    # a row outside on a PSM that does not contribute for another reason is left out silently, as is a negative row
    row = np.arange(300, dtype=np.int32)
    row[[i for i in range(300) if i not in who]] = 1 << 30
    row[who[0]] = -1
    got, want = _both(r, values, row, p)
    pc.same(got, want, "rows outside on PSMs that do not contribute")
    assert int(got[1]["n_records"].sum()) == len(who) - 1
    pc.same((got[0],), (_both(r, values, None, p)[0][0],), "the list does not depend on the rows")


def test_what_the_restatement_refuses():
    r = pc.records(14, 30)
    values = pc.matrix(8, 30, 2)
    p = ru.site_quant_params(threshold=0.5, n_channels=2)
    args = [r["site_probs"], r["psm_probs"], r["site_off"], r["best_sig"], r["ascores"], r["group"], values, None, p]
    ru.peptidoform_quant(*args)
    for at, bad in ((0, r["site_probs"][:-1]), (1, r["psm_probs"][:-1]), (3, r["best_sig"][:-1]), (4, r["ascores"][:-1]), (5, r["group"][:-1]),
                    (6, values[:, :1]), (6, values.reshape(-1)), (7, np.zeros(29, np.int32)), (8, dict(p, n_channels=3)), (8, dict(p, threshold=NAN))):
        with pytest.raises(ValueError):
            ru.peptidoform_quant(*(args[:at] + [bad] + args[at + 1:]))
    over = r["best_sig"].copy()
    over[np.flatnonzero((r["psm_probs"]["kind"] == pc.SCORED) & (r["group"] >= 0))[0]] |= np.uint64(1 << 63)
    with pytest.raises(ValueError, match="best_sig"):
        ru.peptidoform_quant(*(args[:3] + [over] + args[4:]))
    with pytest.raises(ValueError):
        ru.peptidoform_quant(*args, prev=(np.zeros(1, ru.PEPTIDOFORM_DTYPE), np.zeros(1, ru.SITE_QUANT_HEAD_DTYPE), np.zeros((1, 3), ru.SITE_QUANT_DTYPE)))


def test_score_batch_request_is_checked_before_anything_runs():
    from pyascore_amd.ascore import _quant_request
    values = np.arange(12.0).reshape(4, 3)
    q = _quant_request(dict(values=values, row=[0, 1, -1, 3, 2], threshold=0.9, scale_log2=4, complete_only=True), 5, True, "peptidoform_quant")
    assert q["params"] == dict(threshold=0.9, scale_log2=4, n_channels=3, complete_only=True) and q["row"].dtype == np.int32
    with pytest.raises(ValueError, match="peptidoforms="):                          # peptidoform_quant= without peptidoforms=
        _quant_request(dict(values=values), 5, False, "peptidoform_quant")
    with pytest.raises(ValueError, match="rollup="):                                # (quant= is as it was)
        _quant_request(dict(values=values), 5, False)
    for bad in (True, dict(), dict(values=None), dict(values=values, window=1), dict(values=values, row=[0, 1]), dict(values=np.zeros((2, 65))),
                dict(values=values, threshold=NAN)):
        with pytest.raises(ValueError):
            _quant_request(bad, 5, True, "peptidoform_quant")
    with pytest.raises(ValueError, match="peptidoform_quant: row"):                 # (the messages name the option)
        _quant_request(dict(values=values, row=[0, 1]), 5, True, "peptidoform_quant")


def test_header_and_bindings_declare_the_interface():
    text = open(os.path.join(ROOT, "include", "pyascore_hip.h")).read()
    assert re.search(r"#define\s+PYA_FLAG_PFORM_QUANT\s+32768u", text)
    assert "THE PAIR IS A FUNCTION OF THE MULTISET OF CONTRIBUTING TUPLES" in text and "ROW-ALIGNED" in text
    from pyascore_amd import build
    build.build()
    lib = _lib.load()
    names = ("pya_plan_peptidoform_quant", "pya_peptidoform_quant_reduce", "pya_peptidoform_quant_reduce_host", "pya_set_peptidoform_quant",
             "pya_last_batch_peptidoform_quant")
    for name in names:
        assert re.search(r"int\s+%s\s*\(" % name, text) and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert re.search(r"uint64_t\s+pya_peptidoform_quant_workspace_bytes\s*\(", text)
    assert _lib.PYA_FLAG_PFORM_QUANT == 32768
    for n in (0, 1, 1023, 1024, 1025, 100_000):
        for n_ch in (1, 64):
            assert lib.pya_peptidoform_quant_workspace_bytes(n, n_ch) >= lib.pya_peptidoform_workspace_bytes(n)
    params = ru.site_quant_c_params(ru.site_quant_params(n_channels=2))
    assert lib.pya_set_peptidoform_quant(None, None, 0, None, 0, C.byref(params)) == _lib.PYA_ERR_ARG       # no handle, no call
    assert lib.pya_last_batch_peptidoform_quant(None, None, None, 0, 2) == _lib.PYA_ERR_ARG
    csrc = os.path.join(ROOT, "pyascore_amd", "csrc")
    rule = open(os.path.join(csrc, "quant_rule.hip.h")).read()
    assert "281474976710656.0" in rule
    wave = open(os.path.join(csrc, "quant_wave.hip.h")).read()                      # the quantum rule exists once, and so does the
    assert '#include "quant_rule.hip.h"' in wave and "281474976710656" not in wave and "qr_quantum(" in wave   # wave reduce that applies it
    for name in ("site_quant.hip", "pform_quant.hip"):
        body = open(os.path.join(csrc, name)).read()
        assert '#include "quant_wave.hip.h"' in body and "281474976710656" not in body and "qw_reduce(" in body, name
        assert "qr_quantum(" not in body and "__ballot(" not in body, name


@pytest.mark.parametrize("n_mod", [None, 1])
def test_planted_reporters_summed_per_peptidoform_through_the_reference_core(n_mod):
    """End to end without a device, on the 120-PSM cfg2 batch of the site quantification's planted test: the peptides of the
    first 30 repeated against every spectrum, ten reporter peaks per spectrum, (10 + k) times its base peak; PepScores from the
    reference core, probabilities through tests/probs_ref.py, records from rollup.markers.  Every cfg2 peptide carries three
    modifications, so the comparison with the site table -- which speaks about sites all of whose peptidoforms are singly
    modified -- finds no such site there; the second case is the same batch made with one modification per peptide, where
    it must find some."""
    base, settings = synth.make_batch("cfg2", 120, seed=3, **({} if n_mod is None else dict(n_mod=n_mod)))
    tol, n, m, scale = 0.05, 120, 30 if n_mod is None else 12, 10           # (ten PSMs per peptide where one of three sites is modified)
    planted, pm, pz, want = mc.with_markers(base, tol)
    kws = [synth.unpack_psm(planted, i) for i in range(n)]
    psms = [dict(mz=kws[i]["mz_arr"], intensity=kws[i]["int_arr"], peptide=kws[i % m]["peptide"], n_of_mod=kws[i % m]["n_of_mod"],
                 max_charge=kws[i % m]["max_fragment_charge"]) for i in range(n)]
    batch = synth.pack_batch(psms)
    chk = harness.make_scorer(orc.OracleAscore, settings, kind=checker_kind())
    exp = harness.collect(chk, batch, synth.unpack_psm)
    site_off, site_probs, psm_probs = probs_ref.batch_records(settings, batch, exp, exp, synth.unpack_psm)
    names = [p["peptide"] for p in psms]
    group, _, gkeys = ru.peptide_groups(names)
    r = dict(site_probs=site_probs, psm_probs=psm_probs, site_off=site_off, best_sig=exp["best_sig"], ascores=exp["ascores"], group=group)
    rec, _ = ru.markers(batch["mz"], batch["intensity"], batch["peak_off"], mc.planted_params(tol), pm, pz)
    values = np.ascontiguousarray(ru.marker_matrix(rec)[:, :10])                    # the fixed targets: the ten reporters
    assert values.tobytes() == np.ascontiguousarray(want[:, :10]).tobytes()
    thr = pc.threshold(r, group)
    p = ru.site_quant_params(threshold=thr, scale_log2=scale, n_channels=10)
    got, yard = _both(r, values, None, p)
    pc.same(got, yard, "planted")
    records, head, cell = got
    assert not cell["n_saturated"].any() and (head["n_complete"] == head["n_records"]).all()
    mp = pc.min_probs(r, group)
    checked = 0
    for j in np.flatnonzero(head["n_records"]):
        key = (int(records["group"][j]), int(records["sig_bits"][j]))
        who = [i for i, q, k in mp if k == key and q >= thr]
        k = int(head["n_records"][j])
        assert len(who) == k and (cell["n"][j] == k).all()
        for c in range(10):
            # one truncation per PSM, each below one quantum: exact - k / 2^scale < sum <= exact
            exact = sum(Fraction(float(want[i, c])) for i in who)
            assert exact - Fraction(k, 1 << scale) < Fraction(int(cell["sum"][j, c]), 1 << scale) <= exact, (key, c)
        checked += 1
    assert checked >= (10 if n_mod is None else 5)
    # against the site table at the same threshold: a site all of whose peptidoforms are singly modified collects, per
    # peptidoform, the PSMs with with_prob(site) >= thr -- and for a singly modified PSM that IS min_prob >= thr; so the site's
    # PSMs are a subset of those of the peptide's peptidoforms, every quantum is non-negative, and the sums over all
    # peptidoforms of the peptide are never less than the site's
    slot, n_slots, skeys = ru.peptide_slots(names, site_off, residues=settings["mod_group"])
    s_head, s_cell = ru.site_quant(site_probs, psm_probs, site_off, exp["best_sig"], slot, n_slots, values, None, p)
    per_peptide = {}
    for j in range(records.size):
        per_peptide.setdefault(int(records["group"][j]), []).append(j)
    compared = 0
    for s in np.flatnonzero(s_head["n_records"]):
        g = gkeys.index(skeys[s][0])
        rows = per_peptide[g]
        if any(bin(int(records["sig_bits"][j])).count("1") != 1 for j in rows):
            continue
        total = cell["sum"][rows].astype(object).sum(axis=0)
        assert all(int(total[c]) >= int(s_cell["sum"][s, c]) for c in range(10)), skeys[s]
        compared += 1
    assert compared >= 5 if n_mod == 1 else (base["n_of_mod"] > 1).all()


def test_command_line_options_and_fields(tmp_path):
    from pyascore_amd import batch_cli
    from pyascore_amd.__main__ import parse_args, peptidoform_quant_request
    files = ["spec.mzML", "ident.pepXML", "out.tsv"]
    assert peptidoform_quant_request(parse_args(files)) is None
    args = parse_args(["--marker_mz", "126.5,127.5", "--peptidoform_quant", "q.tsv", "--peptidoform_quant_threshold", "0.9",
                       "--peptidoform_quant_scale", "4", "--peptidoform_quant_complete"] + files)
    assert peptidoform_quant_request(args) == dict(threshold=0.9, scale_log2=4, complete_only=True)
    assert peptidoform_quant_request(parse_args(["--marker_mz", "126.5", "--peptidoform_quant", "q.tsv"] + files)) == \
        dict(threshold=0.75, scale_log2=10, complete_only=False)
    for bad in (["--peptidoform_quant", "q.tsv"], ["--peptidoform_quant", "q.tsv", "--marker_losses", "98.0"],
                ["--peptidoform_quant", "q.tsv", "--marker_mz", "126.5", "--peptidoform_quant_scale", "65"]):
        with pytest.raises(ValueError, match="marker|scale"):
            parse_args(bad + files)
    cols = batch_cli.peptidoform_quant_columns((126.5, 127.5))
    assert cols[:len(batch_cli.PEPTIDOFORM_TABLE_COLUMNS)] == tuple(batch_cli.PEPTIDOFORM_TABLE_COLUMNS)
    assert cols[len(batch_cli.PEPTIDOFORM_TABLE_COLUMNS):] == ("Records", "Complete", "mz126.5", "mz127.5")


@pytest.mark.parametrize("seed,n,share,rows", [(9810, 300, 5, "psm"), (9811, 300, 5, "fewer"), (9840, 400, 5, "psm")])
def test_the_seeds_of_the_gpu_tests_meet_the_coverage_conditions(seed, n, share, rows):
    """what tests/test_gpu_peptidoform_quant.py asserts of its seeded cfg2 batches on the device, confirmed here through the
    reference core (the repeated goldens are confirmed by test_golden_cases_equal_the_yardstick above)"""
    batch, settings = synth.make_batch("cfg2", n_psm=n, seed=seed)
    batch, names = pc.repeats(batch, share=share)
    group, _, _ = ru.peptide_groups(names)
    r = _rescored(settings, batch)
    row = None if rows == "psm" else (np.arange(n) % (n // 2 + 1) - 1).astype(np.int32)
    pc.threshold(r, group, row, None if row is None else n // 2)


def test_the_shared_and_chunked_inputs_of_the_gpu_tests_meet_the_coverage_conditions():
    """... and of its shared batch (seed 9850, in and out of spectrum order) and its chunked batch (seed 9860, 7 000 PSMs with
    fewer rows than PSMs)"""
    settings, spectra, psms, _, _ = pc.shared_inputs()
    for what, order in pc.SHARED_ORDERS:
        mine = [psms[q] for q in order]
        flat = synth.expand_shared_batch(synth.pack_shared_batch(spectra, mine))
        group, _, _ = ru.peptide_groups([q["peptide"] for q in mine])
        pc.threshold(_rescored(settings, flat), group)
    settings, big, names, row = pc.chunked_inputs()
    group, _, _ = ru.peptide_groups(names)
    pc.threshold(_rescored(settings, big), group, row, pc.CHUNKED_ROWS)
