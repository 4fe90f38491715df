"""Site quantification on the host (include/pyascore_hip.h: pya_site_quant): the numpy restatement pyascore_amd.rollup.site_quant
against the plain-Python yardstick tests/site_quant_ref.py, byte for byte; the multiset property; the value rule; what is
refused; and planted reporter intensities recovered through the reference core's PepScores.  No GPU."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import markers_cases as mc
import probs_ref
import site_quant_ref as ref
from conftest import ROOT, checker_kind
from oracle import harness, orc
from pyascore_amd import _lib, rollup as ru, synth

NAN, INF = float("nan"), float("inf")
SCORED, NONE, OVER = _lib.PYA_SITE_SCORED, _lib.PYA_SITE_NONE, _lib.PYA_SITE_OVER


def _same(got, want, what):
    for g, w, name in zip(got, want, ("head", "cell")):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        assert g.tobytes() == w.tobytes(), "%s: %s differs at %s" % (what, name, np.argwhere(g != w)[:4].tolist())


def _records(seed, n_psm, n_ch, n_slots, n_rows, thr):
    """a random record set made directly, with everything the rule names"""
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, 7, n_psm)
    site_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    n_rec = int(site_off[-1])
    psm_probs = np.zeros(n_psm, probs_ref.PSM_DTYPE)
    psm_probs["kind"] = rng.choice([SCORED, SCORED, SCORED, SCORED, NONE, OVER], n_psm)
    site_probs = np.zeros(n_rec, probs_ref.SITE_DTYPE)
    site_probs["with_prob"] = rng.choice([0.0, 1.0, thr, np.nextafter(thr, 0.0), np.nextafter(thr, 1.0)], n_rec)
    mix = rng.random(n_rec) < 0.6
    site_probs["with_prob"][mix] = rng.random(int(mix.sum()))
    site_probs["with_prob"][rng.random(n_rec) < 0.02] = -1.0                        # (what an OVER PSM's records hold)
    best_sig = np.array([int(rng.integers(0, 1 << int(c))) if c else 0 for c in counts], np.uint64)
    best_sig[rng.random(n_psm) < 0.1] |= np.uint64(1 << 63)                          # (a bit no record has)
    slot = rng.integers(-2, n_slots + 2, n_rec).astype(np.int32)
    for i in np.flatnonzero(counts >= 2):                                            # two records of one PSM on one slot
        if rng.random() < 0.5:
            slot[site_off[i] + 1] = slot[site_off[i]]
    row = rng.integers(-2, n_rows + 2, n_psm).astype(np.int32)
    values = rng.random((n_rows, n_ch)) * 10.0 ** rng.integers(-6, 9, (n_rows, n_ch))
    kind = rng.random((n_rows, n_ch))
    whole = rng.random(n_rows) < 0.4                                                 # rows with a reading in every channel
    kind[whole] = 0.2 + 0.8 * kind[whole]
    values[kind < 0.08] = NAN
    values[(kind >= 0.08) & (kind < 0.14)] = 0.0
    values[(kind >= 0.14) & (kind < 0.17)] = -0.0
    values[(kind >= 0.17) & (kind < 0.20)] = -3.5
    values[(kind >= 0.20) & (kind < 0.22)] = INF
    values[(kind >= 0.22) & (kind < 0.24)] = 1e300
    return dict(site_probs=site_probs, psm_probs=psm_probs, site_off=site_off, best_sig=best_sig, slot=slot, values=values, row=row)


def _would_contribute(r, thr):
    """records that meet every condition but the two ranges"""
    owner = np.repeat(np.arange(r["row"].size), np.diff(r["site_off"]))
    k = np.arange(owner.size) - r["site_off"][owner]
    in_best = np.array([(int(r["best_sig"][p]) >> int(j)) & 1 for p, j in zip(owner, k)], bool)
    return (r["slot"] >= 0) & (r["psm_probs"]["kind"][owner] == SCORED) & in_best & (r["site_probs"]["with_prob"] >= thr) & (r["row"][owner] >= 0), owner


def _both(r, n_slots, p, into=None):
    got = ru.site_quant(r["site_probs"], r["psm_probs"], r["site_off"], r["best_sig"], r["slot"], n_slots, r["values"], r["row"], p, into=into)
    want = ref.table(r["site_probs"], r["psm_probs"], r["site_off"], r["best_sig"], r["slot"], n_slots, r["values"], r["row"], p["threshold"],
                     p["scale_log2"], p["complete_only"], into=into)
    return got, want


@pytest.mark.parametrize("n_ch", [1, 18, 63, 64])
@pytest.mark.parametrize("complete_only", [False, True])
def test_restatement_equals_the_yardstick_on_random_records(n_ch, complete_only):
    n_slots, n_rows, thr = 23, 31, 0.4
    p = ru.site_quant_params(threshold=thr, scale_log2=7, n_channels=n_ch, complete_only=complete_only)
    r = _records(100 + n_ch, 900, n_ch, n_slots, n_rows, thr)
    cand, owner = _would_contribute(r, thr)
    outside = cand & ((r["slot"] >= n_slots) | (r["row"][owner] >= n_rows))
    assert outside.any() and (cand & ~outside).sum() > 100
    with pytest.raises(ValueError):                                                  # the library answers PYA_ERR_LIMIT
        ru.site_quant(r["site_probs"], r["psm_probs"], r["site_off"], r["best_sig"], r["slot"], n_slots, r["values"], r["row"], p)
    with pytest.raises(ref.Outside):
        ref.table(r["site_probs"], r["psm_probs"], r["site_off"], r["best_sig"], r["slot"], n_slots, r["values"], r["row"], thr, 7, complete_only)
    r["slot"][outside] = -1
    # slots and rows outside remain, on records that do not contribute for another reason: they are left out silently
    assert ((r["slot"] >= n_slots) & ~cand).any() and ((r["row"][owner] >= n_rows) & ~cand).any()
    got, want = _both(r, n_slots, p)
    _same(got, want, "%d channels" % n_ch)
    head, cell = got
    assert head["n_records"].sum() == int((cand & ~outside).sum()) and (head["n_complete"] <= head["n_records"]).all()
    assert cell["n_saturated"].any() and (cell["n_saturated"] <= cell["n"]).all() and (cell["n"] <= head["n_records"][:, None]).all()
    if complete_only:
        assert (cell["n"] == head["n_complete"][:, None]).all()
    if n_ch == 1:
        assert head["n_complete"].any() and (head["n_complete"] < head["n_records"]).any()
    sums = ru.site_quant_sums(head, cell, p)
    assert sums.shape == (n_slots, n_ch) and np.isnan(sums[cell["n"] == 0]).all() and (sums[cell["n"] != 0] >= 0).all()


def test_known_answer_of_five_records():
    """three PSMs, five records, two slots, two channels, scale 2^2, threshold 0.5 -- worked by hand:
    PSM 0 (row 1: 1.3, NaN)  records 0, 1, best_sig 0b01: record 0 (p 0.9, slot 0) contributes; record 1 is not in best.
    PSM 1 (row 0: 2.5, 0.26) records 2, 3, best_sig 0b11: record 2 (p 0.5, slot 0) and record 3 (p 0.7, slot 1) contribute.
    PSM 2 (row 0)            record 4, best_sig 0b1, p 0.49: below the threshold.
    slot 0: records 0 and 2: n_records 2, n_complete 1; channel 0: int(5.2) + int(10.0) = 15, n 2; channel 1: int(1.04) = 1, n 1.
    slot 1: record 3: n_records 1, n_complete 1; channel 0: 10, n 1; channel 1: 1, n 1."""
    site_off = np.array([0, 2, 4, 5], np.int64)
    site_probs = np.zeros(5, probs_ref.SITE_DTYPE)
    site_probs["with_prob"] = [0.9, 0.95, 0.5, 0.7, 0.49]
    psm_probs = np.zeros(3, probs_ref.PSM_DTYPE)
    psm_probs["kind"] = SCORED
    best_sig = np.array([0b01, 0b11, 0b1], np.uint64)
    slot = np.array([0, 1, 0, 1, 1], np.int32)
    values = np.array([[2.5, 0.26], [1.3, NAN]])
    row = np.array([1, 0, 0], np.int32)
    p = ru.site_quant_params(threshold=0.5, scale_log2=2, n_channels=2)
    head, cell = ru.site_quant(site_probs, psm_probs, site_off, best_sig, slot, 2, values, row, p)
    assert head.tolist() == [(2, 1), (1, 1)]
    assert cell.tolist() == [[(15, 2, 0), (1, 1, 0)], [(10, 1, 0), (1, 1, 0)]]
    _same((head, cell), ref.table(site_probs, psm_probs, site_off, best_sig, slot, 2, values, row, 0.5, 2), "known answer")
    assert ru.site_quant_sums(head, cell, p).tolist() == [[3.75, 0.25], [2.5, 0.25]]
    only = ru.site_quant(site_probs, psm_probs, site_off, best_sig, slot, 2, values, row, dict(p, complete_only=True))
    assert only[0].tolist() == head.tolist() and only[1].tolist() == [[(10, 1, 0), (1, 1, 0)], [(10, 1, 0), (1, 1, 0)]]
    assert ru.site_quant(site_probs, psm_probs, site_off, best_sig, slot, 2, values, None, p)[1].tolist() == \
        [[(15, 2, 0), (1, 1, 0)], [(5, 1, 0), (0, 0, 0)]]                          # row None: PSM i has row i


def _take(r, psms):
    """the record set of the PSMs `psms`, in that order"""
    psms = np.asarray(psms, np.int64)
    n_rec = np.diff(r["site_off"])[psms]
    off = np.concatenate([[0], np.cumsum(n_rec)]).astype(np.int64)
    take = np.repeat(r["site_off"][:-1][psms] - off[:-1], n_rec) + np.arange(int(n_rec.sum()))
    return dict(site_probs=r["site_probs"][take], psm_probs=r["psm_probs"][psms], site_off=off, best_sig=r["best_sig"][psms],
                slot=r["slot"][take], values=r["values"], row=r["row"][psms])


def test_the_table_is_a_function_of_the_multiset():
    n_slots, n_rows, thr = 9, 40, 0.3
    p = ru.site_quant_params(threshold=thr, scale_log2=10, n_channels=18)
    r = _records(7, 300, 18, n_slots, n_rows, thr)
    r["slot"] = np.clip(r["slot"], -1, n_slots - 1).astype(np.int32)
    r["row"] = np.clip(r["row"], -1, n_rows - 1).astype(np.int32)
    whole, want = _both(r, n_slots, p)
    _same(whole, want, "whole")
    assert (whole[0]["n_records"] >= 5).all()
    perm = np.random.default_rng(1).permutation(300)
    _same(_both(_take(r, perm), n_slots, p)[0], whole, "permuted")
    a, b = _take(r, perm[:130]), _take(r, perm[130:])
    first, _ = _both(a, n_slots, p)
    second, second_ref = _both(b, n_slots, p, into=first)
    _same(second, whole, "two calls with into=")
    _same(second_ref, whole, "the yardstick, two calls")
    assert first[0].tobytes() != whole[0].tobytes()                                 # (into= is copied, not written)
    _same(ru.merge_site_quant(first, _both(b, n_slots, p)[0]), whole, "merged halves")
    _same(ru.merge_site_quant(whole), whole, "merge of one")
    _same(ru.merge_site_quant(ru.empty_site_quant(n_slots, 18), whole), whole, "the empty table is the neutral element")
    for bad in ((), (whole, ru.empty_site_quant(n_slots, 17)), (whole, ru.empty_site_quant(n_slots + 1, 18))):
        with pytest.raises(ValueError):
            ru.merge_site_quant(*bad)


def _one_value(v, scale_log2, complete_only=False, other=1.0):
    """the cells of one contributing record whose row is (v, other)"""
    site_probs = np.zeros(1, probs_ref.SITE_DTYPE)
    site_probs["with_prob"] = 1.0
    psm_probs = np.zeros(1, probs_ref.PSM_DTYPE)
    psm_probs["kind"] = SCORED
    p = ru.site_quant_params(threshold=0.75, scale_log2=scale_log2, n_channels=2, complete_only=complete_only)
    args = (site_probs, psm_probs, np.array([0, 1], np.int64), np.array([1], np.uint64), np.array([0], np.int32), 1, np.array([[v, other]]), None)
    got = ru.site_quant(*args, p)
    _same(got, ref.table(*args, 0.75, scale_log2, complete_only), "value %r" % v)
    return got[0].tolist()[0], got[1].tolist()[0]


@pytest.mark.parametrize("scale_log2", [-64, -3, 0, 10, 64])
def test_value_rule(scale_log2):
    # the second channel holds 1.0: 2^scale_log2 quanta, none below 2^0 and saturated from 2^48 on
    other = (1 << 48, 1, 1) if scale_log2 >= 48 else (1 << scale_log2, 1, 0) if scale_log2 >= 0 else (0, 1, 0)
    for v in (NAN, 0.0, -0.0, -1.0, -INF, -5e-324):                                 # no reading
        assert _one_value(v, scale_log2) == ((1, 0), [(0, 0, 0), other])
        assert _one_value(v, scale_log2, complete_only=True) == ((1, 0), [(0, 0, 0), (0, 0, 0)])
    assert _one_value(INF, scale_log2) == ((1, 1), [(1 << 48, 1, 1), other])
    edge = 2.0 ** (48 - scale_log2)
    assert _one_value(edge, scale_log2) == ((1, 1), [(1 << 48, 1, 1), other])
    assert _one_value(np.nextafter(edge, INF), scale_log2) == ((1, 1), [(1 << 48, 1, 1), other])
    assert _one_value(np.nextafter(edge, 0.0), scale_log2) == ((1, 1), [((1 << 48) - 1, 1, 0), other])
    assert _one_value(1.5 * edge / 4.0, scale_log2) == ((1, 1), [(3 << 45, 1, 0), other])
    small = np.nextafter(2.0 ** -scale_log2, 0.0)                                   # below one quantum: q = 0, n counted
    assert _one_value(small, scale_log2) == ((1, 1), [(0, 1, 0), other])
    assert _one_value(2.0 ** -scale_log2, scale_log2) == ((1, 1), [(1, 1, 0), other])
    assert _one_value(5e-324, scale_log2) == ((1, 1), [(0, 1, 0), other])
    assert _one_value(7.75 * 2.0 ** -scale_log2, scale_log2, complete_only=True) == ((1, 1), [(7, 1, 0), other])


def test_params_and_their_faults():
    assert ru.site_quant_params(n_channels=10) == dict(threshold=0.75, scale_log2=10, n_channels=10, complete_only=False)
    assert ru.check_site_quant_params(dict(threshold=1, scale_log2=np.int64(-64), n_channels=64.0, complete_only=np.True_)) == \
        dict(threshold=1.0, scale_log2=-64, n_channels=64, complete_only=True)
    assert ru.site_quant_params(threshold=-INF, n_channels=1)["threshold"] == -INF
    good = ru.site_quant_params(n_channels=3)
    for bad in (dict(good, threshold=NAN), dict(good, threshold="x"), dict(good, threshold=None), dict(good, scale_log2=65), dict(good, scale_log2=-65),
                dict(good, scale_log2=1.5), dict(good, scale_log2=True), dict(good, scale_log2=None), dict(good, n_channels=0),
                dict(good, n_channels=65), dict(good, n_channels=2.5), dict(good, n_channels="3x"), dict(good, complete_only=1),
                dict(good, complete_only=None), {k: v for k, v in good.items() if k != "threshold"}, None, 3):
        with pytest.raises(ValueError):
            ru.check_site_quant_params(bad)
    with pytest.raises(ValueError):
        ru.site_quant_params()                                                      # n_channels has no default
    c = ru.site_quant_c_params(dict(good, complete_only=True, scale_log2=-7))
    assert (c.threshold, c.scale_log2, c.n_channels, c.flags, c.reserved) == (0.75, -7, 3, _lib.PYA_QUANT_COMPLETE_ONLY, 0)
    assert C.sizeof(c) == 24 and ru.SITE_QUANT_HEAD_DTYPE.itemsize == 8 and ru.SITE_QUANT_DTYPE.itemsize == 16
    assert ru.SITE_QUANT_DTYPE.fields["n"][1] == 8 and ru.SITE_QUANT_DTYPE.fields["n_saturated"][1] == 12


def test_what_the_restatement_refuses():
    r = _records(3, 20, 2, 5, 6, 0.5)
    p = ru.site_quant_params(threshold=2.0, n_channels=2)                           # (nothing contributes: nothing is outside)
    args = [r["site_probs"], r["psm_probs"], r["site_off"], r["best_sig"], r["slot"], 5, r["values"], r["row"], p]
    assert not ru.site_quant(*args)[0]["n_records"].any()
    for at, bad in ((0, r["site_probs"][:-1]), (1, r["psm_probs"][:-1]), (3, r["best_sig"][:-1]), (4, r["slot"][:-1]), (6, r["values"][:, :1]),
                    (6, r["values"].reshape(-1)), (7, r["row"][:-1]), (8, dict(p, n_channels=3))):
        with pytest.raises(ValueError):
            ru.site_quant(*(args[:at] + [bad] + args[at + 1:]))
    with pytest.raises(ValueError):
        ru.site_quant(*args, into=ru.empty_site_quant(4, 2))


def test_score_batch_request_is_checked_before_anything_runs():
    from pyascore_amd.ascore import _quant_request
    values = np.arange(12.0).reshape(4, 3)
    q = _quant_request(dict(values=values, row=[0, 1, -1, 3, 2], threshold=0.9, scale_log2=4, complete_only=True), 5, True)
    assert q["params"] == dict(threshold=0.9, scale_log2=4, n_channels=3, complete_only=True) and q["row"].dtype == np.int32
    assert q["values"].flags["C_CONTIGUOUS"] and q["c_params"].n_channels == 3
    assert _quant_request(dict(values=values.astype(np.float32)), 5, True)["params"] == ru.site_quant_params(n_channels=3)
    with pytest.raises(ValueError, match="rollup="):                                # score_batch(quant=) without rollup=
        _quant_request(dict(values=values), 5, False)
    for bad in (True, dict(), dict(values=None), dict(values=values, window=1), dict(values=values.reshape(-1)), dict(values=values, row=[0, 1]),
                dict(values=values, row=[0.0] * 5), dict(values=values, row=[1 << 31] * 5), dict(values=values, scale_log2=99),
                dict(values=values[:, :0]), dict(values=np.zeros((2, 65))), dict(values=values, threshold=NAN), dict(values="x")):
        with pytest.raises(ValueError):
            _quant_request(bad, 5, True)


def test_header_and_bindings_declare_the_interface():
    text = open(os.path.join(ROOT, "include", "pyascore_hip.h")).read()
    assert re.search(r"#define\s+PYA_FLAG_QUANT\s+16384u", text) and re.search(r"#define\s+PYA_QUANT_COMPLETE_ONLY\s+1u", text)
    for name in ("pya_site_quant_params", "pya_site_quant_head", "pya_site_quant"):
        assert re.search(r"typedef struct %s \{" % name, text), name
    assert "THE TABLE IS A FUNCTION OF THE MULTISET OF CONTRIBUTING RECORDS (slot, the row's values)" in text
    assert "MERGE BY ADDING EVERY FIELD" in text and "65 535 contributing records" in text
    from pyascore_amd import build, device
    build.build()
    lib = _lib.load()
    names = ("pya_plan_site_quant", "pya_set_site_quant", "pya_last_batch_site_quant", "pya_marker_values")
    for name in names:
        assert re.search(r"int\s+%s\s*\(" % name, text) and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert _lib.PYA_FLAG_QUANT == 16384
    params = ru.site_quant_c_params(ru.site_quant_params(n_channels=2))
    assert lib.pya_set_site_quant(None, None, 0, None, 0, C.byref(params)) == _lib.PYA_ERR_ARG       # no handle, no call
    assert lib.pya_last_batch_site_quant(None, None, None, 0, 2) == _lib.PYA_ERR_ARG
    assert lib.pya_marker_values(None, None, 0, 1, 1, None, None) == _lib.PYA_ERR_ARG
    assert lib.pya_plan_site_quant(None, None, None, None, None, None, 0, None, 0, None, 0, C.byref(params), None, None) == _lib.PYA_ERR_ARG
    head, cell = device.site_quant_records((np.arange(16, dtype=np.uint8).reshape(2, 8), np.arange(96, dtype=np.uint8).reshape(2, 3, 16)))
    assert head.shape == (2,) and cell.shape == (2, 3) and head.dtype == ru.SITE_QUANT_HEAD_DTYPE and cell.dtype == ru.SITE_QUANT_DTYPE
    assert head["n_complete"][1] == int.from_bytes(bytes(range(12, 16)), "little")
    assert cell["n_saturated"][1, 2] == int.from_bytes(bytes(range(92, 96)), "little")
    with pytest.raises(ValueError):
        device.site_quant_records((np.zeros((2, 8), np.uint8), np.zeros((3, 3, 16), np.uint8)))


def test_planted_reporters_summed_per_site_through_the_reference_core():
    """End to end without a device: the 120 cfg2 PSMs of the marker stage's planting, the peptides of the first 30 repeated
    against every spectrum so that four PSMs share a slot; ten reporter peaks per spectrum, (10 + k) times its base peak;
    PepScores from the reference core, probabilities through tests/probs_ref.py, records from rollup.markers."""
    base, settings = synth.make_batch("cfg2", 120, seed=3)
    tol, n, m, scale = 0.05, 120, 30, 10
    planted, pm, pz, want = mc.with_markers(base, tol)
    kws = [synth.unpack_psm(planted, i) for i in range(n)]
    psms = [dict(mz=kws[i]["mz_arr"], intensity=kws[i]["int_arr"], peptide=kws[i % m]["peptide"], n_of_mod=kws[i % m]["n_of_mod"],
                 max_charge=kws[i % m]["max_fragment_charge"]) for i in range(n)]
    batch = synth.pack_batch(psms)
    assert batch["mz"].tobytes() == np.asarray(planted["mz"], np.float64).tobytes()
    chk = harness.make_scorer(orc.OracleAscore, settings, kind=checker_kind())
    exp = harness.collect(chk, batch, synth.unpack_psm)
    site_off, site_probs, psm_probs = probs_ref.batch_records(settings, batch, exp, exp, synth.unpack_psm)
    slot, n_slots, keys = ru.peptide_slots([p["peptide"] for p in psms], site_off, residues=settings["mod_group"])
    rec, _ = ru.markers(batch["mz"], batch["intensity"], batch["peak_off"], mc.planted_params(tol), pm, pz)
    values = np.ascontiguousarray(ru.marker_matrix(rec)[:, :10])                    # the fixed targets: the ten reporters
    assert values.tobytes() == np.ascontiguousarray(want[:, :10]).tobytes()
    in_best = np.array([(int(exp["best_sig"][i]) >> r) & 1 for i in range(n) for r in range(int(site_off[i + 1] - site_off[i]))], bool)
    thr = float(np.median(site_probs["with_prob"][in_best]))
    p = ru.site_quant_params(threshold=thr, scale_log2=scale, n_channels=10)
    head, cell = ru.site_quant(site_probs, psm_probs, site_off, exp["best_sig"], slot, n_slots, values, None, p)
    _same((head, cell), ref.table(site_probs, psm_probs, site_off, exp["best_sig"], slot, n_slots, values, None, thr, scale), "planted")
    assert (head["n_records"] >= 3).any() and not cell["n_saturated"].any() and (head["n_complete"] == head["n_records"]).all()
    owner = np.repeat(np.arange(n), np.diff(site_off))
    contributes = in_best & (site_probs["with_prob"] >= thr)
    assert 0.25 * in_best.sum() <= contributes.sum() <= 0.75 * in_best.sum() + 1
    checked = 0
    for s in np.flatnonzero(head["n_records"]):
        who = owner[contributes & (slot == s)]
        k = int(head["n_records"][s])
        assert who.size == k and (cell["n"][s] == k).all()
        exact = [sum(Fraction(float(want[i, c])) for i in who) for c in range(10)]
        for c in range(10):
            # one truncation per record, each below one quantum: exact - k / 2^scale < sum <= exact
            got = Fraction(int(cell["sum"][s, c]), 1 << scale)
            assert exact[c] - Fraction(k, 1 << scale) < got <= exact[c], (keys[s], c)
        # the ratios follow: planted[c] / planted[0] is (10 + c) / 10 up to a rounding of each product, the sums are off by
        # less than k quanta each, so the ratio of the sums is off by less than (k / 2^scale) (1 + ratio) / sum[0] + 2^-50
        sums = ru.site_quant_sums(head, cell, p)[s]
        for c in range(1, 10):
            ratio = (10.0 + c) / 10.0
            assert abs(sums[c] / sums[0] - ratio) <= (k / 2.0 ** scale) * (1.0 + ratio) / sums[0] + 2.0 ** -50, (keys[s], c)
        checked += 1
    assert checked >= 10


def test_command_line_options_and_fields(tmp_path):
    from pyascore_amd import batch_cli
    from pyascore_amd.__main__ import markers_request, parse_args, site_quant_request
    files = ["spec.mzML", "ident.pepXML", "out.tsv"]
    assert site_quant_request(parse_args(files)) is None and markers_request(parse_args(files)) is None
    args = parse_args(["--site_table", "sites.tsv", "--marker_mz", "126.5,127.5", "--site_quant", "q.tsv", "--site_quant_threshold", "0.9",
                       "--site_quant_scale", "4", "--site_quant_complete"] + files)
    assert site_quant_request(args) == dict(threshold=0.9, scale_log2=4, complete_only=True)
    assert markers_request(args)["mz"] == (126.5, 127.5)                        # the targets are read without --markers FILE
    assert site_quant_request(parse_args(["--site_table", "s.tsv", "--marker_mz", "126.5", "--site_quant", "q.tsv"] + files)) == \
        dict(threshold=0.75, scale_log2=10, complete_only=False)
    for bad in (["--site_quant", "q.tsv"], ["--site_quant", "q.tsv", "--site_table", "s.tsv"], ["--site_quant", "q.tsv", "--marker_mz", "126.5"],
                ["--site_quant", "q.tsv", "--site_table", "s.tsv", "--marker_losses", "98.0"],
                ["--site_quant", "q.tsv", "--site_table", "s.tsv", "--marker_mz", "126.5", "--site_quant_scale", "65"]):
        with pytest.raises(ValueError):
            parse_args(bad + files)
    assert batch_cli.site_quant_columns((126.5, 127.5)) == ("Peptide", "Position", "Residue", "Records", "Complete", "mz126.5", "mz127.5")
    head = np.zeros(1, ru.SITE_QUANT_HEAD_DTYPE)
    head["n_records"], head["n_complete"] = 3, 2
    row = batch_cli.site_quant_fields(("PEPSTIDE", 4), head[0], np.array([1.5, NAN]))
    assert row == ["PEPSTIDE", "4", "S", "3", "2", "1.5", ""]
    path = tmp_path / "q.tsv"
    batch_cli.write_site_quant_tsv([row], str(path), mz=(126.5, 127.5))
    assert path.read_text() == "Peptide\tPosition\tResidue\tRecords\tComplete\tmz126.5\tmz127.5\nPEPSTIDE\t4\tS\t3\t2\t1.5\t\n"
    for bad in (dict(site_quant=dict(threshold=0.5), site_quant_rows=None, site_table=[], markers=dict(mz=(1.0,)), marker_rows=[]),
                dict(site_quant=dict(threshold=0.5), site_quant_rows=[], markers=dict(mz=(1.0,)), marker_rows=[]),
                dict(site_quant=dict(threshold=0.5), site_quant_rows=[], site_table=[]),
                dict(site_quant=dict(threshold=0.5), site_quant_rows=[], site_table=[], markers=dict(losses=(1.0,)), marker_rows=[]),
                dict(site_quant=dict(values=3), site_quant_rows=[], site_table=[], markers=dict(mz=(1.0,)), marker_rows=[]),
                dict(site_quant=dict(scale_log2=99), site_quant_rows=[], site_table=[], markers=dict(mz=(1.0,)), marker_rows=[])):
        with pytest.raises(ValueError):
            batch_cli.localize(None, [], {}, "STY", 79.966331, **bad)
