"""The host side of deisotoping (pya_deisotope_params): the numpy restatement pyascore_amd.rollup.deisotope on hand-made spectra
whose outcome is written out by hand (tests/deisotope_cases.py), its properties on dense spectra, what satellites cost and what
the rule gives back with the reference core as the scorer, and the public surface (header, bindings, argument checks).  No GPU."""
import os
import re

import numpy as np
import pytest

import deisotope_cases as dc
from conftest import checker_kind
from oracle import harness, orc
from pyascore_amd import _lib, rollup as ru, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = dc.hand_cases()


# ---- the rule, one case each ----

@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hand_made_spectrum(case):
    x, y = case["mz"], case["intensity"]
    mz, it, off, keep = ru.deisotope(x, y, [0, x.size], case["params"])
    assert keep.tolist() == case["keep"].tolist()
    assert mz.dtype == x.dtype and it.dtype == y.dtype
    assert mz.tobytes() == x[case["keep"]].tobytes() and it.tobytes() == y[case["keep"]].tobytes()
    assert off.dtype == np.int64 and off.tolist() == [0, int(case["keep"].sum())]


def test_the_exact_edges_are_exact():
    """the construction behind the tolerance cases: x[j] - x[i] - spacing has no rounding, so fabs(e) == tol is hit"""
    p = dc.P_EXACT
    for base, sp in ((100.0, p["spacing"][0]), (300.0, p["spacing"][1])):
        for t in (np.float64, np.float32):
            for side in (1.0, -1.0):
                x = float(t(base + sp + side * dc.TOL_EXACT))
                assert x == base + sp + side * dc.TOL_EXACT and abs((x - base) - sp) == p["tol"]


def test_unordered_spectra_come_back_unchanged_among_others():
    """a descending pair or a NaN m/z: that spectrum keeps every peak, its neighbours are filtered as if it were not there"""
    good = [c for c in CASES if not c["unordered"] and c["params"] is dc.P0 and c["mz"].dtype == np.float64]
    bad = [c for c in CASES if c["unordered"]]
    assert len(bad) == 3 and len(good) > 10
    order = good[:3] + bad[:1] + good[3:6] + bad[1:] + good[6:]
    mz, it, off = dc.pack([(c["mz"], c["intensity"]) for c in order], gaps=False)
    want = np.concatenate([c["keep"] for c in order])
    f_mz, f_it, f_off, keep = ru.deisotope(mz, it, off, dc.P0)
    assert keep.tolist() == want.tolist()
    assert f_off.tolist() == np.concatenate([[0], np.cumsum([int(c["keep"].sum()) for c in order])]).tolist()
    assert f_mz.tobytes() == mz[want].tobytes() and f_it.tobytes() == it[want].tobytes()


def test_empty_spectra_between_full_ones_and_offsets_that_do_not_start_at_zero():
    spectra = [(c["mz"], c["intensity"]) for c in CASES if c["params"] is dc.P0 and c["mz"].dtype == np.float64]
    want = np.concatenate([c["keep"] for c in CASES if c["params"] is dc.P0 and c["mz"].dtype == np.float64])
    mz, it, off = dc.pack(spectra, gaps=True)
    assert (np.diff(off) == 0).sum() == len(spectra)
    f_mz, f_it, f_off, keep = ru.deisotope(mz, it, off, dc.P0)
    assert keep.tolist() == want.tolist() and f_mz.tobytes() == mz[want].tobytes()
    assert np.diff(f_off)[1::2].tolist() == [0] * len(spectra)
    assert np.diff(f_off)[0::2].tolist() == [int(c["keep"].sum()) for c in CASES if c["params"] is dc.P0 and c["mz"].dtype == np.float64]
    # the same spectra behind 5 peaks nobody names: the filtered arrays start at 0 all the same
    pad = np.full(5, 123.0)
    g_mz, g_it, g_off, g_keep = ru.deisotope(np.concatenate([pad, mz]), np.concatenate([pad, it]), off + 5, dc.P0)
    assert g_keep.tolist() == keep.tolist() and g_off.tolist() == f_off.tolist() and g_mz.tobytes() == f_mz.tobytes()
    # an empty spectrum at the very end, behind a spectrum that loses a peak
    t = ru.deisotope(np.array([500.0, 500.0 + dc.S / 2, 500.0 + dc.S, 500.0, 500.0 + dc.S]), np.array([10.0, 9, 8, 10, 8]), [0, 3, 3, 5, 5],
                     dc.P_ONLY_PER_MZ)
    assert t[2].tolist() == [0, 1, 1, 3, 3] and t[3].tolist() == [True, False, False, True, True]
    # no spectra at all, and spectra without a peak
    e = np.zeros(0)
    assert ru.deisotope(e, e, [0], dc.P0)[2].tolist() == [0]
    assert ru.deisotope(e, e, [0, 0, 0], dc.P0)[2].tolist() == [0, 0, 0]


def test_mixed_dtypes_keep_their_dtype():
    x = np.array([500.0, 500.0 + dc.S, 600.0], np.float64)
    y = np.array([10.0, 5.0, 1.0], np.float32)
    mz, it, off, keep = ru.deisotope(x, y, [0, 3], dc.P0)
    assert mz.dtype == np.float64 and it.dtype == np.float32 and keep.tolist() == [True, False, True]
    with pytest.raises(ValueError):
        ru.deisotope(x.astype(np.int64), y, [0, 3], dc.P0)
    with pytest.raises(ValueError):
        ru.deisotope(x, y, [0, 4], dc.P0)
    with pytest.raises(ValueError):
        ru.deisotope(x, y, [0, 2, 1], dc.P0)


def test_parameters_that_are_refused():
    ok = ru.deisotope_params()
    assert ok["tol"] == 0.01 and ok["max_charge"] == 3 and ok["ratio0"] == 1.0 and ok["ratio_per_mz"] == 0.0
    assert ok["spacing"] == (dc.S / 1.0, dc.S / 2.0, dc.S / 3.0)
    assert len(ru.deisotope_params(max_charge=8)["spacing"]) == 8
    for bad in (dict(tol=-0.001), dict(tol=float("nan")), dict(tol=float("inf")), dict(max_charge=0), dict(max_charge=9), dict(max_charge=2.5),
                dict(step=0.0), dict(step=-1.0), dict(step=float("nan")), dict(ratio=float("inf")), dict(ratio_per_mz=float("nan")),
                dict(tol=0.2), dict(tol=dc.S / 6.0)):                 # (the last two: step / 3 is not above 2 tol)
        with pytest.raises(ValueError):
            ru.deisotope_params(**bad)
    assert ru.deisotope_params(tol=0.0)["tol"] == 0.0
    base = dict(tol=0.01, ratio0=1.0, ratio_per_mz=0.0, max_charge=2, spacing=(1.0, 0.5))
    assert ru.check_deisotope_params(base) == base
    for bad in (dict(base, spacing=(0.5, 1.0)), dict(base, spacing=(1.0, 1.0)), dict(base, spacing=(1.0,)), dict(base, spacing=(1.0, 0.0)),
                dict(base, spacing=(float("inf"), 0.5)), dict(base, spacing=(1.0, 0.02)), dict(base, max_charge=0), {}, None):
        with pytest.raises(ValueError):
            ru.check_deisotope_params(bad)
    c = ru.deisotope_c_params(base)
    assert (c.tol, c.ratio0, c.ratio_per_mz, c.max_charge, c.reserved) == (0.01, 1.0, 0.0, 2, 0) and list(c.spacing) == [1.0, 0.5] + [0.0] * 6


# ---- properties on dense spectra ----

@pytest.fixture(scope="module")
def dense():
    batch, _ = dc.dense_batch()
    return batch, ru.deisotope(batch["mz"], batch["intensity"], batch["peak_off"], dc.P0)


def test_the_output_is_a_subsequence_and_the_offsets_agree_with_keep(dense):
    batch, (mz, it, off, keep) = dense
    assert keep.dtype == bool and keep.size == batch["mz"].size
    assert mz.tobytes() == batch["mz"][keep].tobytes() and it.tobytes() == batch["intensity"][keep].tobytes()
    per = [int(keep[a:b].sum()) for a, b in zip(batch["peak_off"][:-1], batch["peak_off"][1:])]
    assert off.tolist() == np.concatenate([[0], np.cumsum(per)]).tolist()
    assert 0.25 < keep.mean() < 0.6                                       # (satellites are two thirds of the peaks)
    for a, b in zip(off[:-1], off[1:]):
        assert (np.diff(mz[a:b]) >= 0).all()


def test_every_spectrum_keeps_its_first_peak(dense):
    batch, (_, _, off, keep) = dense
    assert keep[batch["peak_off"][:-1]].all() and (np.diff(off) >= 1).all()


def test_a_second_pass_removes_only_peaks_whose_parent_survived(dense):
    """idempotent: a second pass can only remove a peak that has a parent in ITS input, a survivor of the first pass -- and a
    peak with such a parent had it in the first pass too and went then.  So the second pass removes nothing."""
    _, (mz, it, off, _) = dense
    mz2, it2, off2, keep2 = ru.deisotope(mz, it, off, dc.P0)
    assert keep2.all() and off2.tolist() == off.tolist() and mz2.tobytes() == mz.tobytes() and it2.tobytes() == it.tobytes()


def test_all_pairs_agree_with_the_restatement(dense):
    """the definition with no search at all: every pair of the first spectra, in Python floats"""
    batch, (_, _, _, keep) = dense
    p = dc.P0
    for s in range(3):
        a, b = int(batch["peak_off"][s]), int(batch["peak_off"][s + 1])
        x, y = batch["mz"][a:b].tolist(), batch["intensity"][a:b].tolist()
        want = []
        for j in range(len(x)):
            gone = False
            for z, sp in enumerate(p["spacing"], 1):
                for i in range(len(x)):
                    d = x[j] - x[i]
                    e = d - sp
                    if abs(e) <= p["tol"] and y[j] <= y[i] * (p["ratio0"] + p["ratio_per_mz"] * (x[i] * float(z))):
                        gone = True
            want.append(not gone)
        assert keep[a:b].tolist() == want, s


# ---- what satellites cost, with the reference core as the scorer ----

def _reference(settings, mz_error):
    return harness.make_scorer(orc.OracleAscore, dict(settings, mz_error=mz_error), kind=checker_kind())


def test_satellites_cost_score_and_the_rule_gives_it_back():
    """120 cfg2 PSMs generated for a 0.05 Da tolerance; every peak gets two satellites (deisotope_cases.with_satellites); the
    dirty batch is filtered with the defaults (0.01 Da, charges 1 .. 3, ratio 1).  Measured with the definitions here: the rule
    keeps 0.3307 of the dirty peaks (ideal 0.3333) and removes 0.0044 of the peaks of the clean batch (chance pairs one isotope
    spacing apart); mean best_score clean 307.9, dirty 280.0, filtered 307.9; best_sig equal to the clean run's on 116 of 120
    PSMs dirty and 119 filtered.  The bounds below stand against these: satellites cost 27.9, the rule gives back all of it."""
    batch, settings = synth.make_batch("cfg2", n_psm=120, seed=5, mz_error=0.05)
    dirty = dc.with_satellites(batch)
    mz, it, off, keep = ru.deisotope(dirty["mz"], dirty["intensity"], dirty["peak_off"], dc.P0)
    deiso = dict(dirty, mz=mz, intensity=it, peak_off=off)
    removed_clean = 1.0 - ru.deisotope(batch["mz"], batch["intensity"], batch["peak_off"], dc.P0)[3].mean()
    scorer = _reference(settings, 0.05)
    clean_r, dirty_r, deiso_r = (dict(scorer.score_batch(b)) for b in (batch, dirty, deiso))
    before = int((dirty_r["best_sig"] == clean_r["best_sig"]).sum())
    after = int((deiso_r["best_sig"] == clean_r["best_sig"]).sum())
    m_clean, m_dirty, m_deiso = (float(r["best_score"].mean()) for r in (clean_r, dirty_r, deiso_r))
    print("kept share of dirty %.4f; removed share of clean %.4f; mean best_score clean %.1f dirty %.1f deiso %.1f; best_sig agreement "
          "before %d after %d of 120" % (keep.mean(), removed_clean, m_clean, m_dirty, m_deiso, before, after))
    assert 0.32 <= keep.mean() <= 0.34
    assert removed_clean <= 0.01
    assert m_dirty <= m_clean - 15.0 and abs(m_deiso - m_clean) <= 2.0
    assert after >= before and after >= 117


# ---- the surface ----

def test_header_and_bindings_declare_the_interface():
    text = open(os.path.join(ROOT, "include", "pyascore_hip.h")).read()
    assert re.search(r"#define\s+PYA_DEISO_MAX_CHARGE\s+8\b", text) and _lib.PYA_DEISO_MAX_CHARGE == 8
    assert "typedef struct pya_deisotope_params {" in text
    assert re.search(r"uint64_t\s+pya_deisotope_workspace_bytes\s*\(", text)
    for name in ("pya_deisotope_spectra", "pya_deisotope_spectra_host"):
        assert re.search(r"int\s+%s\s*\(" % name, text), name
    for name in ("pya_deisotope_workspace_bytes", "pya_deisotope_spectra", "pya_deisotope_spectra_host"):
        assert name in _lib.SYMBOLS, name
    p = _lib.DeisotopeParams
    assert (p.tol.offset, p.ratio0.offset, p.ratio_per_mz.offset, p.spacing.offset, p.max_charge.offset, p.reserved.offset) == (0, 8, 16, 24, 88, 92)
    assert not [k for k in dir(_lib) if k.startswith("PYA_FLAG_") and "DEISO" in k]      # a transform in front of a plan, not a flag


def test_score_batch_argument_checking():
    from pyascore_amd.ascore import _deisotope_request
    assert _deisotope_request(True) == ru.deisotope_params()
    assert _deisotope_request(dict(tol=0.02, max_charge=2, ratio=0.8, ratio_per_mz=1e-4, step=1.003)) == \
        ru.deisotope_params(0.02, 2, 1.003, 0.8, 1e-4)
    for bad in ([0.01], "yes", 3, dict(tolerance=0.01), dict(tol="wide"), dict(tol=-1.0), dict(max_charge=9), dict(max_charge=0),
                dict(tol=0.3), dict(ratio=float("nan")), dict(step=0.0)):
        with pytest.raises(ValueError):
            _deisotope_request(bad)


def test_command_line_argument_checking():
    from pyascore_amd.__main__ import parse_args
    files = ["spec.mzML", "ident.pepXML", "out.tsv"]
    args = parse_args(files)
    assert args.deisotope is False and args.deisotope_tol == 0.01 and args.deisotope_charge == 3 and args.deisotope_ratio == 1.0
    args = parse_args(["--deisotope", "--deisotope_tol", "0.02", "--deisotope_charge", "2", "--deisotope_ratio", "0.8"] + files)
    assert args.deisotope is True and (args.deisotope_tol, args.deisotope_charge, args.deisotope_ratio) == (0.02, 2, 0.8)
    for bad in (["--deisotope_charge", "9"], ["--deisotope_charge", "0"], ["--deisotope_tol", "-0.01"], ["--deisotope_tol", "0.2"],
                ["--deisotope_ratio", "nan"]):
        with pytest.raises(ValueError):
            parse_args(["--deisotope"] + bad + files)
        parse_args(bad + files)                                            # (without --deisotope the values are not looked at)
