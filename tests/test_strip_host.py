"""The host side of precursor stripping (pya_strip_params): the numpy restatement pyascore_amd.rollup.strip on hand-made spectra
whose outcome is written out by hand (tests/strip_cases.py), the windows against the header's numbers, what a planted precursor
costs with the reference core as the scorer, and the public surface (header, bindings, argument checks).  No GPU."""
import os
import re

import numpy as np
import pytest

import strip_cases as sc
from conftest import checker_kind
from oracle import harness, orc
from pyascore_amd import _lib, rollup as ru, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sc.hand_cases()


# ---- the rule, one case each ----

@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hand_made_spectrum(case):
    x, y, keep = case["mz"], case["intensity"], case["keep"]
    mz, it, off, report = ru.strip(x, y, [0, x.size], [case["prec_mz"]], [case["prec_z"]], case["params"])
    assert mz.dtype == x.dtype and it.dtype == y.dtype
    assert mz.tobytes() == x[keep].tobytes() and it.tobytes() == y[keep].tobytes()
    assert off.dtype == np.int64 and off.tolist() == [0, int(keep.sum())]
    assert report.dtype == ru.STRIP_REPORT_DTYPE and report.shape == (1,)
    assert (int(report["hit"][0]), int(report["n_removed"][0]), int(report["n_windows"][0])) == \
        (case["hit"], int((~keep).sum()), case["n_windows"])


def test_windows_against_the_numbers_of_the_header():
    lo, hi, active = ru.strip_windows(400.0, 2, sc.P_BASE)
    assert lo.shape == hi.shape == active.shape == (64,) and active.tolist() == [True, True] + [False] * 62
    assert lo[:2].tolist() == [399.9921875, 383.9921875] and hi[:2].tolist() == [400.0078125, 384.0078125]
    assert np.isnan(lo[2:]).all() and np.isnan(hi[2:]).all()
    lo, hi, active = ru.strip_windows(400.0, 2, sc.P_ISO2)
    assert lo[:2].tolist() == [399.9921875, 383.9921875] and hi[:2].tolist() == [401.0078125, 385.0078125]
    # reduced: w = c (n_loss + 1) + l with z' = 2, 1
    lo, hi, active = ru.strip_windows([400.0, 300.0], [2, 3], sc.P_REDUCED)
    assert lo.shape == (2, 64) and active.sum(axis=1).tolist() == [4, 6]
    assert (lo[0, :4] + sc.TOL).tolist() == [400.0, 384.0, 800.0, 768.0]
    assert lo[1, :6].tolist() == [cen - sc.TOL for cen in (300.0, 868.0 / 3.0, 450.0, 434.0, 900.0, 868.0)]
    # all 64, and the step of a real isotope spacing divided by the reduced charge
    p = ru.strip_params(0.01, losses=sc.LOSSES_64, reduced=True, isotopes=3)
    lo, hi, active = ru.strip_windows(100.0, 8, p)
    assert active.all()
    for w in (0, 31, 32, 63):
        c, l = divmod(w, 8)
        cen = (100.0 * 8.0 - p["loss"][l]) / float(8 - c)
        assert lo[w] == cen - 0.01 and hi[w] == (cen + 3.0 * (1.0033548378 / float(8 - c))) + 0.01
    # no windows
    for pm, pz in ((400.0, 0), (400.0, -1), (400.0, 9), (float("nan"), 2), (float("inf"), 2), (0.0, 2), (-1.0, 2)):
        assert not ru.strip_windows(pm, pz, sc.P_BASE)[2].any()
    # inactive: the loss is the whole mass, or more
    assert ru.strip_windows(400.0, 2, sc.P_BIG_LOSS)[2][:4].tolist() == [True, True, False, False]
    assert ru.strip_hits(np.array([(0b110, 1, 3)], ru.STRIP_REPORT_DTYPE), sc.P_TWICE).tolist() == [[[False, True, True]]]
    assert ru.strip_hits(np.array([(1 << 63, 1, 64)], ru.STRIP_REPORT_DTYPE), sc.P_64)[0, 7, 7]


def test_boundary_spectra_lose_exactly_the_planted_peaks():
    spectra, planted = sc.boundary_spectra()
    mz, it, off = sc.pack(spectra, gaps=False)
    n = len(spectra)
    assert np.diff(off).tolist() == list(sc.BOUNDARY_LENGTHS)
    want = ~np.concatenate(planted)
    f_mz, f_it, f_off, report = ru.strip(mz, it, off, np.full(n, sc.BOUNDARY_PREC[0]), np.full(n, sc.BOUNDARY_PREC[1]), sc.P_BASE)
    assert f_mz.tobytes() == mz[want].tobytes() and f_it.tobytes() == it[want].tobytes()
    assert report["n_removed"].tolist() == [int(m.sum()) for m in planted] and (report["n_windows"] == 2).all()
    assert np.diff(f_off).tolist() == [int((~m).sum()) for m in planted]
    assert np.diff(f_off)[11:].tolist() == [0, 0] and report["n_removed"][11:].tolist() == [64, 1]     # removed entirely
    assert report["hit"][9] == 0b11 and report["hit"][0] == 0


def test_offsets_that_do_not_start_at_zero_and_empty_spectra_in_between():
    group = [c for c in CASES if c["params"] is sc.P_BASE and c["mz"].dtype == np.float64]
    assert len(group) >= 5
    mz, it, off, pm, pz = sc.pack_cases(group, gaps=True)
    want = np.concatenate([c["keep"] for c in group])
    f_mz, f_it, f_off, report = ru.strip(mz, it, off, pm, pz, sc.P_BASE)
    assert f_mz.tobytes() == mz[want].tobytes() and f_it.tobytes() == it[want].tobytes()
    assert np.diff(f_off)[0::2].tolist() == [int(c["keep"].sum()) for c in group] and not np.diff(f_off)[1::2].any()
    assert report["hit"][0::2].tolist() == [c["hit"] for c in group] and not report["hit"][1::2].any()
    assert report["n_windows"].tolist() == [c["n_windows"] for c in group for _ in (0, 1)]           # (an empty spectrum has windows too)
    # the same spectra behind 5 peaks nobody names: the stripped arrays start at 0 all the same
    pad = np.full(5, 400.0)
    g = ru.strip(np.concatenate([pad, mz]), np.concatenate([pad, it]), off + 5, pm, pz, sc.P_BASE)
    assert g[0].tobytes() == f_mz.tobytes() and g[2].tolist() == f_off.tolist() and g[3].tobytes() == report.tobytes()
    # no spectra at all, and spectra without a peak
    e = np.zeros(0)
    assert ru.strip(e, e, [0], e, np.zeros(0, np.int32), sc.P_BASE)[2].tolist() == [0]
    r = ru.strip(e, e, [0, 0, 0], [400.0, 0.0], [2, 0], sc.P_BASE)
    assert r[2].tolist() == [0, 0, 0] and r[3]["n_windows"].tolist() == [2, 0]


def test_dtypes_are_kept_and_bad_arrays_refused():
    x = np.array([400.0, 384.0, 600.0], np.float64)
    y = np.array([10.0, 5.0, 1.0], np.float32)
    mz, it, off, report = ru.strip(x, y, [0, 3], [400.0], [2], sc.P_BASE)
    assert mz.dtype == np.float64 and it.dtype == np.float32 and mz.tolist() == [600.0] and it.tolist() == [1.0]
    mz, it, _, _ = ru.strip(x.astype(np.float32), y, [0, 3], [400.0], [2], sc.P_BASE)
    assert mz.dtype == np.float32 and it.dtype == np.float32
    for bad in (dict(mz=x.astype(np.int64)), dict(off=[0, 4]), dict(off=[0, 2, 1]), dict(off=[-1, 3]), dict(pm=[400.0, 400.0]), dict(pz=[2, 2]),
                dict(pz=[2.0]), dict(pm=[[400.0]], pz=[[2]]), dict(pz=[2 ** 40])):
        with pytest.raises(ValueError):
            ru.strip(bad.get("mz", x), y, bad.get("off", [0, 3]), bad.get("pm", [400.0]), bad.get("pz", [2]), sc.P_BASE)


def test_parameters_that_are_refused():
    ok = ru.strip_params(0.05)
    assert ok == dict(tol=0.05, step=1.0033548378, mz_lo=float("-inf"), mz_hi=float("inf"), loss=(0.0,), reduced=0, isotopes=0)
    full = ru.strip_params(0.0, losses=(1, 2, 3, 4, 5, 6, 7), reduced=True, isotopes=4, step=1.0, mz_lo=100, mz_hi=100)
    assert full["loss"] == (0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0) and full["reduced"] == 1 and full["isotopes"] == 4
    for bad in (dict(tol=-0.001), dict(tol=float("nan")), dict(tol=float("inf")), dict(step=0.0), dict(step=-1.0), dict(step=float("inf")),
                dict(mz_lo=float("nan")), dict(mz_hi=float("nan")), dict(mz_lo=2.0, mz_hi=1.0), dict(losses=(1,) * 8), dict(losses=(-1.0,)),
                dict(losses=(float("inf"),)), dict(losses=(float("nan"),)), dict(losses=5.0), dict(isotopes=5), dict(isotopes=-1),
                dict(isotopes=1.5), dict(reduced=2), dict(reduced="yes")):
        with pytest.raises(ValueError):
            ru.strip_params(**dict(dict(tol=0.05), **bad))
    assert ru.check_strip_params(ok) == ok
    for bad in (dict(ok, loss=(1.0,)), dict(ok, loss=()), dict(ok, loss=(0.0,) * 9), {}, None, dict(ok, tol="wide")):
        with pytest.raises(ValueError):
            ru.check_strip_params(bad)
    c = ru.strip_c_params(ru.strip_params(0.25, losses=(97.0, 18.0), reduced=True, isotopes=2, mz_lo=140.0))
    assert (c.tol, c.step, c.mz_lo, c.mz_hi, c.n_loss, c.reduced, c.isotopes, c.reserved) == (0.25, 1.0033548378, 140.0, float("inf"), 2, 1, 2, 0)
    assert list(c.loss) == [0.0, 97.0, 18.0] + [0.0] * 5


# ---- what a planted precursor costs, with the reference core as the scorer ----

def test_precursor_peaks_cost_score_and_the_rule_gives_it_back():
    """120 cfg2 PSMs generated for a 0.05 Da tolerance; every spectrum gets a precursor at charge 2, its - H3PO4 and - H2O forms
    and one isotope peak of each at ten times its largest intensity (strip_cases.with_precursors, which draws the precursor so
    that no original peak lies in a window).  Asserted: stripping gives the clean arrays back byte for byte, and the dirty arrays
    change the reference's PepScore of at least one PSM -- a planted base peak takes the first rank of its 100 m/z window and
    moves every real peak of it one rank down.  Measured with the definitions here (printed, not asserted): the PepScore changes
    on 97 of 120 PSMs, best_sig on 1; mean PepScore 307.9 clean, 292.4 dirty."""
    batch, settings = synth.make_batch("cfg2", n_psm=120, seed=5, mz_error=0.05)
    dirty, prec_mz, prec_z = sc.with_precursors(batch, 0.05)
    assert dirty["mz"].size == batch["mz"].size + 6 * 120
    p = sc.effect_params(0.05)
    mz, it, off, report = ru.strip(dirty["mz"], dirty["intensity"], dirty["peak_off"], prec_mz, prec_z, p)
    assert mz.tobytes() == np.asarray(batch["mz"], np.float64).tobytes() and it.tobytes() == np.asarray(batch["intensity"], np.float64).tobytes()
    assert off.tobytes() == np.asarray(batch["peak_off"], np.int64).tobytes()
    assert (report["hit"] == 0b111).all() and (report["n_removed"] == 6).all() and (report["n_windows"] == 3).all()
    scorer = harness.make_scorer(orc.OracleAscore, dict(settings, mz_error=0.05), kind=checker_kind())
    clean_r, dirty_r = (dict(scorer.score_batch(b)) for b in (batch, dirty))
    n_score = int((dirty_r["best_score"] != clean_r["best_score"]).sum())
    n_sig = int((dirty_r["best_sig"] != clean_r["best_sig"]).sum())
    print("PepScore differs on %d of 120 PSMs, best_sig on %d; mean PepScore clean %.1f dirty %.1f"
          % (n_score, n_sig, float(clean_r["best_score"].mean()), float(dirty_r["best_score"].mean())))
    assert n_score >= 1


# ---- the surface ----

def test_header_and_bindings_declare_the_interface():
    text = open(os.path.join(ROOT, "include", "pyascore_hip.h")).read()
    assert re.search(r"#define\s+PYA_STRIP_MAX_CHARGE\s+8\b", text) and _lib.PYA_STRIP_MAX_CHARGE == 8
    assert re.search(r"#define\s+PYA_STRIP_MAX_LOSS\s+7\b", text) and _lib.PYA_STRIP_MAX_LOSS == 7
    assert re.search(r"#define\s+PYA_STRIP_MAX_ISOTOPES\s+4\b", text) and _lib.PYA_STRIP_MAX_ISOTOPES == 4
    assert re.search(r"#define\s+PYA_STRIP_STEP\s+1\.0033548378\b", text) and _lib.PYA_STRIP_STEP == 1.0033548378
    assert "typedef struct pya_strip_params {" in text and "typedef struct pya_strip_report {" in text
    assert re.search(r"uint64_t\s+pya_strip_workspace_bytes\s*\(", text)
    for name in ("pya_strip_spectra", "pya_strip_spectra_host"):
        assert re.search(r"int\s+%s\s*\(" % name, text), name
    for name in ("pya_strip_workspace_bytes", "pya_strip_spectra", "pya_strip_spectra_host"):
        assert name in _lib.SYMBOLS, name
    p = _lib.StripParams
    assert (p.tol.offset, p.step.offset, p.mz_lo.offset, p.mz_hi.offset, p.loss.offset, p.n_loss.offset, p.reduced.offset, p.isotopes.offset,
            p.reserved.offset) == (0, 8, 16, 24, 32, 96, 100, 104, 108)
    r = _lib.StripReport
    assert (r.hit.offset, r.n_removed.offset, r.n_windows.offset) == (0, 8, 12)
    assert [ru.STRIP_REPORT_DTYPE.fields[k][1] for k in ("hit", "n_removed", "n_windows")] == [0, 8, 12]
    assert not [k for k in dir(_lib) if k.startswith("PYA_FLAG_") and "STRIP" in k]       # a transform in front of a plan, not a flag
    host = open(os.path.join(ROOT, "pyascore_amd", "csrc", "host_strip.cpp")).read()
    assert "static_assert(sizeof(pya_strip_params) == 112" in host and "static_assert(sizeof(pya_strip_report) == 16" in host
    lib = _lib.load()                                                     # (loading needs no device)
    for name in ("pya_strip_workspace_bytes", "pya_strip_spectra", "pya_strip_spectra_host"):
        assert hasattr(lib, name), name
    assert lib.pya_strip_workspace_bytes(0, 0) == 8 and lib.pya_strip_workspace_bytes(3, 1000) == lib.pya_deisotope_workspace_bytes(3, 1000)


def test_score_batch_argument_checking():
    from pyascore_amd.ascore import _strip_request
    pm, pz = np.array([400.0, 500.0]), np.array([2, 3])
    params, g_pm, g_pz = _strip_request(dict(precursor_mz=pm, precursor_charge=pz), 0.25, 2)
    assert params == ru.strip_params(0.25) and g_pm.dtype == np.float64 and g_pz.dtype == np.int32 and g_pz.tolist() == [2, 3]
    params, _, g_pz = _strip_request(dict(precursor_mz=pm, precursor_charge=np.array([2 ** 40, -2 ** 40]), tol=0.02, losses=[97.976896],
                                          reduced=True, isotopes=2, mz_lo=140.0, mz_hi=2000.0, step=1.003), 0.25)
    assert params == ru.strip_params(0.02, (97.976896,), True, 2, 1.003, 140.0, 2000.0)
    assert g_pz.tolist() == [0x7FFFFFFF, -1]                                # (both mean "no windows")
    ok = dict(precursor_mz=pm, precursor_charge=pz)
    for bad in (True, [0.01], "yes", dict(tol=0.1), dict(precursor_mz=pm), dict(ok, tolerance=0.01), dict(ok, tol="wide"), dict(ok, tol=-1.0),
                dict(ok, isotopes=9), dict(ok, losses=(1,) * 8), dict(ok, mz_lo=5.0, mz_hi=1.0), dict(ok, precursor_charge=np.array([2.0, 3.0])),
                dict(ok, precursor_charge=pz[:1]), dict(ok, precursor_mz=pm.reshape(1, 2)), dict(ok, precursor_mz=["a", "b"])):
        with pytest.raises(ValueError):
            _strip_request(bad, 0.25, 2)
    with pytest.raises(ValueError):
        _strip_request(ok, 0.25, 3)                                         # one precursor per spectrum


def test_command_line_argument_checking():
    from pyascore_amd.__main__ import parse_args, strip_request
    files = ["spec.mzML", "ident.pepXML", "out.tsv"]
    args = parse_args(files)
    assert args.strip_precursor is False and args.strip_tol is None and args.strip_losses == "" and args.strip_reduced is False
    assert args.strip_isotopes == 0 and args.strip_mz_min == float("-inf") and args.strip_mz_max == float("inf")
    assert strip_request(args) is None
    args = parse_args(["--strip_precursor", "--strip_tol", "0.02", "--strip_losses", "97.976896,18.010565", "--strip_reduced",
                       "--strip_isotopes", "2", "--strip_mz_min", "140", "--strip_mz_max", "2000"] + files)
    assert strip_request(args) == dict(tol=0.02, losses=(97.976896, 18.010565), reduced=True, isotopes=2, mz_lo=140.0, mz_hi=2000.0)
    assert strip_request(parse_args(["--strip_precursor"] + files))["tol"] is None         # (the scorer's mz_error)
    for bad in (["--strip_tol", "-0.01"], ["--strip_tol", "nan"], ["--strip_losses", "97.9,x"], ["--strip_losses", "1,2,3,4,5,6,7,8"],
                ["--strip_losses", "-18.0"], ["--strip_isotopes", "5"], ["--strip_mz_min", "500", "--strip_mz_max", "100"],
                ["--strip_mz_min", "nan"]):
        with pytest.raises(ValueError):
            parse_args(["--strip_precursor"] + bad + files)
        parse_args(bad + files)                                            # (without --strip_precursor the values are not looked at)
    # --strip_precursor goes with each of the other three
    parse_args(["--strip_precursor", "--deisotope"] + files)
    parse_args(["--strip_precursor", "--decharge"] + files)


def test_the_batch_driver_takes_the_precursors_from_the_spectra():
    from pyascore_amd import batch_cli
    a, b = dict(mz=np.zeros(3), intensity=np.zeros(3)), dict(mz=np.zeros(2), intensity=np.zeros(2))
    picked = [dict(a, precursor_mz=500.25, precursor_charge=3), dict(a, precursor_mz=500.25, precursor_charge=3),
              dict(b, precursor_mz=None, precursor_charge=2), dict(mz=np.zeros(1), intensity=np.zeros(1))]
    pm, pz = batch_cli.hit_precursors(picked, ["s1", "s1", "s2", "s3"])
    assert pm.dtype == np.float64 and pz.dtype == np.int32
    assert pm.tolist() == [500.25, 0.0, 0.0] and pz.tolist() == [3, 2, 0]  # the two hits of s1 share a spectrum; a missing value is 0
    assert not ru.strip_windows(pm, pz, sc.P_BASE)[2][1:].any()
    with pytest.raises(ValueError):                                        # refused before anything is read: there is no scorer here
        batch_cli.localize(None, [], {}, "STY", 79.9, strip=dict(tol=-1.0))
    with pytest.raises(ValueError):
        batch_cli.localize(None, [], {}, "STY", 79.9, strip=dict(precursor_mz=[1.0], precursor_charge=[2]))
    with pytest.raises(TypeError):
        batch_cli.localize(None, [], {}, "STY", 79.9, strip=dict(tol=0.1))
