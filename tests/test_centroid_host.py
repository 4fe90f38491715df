"""The host side of centroiding (pya_centroid_params): the numpy restatement pyascore_amd.rollup.centroid on hand-made spectra
whose apexes, centroids and intensities are written out by hand (tests/centroid_cases.py), its properties (ascending output,
pass-through), its accuracy on sampled Gaussians, what profile-mode spectra cost and what the rule gives back with the
reference core as the scorer, the reader of the files' own declaration, and the public surface.  No GPU."""
import os
import re

import numpy as np
import pytest

import centroid_cases as cc
from conftest import checker_kind
from oracle import harness, orc
from pyascore_amd import _lib, ingest, rollup as ru, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ingest")
CASES = cc.hand_cases()


# ---- the rule, one case each ----

@pytest.mark.parametrize("area", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hand_made_spectrum(case, area):
    x, y = case["mz"], case["intensity"]
    select = None if case["select"] else [False]
    mz, it, off, unordered = ru.centroid(x, y, [0, x.size], dict(case["params"], area=area), select)
    want_mz, want_it = cc.expected(case, area)
    assert mz.dtype == x.dtype and it.dtype == y.dtype
    assert mz.tobytes() == want_mz.tobytes(), (mz.tolist(), want_mz.tolist())
    assert it.tobytes() == want_it.tobytes(), (it.tolist(), want_it.tolist())
    assert off.dtype == np.int64 and off.tolist() == [0, len(case["apex"])]
    assert unordered.tolist() == [case["unordered"]]
    if not case["unordered"] and case["select"]:                           # (the intensities of the apexes, bits copied)
        assert want_it.tobytes() == y[case["apex"]].tobytes() or area


def test_the_hand_cases_cover_what_they_should():
    names = " | ".join(c["name"] for c in CASES)
    for word in ("symmetric", "dyadic", "plateau: the first", "plateau followed by a rise", "sharing a valley", "exactly at the limit float64",
                 "one ulp above the limit float32", "min_height", "NaN and zero", "cut by half_width", "half_width 1", "half_width 8",
                 "passes through", "unselected", "descending", "NaN m/z", "clamp"):
        assert word in names, word
    assert {c["mz"].dtype for c in CASES} == {np.dtype(np.float64), np.dtype(np.float32)}


def test_the_gap_edges_are_exact():
    """the construction behind the gap cases: x[k] - x[k - 1] and gap0 + gap_per_mz x[k - 1] have no rounding"""
    for p, base in ((cc.P, 100.0), (cc.P_PPM, 128.0), (cc.P_BOTH, 128.0)):
        assert p["gap0"] + p["gap_per_mz"] * base == 2 * cc.DX
        for t in (np.float64, np.float32):
            far = t(base + 2 * cc.DX)
            assert float(far) - base == 2 * cc.DX and float(np.nextafter(far, t(np.inf))) - base > 2 * cc.DX


def test_cases_among_others_with_gaps_select_and_offsets_that_do_not_start_at_zero():
    group = [c for c in CASES if c["params"] is cc.P and c["mz"].dtype == np.float64]
    assert len(group) >= 15 and any(c["unordered"] for c in group) and any(not c["select"] for c in group)
    mz, it, off = cc.pack([(c["mz"], c["intensity"]) for c in group], gaps=True)
    select = np.repeat([c["select"] for c in group], 2)
    for area in (0, 1):
        f_mz, f_it, f_off, unordered = ru.centroid(mz, it, off, dict(cc.P, area=area), select)
        assert f_mz.tobytes() == np.concatenate([c["out_mz"] for c in group]).tobytes()
        assert f_it.tobytes() == np.concatenate([cc.expected(c, area)[1] for c in group]).tobytes()
        assert np.diff(f_off)[0::2].tolist() == [len(c["apex"]) for c in group] and not np.diff(f_off)[1::2].any()
        assert unordered[0::2].tolist() == [c["unordered"] for c in group] and not unordered[1::2].any()
    # offsets from the middle of the arrays: the output starts at 0
    k = 5
    part = ru.centroid(mz, it, off[2 * k:], cc.P, select[2 * k:])
    assert part[2][0] == 0 and part[0].tobytes() == np.concatenate([c["out_mz"] for c in group[k:]]).tobytes()
    # select = None is "all"; a spectrum that is not selected is not reported whatever its order
    every = ru.centroid(mz, it, off, cc.P)
    assert every[3].sum() == sum(c["unordered"] for c in group)
    none = ru.centroid(mz, it, off, cc.P, np.zeros(select.size, bool))
    assert none[0].tobytes() == mz.tobytes() and none[1].tobytes() == it.tobytes() and none[2].tolist() == off.tolist() and not none[3].any()


# ---- properties ----

def _random_spectra(seed, n_spec=400):
    """ascending spectra of 0 .. 40 points with steps of 0, 1 or 3 DX -- or of one ulp --, intensities from a few values, so
    that plateaus, flat valleys and repeated m/z are everywhere"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_spec):
        n = int(rng.integers(0, 41))
        if rng.random() < 0.25:
            x = 500.0 + np.cumsum(rng.integers(0, 3, n)) * np.spacing(500.0)
        else:
            x = 100.0 + np.cumsum(rng.choice([0.0, 1.0, 1.0, 1.0, 3.0], size=n)) * cc.DX * rng.choice([1.0, 1.0 / 3.0])
        y = rng.choice([0.0, 1.0, 1.0, 2.0, 3.0, 7.0, 1e-3, 1e6], size=n) * rng.choice([1.0, 1.0, 0.1 + rng.random()])
        out.append((x, y))
    return out


@pytest.mark.parametrize("types", [(np.float64, np.float64), (np.float64, np.float32), (np.float32, np.float32)], ids=["f64/f64", "f64/f32", "f32/f32"])
def test_the_output_ascends_whenever_the_input_does(types):
    for seed, p in ((1, cc.P), (2, cc.P_W1), (3, cc.P_W8_AREA), (4, ru.centroid_params(1e-3, gap_ppm=20.0, half_width=3))):
        mz, it, off = cc.pack(_random_spectra(seed) + cc.boundary_spectra(seed)[0], types[0], types[1], gaps=False)
        o_mz, o_it, o_off, unordered = ru.centroid(mz, it, off, p)
        assert not unordered.any() and 0 < o_mz.size < mz.size
        inside = np.ones(o_mz.size, bool)
        inside[o_off[1:-1][o_off[1:-1] < o_mz.size]] = False                 # (the first peak of a spectrum has no predecessor)
        assert (np.diff(o_mz.astype(np.float64))[inside[1:]] >= 0.0).all()
        # every output lies inside its spectrum's range and apexes keep their number under area
        again = ru.centroid(mz, it, off, dict(p, area=1 - p["area"]))
        assert again[0].tobytes() == o_mz.tobytes() and again[2].tobytes() == o_off.tobytes()


def test_planted_apexes_sit_on_the_stride_edges():
    spectra, planted = cc.boundary_spectra()
    assert [len(x) for x, _ in spectra] == list(cc.BOUNDARY_LENGTHS)
    seen = set()
    for (x, y), at in zip(spectra, planted):
        o_mz, o_it, _, _ = ru.centroid(x, y, [0, x.size], cc.P)
        assert (o_it == 16.0).sum() == len(at) and (y == 16.0).sum() == len(at)
        seen.update(at)
    assert {0, 62, 63, 64, 65, 126, 127, 128, 4096} <= seen
    for t in (np.float32,):                                                # (the grid is exact in float32)
        mz, _, _ = cc.pack(spectra, t, t, gaps=False)
        assert mz.astype(np.float64).tobytes() == cc.pack(spectra, gaps=False)[0].tobytes()


def test_a_centroided_spectrum_passes_through():
    """no two adjacent points connected: the points with y > 0 and y >= min_height come out, every byte copied"""
    batch, _ = synth.make_batch("cfg2", n_psm=40, seed=3)
    mz, it, off = batch["mz"], batch["intensity"], batch["peak_off"]
    gap = float(np.diff(mz)[np.diff(mz) > 0].min()) * 0.5
    assert gap > 0
    for t_mz, t_it in ((np.float64, np.float64), (np.float64, np.float32)):
        x, y = mz.astype(t_mz), it.astype(t_it).copy()
        y[::7] = 0.0
        y[3::11] = np.nan
        floor = float(np.nanmedian(y))
        for p in (ru.centroid_params(gap), ru.centroid_params(gap, min_height=floor, area=True, half_width=8)):
            o_mz, o_it, o_off, unordered = ru.centroid(x, y, off, p)
            keep = (y > 0.0) & (y >= p["min_height"])
            assert 0 < keep.sum() < keep.size and not unordered.any()
            assert o_mz.tobytes() == x[keep].tobytes() and o_it.tobytes() == y[keep].tobytes()
            assert o_off.tolist() == np.concatenate([[0], np.cumsum(keep)])[off].tolist()
    same = ru.centroid(mz, it, off, ru.centroid_params(gap))
    assert same[0].tobytes() == mz.tobytes() and same[1].tobytes() == it.tobytes() and same[2].tobytes() == np.asarray(off, np.int64).tobytes()


def test_parameters_that_are_refused():
    ok = ru.centroid_params(0.01)
    assert ok == dict(gap0=0.01, gap_per_mz=0.0, min_height=0.0, half_width=4, area=0)
    assert ru.centroid_params(0.0, gap_ppm=20.0)["gap_per_mz"] == 20.0 * 1e-6 and ru.centroid_params(0.01, area=True)["area"] == 1
    nan, inf = float("nan"), float("inf")
    for bad in (dict(gap=-0.01), dict(gap=nan), dict(gap=inf), dict(gap=0.0), dict(gap=0.01, gap_ppm=-1.0), dict(gap=0.01, gap_ppm=nan),
                dict(gap=0.01, gap_ppm=inf), dict(gap=0.01, min_height=-1.0), dict(gap=0.01, min_height=nan), dict(gap=0.01, min_height=inf),
                dict(gap=0.01, half_width=0), dict(gap=0.01, half_width=9), dict(gap=0.01, half_width=2.5), dict(gap=0.01, area=2),
                dict(gap=0.01, area=-1), dict(gap=0.01, gap_ppm="x")):
        with pytest.raises(ValueError):
            ru.centroid_params(**bad)
    assert ru.check_centroid_params(ok) == ok
    for bad in ({}, None, dict(ok, half_width=None), dict(ok, gap0=0.0)):
        with pytest.raises(ValueError):
            ru.check_centroid_params(bad)
    c = ru.centroid_c_params(dict(ok, half_width=8, area=1, min_height=3.0))
    assert (c.gap0, c.gap_per_mz, c.min_height, c.half_width, c.area, c.reserved) == (0.01, 0.0, 3.0, 8, 1, 0)
    x = np.array([1.0, 2.0])
    for bad in (dict(mz=x.astype(np.float16)), dict(peak_off=[0, 3]), dict(peak_off=[2, 0]), dict(select=[True, False]), dict(select=[0.5])):
        a = dict(dict(mz=x, intensity=x, peak_off=[0, 2], params=ok, select=None), **bad)
        with pytest.raises(ValueError):
            ru.centroid(a["mz"], a["intensity"], a["peak_off"], a["params"], a["select"])


# ---- accuracy ----

@pytest.mark.parametrize("dtype,sigma,dx", [(np.float64, 0.008, 0.004), (np.float64, 0.01, 0.005), (np.float32, 0.008, 0.004),
                                            (np.float32, 0.01, 0.005), (np.float64, 0.009, 0.0045)])
def test_a_sampled_gaussian_comes_back_at_its_centre(dtype, sigma, dx):
    """isolated Gaussians of sigma 0.008 .. 0.01 sampled every 0.004 .. 0.005 between m/z 100 and 2 000, half_width 8 and a gap
    of 2.5 dx: exactly one apex per peak, within 1e-3 m/z of the planted centre -- a fiftieth of cfg2's 0.05 Da window.
    Measured with the rule as it stands and samples out to 4 sigma: at most 2.7e-6 in float64 (the tails beyond the rendered
    samples); in float32 the centroid rounds to the float32 value of the centre itself (one ulp at 2 000 is 1.2e-4)."""
    rng = np.random.default_rng(17)
    centres = np.sort(100.0 + 1.9 * np.arange(1000) + rng.uniform(0.0, 0.9, 1000))
    heights = rng.uniform(10.0, 1e5, centres.size)
    off = np.arange(0, 1001, 50)
    prof = cc.profile_of(dict(mz=centres.astype(dtype), intensity=heights.astype(dtype), peak_off=off), sigma, dx)
    assert prof["mz"].dtype == dtype and 14 * centres.size < prof["mz"].size < 18 * centres.size
    p = ru.centroid_params(2.5 * dx, half_width=8)
    o_mz, o_it, o_off, unordered = ru.centroid(prof["mz"], prof["intensity"], prof["peak_off"], p)
    assert not unordered.any() and o_off.tolist() == off.tolist()
    err = np.abs(o_mz.astype(np.float64) - centres.astype(dtype).astype(np.float64))
    print("sigma %g dx %g %s: worst |centroid - centre| %.3g m/z" % (sigma, dx, np.dtype(dtype).name, err.max()))
    assert err.max() <= 1e-3
    assert (o_it.astype(np.float64) <= heights.astype(dtype) * (1 + 1e-6)).all() and (o_it > 0.8 * heights.astype(dtype)).all()
    area = ru.centroid(prof["mz"], prof["intensity"], prof["peak_off"], dict(p, area=1))[1].astype(np.float64)
    assert np.allclose(area, heights * sigma * np.sqrt(2 * np.pi) / dx, rtol=2e-2)


# ---- what profile mode costs, with the reference core as the scorer ----

def _reference(settings, mz_error):
    return harness.make_scorer(orc.OracleAscore, dict(settings, mz_error=mz_error), kind=checker_kind())


SIGMA, STEP = 0.008, 0.004
RULE = dict(gap=2.5 * STEP, half_width=8)


def test_profile_spectra_cost_localisations_and_the_rule_gives_them_back():
    """120 cfg2 PSMs generated for a 0.05 Da tolerance; every peak rendered as a Gaussian of sigma 0.008 on a 0.004 grid
    (centroid_cases.profile_of: about 17 samples a peak); the profile batch centroided with half_width 8 and a gap of 2.5
    steps.  Measured with the definitions here (reference core): see DESIGN section 8 for the three rows.  Asserted: the
    centroided batch finds the clean batch's best_sig on at least as many PSMs as the profile batch as it is, and on at
    least 95 % of them (114 of 120)."""
    batch, settings = synth.make_batch("cfg2", n_psm=120, seed=5, mz_error=0.05)
    prof = cc.profile_of(batch, SIGMA, STEP)
    mz, it, off, unordered = ru.centroid(prof["mz"], prof["intensity"], prof["peak_off"], ru.centroid_params(**RULE))
    picked = dict(prof, mz=mz, intensity=it, peak_off=off)
    assert not unordered.any()
    scorer = _reference(settings, 0.05)
    clean_r, prof_r, cen_r = (dict(scorer.score_batch(b)) for b in (batch, prof, picked))
    as_is = int((prof_r["best_sig"] == clean_r["best_sig"]).sum())
    after = int((cen_r["best_sig"] == clean_r["best_sig"]).sum())
    m_clean, m_prof, m_cen = (float(r["best_score"].mean()) for r in (clean_r, prof_r, cen_r))
    print("points per peak %.1f; peaks after / clean %.4f; mean best_score clean %.1f profile %.1f centroided %.1f; best_sig equal to "
          "clean: profile %d, centroided %d of 120" % (prof["mz"].size / batch["mz"].size, mz.size / batch["mz"].size, m_clean, m_prof, m_cen,
                                                       as_is, after))
    assert after >= as_is and after >= 114


# ---- what the files declare ----

@pytest.mark.parametrize("fmt,name", [("mzML", "modes.mzML"), ("mzXML", "modes.mzXML")])
def test_the_reader_keeps_what_the_file_says(fmt, name):
    recs = ingest.SpectraParser(os.path.join(GOLDEN, name), fmt).to_list()
    assert [r["scan"] for r in recs] == [1, 2, 3]
    assert [r["profile"] for r in recs] == [True, False, None]
    assert [r["mz_values"].size for r in recs] == [5, 2, 2]
    as_dict = ingest.SpectraParser(os.path.join(GOLDEN, name), fmt, native_precision=True).to_dict()
    assert [as_dict[k]["profile"] for k in (1, 2, 3)] == [True, False, None]


def test_the_cli_selects_what_is_not_declared_centroided():
    from pyascore_amd import batch_cli
    a, b, c = (np.zeros(1), np.zeros(1)), (np.zeros(1), np.zeros(1)), (np.zeros(1), np.zeros(1))
    picked = [dict(mz=a[0], intensity=a[1], profile=True), dict(mz=a[0], intensity=a[1], profile=True),
              dict(mz=b[0], intensity=b[1], profile=False), dict(mz=c[0], intensity=c[1], profile=None), dict(mz=c[0], intensity=c[1])]
    assert batch_cli.hit_profiles(picked, [1, 1, 2, 3, 4]).tolist() == [True, False, True, True]
    from pyascore_amd.__main__ import build_parser, centroid_request, validate_args
    base = ["--residues", "STY", "--mod_mass", "79.966331", "s.mzML", "i.pep.xml", "o.tsv"]
    assert centroid_request(build_parser().parse_args(base)) is None
    args = build_parser().parse_args(["--centroid", "--centroid_gap", "0.01", "--centroid_gap_ppm", "5", "--centroid_width", "6",
                                      "--centroid_min_height", "3", "--centroid_area"] + base)
    assert centroid_request(args) == dict(gap=0.01, gap_ppm=5.0, half_width=6, min_height=3.0, area=True)
    for bad in (["--centroid"], ["--centroid", "--centroid_gap", "0.01", "--centroid_width", "9"], ["--centroid", "--centroid_gap", "-1"]):
        with pytest.raises(ValueError):
            centroid_request(build_parser().parse_args(bad + base))
    assert centroid_request(build_parser().parse_args(["--centroid_width", "99"] + base)) is None     # (not looked at without the flag)
    del validate_args


# ---- the surface ----

def test_header_and_bindings_declare_the_interface():
    text = open(os.path.join(ROOT, "include", "pyascore_hip.h")).read()
    assert re.search(r"#define\s+PYA_CENTROID_MAX_HALF_WIDTH\s+8\b", text) and _lib.PYA_CENTROID_MAX_HALF_WIDTH == 8
    assert "typedef struct pya_centroid_params {" in text
    assert re.search(r"uint64_t\s+pya_centroid_workspace_bytes\s*\(", text)
    for name in ("pya_centroid_spectra", "pya_centroid_spectra_host"):
        assert re.search(r"int\s+%s\s*\(" % name, text), name
    for name in ("pya_centroid_workspace_bytes", "pya_centroid_spectra", "pya_centroid_spectra_host"):
        assert name in _lib.SYMBOLS, name
    p = _lib.CentroidParams
    assert (p.gap0.offset, p.gap_per_mz.offset, p.min_height.offset, p.half_width.offset, p.area.offset, p.reserved.offset) == (0, 8, 16, 24, 28, 32)
    assert not [k for k in dir(_lib) if k.startswith("PYA_FLAG_") and "CENTROID" in k]     # a transform in front of a plan, not a flag


def test_score_batch_argument_checking():
    from pyascore_amd.ascore import _centroid_request
    params, select = _centroid_request(dict(gap=0.01, half_width=8, select=[1, 0, 1]), 3)
    assert params == ru.centroid_params(0.01, half_width=8) and select.dtype == np.uint8 and select.tolist() == [1, 0, 1]
    assert _centroid_request(dict(gap=0.01))[1] is None
    for bad in (True, dict(), dict(gap=None), dict(gap=0.01, width=3), dict(gap=0.01, half_width=0), dict(gap=[1, 2]),
                dict(gap=0.01, select=[1, 0]), dict(gap=0.01, select=[[1, 0, 1]]), dict(gap=0.01, select=[0.5, 1.0, 1.0])):
        with pytest.raises(ValueError):
            _centroid_request(bad, 3)
