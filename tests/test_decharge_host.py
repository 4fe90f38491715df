"""The host side of charge deconvolution (pya_decharge_params): the numpy restatement pyascore_amd.rollup.decharge on hand-made
spectra whose outcome is written out by hand (tests/decharge_cases.py), its properties on dense spectra and on ladders, what
multiply charged fragments cost and what the rule gives back with the reference core as the scorer, and the public surface
(header, bindings, argument checks).  No GPU."""
import os
import re

import numpy as np
import pytest

import decharge_cases as cc
import deisotope_cases as dc
from conftest import checker_kind
from oracle import harness, orc
from pyascore_amd import _lib, rollup as ru, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = cc.hand_cases()


# ---- the rule, one case each ----

@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hand_made_spectrum(case):
    x, y = case["mz"], case["intensity"]
    mz, it, off, charge, keep = ru.decharge(x, y, [0, x.size], case["params"])
    assert keep.tolist() == case["keep"].tolist()
    assert mz.dtype == x.dtype and it.dtype == y.dtype and charge.dtype == np.uint8
    assert charge.tolist() == case["charge"].tolist()
    assert mz.tobytes() == case["out_mz"].tobytes(), (mz.tolist(), case["out_mz"].tolist())
    assert it.tobytes() == case["out_it"].tobytes()
    assert off.dtype == np.int64 and off.tolist() == [0, int(case["keep"].sum())]
    # the kept set is deisotoping's, whatever moved
    assert ru.deisotope(x, y, [0, x.size], case["params"])[3].tolist() == case["keep"].tolist()


def test_hand_made_spectra_agree_with_all_pairs():
    for case in CASES:
        if case["unordered"]:
            continue
        order, value, c, keep = cc.all_pairs(case["mz"], case["intensity"], case["params"], case["mz"].dtype)
        assert keep.tolist() == case["keep"].tolist(), case["name"]
        assert value[order].tolist() == case["out_mz"].astype(np.float64).tolist() and c[order].tolist() == case["charge"].tolist(), case["name"]
        assert case["intensity"][order].tobytes() == case["out_it"].tobytes(), case["name"]


def test_a_descending_spectrum_among_good_ones_empty_spectra_and_offsets_that_do_not_start_at_zero():
    group = [c for c in CASES if c["params"] is cc.P_EXACT and c["mz"].dtype == np.float64]
    assert sum(c["unordered"] for c in group) == 1 and not group[0]["unordered"] and not group[-1]["unordered"] and len(group) >= 10
    mz, it, off = cc.pack([(c["mz"], c["intensity"]) for c in group], gaps=True)
    assert (np.diff(off) == 0).sum() == len(group)
    f_mz, f_it, f_off, charge, keep = ru.decharge(mz, it, off, cc.P_EXACT)
    assert keep.tolist() == np.concatenate([c["keep"] for c in group]).tolist()
    assert f_mz.tobytes() == np.concatenate([c["out_mz"] for c in group]).tobytes()
    assert f_it.tobytes() == np.concatenate([c["out_it"] for c in group]).tobytes()
    assert charge.tolist() == np.concatenate([c["charge"] for c in group]).tolist()
    assert np.diff(f_off)[0::2].tolist() == [int(c["keep"].sum()) for c in group] and np.diff(f_off)[1::2].tolist() == [0] * len(group)
    # the same spectra behind 5 peaks nobody names: the output starts at 0 all the same
    pad = np.full(5, 123.0)
    g = ru.decharge(np.concatenate([pad, mz]), np.concatenate([pad, it]), off + 5, cc.P_EXACT)
    assert g[0].tobytes() == f_mz.tobytes() and g[2].tolist() == f_off.tolist() and g[3].tolist() == charge.tolist() and g[4].tolist() == keep.tolist()
    # no spectra at all, and spectra without a peak
    e = np.zeros(0)
    assert ru.decharge(e, e, [0], cc.P0)[2].tolist() == [0]
    r = ru.decharge(e, e, [0, 0, 0], cc.P0)
    assert r[2].tolist() == [0, 0, 0] and r[3].size == 0 and r[3].dtype == np.uint8
    with pytest.raises(ValueError):
        ru.decharge(np.zeros(mz.size, np.int64), it, off, cc.P_EXACT)
    with pytest.raises(ValueError):
        ru.decharge(mz, it, off + 5, cc.P_EXACT)
    with pytest.raises(ValueError):
        ru.decharge(mz, it, off[::-1], cc.P_EXACT)


def test_parameters_that_are_refused():
    ok = ru.decharge_params()
    iso = ru.deisotope_params()
    assert {k: ok[k] for k in iso} == iso and ok["carrier"] == 1.007825 == synth.PROTON == _lib.PYA_DECHARGE_CARRIER and ok["witness"] == 0.3
    assert ru.decharge_params(0.02, 2, 1.003, 0.8, 1e-4, 1.00728, 0.1) == dict(ru.deisotope_params(0.02, 2, 1.003, 0.8, 1e-4), carrier=1.00728,
                                                                                  witness=0.1)
    for bad in (dict(tol=-0.001), dict(max_charge=0), dict(max_charge=9), dict(step=0.0), dict(ratio=float("inf")), dict(tol=0.2),
                dict(carrier=0.0), dict(carrier=-1.0), dict(carrier=float("nan")), dict(carrier=float("inf")), dict(witness=-0.1),
                dict(witness=float("nan")), dict(witness=float("inf"))):
        with pytest.raises(ValueError):
            ru.decharge_params(**bad)
    assert ru.decharge_params(witness=0.0)["witness"] == 0.0
    base = dict(tol=0.01, ratio0=1.0, ratio_per_mz=0.0, max_charge=2, spacing=(1.0, 0.5), carrier=1.0, witness=0.25)
    assert ru.check_decharge_params(base) == base
    for bad in (dict(base, spacing=(0.5, 1.0)), dict(base, carrier=0.0), dict(base, witness=-1.0), {k: v for k, v in base.items() if k != "carrier"},
                {k: v for k, v in base.items() if k != "witness"}, ru.deisotope_params(), {}, None):
        with pytest.raises(ValueError):
            ru.check_decharge_params(bad)
    c = ru.decharge_c_params(base)
    assert (c.iso.tol, c.iso.ratio0, c.iso.ratio_per_mz, c.iso.max_charge, c.iso.reserved) == (0.01, 1.0, 0.0, 2, 0)
    assert list(c.iso.spacing) == [1.0, 0.5] + [0.0] * 6 and (c.carrier, c.witness) == (1.0, 0.25)


# ---- properties on dense spectra and on ladders ----

def _inputs():
    batch, _ = dc.dense_batch()
    yield "dense", batch["mz"], batch["intensity"], batch["peak_off"]
    yield "boundary", *dc.pack(dc.boundary_spectra(), gaps=False)
    yield "charged boundary", *cc.pack(cc.charged_boundary_spectra(), gaps=False)


@pytest.fixture(scope="module", params=["dense", "boundary", "charged boundary"])
def spectra(request):
    name, mz, it, off = next(i for i in _inputs() if i[0] == request.param)
    return name, mz, it, off, ru.decharge(mz, it, off, cc.P0), ru.deisotope(mz, it, off, cc.P0)


def test_the_kept_peaks_are_deisotopings(spectra):
    name, mz, it, off, (o_mz, o_it, o_off, charge, keep), (d_mz, d_it, d_off, d_keep) = spectra
    assert keep.tolist() == d_keep.tolist() and o_off.tobytes() == d_off.tobytes()
    assert o_mz.size == o_it.size == charge.size == int(o_off[-1])
    for a, b in zip(o_off[:-1], o_off[1:]):                               # the same intensities, bit for bit, as a multiset
        assert np.sort(o_it[a:b].view(np.uint64)).tobytes() == np.sort(d_it[a:b].view(np.uint64)).tobytes()
    assert (charge > 1).any() and charge.max() <= 3 and charge.min() == 1, name


def test_max_charge_1_gives_deisotopes_bytes(spectra):
    name, mz, it, off = spectra[:4]
    for types in ((np.float64, np.float64), (np.float64, np.float32), (np.float32, np.float32)):
        x, y = mz.astype(types[0]), it.astype(types[1])
        p1 = ru.decharge_params(max_charge=1)
        got, want = ru.decharge(x, y, off, p1), ru.deisotope(x, y, off, ru.deisotope_params(max_charge=1))
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and got[2].tobytes() == want[2].tobytes()
        assert got[0].dtype == types[0] and got[1].dtype == types[1] and (got[3] == 1).all() and got[4].tolist() == want[3].tolist()


def test_the_output_ascends(spectra):
    o_mz, _, o_off = spectra[4][:3]
    for a, b in zip(o_off[:-1], o_off[1:]):
        assert (np.diff(o_mz[a:b]) >= 0).all()


def test_all_pairs_agree_and_charge_1_means_the_bits_of_the_peak(spectra):
    """the definition with no search, no walk and no sort of the whole: all pairs of a spectrum as matrices (spectra of up to
    2 000 peaks); with the raw index of every output peak known, charge == 1 <=> its m/z bits are the raw peak's"""
    name, mz, it, off, (o_mz, o_it, o_off, charge, keep), _ = spectra
    done = 0
    for s in range(off.size - 1):
        a, b = int(off[s]), int(off[s + 1])
        if b - a > 2000 or (name == "dense" and done >= 3):
            continue
        done += 1
        order, value, c, k = cc.all_pairs(mz[a:b], it[a:b], cc.P0, np.float64)
        oa, ob = int(o_off[s]), int(o_off[s + 1])
        assert k.tolist() == keep[a:b].tolist(), (name, s)
        assert o_mz[oa:ob].tobytes() == value[order].tobytes() and charge[oa:ob].tolist() == c[order].tolist(), (name, s)
        assert o_it[oa:ob].tobytes() == it[a:b][order].tobytes(), (name, s)
        same_bits = o_mz[oa:ob].view(np.uint64) == mz[a:b][order].view(np.uint64)
        assert (same_bits == (charge[oa:ob] == 1)).all(), (name, s)
    assert done >= 3


def test_float32_spectra_agree_with_all_pairs():
    mz, it, off = cc.pack(cc.charged_boundary_spectra(seed=5)[:9], np.float32, np.float32, gaps=False)
    o_mz, o_it, o_off, charge, _ = ru.decharge(mz, it, off, cc.P0)
    assert o_mz.dtype == np.float32 and (charge > 1).any()
    for s in range(off.size - 1):
        a, b = int(off[s]), int(off[s + 1])
        order, value, c, _ = cc.all_pairs(mz[a:b], it[a:b], cc.P0, np.float32)
        oa, ob = int(o_off[s]), int(o_off[s + 1])
        assert o_mz[oa:ob].tobytes() == value[order].astype(np.float32).tobytes() and charge[oa:ob].tolist() == c[order].tolist(), s
        assert ((o_mz[oa:ob].view(np.uint32) == mz[a:b][order].view(np.uint32)) == (charge[oa:ob] == 1)).all(), s


def test_every_and_no_kept_peak_moved():
    x, y = cc.all_moved_spectrum()
    mz, it, off, charge, keep = ru.decharge(x, y, [0, x.size], cc.P0)
    assert keep.tolist() == [True, False] * 150 and (charge == 2).all() and mz.tobytes() == (x[0::2] * 2.0 - 1.007825).tobytes()
    x, y = cc.none_moved_spectrum()
    mz, it, off, charge, keep = ru.decharge(x, y, [0, x.size], cc.P0)
    assert keep.tolist() == [True, False] * 150 and (charge == 1).all() and mz.tobytes() == x[0::2].tobytes()


# ---- what multiply charged fragments cost, with the reference core as the scorer ----

def test_charged_fragments_cost_score_and_the_rule_gives_it_back():
    """120 cfg2 PSMs generated for a 0.05 Da tolerance, plain settings (b/y at 1+).  With decharge_cases.charged(batch, 0.6) --
    60 % of the peaks at 2+ or 3+, two satellites behind every peak -- and the default parameters, measured with the
    definitions here: mean best_score clean 307.9, charged 92.3, deisotoped 100.3, decharged 307.0; best_sig equal to the clean
    run's on 71, 71 and 120 of 120 PSMs.  With share 0 (every peak 1+ with its satellites): 280.0, 307.9 and 307.6; 116, 119
    and 119; 166 of 38 357 kept peaks moved wrongly by chance witnesses.  The bounds below are the issue's and stand against
    these."""
    batch, settings = synth.make_batch("cfg2", n_psm=120, seed=5, mz_error=0.05)
    scorer = harness.make_scorer(orc.OracleAscore, dict(settings, mz_error=0.05), kind=checker_kind())
    clean_r = dict(scorer.score_batch(batch))
    m_clean = float(clean_r["best_score"].mean())
    seen = {}
    for share in (0.6, 0.0):
        dirty = cc.charged(batch, share)
        mz, it, off, _ = ru.deisotope(dirty["mz"], dirty["intensity"], dirty["peak_off"], dc.P0)
        deiso = dict(dirty, mz=mz, intensity=it, peak_off=off)
        mz, it, off, charge, _ = ru.decharge(dirty["mz"], dirty["intensity"], dirty["peak_off"], cc.P0)
        dechg = dict(dirty, mz=mz, intensity=it, peak_off=off)
        res = [dict(scorer.score_batch(b)) for b in (dirty, deiso, dechg)]
        means = [float(r["best_score"].mean()) for r in res]
        agree = [int((r["best_sig"] == clean_r["best_sig"]).sum()) for r in res]
        print("share %.1f: mean best_score clean %.1f charged %.1f deisotoped %.1f decharged %.1f; best_sig agreement %d / %d / %d of 120; "
              "%d of %d kept peaks moved" % (share, m_clean, means[0], means[1], means[2], agree[0], agree[1], agree[2],
                                             int((charge > 1).sum()), charge.size))
        seen[share] = (means, agree)
    means, agree = seen[0.6]
    assert means[0] <= m_clean - 150.0 and means[1] <= m_clean - 150.0
    assert abs(means[2] - m_clean) <= 3.0
    assert agree[2] >= 118 and agree[2] >= agree[1]
    means, agree = seen[0.0]
    assert abs(means[2] - m_clean) <= 2.0


# ---- the surface ----

def test_header_and_bindings_declare_the_interface():
    text = open(os.path.join(ROOT, "include", "pyascore_hip.h")).read()
    assert "typedef struct pya_decharge_params {" in text and re.search(r"#define\s+PYA_DECHARGE_CARRIER\s+1\.007825\b", text)
    assert re.search(r"uint64_t\s+pya_decharge_workspace_bytes\s*\(", text)
    for name in ("pya_decharge_spectra", "pya_decharge_spectra_host"):
        assert re.search(r"int\s+%s\s*\(" % name, text), name
    for name in ("pya_decharge_workspace_bytes", "pya_decharge_spectra", "pya_decharge_spectra_host"):
        assert name in _lib.SYMBOLS, name
    p = _lib.DechargeParams
    assert (p.iso.offset, p.iso.size, p.carrier.offset, p.witness.offset) == (0, 96, 96, 104)
    assert not [k for k in dir(_lib) if k.startswith("PYA_FLAG_") and "DECHARGE" in k]    # a transform in front of a plan, not a flag
    # the carrier is the scorer's: the literal the kernels add per charge
    src = open(os.path.join(ROOT, "pyascore_amd", "csrc", "device_common.hip.h")).read()
    assert "(float)(m + 1.007825)" in src


def test_score_batch_argument_checking():
    from pyascore_amd.ascore import PyAscore, _decharge_request
    assert _decharge_request(True) == ru.decharge_params()
    assert _decharge_request(dict(tol=0.02, max_charge=2, ratio=0.8, ratio_per_mz=1e-4, step=1.003, carrier=1.00728, witness=0.1)) == \
        ru.decharge_params(0.02, 2, 1.003, 0.8, 1e-4, 1.00728, 0.1)
    for bad in ([0.01], "yes", 3, dict(tolerance=0.01), dict(tol="wide"), dict(tol=-1.0), dict(max_charge=9), dict(witness=-0.5),
                dict(witness=float("nan")), dict(carrier=0.0), dict(witness="high")):
        with pytest.raises(ValueError):
            _decharge_request(bad)
    # the two combinations that are refused, before anything touches a device (no scorer is needed to see them)
    batch = dict(n_psm=0)
    with pytest.raises(ValueError, match="contains deisotoping"):
        PyAscore.score_batch(None, batch, decharge=True, deisotope=True)
    with pytest.raises(ValueError) as err:
        PyAscore.score_batch(None, batch, decharge=dict(witness=0.2), recalibrate=dict(calibration=None))
    for name in ("pya_recalibrate_spectra", "DevicePlan.recalibrate", "rollup.recalibrate"):
        assert name in str(err.value), name


def test_command_line_argument_checking():
    from pyascore_amd.__main__ import build_parser, parse_args
    files = ["spec.mzML", "ident.pepXML", "out.tsv"]
    args = parse_args(files)
    assert args.decharge is False and (args.decharge_tol, args.decharge_charge, args.decharge_ratio, args.decharge_witness) == (0.01, 3, 1.0, 0.3)
    args = parse_args(["--decharge", "--decharge_tol", "0.02", "--decharge_charge", "2", "--decharge_ratio", "0.8", "--decharge_witness", "0.1"] + files)
    assert args.decharge is True and (args.decharge_tol, args.decharge_charge, args.decharge_ratio, args.decharge_witness) == (0.02, 2, 0.8, 0.1)
    for bad in (["--decharge_charge", "9"], ["--decharge_charge", "0"], ["--decharge_tol", "-0.01"], ["--decharge_tol", "0.2"],
                ["--decharge_ratio", "nan"], ["--decharge_witness", "-1"], ["--decharge_witness", "nan"]):
        with pytest.raises(ValueError):
            parse_args(["--decharge"] + bad + files)
        parse_args(bad + files)                                            # (without --decharge the values are not looked at)
    with pytest.raises(ValueError, match="--deisotope"):
        parse_args(["--decharge", "--deisotope"] + files)
    with pytest.raises(ValueError, match="--mz_calibration"):
        parse_args(["--decharge", "--mz_calibration", "cal.tsv"] + files)
    parse_args(["--deisotope", "--mz_calibration", "cal.tsv"] + files)     # (deisotoping alone goes with a calibration)
    text = " ".join(build_parser().format_help().split())
    assert "leave --max_fragment_charge at 1" in text
