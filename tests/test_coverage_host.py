"""The host restatement of the coverage records (pyascore_amd.rollup.coverage) held to the yardstick of tests/coverage_ref.py,
the record's invariants, and the public surface: header, bindings, record size, command line.  Winners and cumulative counts
come from the reference's C++ core (oracle/_ref).  No GPU."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import coverage_ref
import strip_cases as sc
from conftest import checker_kind
from oracle import harness, orc
from pyascore_amd import _lib, rollup as ru, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}


def _reference(settings, batch):
    """best_sig, n_sig, ps_off, ps_bits and ps_counts of a float64 batch from the reference's core"""
    scorer = harness.make_scorer(orc.OracleAscore, settings, kind=checker_kind())
    return harness.collect(scorer, batch, synth.unpack_psm)


def _case(name):
    """(settings, batch, reference results, yardstick) of a named batch, computed once"""
    if name not in _CACHE:
        if name == "cfg2":
            batch, settings = synth.make_batch("cfg2", n_psm=24, seed=4100)
        elif name == "general":                              # b/y/c/z, charges up to 3, one neutral loss
            batch, settings = synth.make_batch("cfg4", n_psm=12, seed=4101, max_charge=3)
        else:
            base, settings = synth.make_batch("cfg2", n_psm=24, seed=4100)
            batch = synth.narrow_batch(base, *{"f64_f32": (np.float64, np.float32), "f32_f32": (np.float32, np.float32)}[name])
        ref = _reference(settings, synth.widen_batch(batch))
        _CACHE[name] = (settings, batch, ref, coverage_ref.batch_records(settings, batch, ref, synth.unpack_psm))
    return _CACHE[name]


def _restated(settings, batch, ref, yard):
    off, ions, _, kept = yard
    fwd = "".join(c for c in settings["fragment_types"] if c in "bc")
    return ru.coverage(off, ions, batch["mz"], batch["intensity"], batch["peak_off"], np.diff(batch["pep_off"]), fwd, ref["n_sig"] > 0,
                       n_retained=kept)


def _same_bytes(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype == ru.COVERAGE_DTYPE and got.shape == want.shape, what
    bad = [i for i in range(got.size) if got[i].tobytes() != want[i].tobytes()]
    assert not bad, "%s: %d records differ, first PSM %d: got %r, want %r" % (what, len(bad), bad[0], got[bad[0]], want[bad[0]])


@pytest.mark.parametrize("name", ["cfg2", "general", "f64_f32", "f32_f32"])
def test_restatement_equals_the_yardstick(name):
    settings, batch, ref, yard = _case(name)
    got = _restated(settings, batch, ref, yard)
    _same_bytes(got, yard[2], name)
    assert (got["kind"] == _lib.PYA_COV_SCORED).all() and (got["n_fragments"] > 0).all() and (got["n_explained"] > 0).all(), name
    assert (got["pad"] == 0).all()
    if name == "general":
        ions = yard[1]
        assert set(chr(t) for t in ions["type"]) == set("bycz") and ions["charge"].max() == 3 and (ions["flags"] & 1).any()
        assert (got["nterm_current"] > 0).all() and (got["cterm_current"] > 0).all()


@pytest.mark.parametrize("name", ["cfg2", "general"])
def test_n_fragments_is_the_winners_deepest_cumulative_count(name):
    settings, batch, ref, yard = _case(name)
    for i in range(batch["n_psm"]):
        lo, hi = int(ref["ps_off"][i]), int(ref["ps_off"][i + 1])
        winner = lo + list(ref["ps_bits"][lo:hi]).index(ref["best_sig"][i])
        assert yard[2]["n_fragments"][i] == ref["ps_counts"][winner][settings["n_top"] - 1], (name, i)


@pytest.mark.parametrize("name", ["cfg2", "general", "f64_f32", "f32_f32"])
def test_currents_are_ordered_without_tolerance(name):
    settings, batch, ref, yard = _case(name)
    it = np.asarray(batch["intensity"], np.float64)
    assert np.isfinite(it).all() and (it >= 0).all()                   # (the condition of the claim)
    rec = yard[2]
    assert (rec["nterm_current"] <= rec["explained_current"]).all() and (rec["cterm_current"] <= rec["explained_current"]).all()
    assert (rec["explained_current"] <= rec["total_current"]).all()


@pytest.mark.parametrize("name", ["cfg2", "general", "f64_f32", "f32_f32"])
def test_explained_peaks_on_distinct_m_over_z(name):
    settings, batch, ref, yard = _case(name)
    off, ions, rec, _ = yard
    po = batch["peak_off"]
    for i in range(batch["n_psm"]):
        x = np.asarray(batch["mz"][po[i]:po[i + 1]]).astype(np.float32)
        assert np.unique(x).size == x.size, (name, i, "the generator repeats a float32 m/z")
        assert rec["n_explained"][i] == np.unique(ions["peak_mz"][off[i]:off[i + 1]]).size, (name, i)
        assert rec["n_explained"][i] <= rec["n_retained"][i] <= rec["n_peaks"][i] == x.size, (name, i)


def test_two_raw_peaks_of_one_float32_m_over_z_are_both_explained():
    """b1 of S + phospho and y1 of K; the y1 peak twice as float32 (two float64 values one float32 apart from nothing), and
    a NaN m/z that is never explained"""
    settings = dict(bin_size=100.0, n_top=10, mod_group="STY", mod_mass=79.966331, mz_error=0.05, fragment_types="by", neutral_losses=[])
    y1 = 147.113
    twin = float(np.nextafter(np.float64(np.float32(y1)), np.inf))           # rounds to the same float32
    assert np.float32(twin) == np.float32(y1) and twin != float(np.float32(y1))
    mz = np.array([88.04, y1, twin, 168.006, 227.08, 300.0])
    it = np.array([1.0, 20.0, 300.0, 4000.0, 50000.0, 600000.0])
    kw = dict(mz_arr=mz, int_arr=it, peptide="SK", n_of_mod=1, max_fragment_charge=1)
    ions = coverage_ref.section_one(settings, kw, 1)
    assert sorted(chr(t) for t in ions["type"]) == ["b", "y"]
    want = coverage_ref.record(settings, kw, ions)
    assert want["n_explained"] == 3 and want["n_fragments"] == 2 and want["explained_current"] == 4320.0
    assert want["nterm_current"] == 4000.0 and want["cterm_current"] == 320.0 and want["total_current"] == 654321.0
    assert (want["nterm_sizes"], want["cterm_sizes"], want["nterm_run"], want["cterm_run"], want["bonds"]) == (1, 1, 1, 1, 1)
    got = ru.coverage([0, ions.size], ions, mz, it, [0, mz.size], [2], "b", [True], n_retained=[int(want["n_retained"])])
    _same_bytes(got, np.array([want]), "twin peaks")
    # a NaN m/z takes part in the total only (appended behind the retained peaks: the yardstick's binning does not see it)
    mz2, it2 = np.append(mz, np.nan), np.append(it, 7000000.0)
    got2 = ru.coverage([0, ions.size], ions, mz2, it2, [0, mz2.size], [2], "b", [True], n_retained=[int(want["n_retained"])])[0]
    assert got2["n_explained"] == 3 and got2["explained_current"] == 4320.0 and got2["total_current"] == 7654321.0 and got2["n_peaks"] == 7
    # not scored: the all-zero record
    none = ru.coverage([0, 0], ions[:0], mz, it, [0, mz.size], [2], "b", [False])
    assert none.tobytes() == bytes(64)


def test_the_sum_is_in_the_stated_order():
    """values whose sum depends on the order: lane 0 takes elements 0 and 64, the partials are added in lane order"""
    y = np.zeros(130)
    y[0], y[1], y[64], y[65] = 1e16, 1.0, -1e16, 1.0
    # p[0] = (0 + 1e16) + -1e16 = 0, p[1] = (0 + 1) + 1 = 2: 2.0; in index order 1e16 + 1 loses the 1
    assert coverage_ref.lane_sum(y.tolist()) == 2.0 == ru._lane_sum(y.tolist()) and float(np.cumsum(y)[-1]) != 2.0
    ions = np.zeros(0, np.dtype(_lib.ION_DTYPE))
    rec = ru.coverage([0, 0], ions, np.linspace(100.0, 900.0, 130), y, [0, 130], [5], "b", [True])[0]
    assert rec["total_current"] == 2.0 and rec["explained_current"] == 0.0 and rec["kind"] == 1 and rec["n_fragments"] == 0


def test_ratios():
    rec = np.zeros(3, ru.COVERAGE_DTYPE)
    rec["total_current"], rec["explained_current"], rec["nterm_current"], rec["cterm_current"] = [8.0, 0.0, 4.0], [2.0, 0.0, 4.0], [1.0, 0.0, 0.0], [2.0, 0.0, 4.0]
    rec["n_explained"], rec["n_retained"] = [3, 0, 5], [12, 0, 5]
    r = ru.coverage_ratios(rec)
    assert r["explained"].tolist() == [0.25, 0.0, 1.0] and r["nterm"].tolist() == [0.125, 0.0, 0.0]
    assert r["cterm"].tolist() == [0.25, 0.0, 1.0] and r["peaks"].tolist() == [0.25, 0.0, 1.0]


def test_stripping_gives_the_clean_records_and_a_planted_precursor_costs_coverage(capsys):
    """The 120 cfg2 PSMs of tests/test_strip_host.py: clean, with the planted precursor family, stripped.  The direction is
    asserted; the means are printed (DESIGN section 8 records them)."""
    batch, settings = synth.make_batch("cfg2", n_psm=120, seed=5, mz_error=0.05)
    dirty, prec_mz, prec_z = sc.with_precursors(batch, 0.05)
    mz, it, off, _ = ru.strip(dirty["mz"], dirty["intensity"], dirty["peak_off"], prec_mz, prec_z, sc.effect_params(0.05))
    stripped = dict(dirty, mz=mz, intensity=it, peak_off=off)
    means = {}
    recs = {}
    for tag, b in (("clean", batch), ("dirty", dirty), ("stripped", stripped)):
        ref = _reference(settings, b)
        yard = coverage_ref.batch_records(settings, b, ref, synth.unpack_psm)
        recs[tag] = _restated(settings, b, ref, yard)
        _same_bytes(recs[tag], yard[2], tag)
        means[tag] = float(ru.coverage_ratios(recs[tag])["explained"].mean())
    _same_bytes(recs["stripped"], recs["clean"], "stripped against clean")
    with capsys.disabled():
        print("\nmean explained ratio, 120 cfg2 PSMs: clean %.4f, with the precursor family %.4f, stripped %.4f"
              % (means["clean"], means["dirty"], means["stripped"]))
    assert means["dirty"] < means["clean"]


def test_header_and_bindings_declare_the_interface():
    text = open(os.path.join(ROOT, "include", "pyascore_hip.h")).read()
    assert re.search(r"#define\s+PYA_FLAG_COVERAGE\s+8192u", text)
    assert re.search(r"int\s+pya_plan_coverage\s*\(\s*pya_plan\s*\*", text) and re.search(r"int\s+pya_last_batch_coverage\s*\(\s*pya_handle\s*\*", text)
    assert "typedef struct pya_coverage" in text and "#define PYA_COV_NONE 0" in text and "#define PYA_COV_SCORED 1" in text
    from pyascore_amd import ascore, device
    lib = _lib.load()
    assert _lib.PYA_FLAG_COVERAGE == 8192
    for name in ("pya_plan_coverage", "pya_last_batch_coverage"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert ctypes.sizeof(_lib.Coverage) == 64 == ru.COVERAGE_DTYPE.itemsize
    assert device.COVERAGE_DTYPE == ascore.COVERAGE_DTYPE == ru.COVERAGE_DTYPE == coverage_ref.DTYPE
    assert [f[0] for f in _lib.Coverage._fields_] == list(ru.COVERAGE_DTYPE.names)
    for name, _ in _lib.Coverage._fields_:
        assert getattr(_lib.Coverage, name).offset == ru.COVERAGE_DTYPE.fields[name][1], name
    raw = np.arange(2 * 64, dtype=np.uint8).reshape(2, 64)
    rec = device.coverage_records(raw)
    assert rec.shape == (2,) and rec["n_peaks"][0] == int.from_bytes(bytes(range(32, 36)), "little") and rec["kind"][1] == 64 + 58


def test_command_line_lists_the_option_and_the_fields():
    out = subprocess.run([sys.executable, "-m", "pyascore_amd", "--help"], cwd=ROOT, capture_output=True, text=True, check=True).stdout
    assert "--coverage" in out
    from pyascore_amd import batch_cli
    rec = np.zeros(1, ru.COVERAGE_DTYPE)
    rec[0] = (8.0, 2.0, 1.0, 2.0, 40, 12, 3, 5, 2, 3, 2, 1, 4, 1, [0] * 5)
    ratios = {k: v[0] for k, v in ru.coverage_ratios(rec).items()}
    fields = batch_cli.coverage_fields(rec[0], ratios)
    assert fields == ["1", "8.0", "2.0", "1.0", "2.0", "40", "12", "3", "5", "2", "3", "2", "1", "4", "0.25", "0.125", "0.25", "0.25"]
    assert len(batch_cli.COVERAGE_COLUMNS) == 2 + len(fields)
