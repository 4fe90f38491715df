"""The host side of the fragment m/z recalibration (pya_mz_calibration): the numpy restatements pyascore_amd.rollup.fit_mz_calibration
and .recalibrate on hand-made tables and arrays, the whole loop -- run wide, profile, fit, correct, re-run narrow -- with the
reference core as the scorer, and the public surface (header, bindings, argument checks, the calibration file).  No GPU."""
import os
import re

import numpy as np
import pytest

import evidence_ref
import ions_ref
from conftest import checker_kind
from oracle import harness, orc
from pyascore_amd import _lib, batch_cli, rollup as ru, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINS, BANDS, HALF = ru.MZP_BINS, ru.MZP_BANDS, ru.MZP_BINS // 2
P = ru.mz_profile_params(0.05, ppm_half_width=50.0, band_width=250.0, max_rank=9)
BIN_PPM = 50.0 / HALF                                                 # 1.5625 ppm, exact


def _table(n=1):
    return np.zeros(n, ru.MZ_PROFILE_DTYPE)


# ---- the fit on hand-made tables ----

def test_all_counts_in_one_bin():
    t = _table()
    t["ppm"][0, 3, 40] = 100
    c = ru.fit_mz_calibration(t, P)[0]
    assert c["ppm"][3] == (40.5 - HALF) / P["inv_ppm"] == 8.5 * BIN_PPM           # the bin's centre
    assert c["spread_ppm"][3] == np.float32(0.5 * (40.84 - 40.16) / P["inv_ppm"])  # 0.34 of a bin
    assert c["spread_ppm"][3] == pytest.approx(0.34 * BIN_PPM, rel=1e-6)
    assert list(c["n_signal"]) == [0, 0, 0, 100, 0, 0, 0, 0]
    assert (c["ppm"] == c["ppm"][3]).all()                                        # one fitted band among eight: the others copy it
    assert (np.delete(c["spread_ppm"], 3) == 0).all()


def test_flat_histogram_and_edge_bins_are_not_fitted():
    t = _table(2)
    t["ppm"][0, 2, :] = 7                                                         # flat: 4 h == floor4 everywhere, E == 0
    t["ppm"][1, 2, [0, 1, BINS - 2, BINS - 1]] = 1000                             # counts only in the four edge bins
    c = ru.fit_mz_calibration(t, P, min_ions=1)
    assert c[0].tobytes() == bytes(128)
    assert c[1].tobytes() == bytes(128)                                           # 4 x 1000 - 4000 == 0 in every edge bin


def test_threshold_at_four_times_min_ions():
    t = _table(2)
    t["ppm"][:, 1, 10] = 5                                                        # (the edge bins are empty: no floor)
    t["ppm"][0, 5, 20] = 19                                                       # E = 76, one ion below 4 x 20
    t["ppm"][1, 5, 20] = 20                                                       # E = 80 == 4 x 20
    c = ru.fit_mz_calibration(t, P, min_ions=20)
    assert list(c["n_signal"][0][[1, 5]]) == [5, 19] and list(c["n_signal"][1][[1, 5]]) == [5, 20]
    assert c[0]["ppm"].tobytes() == bytes(64) and (c[0]["spread_ppm"] == 0).all()  # nothing fitted: all zero apart from n_signal
    assert (c[1]["ppm"] == (20.5 - HALF) / P["inv_ppm"]).all() and c[1]["spread_ppm"][5] > 0
    # a floor shifts the threshold: E counts what stands ABOVE it
    t2 = _table()
    t2["ppm"][0, 5, :] = 3
    t2["ppm"][0, 5, 20] = 3 + 20
    c2 = ru.fit_mz_calibration(t2, P, min_ions=20)[0]
    assert c2["n_signal"][5] == 20 and c2["ppm"][5] == (20.5 - HALF) / P["inv_ppm"]
    assert ru.fit_mz_calibration(t2, P, min_ions=21)[0]["ppm"].tobytes() == bytes(64)


def test_nearest_fitted_band_and_ties():
    t = _table()
    t["ppm"][0, 2, 36] = 50
    t["ppm"][0, 6, 28] = 50
    c = ru.fit_mz_calibration(t, P)[0]
    lo, hi = (36.5 - HALF) / P["inv_ppm"], (28.5 - HALF) / P["inv_ppm"]
    assert list(c["ppm"]) == [lo, lo, lo, lo, lo, hi, hi, hi]                      # band 4 is as far from 2 as from 6: the lower
    assert list(c["spread_ppm"] > 0) == [False, False, True, False, False, False, True, False]


def test_quantiles_interpolate_inside_the_bin():
    t = _table()
    t["ppm"][0, 0, 30:34] = [10, 30, 40, 20]                                      # E = 400; 16 % = 64, 50 % = 200, 84 % = 336
    c = ru.fit_mz_calibration(t, P, min_ions=1)[0]
    p16, p50, p84 = 31 + (6400 - 4000) / 12000, 32 + (20000 - 16000) / 16000, 33 + (33600 - 32000) / 8000
    assert c["ppm"][0] == (p50 - HALF) / P["inv_ppm"]
    assert c["spread_ppm"][0] == np.float32(0.5 * (p84 - p16) / P["inv_ppm"])
    assert c["n_signal"][0] == 100


def test_counts_near_2_32_do_not_overflow():
    t = _table()
    big = 0xFFFFFFFF
    t["ppm"][0, 4, 33] = big
    t["ppm"][0, 4, 34] = big
    t["ppm"][0, 7, :] = big                                                       # flat at the top of the range: floor4 = 4 x big, E == 0
    c = ru.fit_mz_calibration(t, P)[0]
    assert c["n_signal"][4] == 0xFFFFFFFF                                         # 2 x big saturates the 32-bit count
    assert c["n_signal"][7] == 0
    assert c["ppm"][4] == (34.0 - HALF) / P["inv_ppm"]                            # the median is the edge between the two bins
    t["ppm"][0, 4, 34] = 0
    assert ru.fit_mz_calibration(t, P)[0]["n_signal"][4] == big


def test_empty_table_and_independent_slots():
    assert ru.fit_mz_calibration(_table(0), P).shape == (0,)
    t = _table(3)
    t["ppm"][0, 1, 40] = 30
    t["ppm"][2, 6, 20] = 30
    c = ru.fit_mz_calibration(t, P)
    assert c[1].tobytes() == bytes(128)
    one = _table()
    one["ppm"][0] = t["ppm"][2]
    assert ru.fit_mz_calibration(one, P)[0].tobytes() == c[2].tobytes() != c[0].tobytes()
    for bad in (0, -1, 2.5, 1 << 32):
        with pytest.raises(ValueError):
            ru.fit_mz_calibration(t, P, min_ions=bad)


# ---- the apply ----

KNOTS = [32.0, 28.0, 22.0, 15.0, 9.0, 4.0, 0.0, -3.0]


def _cal(knots=KNOTS, n=1):
    c = np.zeros(n, ru.MZ_CALIBRATION_DTYPE)
    c["ppm"][:] = knots
    return c


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_zero_record_is_the_identity(dtype):
    rng = np.random.default_rng(1)
    mz = np.sort(rng.uniform(50.0, 2500.0, 500)).astype(dtype)
    got = ru.recalibrate(mz, [0, 200, 200, 500], None, _cal([0.0] * 8))
    assert got.dtype == mz.dtype and got.tobytes() == mz.tobytes() and got is not mz


def test_knots_at_band_centres_and_clamping():
    centres = (np.arange(BANDS) + 0.5) * 250.0
    got = ru.recalibrate(centres, [0, BANDS], None, _cal())
    assert np.array_equal(got, centres - centres * (np.array(KNOTS) * 1e-6))
    # below the centre of band 0 and above that of band 7 the error is the end knot's
    ends = np.array([1.0, 60.0, 124.9, 1875.1, 3000.0, 1e6])
    got = ru.recalibrate(ends, [0, 6], None, _cal())
    e = np.array([32.0, 32.0, 32.0, -3.0, -3.0, -3.0])
    assert np.array_equal(got, ends - ends * (e * 1e-6))
    # halfway between two centres: the mean of the knots
    assert ru.recalibrate(np.array([250.0]), [0, 1], None, _cal())[0] == 250.0 - 250.0 * (30.0 * 1e-6)
    f32 = ru.recalibrate(centres.astype(np.float32), [0, BANDS], None, _cal())
    assert f32.dtype == np.float32 and np.array_equal(f32, got_f32(centres))


def got_f32(centres):
    c32 = centres.astype(np.float32).astype(np.float64)
    return (c32 - c32 * (np.array(KNOTS) * 1e-6)).astype(np.float32)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_values_that_are_no_mz_pass_through(dtype):
    mz = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -5.0, 500.0], dtype)
    got = ru.recalibrate(mz, [0, 7], None, _cal())
    assert got[:6].tobytes() == mz[:6].tobytes() and got[6] < mz[6]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_ascending_spectra_stay_non_descending(dtype):
    rng = np.random.default_rng(2)
    for trial in range(20):
        knots = rng.uniform(-1000.0, 1000.0, 8)
        if trial == 0:
            knots = np.array([1000.0, -1000.0] * 4)
        mz = np.sort(np.concatenate([rng.uniform(1.0, 2500.0, 4000), (np.arange(BANDS) + 0.5) * 250.0,
                                     np.nextafter((np.arange(1, BANDS) + 0.5) * 250.0, 0)])).astype(dtype)
        got = ru.recalibrate(mz, [0, mz.size], None, _cal(knots))
        assert (np.diff(got.astype(np.float64)) >= 0).all(), knots


def test_slots():
    mz = np.full(6, 500.0)
    cal = _cal(n=2)
    cal["ppm"][1] = 10.0
    got = ru.recalibrate(mz, [0, 2, 4, 6], [1, -1, 0], cal)
    assert got[0] == got[1] == 500.0 - 500.0 * (10.0 * 1e-6) and got[2] == got[3] == 500.0
    assert got[4] == 500.0 - 500.0 * ((28.0 + (22.0 - 28.0) * 0.5) * 1e-6)                # u = 1.5: halfway between the centres of bands 1 and 2
    with pytest.raises(ValueError, match="slot 2"):
        ru.recalibrate(mz, [0, 2, 4, 6], [1, 2, 0], cal)
    with pytest.raises(ValueError):
        ru.recalibrate(mz, [0, 2, 4, 6], [0, 0], cal)
    for bad in (np.nan, np.inf, 1000.5, -1001.0):
        c = _cal()
        c["ppm"][0, 4] = bad
        with pytest.raises(ValueError, match="knot"):
            ru.recalibrate(mz, [0, 6], None, c)
    with pytest.raises(ValueError):
        ru.recalibrate(mz.astype(np.int32), [0, 6], None, cal)
    # peak_off that does not start at 0: what lies in front is copied
    got = ru.recalibrate(mz, [2, 6], None, cal)
    assert got[0] == got[1] == 500.0 and got[2] < 500.0


def test_suggest_mz_error():
    c = _cal(n=2)
    c["spread_ppm"][1, 3] = 2.5
    assert ru.suggest_mz_error(c, 2000.0) == 3.0 * 2.5 * 1e-6 * 2000.0
    assert ru.suggest_mz_error(c[:1], 2000.0) == 0.0 and ru.suggest_mz_error(c[:0], 2000.0) == 0.0


# ---- the loop, with the reference core as the scorer ----

def _reference(settings, mz_error):
    return harness.make_scorer(orc.OracleAscore, dict(settings, mz_error=mz_error), kind=checker_kind())


def test_the_loop_recovers_an_injected_drift():
    """120 cfg2 PSMs generated for a 0.01 Da tolerance, their m/z drifted by 32 .. -3 ppm over the bands.  Measured with the
    definitions here: the uncorrected narrow run agrees with the clean run's best_sig on 101 of 120 PSMs, the corrected one
    on 120; the largest distance of a fitted knot from the injected one is 1.06 ppm; the thinnest band has 82 signal ions."""
    batch, settings = synth.make_batch("cfg2", n_psm=120, seed=3, mz_error=0.01)
    drift = _cal()
    clean = _reference(settings, 0.01).score_batch(batch)
    # the drift is the inverse direction of the correction: observed = true (1 + e 1e-6), e interpolated as the apply does
    e = (batch["mz"] - ru.recalibrate(batch["mz"], batch["peak_off"], None, drift)) / batch["mz"] * 1e6
    drifted = dict(batch, mz=batch["mz"] * (1.0 + e * 1e-6))
    narrow = _reference(settings, 0.01).score_batch(drifted)
    agree_before = int((narrow["best_sig"] == clean["best_sig"]).sum())
    wide_settings = dict(settings, mz_error=0.05)
    wide = _reference(settings, 0.05).score_batch(drifted)
    none = np.zeros((120, wide["ascores"].shape[1]), evidence_ref.DTYPE)          # (no evidence rows: the winner's section alone)
    off, rec = ions_ref.batch_records(wide_settings, drifted, wide, none, synth.unpack_psm)
    params = ru.mz_profile_params(0.05, ppm_half_width=50.0, max_rank=9)
    table = ru.mz_profile(off, rec, wide["n_sig"], None, 1, params)
    cal = ru.fit_mz_calibration(table, params, min_ions=20)
    fitted = cal["n_signal"][0] >= 20
    worst = float(np.abs(cal["ppm"][0] - np.array(KNOTS))[fitted].max())
    corrected = dict(drifted, mz=ru.recalibrate(drifted["mz"], drifted["peak_off"], None, cal))
    again = _reference(settings, 0.01).score_batch(corrected)
    agree_after = int((again["best_sig"] == clean["best_sig"]).sum())
    print("agree before %d, after %d of 120; worst fitted knot %.3f ppm off; signal ions %s; mean best_score clean %.1f, drifted %.1f, "
          "corrected %.1f" % (agree_before, agree_after, worst, cal["n_signal"][0].tolist(), clean["best_score"].mean(),
                              narrow["best_score"].mean(), again["best_score"].mean()))
    assert agree_before <= 108                                                    # the input is hard
    assert agree_after >= 114
    assert fitted.sum() >= 6 and worst <= 2 * BIN_PPM


# ---- the surface ----

def test_header_and_bindings_declare_the_interface():
    text = open(os.path.join(ROOT, "include", "pyascore_hip.h")).read()
    assert re.search(r"#define\s+PYA_FLAG_RECALIBRATE\s+4096u", text) and _lib.PYA_FLAG_RECALIBRATE == 4096
    assert re.search(r"#define\s+PYA_MZC_MAX_PPM\s+1000\b", text) and _lib.PYA_MZC_MAX_PPM == 1000
    for name in ("pya_mz_profile_fit", "pya_mz_profile_fit_host", "pya_recalibrate_spectra", "pya_set_recalibration"):
        assert re.search(r"int\s+%s\s*\(" % name, text), name
        assert name in _lib.SYMBOLS, name
    assert "typedef struct pya_mz_calibration {" in text
    d = ru.MZ_CALIBRATION_DTYPE
    assert d.itemsize == 128 and d.fields["ppm"][1] == 0 and d.fields["spread_ppm"][1] == 64 and d.fields["n_signal"][1] == 96
    flags = [getattr(_lib, k) for k in dir(_lib) if k.startswith("PYA_FLAG_")]
    assert len(set(flags)) == len(flags)                                          # no flag bit is taken twice


def test_score_batch_argument_checking():
    from pyascore_amd.ascore import _recalibrate_request
    cal = _cal(n=2)
    ok = _recalibrate_request(dict(calibration=cal, run=[0, 1, -1]), 3)
    assert ok["run"].dtype == np.int32 and ok["inv_band"] == 1.0 / 250.0 and ok["cal"].tobytes() == cal.tobytes()
    assert _recalibrate_request(dict(calibration=cal), 3)["run"] is None
    bad_knot = _cal()
    bad_knot["ppm"][0, 0] = np.nan
    for bad in (True, [cal], dict(), dict(calibration=None), dict(calibration=cal, slots=1), dict(calibration=cal, run=[0, 1]),
                dict(calibration=cal, run=[0.5, 1.0, 2.0]), dict(calibration=cal, run=[0, 1, 1 << 31]), dict(calibration=cal, band_width=0.0),
                dict(calibration=cal, band_width=-250.0), dict(calibration=cal, band_width=float("nan")), dict(calibration=bad_knot)):
        with pytest.raises(ValueError):
            _recalibrate_request(bad, 3)


def test_the_calibration_file_round_trips(tmp_path):
    rng = np.random.default_rng(4)
    cal = np.zeros(3, ru.MZ_CALIBRATION_DTYPE)
    cal["ppm"] = rng.uniform(-40.0, 40.0, (3, 8))
    cal["ppm"][1, 2] = -0.0
    cal["spread_ppm"] = rng.uniform(0.0, 6.0, (3, 8)).astype(np.float32)
    cal["n_signal"] = rng.integers(0, 1 << 32, (3, 8), dtype=np.uint64)
    path = tmp_path / "cal.tsv"
    batch_cli.write_mz_calibration_tsv(cal, 1.0 / (1.0 / 300.0), str(path))
    lines = path.read_text().splitlines()
    assert lines[0].split("\t") == list(batch_cli.MZ_CALIBRATION_COLUMNS) and len(lines) == 1 + 3 * BANDS
    assert lines[1].split("\t")[:3] == ["0", "0", "150.0"]
    back, width = ru.read_mz_calibration(str(path))
    assert back.tobytes() == cal.tobytes() and width == 300.0
    path.write_text("\n".join(lines[:-1]) + "\n")                                # a band is missing
    with pytest.raises(ValueError):
        ru.read_mz_calibration(str(path))
    path.write_text(lines[0] + "\n")
    empty, _ = ru.read_mz_calibration(str(path))
    assert empty.shape == (0,)
