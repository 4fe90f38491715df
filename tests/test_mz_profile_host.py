"""The host side of the fragment mass-error profile (pya_mz_profile): the numpy restatement pyascore_amd.rollup.mz_profile over
the ion records tests/ions_ref.py builds for the golden vectors, its bin rules on hand-made records, merging, the summary, and
the public surface (header, bindings).  No GPU."""
import os
import re

import numpy as np
import pytest

import evidence_ref
import ions_ref
from conftest import GOLDEN
from oracle import harness
from pyascore_amd import _lib, rollup as ru, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["edge_err05", "edge_nl", "edge_Zc", "velos_z1"]
BINS, BANDS, HALF = ru.MZP_BINS, ru.MZP_BANDS, ru.MZP_BINS // 2
_cache = {}


def _golden(case):
    """(settings, ion_off, ions, n_sig) of a golden case, built once"""
    if case not in _cache:
        settings, batch, exp = harness.load_case(os.path.join(GOLDEN, case + ".npz"))
        res = dict(best_sig=exp["best_sig"], alt_mask=exp["alt_mask"], ascores=exp["ascores"], n_sig=exp["n_sig"])
        ev, _ = evidence_ref.batch_rows(settings, batch, res, exp, synth.unpack_psm)
        off, rec = ions_ref.batch_records(settings, batch, res, ev, synth.unpack_psm)
        _cache[case] = (settings, off, rec, np.asarray(exp["n_sig"]))
    return _cache[case]


def _params(settings, **kw):
    kw.setdefault("max_rank", settings["n_top"] - 1)
    return ru.mz_profile_params(kw.pop("da_half_width", float(np.float32(settings["mz_error"]))), **kw)


def _check_invariants(table, off, rec, n_sig, run):
    run = np.zeros(n_sig.size, np.int64) if run is None else np.asarray(run)
    psm = np.repeat(np.arange(n_sig.size), np.diff(off))
    first = rec["site"] == ions_ref.WINNER
    for s, t in enumerate(table):
        assert int(t["da"].sum()) + int(t["out_da"].sum()) == t["n_ions"], s
        assert int(t["ppm"].sum()) + int(t["out_ppm"].sum()) == t["n_ions"], s
        mine = (run == s) & (n_sig > 0)
        assert t["n_psm"] == mine.sum(), s
        assert int(t["n_ions"]) + int(t["n_rank_skipped"]) == int((first & mine[psm]).sum()), s
        assert t["reserved"] == 0


def _hand(theo, peak, rank=None):
    rec = np.zeros(len(theo), ions_ref.DTYPE)
    rec["theo_mz"], rec["peak_mz"], rec["site"] = theo, peak, ions_ref.WINNER
    rec["rank"] = 0 if rank is None else rank
    return np.array([0, len(theo)], np.int64), rec, np.array([1], np.int32)


@pytest.mark.parametrize("case", CASES)
def test_goldens_keep_the_invariants(case):
    settings, off, rec, n_sig = _golden(case)
    table = ru.mz_profile(off, rec, n_sig, None, 1, _params(settings))
    assert table.dtype.itemsize == 4128 and table.shape == (1,)
    assert table["n_ions"][0] > 0 and np.count_nonzero(table["da"][0].sum(axis=0)) >= 2, case
    _check_invariants(table, off, rec, n_sig, None)
    # section 2 and unmatched records are not ions of the profile
    assert table["n_ions"][0] + table["n_rank_skipped"][0] <= (rec["site"] == ions_ref.WINNER).sum() < rec.size
    # three slots, one of them empty, some PSMs left out
    run = np.arange(n_sig.size) % 3
    run[run == 1] = -1
    three = ru.mz_profile(off, rec, n_sig, run, 3, _params(settings))
    _check_invariants(three, off, rec, n_sig, run)
    assert three[1].tobytes() == bytes(4128) and three["n_psm"][[0, 2]].all()
    kept = ru.mz_profile(off, rec, n_sig, np.where(run < 0, -1, 0), 1, _params(settings))
    assert ru.merge_mz_profiles(three[:1], three[2:]).tobytes() == kept.tobytes()      # negative slots are left out, the rest add up
    assert kept["n_ions"][0] < table["n_ions"][0]


@pytest.mark.parametrize("case", CASES)
def test_out_of_range_and_max_rank(case):
    settings, off, rec, n_sig = _golden(case)
    err = float(np.float32(settings["mz_error"]))
    full = ru.mz_profile(off, rec, n_sig, None, 1, _params(settings))
    narrow = ru.mz_profile(off, rec, n_sig, None, 1, _params(settings, da_half_width=err / 8, ppm_half_width=1.0))
    _check_invariants(narrow, off, rec, n_sig, None)
    first = rec[(rec["site"] == ions_ref.WINNER) & (n_sig > 0)[np.repeat(np.arange(n_sig.size), np.diff(off))]]
    d = first["peak_mz"].astype(np.float64) - first["theo_mz"].astype(np.float64)
    assert narrow["out_da"][0, 0] == (d < -err / 8).sum() and narrow["out_da"][0, 1] == (d >= err / 8).sum()
    assert narrow["out_da"][0].sum() > 0 and narrow["out_ppm"][0].sum() > 0, case
    assert narrow["n_ions"][0] == full["n_ions"][0]
    top = ru.mz_profile(off, rec, n_sig, None, 1, _params(settings, max_rank=0))
    _check_invariants(top, off, rec, n_sig, None)
    assert top["n_ions"][0] == (first["rank"] == 0).sum() and top["n_rank_skipped"][0] == (first["rank"] > 0).sum()
    assert 0 < top["n_ions"][0] < full["n_ions"][0] and full["n_rank_skipped"][0] == 0


def test_permuting_and_splitting_gives_the_same_bytes():
    settings, off, rec, n_sig = _golden("velos_z1")
    n = n_sig.size
    run = np.arange(n) % 2
    p = _params(settings)
    want = ru.mz_profile(off, rec, n_sig, run, 2, p)
    perm = np.random.default_rng(5).permutation(n)
    parts = [rec[off[i]:off[i + 1]] for i in perm]
    p_off = np.concatenate([[0], np.cumsum([x.size for x in parts])]).astype(np.int64)
    got = ru.mz_profile(p_off, np.concatenate(parts), n_sig[perm], run[perm], 2, p)
    assert got.tobytes() == want.tobytes()
    cut = n // 3
    a = ru.mz_profile(off[:cut + 1], rec[:off[cut]], n_sig[:cut], run[:cut], 2, p)
    b = ru.mz_profile(off[cut:] - off[cut], rec[off[cut]:], n_sig[cut:], run[cut:], 2, p)
    assert ru.merge_mz_profiles(a, b).tobytes() == want.tobytes()
    assert ru.merge_mz_profiles(want).tobytes() == want.tobytes()
    with pytest.raises(ValueError):
        ru.merge_mz_profiles(want, want[:1])
    with pytest.raises(ValueError):
        ru.mz_profile(off, rec, n_sig, run, 1, p)                                       # a slot at or above n_slots


def test_bin_edges_on_hand_made_records():
    p = ru.mz_profile_params(0.5, ppm_half_width=64.0, band_width=256.0, max_rank=9)    # powers of two: every edge is exact
    assert p == dict(inv_da=64.0, inv_ppm=0.5, inv_band=1.0 / 256.0, max_rank=9)
    w = 1.0 / 64.0
    theo = np.full(8, 512.0, np.float32)
    delta = np.array([0.0, w, -w, 3 * w, -0.5, 0.5, 0.5 - w, -0.5 - w])
    off, rec, n_sig = _hand(theo, (theo + delta).astype(np.float32))
    assert np.array_equal(rec["peak_mz"].astype(np.float64) - 512.0, delta)            # (exact in float32 at 512)
    t = ru.mz_profile(off, rec, n_sig, None, 1, p)[0]
    want = np.zeros(BINS, np.int64)
    for q in (HALF, HALF + 1, HALF - 1, HALF + 3, 0, BINS - 1):                          # d == 0 -> bin 32; an edge -> the upper bin
        want[q] += 1
    assert np.array_equal(t["da"][2], want) and t["da"].sum() == 6                       # band 2 = [512, 768)
    assert list(t["out_da"]) == [1, 1]                                                   # -0.5 - w below, +0.5 at or above
    assert t["n_ions"] == 8 and t["n_psm"] == 1
    # ppm: 2^-10 at m/z 512 is 1.9 ppm, inside the 2-ppm bin that starts at 0; 2^-9 is 3.8 ppm, the next bin
    step = 2.0 ** -10
    off, rec, n_sig = _hand(np.full(5, 512.0, np.float32), (512.0 + np.array([0.0, step, -step, 2 * step, 40 * step])).astype(np.float32))
    t = ru.mz_profile(off, rec, n_sig, None, 1, p)[0]
    assert list(t["ppm"][2][HALF - 1:HALF + 2]) == [1, 2, 1] and t["ppm"].sum() == 4 and list(t["out_ppm"]) == [0, 1]
    # bands: the lower edge belongs to the band, the last band is open-ended
    off, rec, n_sig = _hand(np.array([255.9, 256.0, 1792.0, 5000.0], np.float32), np.array([255.9, 256.0, 1792.0, 5000.0], np.float32))
    t = ru.mz_profile(off, rec, n_sig, None, 1, p)[0]
    assert list(t["da"][:, HALF]) == [1, 1, 0, 0, 0, 0, 0, 2]
    # ranks and section-2 records
    off, rec, n_sig = _hand(np.full(4, 300.0, np.float32), np.full(4, 300.0, np.float32), rank=[0, 3, 4, 9])
    rec["site"][3] = 0
    t = ru.mz_profile(off, rec, n_sig, None, 1, dict(p, max_rank=3))[0]
    assert (t["n_ions"], t["n_rank_skipped"]) == (2, 1)
    assert ru.mz_profile(off, rec, np.array([0]), None, 1, p)[0].tobytes() == bytes(4128)      # n_sig 0: the PSM does not contribute
    assert ru.mz_profile(off, rec, np.array([-1]), None, 1, p)[0].tobytes() == bytes(4128)


def test_params_refuse_what_the_abi_refuses():
    for bad in (dict(da_half_width=0.0), dict(da_half_width=-1.0), dict(da_half_width=float("nan")), dict(da_half_width=float("inf")),
                dict(da_half_width=0.5, ppm_half_width=0.0), dict(da_half_width=0.5, band_width=-250.0),
                dict(da_half_width=0.5, band_width=float("inf")), dict(da_half_width=1e-320),
                dict(da_half_width=0.5, max_rank=16), dict(da_half_width=0.5, max_rank=-1), dict(da_half_width=0.5, max_rank=2.5)):
        with pytest.raises(ValueError):
            ru.mz_profile_params(**bad)
    p = ru.mz_profile_params(0.05, max_rank=15)
    assert p["inv_da"] == 32 / 0.05 and p["inv_ppm"] == 32 / 50.0 and p["inv_band"] == 1.0 / 250.0 and p["max_rank"] == 15


def test_summary_of_a_hand_made_table():
    p = ru.mz_profile_params(0.5, ppm_half_width=64.0, band_width=256.0)
    t = np.zeros(2, ru.MZ_PROFILE_DTYPE)
    t["da"][0, 1, HALF + 2] = 10            # everything in [2 w, 3 w): the median is the middle of the bin
    t["da"][0, 3, HALF + 2] = 10
    t["ppm"][0, 0, :] = 4                   # flat: median 0, quantiles at +-90 % of the half width, background 4 per bin
    t["n_ions"][0], t["n_psm"][0] = 20, 2
    t["out_da"][0] = [1, 2]
    rows = ru.mz_profile_summary(t, p)
    da, ppm = rows[0]["da"], rows[0]["ppm"]
    w = 1.0 / 64.0
    assert da["total"] == 20 and (da["below"], da["above"]) == (1, 2) and da["median"] == 2.5 * w
    assert da["q05"] == pytest.approx(2.05 * w, rel=1e-12) and da["q95"] == pytest.approx(2.95 * w, rel=1e-12) and da["background"] == 0.0
    assert da["band_medians"][1] == 2.5 * w and da["band_medians"][3] == 2.5 * w and np.isnan(da["band_medians"][0])
    assert ppm["total"] == 256 and ppm["median"] == 0.0 and ppm["background"] == 4.0
    assert ppm["q05"] == pytest.approx(-57.6) and ppm["q95"] == pytest.approx(57.6)
    assert rows[0]["n_psm"] == 2 and rows[0]["n_ions"] == 20
    assert rows[1]["da"]["total"] == 0 and np.isnan(rows[1]["da"]["median"])
    assert ru.mz_profile_summary(t)[0]["da"]["median"] == 2.5                             # without params: in bins


def test_header_and_bindings_declare_the_interface():
    text = open(os.path.join(ROOT, "include", "pyascore_hip.h")).read()
    assert re.search(r"#define\s+PYA_FLAG_MZ_PROFILE\s+2048u", text)
    assert re.search(r"#define\s+PYA_MZP_BANDS\s+8\b", text) and re.search(r"#define\s+PYA_MZP_BINS\s+64\b", text)
    assert re.search(r"#define\s+PYA_MZP_CHUNK\s+%du" % _lib.PYA_MZP_CHUNK, text)
    for name in ("pya_plan_mz_profile", "pya_set_mz_profile", "pya_last_batch_mz_profile"):
        assert re.search(r"int\s+%s\s*\(" % name, text), name
    assert "typedef struct pya_mz_profile {" in text and "typedef struct pya_mz_profile_params" in text
    assert _lib.PYA_FLAG_MZ_PROFILE == 2048 and (_lib.PYA_MZP_BANDS, _lib.PYA_MZP_BINS) == (8, 64)
    assert ru.MZ_PROFILE_DTYPE.itemsize == 4128 and ru.MZ_PROFILE_DTYPE.fields["da"][1] == 32
    assert ru.MZ_PROFILE_DTYPE.fields["ppm"][1] == 32 + 4 * BANDS * BINS
