"""The precursor-purity stage on the host (pya_purity_params): tests/purity_ref.py, the rule in plain Python, pinned by the hand
cases of tests/purity_cases.py; pyascore_amd.rollup.purity / purity_gate byte for byte against it; planted survey scans; the
survey index, the ingest fields and every request check that needs no device."""
import math
import os

import numpy as np
import pytest

import purity_cases as pc
import purity_ref as ref
from pyascore_amd import _lib, rollup as ru

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ingest")
CASES = pc.hand_cases()


def _rollup_bytes(spectra, queries, params, mz_t=np.float64, it_t=np.float64):
    mz, it, off = pc.pack(spectra, mz_t, it_t)
    rec, over = ru.purity(mz, it, off, *queries, params)
    want, w_over = ref.purity(pc.as_lists(mz, it, off), pc.as_queries(*queries), params)
    assert rec.tobytes() == ref.to_bytes(want) and over == w_over
    return rec, over


# ---- the rule, pinned by hand ----

def test_the_records_are_48_bytes_and_the_parameters_40():
    assert ru.PURITY_DTYPE.itemsize == 48 == ref.RECORD.size and _lib.C.sizeof(_lib.PurityParams) == 40
    assert [ru.PURITY_DTYPE.fields[n][1] for n in ru.PURITY_DTYPE.names] == [0, 8, 16, 24, 32, 36, 40, 44]
    p = ru.purity_c_params(ru.purity_params())
    assert (p.tol, p.tol_ppm, p.step, p.below, p.isotopes, list(p.reserved)) == (0.0, 10.0, ru.STRIP_STEP, 0, 3, [0, 0])


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hand_pinned_records(case):
    sv, pm, pz, wl, wh = case["query"]
    got, over = ref.purity([case["peaks"]], [case["query"]], case["params"])
    assert ref.to_bytes(got) == ref.to_bytes([case["record"]]) and over == (0, None), (got, case["record"])
    for mz_t, it_t in ((np.float64, np.float64), (np.float64, np.float32), (np.float32, np.float32)):
        if mz_t == np.float32 and case["f64_only"]:
            continue
        mz, it, off, *queries = pc.pack_cases([case], mz_t, it_t, gaps=False)
        assert mz.astype(np.float64).tobytes() == np.asarray([p[0] for p in case["peaks"]]).tobytes()      # (nothing was rounded)
        assert it.astype(np.float64).tobytes() == np.asarray([p[1] for p in case["peaks"]]).tobytes()
        rec, _ = ru.purity(mz, it, off, *queries, case["params"])
        assert rec.tobytes() == ref.to_bytes([case["record"]]), (mz_t, it_t, rec)


def test_the_cases_cover_what_they_should():
    names = " | ".join(c["name"] for c in CASES)
    for what in ("window bounds", "bounds of centre 1", "(float32)", "outside the isolation window", "two centre windows", "NaN m/z",
                 "empty window", "win_lo > win_hi", "charge 0", "NaN precursor", "survey = -1", "below = 4 with isotopes = 11", "n_c = 1",
                 "larger y wins", "smaller x", "duplicate"):
        assert what in names, what
    assert sum(c["f64_only"] for c in CASES) == 2
    # one ulp is one ulp: the neighbours of the bounds differ from them in float32 as in float64
    assert pc.down(pc.WL) < pc.WL < pc.up(pc.WL) and pc.up(pc.WL, np.float32) - pc.WL == 2.0 ** -15 and pc.up(pc.WL) - pc.WL == 2.0 ** -44


def test_every_case_of_a_parameter_set_in_one_call():
    groups = {}
    for c in CASES:
        groups.setdefault(pc.params_key(c["params"]), []).append(c)
    assert len(groups) == 4
    for group in groups.values():
        mz, it, off, *queries = pc.pack_cases(group, gaps=True)
        rec, over = ru.purity(mz, it, off, *queries, group[0]["params"])
        assert rec.tobytes() == ref.to_bytes([c["record"] for c in group]) and over == (0, None)


def test_out_of_range_survey_and_the_ratio():
    mz, it, off, sv, pm, pz, wl, wh = pc.pack_cases(CASES[4:6], gaps=False)
    sv = np.array([0, 2, 1, 7, -3], np.int64)
    q = (sv, np.full(5, pc.PM), np.full(5, pc.Z, np.int32), np.full(5, pc.WL), np.full(5, pc.WH))
    rec, over = ru.purity(mz, it, off, *q, pc.P_BASE)
    want, w_over = ref.purity(pc.as_lists(mz, it, off), pc.as_queries(*q), pc.P_BASE)
    assert rec.tobytes() == ref.to_bytes(want) and over == w_over == (2, 1)
    assert not rec[[1, 3, 4]].tobytes().strip(b"\0") and rec["flags"][[0, 2]].tolist() == [3, 3]
    ratio = ru.purity_ratio(rec)
    assert ratio[0] == rec["precursor"][0] / rec["window"][0] == ref.ratio(want[0]) and np.isnan(ratio[[1, 3, 4]]).all()
    assert math.isnan(ref.ratio(ref.ZERO))


# ---- rollup against the yardstick ----

@pytest.mark.parametrize("seed", range(6))
def test_rollup_equals_the_yardstick_on_random_inputs(seed):
    params = [pc.P_BASE, pc.P_16, pc.P_WIDE, ru.purity_params(), ru.purity_params(tol=0.01, tol_ppm=20.0, isotopes=4, below=1),
              ru.purity_params(tol=0.0, tol_ppm=0.0, isotopes=0)][seed]
    spectra, queries = pc.random_inputs(seed)
    for mz_t, it_t in ((np.float64, np.float64), (np.float64, np.float32), (np.float32, np.float32)):
        rec, over = _rollup_bytes(spectra, queries, params, mz_t, it_t)
    assert over[0] > 0 and (rec["flags"] == 0).any() and (rec["flags"] == 3).any() and (rec["n_window"] > rec["n_precursor"]).any()
    # the gate, on the same records and a matrix with NaNs, negative zeros and payloads in it
    rng = np.random.default_rng(seed)
    values = rng.choice([1.5, 0.0, -0.0, np.nan, 1e300, -7.0], size=(rec.size, 3))
    values.view(np.uint64)[0, 0] = 0x7FF0000000000123                     # (a signalling NaN with a payload: copied, not quieted)
    rows = values.view(np.uint64).tolist()
    tuples = [tuple(r) for r in rec.tolist()]
    for threshold in (0.0, 0.25, 0.5, 1.0):
        for keep in (True, False):
            select, out = ru.purity_gate(rec, threshold, keep, values)
            w_select, w_rows = ref.gate(tuples, threshold, keep, rows)
            assert select.dtype == np.uint8 and select.tolist() == w_select and out.view(np.uint64).tolist() == w_rows
            assert ru.purity_gate(rec, threshold, keep)[0].tolist() == w_select and ru.purity_gate(rec, threshold, keep)[1] is None
    assert values.view(np.uint64).tolist() == rows                         # (the input is not written)


def test_boundary_spectra_equal_the_yardstick():
    spectra, planted = pc.boundary_spectra()
    n = len(spectra)
    q = (np.arange(n, dtype=np.int64), np.full(n, pc.PM), np.full(n, pc.Z, np.int32), np.full(n, pc.WL), np.full(n, pc.WH))
    rec, _ = _rollup_bytes(spectra, q, pc.P_BASE)
    assert rec["n_window"].tolist() == [len(p) for p in planted] and int(rec["n_window"][9]) == 1 + 2 * 64         # peak 0, and 63 | 64, .. 4 095 | 4 096


# ---- planted ----

def test_planted_envelope_and_interferers():
    (x, y), precursor, window = pc.planted_scan()
    assert (precursor, window) == (2017.0, 2867.0)
    spectra = [(x, y), (x[::-1], y[::-1])]                                 # (exact sums: the order does not show)
    q = (np.array([0, 1, 0], np.int64), np.full(3, pc.PM), np.full(3, pc.Z, np.int32), np.array([pc.WL, pc.WL, 499.75]), np.full(3, pc.WH))
    rec, _ = _rollup_bytes(spectra, q, pc.P_BASE)
    assert rec["precursor"].tolist() == [2017.0] * 3 and rec["window"].tolist() == [2867.0, 2867.0, 2867.0 - 272.0]
    assert rec["n_window"].tolist() == [6, 6, 5] and (rec["n_precursor"] == 3).all() and (rec["iso_hit"] == 7).all()
    assert rec[["other_mz", "other_intensity"]][0].tolist() == (500.75, 512.0)
    # the gate where precursor == threshold * window holds exactly: 2017 = t * 2867 has no such t in double, so plant one that has
    recs = np.zeros(4, ru.PURITY_DTYPE)
    recs["flags"] = 3
    recs["window"] = 2048.0
    t = 0.75
    recs["precursor"] = [1536.0, pc.down(1536.0), 1536.0, 0.0]
    recs["window"][2], recs["flags"][3] = 0.0, 0                            # an empty window and an inactive row: unknown
    assert 1536.0 == t * 2048.0
    select, out = ru.purity_gate(recs, t, True, np.arange(8.0).reshape(4, 2))
    assert select.tolist() == [1, 0, 1, 1] and ref.gate([tuple(r) for r in recs.tolist()], t, True)[0] == [1, 0, 1, 1]
    assert out[0].tolist() == [0.0, 1.0] and out.view(np.uint64)[1].tolist() == [ref.NO_READING] * 2 and out[2:].tolist() == [[4.0, 5.0], [6.0, 7.0]]
    assert ru.purity_gate(recs, t, False)[0].tolist() == [1, 0, 0, 0]
    assert ru.purity_gate(recs, pc.up(t), True)[0].tolist() == [0, 0, 1, 1]  # (one ulp above the exact threshold: the exact row fails)


# ---- the survey index ----

def test_survey_index_by_parent_and_by_order():
    survey = [10, 20, 30]
    assert ru.survey_index(survey, [11, 12, 21, 35, 5, 10, 20]).tolist() == [0, 0, 1, 2, -1, -1, 0]        # the last one BEFORE the scan
    assert ru.survey_index(survey, [11, 12, 21, 35, 5], [None, 30, 10, 25, 20]).tolist() == [0, 2, 0, 2, 1]  # 25 is no survey scan: by order
    assert ru.survey_index(survey, [11, 12], [-1, None]).tolist() == [0, 0]
    assert ru.survey_index([], [1, 2]).tolist() == [-1, -1] and ru.survey_index(survey, []).tolist() == []
    assert ru.survey_index(survey, [11]).dtype == np.int64
    for bad in (dict(survey_scans=[3, 2], scans=[1]), dict(survey_scans=[1, 2], scans=[1], parent_scans=[1, 2])):
        with pytest.raises(ValueError):
            ru.survey_index(**bad)


# ---- ingest ----

MZXML = """<?xml version="1.0"?>
<mzXML><msRun>
<scan num="1" msLevel="1" centroided="1"><peaks precision="32" byteOrder="network" pairOrder="m/z-int">%s</peaks>
<scan num="2" msLevel="2"><precursorMz precursorCharge="2" precursorScanNum="1" windowWideness="1.5">500.25</precursorMz>
<peaks precision="32" byteOrder="network" pairOrder="m/z-int">%s</peaks></scan>
<scan num="3" msLevel="2"><precursorMz precursorCharge="3">600.5</precursorMz>
<peaks precision="32" byteOrder="network" pairOrder="m/z-int">%s</peaks></scan>
</scan></msRun></mzXML>
"""


def test_ingest_keeps_the_isolation_window_and_the_parent_scan(tmp_path):
    import base64
    from pyascore_amd import ingest
    recs = ingest.SpectraParser(os.path.join(DATA, "test_spectra.mzML"), "mzML").to_list()
    assert recs[0]["isolation"] == (846.640441894531, 0.75, 0.75) and recs[0]["parent_scan"] == 14754
    assert all(len(r["isolation"]) == 3 and isinstance(r["parent_scan"], int) and r["parent_scan"] < r["scan"] for r in recs)
    assert set(recs[0]) == {"scan", "ms_level", "precursor_mz", "precursor_charge", "mz_values", "intensity_values", "profile", "isolation",
                            "parent_scan"}
    peaks = base64.b64encode(np.array([100.0, 1.0, 200.0, 2.0], ">f4").tobytes()).decode()
    path = tmp_path / "t.mzXML"
    path.write_text(MZXML % (peaks, peaks, peaks))
    ms2 = ingest.SpectraParser(str(path), "mzXML").to_list()
    assert [r["scan"] for r in ms2] == [2, 3]
    assert ms2[0]["isolation"] == (500.25, 0.75, 0.75) and ms2[0]["parent_scan"] == 1
    assert ms2[1]["isolation"] is None and ms2[1]["parent_scan"] is None and ms2[1]["precursor_mz"] == 600.5
    ms1 = ingest.SpectraParser(str(path), "mzXML", ms_level=1).to_list()
    assert [r["scan"] for r in ms1] == [1] and ms1[0]["isolation"] is None and ms1[0]["parent_scan"] is None


# ---- requests that need no device ----

def test_parameter_checks():
    assert ru.purity_params() == dict(tol=0.0, tol_ppm=10.0, step=ru.STRIP_STEP, below=0, isotopes=3)
    assert ru.purity_params(below=4, isotopes=11)["isotopes"] == 11 and ru.purity_params(isotopes=15, below=0)["isotopes"] == 15
    nan, inf = float("nan"), float("inf")
    for bad in (dict(tol=-1.0), dict(tol=nan), dict(tol=inf), dict(tol_ppm=-1.0), dict(tol_ppm=nan), dict(tol_ppm=inf), dict(step=0.0),
                dict(step=-1.0), dict(step=nan), dict(step=inf), dict(below=5), dict(below=-1), dict(below=1.5), dict(isotopes=-1),
                dict(isotopes=16), dict(below=4, isotopes=12), dict(isotopes=True), dict(tol="x"), dict(isotopes=None)):
        with pytest.raises(ValueError):
            ru.purity_params(**bad)
    for bad in (None, {}, dict(ru.purity_params(), tol=None)):
        with pytest.raises(ValueError):
            ru.check_purity_params(bad)
    rec = np.zeros(2, ru.PURITY_DTYPE)
    for bad in (dict(threshold=-0.1), dict(threshold=1.1), dict(threshold=nan), dict(threshold="x"), dict(threshold=True),
                dict(threshold=0.5, keep_unknown=1), dict(threshold=0.5, values=np.zeros((3, 2))), dict(threshold=0.5, values=np.zeros(2))):
        with pytest.raises(ValueError):
            ru.purity_gate(rec, **bad)
    with pytest.raises(ValueError):
        ru.purity_gate(np.zeros((2, 2), ru.PURITY_DTYPE), 0.5)
    ok = ([0.0], [0.0], [0, 1], [0], [500.0], [2], [499.0], [501.0])
    assert ru.purity(*ok, ru.purity_params())[0].shape == (1,)
    for i, wrong in ((3, [0, 1]), (3, [0.5]), (4, [500.0, 1.0]), (5, [2.5]), (6, ["a"]), (2, [1, 0]), (2, [0, 2]), (0, [[0.0]])):
        args = list(ok)
        args[i] = wrong
        with pytest.raises(ValueError):
            ru.purity(*args, ru.purity_params())


def test_score_batch_request_checks():
    from pyascore_amd.ascore import _purity_request
    base = dict(ms1_mz=np.array([500.0]), ms1_intensity=np.array([1.0]), ms1_peak_off=[0, 1], survey=[0, -1], precursor_mz=[500.0, 400.0],
                precursor_charge=[2, 300], window_lo=[499.0, 399.0], window_hi=[501.0, 401.0])
    params, spectra, queries, gate = _purity_request(base, 2)
    assert params == ru.purity_params() and gate is None and queries[2].tolist() == [2, 300] and queries[0].dtype == np.int64
    params, _, _, gate = _purity_request(dict(base, tol=0.01, tol_ppm=None, isotopes=2, below=1, step=1.0, gate=dict(threshold=0.7)), 2)
    assert params == ru.purity_params(tol=0.01, isotopes=2, below=1, step=1.0) and gate == (0.7, True)
    assert _purity_request(dict(base, gate=dict(threshold=1, keep_unknown=False)))[3] == (1.0, False)
    for bad in (None, True, dict(base, window=1), {k: v for k, v in base.items() if k != "survey"}, dict(base, survey=None),
                dict(base, survey=[0]), dict(base, precursor_charge=[2.5, 1.0]), dict(base, tol=-1.0), dict(base, below=5),
                dict(base, isotopes="3"), dict(base, gate=0.5), dict(base, gate=dict()), dict(base, gate=dict(threshold=2.0)),
                dict(base, gate=dict(threshold=0.5, keep=True)), dict(base, gate=dict(threshold=0.5, keep_unknown=2))):
        with pytest.raises(ValueError):
            _purity_request(bad, 2)
    with pytest.raises(ValueError):
        _purity_request(base, 3)                                          # one entry per spectrum
    with pytest.raises(ValueError, match="gate needs quant"):
        _purity_request(dict(base, gate=dict(threshold=0.5)), 2, have_quant=False)


def test_command_line_options():
    from pyascore_amd import batch_cli
    from pyascore_amd.__main__ import parse_args, purity_request
    files = ["s.mzML", "i.pep.xml", "o.tsv"]
    assert purity_request(parse_args(files)) is None
    assert purity_request(parse_args(["--purity", "p.tsv"] + files)) == dict(tol=0.0, tol_ppm=10.0, isotopes=3, below=0)
    quant = ["--site_table", "t.tsv", "--site_quant", "q.tsv", "--marker_mz", "126.1277,127.1248"]
    args = parse_args(["--purity", "p.tsv", "--purity_tol", "0.01", "--purity_tol_ppm", "5", "--purity_isotopes", "2", "--purity_below", "1",
                       "--purity_window", "0.8,0.7", "--purity_threshold", "0.7", "--purity_drop_unknown"] + quant + files)
    assert purity_request(args) == dict(tol=0.01, tol_ppm=5.0, isotopes=2, below=1, window=(0.8, 0.7), threshold=0.7, keep_unknown=False)
    for bad in (["--purity_tol", "-1"], ["--purity_tol_ppm", "nan"], ["--purity_isotopes", "16"], ["--purity_below", "5"],
                ["--purity_below", "4", "--purity_isotopes", "12"], ["--purity_window", "1"], ["--purity_window", "1,x"],
                ["--purity_window=-1,1"], ["--purity_window", "1,2,3"], ["--purity_threshold", "0.5"], ["--purity_drop_unknown"]):
        with pytest.raises(ValueError):
            parse_args(["--purity", "p.tsv"] + bad + files)
    for bad in (["--purity_threshold", "1.5"], ["--purity_threshold", "nan"]):
        with pytest.raises(ValueError):
            parse_args(["--purity", "p.tsv"] + bad + quant + files)
    for bad in (["--purity_threshold", "0.5"], ["--purity_drop_unknown"]):       # the gate without the table
        with pytest.raises(ValueError):
            parse_args(bad + quant + files)
    parse_args(["--purity_tol", "-1", "--purity_below", "9"] + files)       # (without --purity the values are not looked at)
    # localize refuses a bad request before anything is read: no scorer, no PSMs
    for bad in (dict(purity=dict(survey=[]), purity_rows=None), dict(purity=dict(), purity_rows=[]), dict(purity=dict(survey=[], tol=-1.0), purity_rows=[]),
                dict(purity=dict(survey=[], windows=(1, 1)), purity_rows=[]), dict(purity=dict(survey=[], window=(1,)), purity_rows=[]),
                dict(purity=dict(survey=[], threshold=0.5), purity_rows=[]), dict(purity=dict(survey=[], keep_unknown=False), purity_rows=[])):
        with pytest.raises(ValueError):
            batch_cli.localize(None, [], {}, "STY", 79.9, **bad)
    with pytest.raises(TypeError):                                         # (a good request gets as far as the scorer check)
        batch_cli.localize(None, [], {}, "STY", 79.9, purity=dict(survey=[], window=(0.8, 0.7)), purity_rows=[])
    assert batch_cli.PURITY_COLUMNS[:4] == ["Scan", "SurveyScan", "WindowLo", "WindowHi"] and len(batch_cli.PURITY_COLUMNS) == 12
    rec = np.zeros(1, ru.PURITY_DTYPE)
    assert batch_cli.purity_fields(rec[0]) == [0.0, 0.0, "", 0, 0, "0", "", ""]
    rec[0] = (8.0, 6.0, 500.25, 2.0, 3, 2, 5, 3)
    assert batch_cli.purity_fields(rec[0]) == [8.0, 6.0, 0.75, 3, 2, "101", 500.25, 2.0]
