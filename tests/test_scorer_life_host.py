"""tests/lifecases.py without a GPU: the pool is what its entries say, the sequences cover it, the growth arithmetic rests on
the constants the library has -- and the plan entry points of the library ask for the settings generation before they enqueue
anything (source pins, in the way of tests/test_manysites_host.py)."""
import os
import re
from math import comb

import numpy as np
import pytest

import lifecases as lc
from oracle import orc
from pyascore_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pyascore_amd", "csrc")
KIND = "ref" if orc.available("ref") else "oracle"


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_the_pool_is_what_it_says():
    assert set(lc.shapes(lc.entry("a_small"))) == {(6, 3)} and int(lc.entry("a_small")["n_psm"]) == 64
    assert set(np.diff(lc.entry("a_small")["pep_off"]).tolist()) == {20} and set(lc.entry("a_small")["max_charge"].tolist()) == {1}
    b = set(lc.shapes(lc.entry("b_shapes")))
    assert not b & set(lc.shapes(lc.entry("a_small"))) and (15, 5) in b and comb(15, 5) == 3003
    assert 100 <= int(lc.entry("b_shapes")["n_psm"]) <= 140
    # the needs on either side of the floor
    assert lc.lut_need(lc.entry("a_small")) == 19 * 1 * 1 * 2 == 38 < lc.LUT_FLOOR
    forty = synth.slice_batch(lc.entry("b_lut"), 0, 4)
    assert set(np.diff(forty["pep_off"]).tolist()) == {40} and set(forty["max_charge"].tolist()) == {3}
    assert lc.lut_need(forty) == 39 * 3 * 2 == 234 > lc.LUT_FLOOR
    assert lc.lut_need(lc.entry("b_lut")) == 50 * 6 * 2 == 600
    g = lc.entry("general")
    assert np.diff(g["pep_off"]).tolist() == [70, 20] and np.diff(g["peak_off"])[1] == 9000 and (np.diff(g["mz"][g["peak_off"][1]:]) >= 0).all()
    assert int(lc.entry("one")["n_psm"]) == 1 and int(lc.entry("empty")["n_psm"]) == 0 and lc.entry("empty")["peak_off"].tolist() == [0]
    s = lc.entry("shared")
    assert s["n_spectra"] == 8 and np.bincount(s["spec_of"]).tolist() == [5] * 8 and (np.diff(s["spec_of"].astype(int)) >= 0).all()
    f = lc.entry("f32")
    assert f["mz"].dtype == np.float32 and f["intensity"].dtype == np.float32
    assert np.array_equal(f["mz"], lc.entry("a_small")["mz"].astype(np.float32)) and np.array_equal(f["pep"], lc.entry("a_small")["pep"])
    assert int(lc.entry("wide")["n_psm"]) == 300 and len(set(lc.shapes(lc.entry("wide")))) > 10
    # the one entry a budget can cut, and no other
    for name in lc.NAMES:
        e = lc.entry(name)
        assert (e["mz"].nbytes + e["intensity"].nbytes >= lc.CHUNK_MIN_BYTES) == (name == "chunked"), name
        assert lc.PURPOSE[name]
    assert "kChunkMin = 32u << 20" in _src("host_batch.cpp")
    assert "bytes < ((uint64_t)16 << 20)" in _src("host_abi.cpp") and lc.SMALL_BUDGET == 16 << 20


def test_the_invalid_psms_are_invalid_by_the_documented_rule():
    """an unknown residue (no mass in host_internal.h: std_residue_mass) and a spectrum without peaks; every other PSM of the
    entry is one the reference scores"""
    e = lc.entry("invalid")
    masses = set(re.findall(r"case '([A-Z])': return", _src("host_internal.h")))
    assert len(masses) == 22 and "X" not in masses
    for i in range(int(e["n_psm"])):
        kw = synth.unpack_psm(e, i)
        known, peaks = set(kw["peptide"]) <= masses, kw["mz_arr"].size
        assert (known and peaks > 0) == bool(lc.valid("invalid")[i]), i
    assert [i for i in range(12) if not lc.valid("invalid")[i]] == list(lc.INVALID_PSMS) == [3, 8]
    assert "X" in synth.unpack_psm(e, 3)["peptide"] and synth.unpack_psm(e, 8)["mz_arr"].size == 0


@pytest.mark.parametrize("name", lc.NAMES)
def test_every_valid_pool_psm_is_scored_by_the_checker(name):
    want = lc.answer(name, KIND)
    ok = lc.valid(name)
    assert want["n_sig"].size == int(ok.sum())
    sh = [s for s, good in zip(lc.shapes(lc.entry(name)), ok) if good]
    assert want["n_sig"].tolist() == [comb(n, k) for n, k in sh] and (want["n_sig"] > 0).all()


def test_the_loss_matters_on_a_small():
    """the settings change of the refusal tests moves the answers of a_small: the new plan's bytes MUST differ from the old"""
    old, new = lc.answer("a_small", KIND), lc.answer("a_small", KIND, with_loss=True)
    assert (old["best_score"] != new["best_score"]).sum() >= 32 and np.array_equal(old["n_sig"], new["n_sig"])


def test_the_sequences_cover_the_pool():
    for seed in lc.SEEDS:
        steps = lc.sequence(seed, lc.N_STEPS)
        assert len(steps) == lc.N_STEPS and steps == lc.sequence(seed, lc.N_STEPS)
        batch = [s for s in steps if s[0] == "batch"]
        score = [s for s in steps if s[0] == "score"]
        assert {s[1] for s in batch} == set(lc.NAMES), seed                       # every entry, in every seed
        for flag in lc.FLAGS:
            assert len({s[1] for s in batch if s[2].get(flag)}) >= 3, (seed, flag)  # every flag with three entries at least
        assert all(s[2].get("ranked", 5) == 5 for s in batch)
        assert all(s[2].get("skip_invalid") for s in batch if s[1] in lc.MUST_SKIP_INVALID)
        assert {s[3] for s in batch} == {0, lc.SMALL_BUDGET}
        assert {s[3] for s in batch if s[1] == "chunked"} == {0, lc.SMALL_BUDGET}, seed   # cut and uncut on one handle
        assert len(score) >= 5 and {s[3] for s in score} == {False, True}, seed
        assert all(s[1] in lc.SCOREABLE and 0 <= s[2] < int(lc.entry(s[1])["n_psm"]) for s in score)
    assert lc.sequence(0) != lc.sequence(1)


def test_expected_growth_is_arithmetic_on_the_library_constants():
    assert "uint32_t target = std::max<uint32_t>(n_max, 128);" in _src("host_tables.cpp") and lc.LUT_FLOOR == 128
    assert "h->lut_uploaded_n = target + 1;" in _src("host_tables.cpp")
    assert "if (N >= 1 && N <= 64) {" in _src("host_tables.cpp") and lc.NODE_SHAPE_MAX == 64
    g = lc.expected_growth([], "a_small")
    assert g["lut_rows"] == (0, 129) and g["order_entries"] == (0, 20 + 2 * 7 * (1 + 3))
    g = lc.expected_growth("a_small", ["b_shapes", "b_lut"])
    assert g["lut"] and g["order"] and g["lut_rows"] == (129, 601) and g["order_entries"][1] > g["order_entries"][0] + 3003
    g = lc.expected_growth("a_small", "b_shapes")
    assert not g["lut"] and g["order"]                                    # 78 trials: under the floor
    g = lc.expected_growth("a_small", "b_lut")
    assert g["lut"] and g["order"] and g["lut_rows"] == (129, 601)
    for name in ("f32", "shared", "one", "invalid", "empty", "chunked"):  # the shape and the need of a_small: nothing moves
        g = lc.expected_growth("a_small", name)
        assert not g["lut"] and not g["order"], name
    assert lc.expected_growth(["a_small", "b_lut"], "general")["lut"] is False and lc.expected_growth("a_small", "general")["lut"]


# ---- source pins: the generation is asked before anything is enqueued ----------------------------------------------------------
ENTRY_POINTS = {
    "host_run.cpp": ["pya_plan_run_typed", "pya_plan_evidence", "pya_plan_named", "pya_plan_sites", "pya_plan_probs", "pya_plan_ranked",
                     "pya_plan_rollup", "pya_plan_site_quant", "pya_plan_peptidoforms", "pya_plan_peptidoform_quant", "pya_plan_mz_profile",
                     "pya_plan_coverage", "pya_plan_ions_count", "pya_plan_ions"],
    "host_abi.cpp": ["pya_calculate_ambiguity"],
}
ENQUEUES = re.compile(r"hipLaunchKernelGGL|HIPCHK|pya_launch_\w+\(|hipMemcpy|hipMemset|hipEventRecord|hipStreamWaitEvent|stage_behind_run|"
                      r"wait_for_run|run_tiny|run_binning|\.begin\(")


def _body(text, name):
    m = re.search(r"^int %s\(.*?\) \{\n(.*?)^\}\n" % re.escape(name), text, re.S | re.M)
    assert m, name
    return m.group(1)


@pytest.mark.parametrize("fname,name", [(f, n) for f, names in ENTRY_POINTS.items() for n in names])
def test_entry_points_ask_for_the_generation_first(fname, name):
    body = _body(_src(fname), name)
    guard = body.find("plan_settings_stale(p, ")
    first = ENQUEUES.search(body)
    assert guard >= 0, "%s does not ask for the settings generation" % name
    assert first is not None and guard < first.start(), "%s enqueues before it asks" % name


def test_the_guard_and_what_bumps_it():
    internal = _src("host_internal.h")
    guard = re.search(r"inline int plan_settings_stale\(pya_plan \*p, const char \*who\) \{\n(.*?)\n\}", internal, re.S).group(1)
    assert "p->settings_gen == p->h->settings_gen" in guard and "PYA_ERR_STATE" in guard and "settings changed since the plan was made" in guard
    assert "pya_plan_run_typed(p, &sp, hip_stream, o)" in _body(_src("host_run.cpp"), "pya_plan_run")     # (one guard for both)
    assert "h->settings_gen++" in _body(_src("host_abi.cpp"), "pya_add_neutral_loss")
    for fname, name in (("host_abi.cpp", "pya_set_debug"), ("host_abi.cpp", "pya_reload_env"), ("host_abi.cpp", "pya_set_workspace_budget"),
                        ("host_abi.cpp", "pya_set_ranked_k"), ("host_abi.cpp", "pya_set_site_sig_cap")):
        assert "settings_gen" not in _body(_src(fname), name), name            # classified in host_internal.h: they end no plan's life
    # a plan takes the generation it is made under: the planner's and the one-PSM path's retained view
    assert "p->settings_gen = h->settings_gen;" in _src("host_plan.cpp") and "p->settings_gen = h->settings_gen;" in _src("host_one.cpp")
    # the read-backs stay valid
    for fname, name in (("host_run.cpp", "pya_plan_check"), ("host_run.cpp", "pya_plan_timings"), ("host_run.cpp", "pya_plan_timings_sum"),
                        ("host_run.cpp", "pya_plan_site_offsets"), ("host_abi.cpp", "pya_get_pep_scores_range")):
        assert "plan_settings_stale" not in _body(_src(fname), name), name


def test_no_handle_table_is_released_under_work_in_flight():
    """the three places that replace a handle-owned device table drain the device before DevBuf::upload releases the old one"""
    tables = _src("host_tables.cpp")
    for fn, first in (("sync_config", "h->d_cfg"), ("ensure_lut", "h->d_lut"), ("upload_shared_tables", "h->d_order")):
        body = _body(tables, fn)
        drain, up = body.find("quiesce_before_reupload(%s.p)" % first), body.find("%s.upload(" % first)
        assert 0 <= drain < up, fn
    assert "return old ? hipDeviceSynchronize() : hipSuccess;" in tables
    # ... and they are the only places that do: five uploads, all in host_tables.cpp
    everywhere = {f: re.findall(r"h->d_(?:cfg|lut|lut_off|order|inv)\.(?:upload|alloc|release|adopt|take_if_fits|give_to)\(", _src(f))
                  for f in os.listdir(CSRC) if f.endswith((".cpp", ".h"))}
    assert {f: len(v) for f, v in everywhere.items() if v} == {"host_tables.cpp": 5}
