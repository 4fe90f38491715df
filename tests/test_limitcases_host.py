"""The limit family of tests/limitcases.py, without a GPU: the CPU restatement against the reference's own core on every case
(score(), PSM by PSM: the checker's batch form cannot hold alternative sites of peptides longer than 64 residues), the
conditions on the INPUTS that keep tests/test_gpu_stage_limits.py from being vacuous -- asserted on the checker's answers and
on the CPU yardsticks, never on the library's output, with the counts printed so that a reader sees the margin -- and the
yardsticks held to their own reference-derived checks on far_positions, ntop16 and long_list: a yardstick that truncates a
position to 8 bits would hide a kernel that does the same."""
import ctypes as C
import time

import numpy as np
import pytest

import limitcases as lc
import test_evidence_ref
import test_ions_ref
import test_named_ref
import test_probs_ref
import test_ranked_ref
import test_sites_ref
from oracle import harness, orc
from pyascore_amd import _lib, synth

needs_ref = pytest.mark.skipif(not orc.available("ref"), reason="oracle/_ref not built")
KIND = "ref" if orc.available("ref") else "oracle"
ALL = list(lc.NAMES)
WINNER = 255                                                     # ions_ref.WINNER: section 1, the winner's matched fragments
COUNTED = 1                                                      # evidence_ref.COUNTED
CPU_SECONDS = 30.0                                               # a case's whole CPU side: the checker and every yardstick


def _yard(name):
    res, ps = lc.answer(name, KIND)
    return res, ps, lc.yardsticks(name, res, ps, key=KIND)


def _matched(ions):
    return ions[ions["rank"] != 255]


def _per_psm(off, rec, i):
    return rec[int(off[i]):int(off[i + 1])]


@needs_ref
@pytest.mark.parametrize("name", ALL)
def test_restatement_equals_the_reference(name):
    """every result, every per-assignment record, best_sequence and the alternative sites as positions, PSM by PSM"""
    (a, pa), (b, pb) = lc.answer(name, "ref"), lc.answer(name, "oracle")
    for key in lc.KEYS:
        assert a[key].tobytes() == b[key].tobytes(), (name, key)
    for key in pa:
        assert pa[key].tobytes() == pb[key].tobytes(), (name, key)
    assert a["best_sequence"] == b["best_sequence"]
    assert [[s.tolist() for s in p] for p in a["alt_sites"]] == [[s.tolist() for s in p] for p in b["alt_sites"]]


@pytest.mark.parametrize("name", ALL)
def test_the_cases_are_what_they_say(name):
    """2 to 4 limit PSMs, six ordinary ones shuffled among them where the case is mixed, 4 to 6 modifiable residues and two
    modifications unless the case says otherwise, and the CPU side of a case within CPU_SECONDS"""
    t0 = time.perf_counter()
    settings, batch, info = lc.case(name)
    res, ps, y = _yard(name)
    spent = time.perf_counter() - t0
    n = int(batch["n_psm"])
    assert 2 <= len(info["limit"]) <= 4 and n == len(info["limit"]) + (lc.N_ORDINARY if info["mixed"] else 0) <= 10
    if info["mixed"]:
        assert info["limit"] != sorted(info["limit"]) or info["limit"][0] != 0 or np.diff(info["limit"]).max() > 1      # shuffled in
    for j in info["limit"]:
        kw = synth.unpack_psm(batch, j)
        ns = len(lc.sites_of(settings, kw["peptide"]))
        if name not in ("many_assignments", "most_peaks"):
            assert 4 <= ns <= 6 and kw["n_of_mod"] == 2, (name, j)
    print("%s: %d PSMs, checker and yardsticks in %.1f s (cached: 0 s)" % (name, n, spent))
    assert spent < CPU_SECONDS


def test_far_positions():
    settings, batch, info = lc.case("far_positions")
    res, ps, y = _yard("far_positions")
    high_winner = comp_above = 0
    for j in info["limit"]:
        kw = synth.unpack_psm(batch, j)
        sites = lc.sites_of(settings, kw["peptide"])
        assert len(kw["peptide"]) == 511 and max(sites) >= 256
        best = int(res["best_sig"][j])
        high_winner += any(best >> s & 1 and sites[s] >= 256 for s in range(len(sites)))
        ev = y["evidence"][j]
        comp_above += int((ev["comp_pos"][ev["kind"] != 0] > 256).sum())
        sizes = _matched(_per_psm(y["ion_off"], y["ions"], j))["size"]
        assert (sizes > 255).any(), j
        print("far_positions PSM %d: sites %s, %d matched ions of size > 255 (largest %d)" % (j, sites, int((sizes > 255).sum()), int(sizes.max())))
        q = y["queries"][j]                                      # the second query moves the highest modification
        assert len(q) == 2 and q[1] != best and bin(q[1]).count("1") == 2
    print("far_positions: %d of %d winners modify a residue at index >= 256; %d evidence rows with comp_pos > 256" % (
        high_winner, len(info["limit"]), comp_above))
    assert 2 * high_winner >= len(info["limit"]) and comp_above >= 1
    assert (y["sites"]["pos"] > 256).any() and (y["named"]["kind"] >= 3).any()


def test_byte_edge():
    settings, batch, info = lc.case("byte_edge")
    res, ps, y = _yard("byte_edge")
    lengths, seen = [], set()
    for j in info["limit"]:
        kw = synth.unpack_psm(batch, j)
        L, sites = len(kw["peptide"]), lc.sites_of(settings, kw["peptide"])
        lengths.append(L)
        assert sites[-1] + 1 in (L - 1, L)                                     # 1-based position L - 1 or L
        best = int(res["best_sig"][j])
        ev = y["evidence"][j]
        on_it = bool(best >> (len(sites) - 1) & 1) or (ev["comp_pos"][ev["kind"] != 0] == sites[-1] + 1).any()
        sizes = set(_matched(_per_psm(y["ion_off"], y["ions"], j))["size"].tolist())
        seen |= sizes & {255, 256}
        print("byte_edge L = %d: last modifiable residue at position %d, winner or competitor on it: %s; matched sizes >= 254: %s" % (
            L, sites[-1] + 1, on_it, sorted(s for s in sizes if s >= 254)))
        assert on_it, L
    assert sorted(lengths) == [255, 256, 257] and seen == {255, 256}
    assert {255, 256, 257} <= set(y["sites"]["pos"].tolist())                    # the site yardstick writes all three positions


@pytest.mark.parametrize("name", ["last_row", "past_last_row"])
def test_last_row(name):
    settings, batch, info = lc.case(name)
    res, ps, y = _yard(name)
    for j in info["limit"]:
        kw = synth.unpack_psm(batch, j)
        tf = ps["total_fragments"][int(ps["rec_off"][j]):int(ps["rec_off"][j + 1])]
        want = (len(kw["peptide"]) - 1) * 8 * 2
        print("%s PSM %d: L = %d, total_fragments %s" % (name, j, len(kw["peptide"]), sorted(set(tf.tolist()))))
        assert kw["max_fragment_charge"] == 8 and (tf == want).any()
        assert (want == 4096) == (j not in info["refused"]) and want in (4096, 4112)
    assert len(info["refused"]) == (1 if name == "past_last_row" else 0)
    if name == "past_last_row":                                  # the yardsticks give the refused PSM all-zero or empty records
        j = info["refused"][0]
        assert not y["evidence"][j].view(np.uint8).any() and y["ion_off"][j] == y["ion_off"][j + 1] and y["site_off"][j] == y["site_off"][j + 1]
        assert not y["ranked"][j].view(np.uint8).any() and not y["coverage"][j:j + 1].view(np.uint8).any() and y["psm_probs"]["kind"][j] == 0


def _lds(fn, l_cap, list_cap):
    f = getattr(_lib.load(), fn)
    f.restype, f.argtypes = C.c_size_t, [C.c_uint32, C.c_uint32]
    return int(f(l_cap, list_cap))


def test_long_list():
    """The dynamic LDS of the stages' general launch at l_cap 511, list_cap 4 080 (the library's own *_lds_bytes expressions,
    which stage_behind_run and the launches use): evidence 102 640 bytes, ions 146 352, named 105 648 -- above the 64 KB a launch
    gets without asking, below the 160 KB (163 840 bytes) of a compute unit; the scoring kernel itself 97 392.  The site stage
    keeps no fragment list: 28 944 bytes by l_cap alone."""
    settings, batch, info = lc.case("long_list")
    res, ps, y = _yard("long_list")
    assert settings["fragment_types"] == "b"
    for j in info["limit"]:
        kw = synth.unpack_psm(batch, j)
        assert len(kw["peptide"]) == 511 and kw["max_fragment_charge"] == 8
        assert (ps["total_fragments"][int(ps["rec_off"][j]):int(ps["rec_off"][j + 1])] == 4080).all()
    got = {fn: _lds("pya_%s_lds_bytes" % fn, 511, 4080) for fn in ("evidence", "ions", "named", "sites", "general")}
    print("long_list: LDS bytes at (511, 4080): %s" % got)
    assert got == dict(evidence=102640, ions=146352, named=105648, sites=28944, general=97392)
    for fn in ("evidence", "ions", "named", "general"):
        assert 64 * 1024 < got[fn] < 160 * 1024
        assert _lds("pya_%s_lds_bytes" % fn, 20, 38) < 16 * 1024                 # what the stages' launches have run with so far
    m = _matched(y["ions"])
    far = m[(m["charge"] == 8) & (m["size"] > 255)]
    print("long_list: %d matched ions of charge 8 and size > 255; evidence comp_pos up to %d" % (far.size, int(y["evidence"]["comp_pos"].max())))
    assert far.size >= 1 and (y["evidence"]["kind"] == COUNTED).any()


@pytest.mark.parametrize("name,z", [("charge_40", 40), ("charge_255", 255)])
def test_charges(name, z):
    settings, batch, info = lc.case(name)
    res, ps, y = _yard(name)
    assert (batch["max_charge"] == z).all()
    m = _matched(y["ions"])
    print("%s: %d matched ions, %d of charge > 16, %d of charge >= 128, %d of charge %d; %d of them site-determining" % (
        name, m.size, int((m["charge"] > 16).sum()), int((m["charge"] >= 128).sum()), int((m["charge"] == z).sum()), z,
        int(((m["charge"] > 16) & (m["site"] != WINNER)).sum())))
    assert (m["charge"] > 16).any() and (m["charge"] == z).any()
    if z == 255:
        assert (m["charge"] >= 128).any() and (ps["total_fragments"] == 4080).all()


@pytest.mark.parametrize("name", ["ntop16", "ntop16_cfg4", "eight_losses_ntop16"])
def test_ntop16(name):
    settings, batch, info = lc.case(name)
    res, ps, y = _yard(name)
    assert settings["n_top"] == 16 and ps["scores"].shape[1] == 16
    ev, m = y["evidence"], _matched(y["ions"])
    deep_ev = int(((ev["kind"] == COUNTED) & (ev["depth"] >= 10)).sum())
    deep_named = int(((y["named"]["kind"] == 4) & (y["named"]["depth"] >= 10)).sum())
    print("%s: %d evidence rows and %d named records with depth >= 10 (deepest %d); matched ions of rank >= 10: %d, rank 15: %d" % (
        name, deep_ev, deep_named, int(ev["depth"].max()), int((m["rank"] >= 10).sum()), int((m["rank"] == 15).sum())))
    assert deep_ev + deep_named >= 1 and (m["rank"] >= 10).any()
    assert (m["rank"] == 15).any()
    if name != "eight_losses_ntop16":                            # by construction: every PSM's b2 ion is retained with rank 15
        for j in info["limit"]:
            r = _per_psm(y["ion_off"], y["ions"], j)
            b2 = r[(r["site"] == WINNER) & (r["type"] == ord("b")) & (r["size"] == 2) & (r["charge"] == 1) & ((r["flags"] & 1) == 0)]
            assert b2.size == 1 and b2["rank"][0] == 15, (name, j, b2)
    if name != "ntop16":
        second = m[m["site"] != WINNER]
        print("%s: %d matched ions carry a loss, %d of them site-determining" % (name, int((m["flags"] & 1).astype(bool).sum()),
                                                                                int((second["flags"] & 1).astype(bool).sum())))
        assert (m["flags"] & 1).any() and (second["flags"] & 1).any()
    if name == "eight_losses_ntop16":
        assert len({float(np.float32(x[1])) for x in settings["neutral_losses"]}) == 8 and (batch["max_charge"] == 2).all()


def test_big_retained():
    settings, batch, info = lc.case("big_retained")
    res, ps, y = _yard("big_retained")
    chk = lc.checker(settings, KIND)
    for j in info["limit"]:
        kw = synth.unpack_psm(batch, j)
        chk.consume_spectra(kw["mz_arr"], kw["int_arr"])
        n = chk.binned()["mz"].size
        print("big_retained PSM %d: %d peaks, %d entries in the binned table (coverage yardstick: %d)" % (
            j, kw["mz_arr"].size, n, int(y["coverage"]["n_retained"][j])))
        assert n > 8192 and n == y["coverage"]["n_retained"][j] and len(kw["peptide"]) == 511
    assert settings["n_top"] == 16 and (_matched(y["ions"])["rank"] == 15).any()


def test_most_peaks():
    settings, batch, info = lc.case("most_peaks")
    res, ps, y = _yard("most_peaks")
    raw = y["coverage"]["n_peaks"][info["limit"]].tolist()
    print("most_peaks: raw-peak counts of the coverage yardstick %s" % raw)
    assert raw == [65535, 8193] and int(np.diff(batch["peak_off"]).max()) == 65535


def test_many_assignments():
    settings, batch, info = lc.case("many_assignments")
    res, ps, y = _yard("many_assignments")
    assert tuple(res["n_sig"][info["limit"]].tolist()) == info["n_sig"] == (15504, 24310)
    assert info["sig_caps"] == tuple(n - 1 for n in info["n_sig"])
    for cap, over in zip(info["sig_caps"], ([True, True], [False, True])):
        t0 = time.perf_counter()
        capped = lc.yardsticks("many_assignments", res, ps, sig_cap=cap, key=KIND)
        kinds = capped["psm_probs"]["kind"][info["limit"]].tolist()
        print("many_assignments, sig_cap %d: probability kinds of the limit PSMs %s, ranked kinds %s (%.1f s)" % (
            cap, kinds, capped["ranked"]["kind"][info["limit"], 0].tolist(), time.perf_counter() - t0))
        assert [k == 2 for k in kinds] == over and [k == 2 for k in capped["ranked"]["kind"][info["limit"], 0]] == over
        ordinary = [i for i in range(int(batch["n_psm"])) if i not in info["limit"]]
        assert (capped["psm_probs"]["kind"][ordinary] == 1).all()
    assert (y["psm_probs"]["n_summed"][info["limit"]] == np.array(info["n_sig"])).all()


def test_forms():
    """the batch of the one-call, chunked and resident forms: 511-residue PSMs with far sites and n_top = 16 PSMs with rank 15"""
    settings, batch, info = lc.case("forms")
    res, ps, y = _yard("forms")
    assert settings["n_top"] == 16 and sorted(np.diff(batch["pep_off"])[info["limit"]].tolist()) == [20, 20, 511, 511]
    m = _matched(y["ions"])
    assert (m["rank"] == 15).any() and (m["size"] > 255).any() and (y["evidence"]["comp_pos"] > 256).any()


# ---- the yardsticks of the stages, held to their own checks at the limits --------------------------------------------------
YARDSTICK_CASES = ["far_positions", "ntop16", "long_list"]


def _as_golden(name):
    settings, batch, _ = lc.case(name)
    res, ps = lc.answer(name, "ref")
    return settings, batch, lc.as_golden(res, ps)


@needs_ref
@pytest.mark.parametrize("name", YARDSTICK_CASES)
@pytest.mark.parametrize("check", [
    test_evidence_ref.test_yardstick_reproduces_golden_ascores,
    test_ions_ref.test_yardstick_adds_up_to_the_golden_counts,
    test_named_ref.test_single_moves_reproduce_golden_ascores_and_evidence,
    test_named_ref.test_any_pair_equals_the_reference,
    test_sites_ref.test_golden_cases_satisfy_the_consequences,
    test_sites_ref.test_the_reference_pep_scores_give_the_same_records,
    test_probs_ref.test_golden_cases_agree_with_the_brute_force,
    test_ranked_ref.test_golden_cases_agree_with_the_brute_force,
], ids=lambda f: f.__module__[5:] + "." + f.__name__[5:30])
def test_yardsticks_pass_their_own_checks(name, check, monkeypatch):
    """evidence_ref, ions_ref, named_ref, sites_ref, probs_ref, ranked_ref: the checks their test_*_ref.py files run on the
    golden files (the reference's Ascores, counts, pep_scores and calculate_ambiguity; a brute force), run on 511-residue
    PSMs with sites above residue 256, on n_top = 16 and on 4 080-entry fragment lists -- the golden file is replaced by the
    reference's answers of now, the checks are those files' own"""
    monkeypatch.setattr(harness, "load_case", lambda path: _as_golden(name))
    check(name)
