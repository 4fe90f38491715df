"""PSMs with 31 to 63 modifiable residues (tests/manysites.py) on the device: both sides of every gate that keeps a kernel with
32-bit signatures away from them, and the 64-bit paths behind the gates, held to the reference's own core bit for bit
(probabilities: probs_ref.RTOL, as everywhere).  tests/test_manysites_host.py holds the inputs to "the winners use the sites
of index 32 and above".

Which gate the suite can SEE: the front end of the probability and ranked stages, through pya_debug_last_probs_launch /
pya_debug_last_ranked_launch (test_front_end_of_probs_and_ranked).  Which scoring kernel took a bucket (host_run.cpp's
pick_score_route), score_big's table and score_cntg's two forms have no read-back and get none: they are pinned by equality
with the reference on both sides of each -- 31 / 32 against 33 sites, k + 1 = 31 against 32, L - 1 = 32 against 33 -- by the
count-node modes agreeing record by record, and by the mixed batches, where one 33-site PSM decides the kernel of every PSM
of its class and the others must not notice."""
import numpy as np
import pytest

import manysites as ms
import test_gpu_general_edges as t_edges
import test_gpu_peptidoforms as t_peptidoforms
import test_gpu_probs as t_probs
import test_gpu_ranked as t_ranked
import test_gpu_rollup as t_rollup
from conftest import checker_kind
from oracle import harness
from pyascore_amd import probs as pb, ranked as rk, synth
from test_gpu_parity import _same_psm_by_psm, path  # noqa: F401  (the route fixture)

pytestmark = pytest.mark.gpu

ALL = list(ms.CASES) + list(ms.MIXED)
_same_results = t_edges._same_results
_three_kernels = t_edges._three_kernels


def _gpu(settings):
    from pyascore_amd import PyAscore
    return harness.make_scorer(PyAscore, settings)


def _case(name):
    """(settings, batch, the checker's results): made once per process (manysites' caches), never changed"""
    settings, batch, _ = ms.case(name)
    return settings, batch, ms.answer(name, checker_kind())


def _keys(batch):
    return t_edges._keys(batch)


def _bits(raw):
    return (raw["signature"].astype(np.uint64) << np.arange(raw["signature"].shape[1], dtype=np.uint64)).sum(axis=1).astype(np.uint64)


# ---- every route, the single-launch kernel ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_every_route_matches_the_reference(name, path):
    settings, batch, want = _case(name)
    _same_results(_gpu(settings).score_batch(batch), want, _keys(batch), "%s on %s" % (name, path))


@pytest.mark.parametrize("name", ALL)
def test_single_launch_kernel_matches_the_reference(name, monkeypatch):
    """no switch at all: a batch of up to 64 PSMs takes the single-launch kernel"""
    for v in ("PYA_NO_TINY", "PYA_PLAIN_MIN", "PYA_DEBUG"):
        monkeypatch.delenv(v, raising=False)
    settings, batch, want = _case(name)
    _same_results(_gpu(settings).score_batch(batch), want, _keys(batch), name)


# ---- score(): every property and record of three PSMs per case -------------------------------------------------------------
@pytest.mark.parametrize("name", list(ms.CASES))
def test_score_psm_by_psm(name):
    """best_sequence, best_score, Ascores, alt_sites as positions, every record of pep_scores in the reference's order; and
    calculate_ambiguity of two records that differ only above bit 31"""
    settings, batch, _ = _case(name)
    gpu, chk = _gpu(settings), ms.checker(settings, checker_kind())
    _same_psm_by_psm(gpu, chk, synth.slice_batch(batch, 0, 3))
    L, s, k, _, _ = ms.CASES[name]
    if s <= 33 or not 0 < k < s or k > 3:
        return                                                  # (33 sites: one high site, no two records differ only there)
    kw = synth.unpack_psm(batch, 0)
    gpu.score(**kw)
    chk.score(**kw)
    raw = chk.raw_pep_scores()
    bits = _bits(raw)
    first, pair = {}, None                                      # the first two records with one low word and different high words
    for i, b in enumerate(bits.tolist()):
        j = first.setdefault(b & 0xFFFFFFFF, i)
        if j != i and b >> 32:
            pair = (j, i)
            break
    assert pair and bits[pair[0]] != bits[pair[1]] and not (int(bits[pair[0]]) ^ int(bits[pair[1]])) & 0xFFFFFFFF
    gpu._ensure_kept()
    mine = gpu.batch_pep_scores()                               # (the records in bulk: pep_scores would build up to 39 711 dicts)
    assert np.array_equal(mine["sig_bits"], bits)

    def rec(scores, ws, i):
        return dict(signature=raw["signature"][i], scores=scores[i], weighted_score=float(ws[i]))

    i, j = pair
    for a, b in ((i, j), (j, i), (0, j)):
        got = gpu.calculate_ambiguity(rec(mine["scores"], mine["weighted_score"], a), rec(mine["scores"], mine["weighted_score"], b))
        assert got == chk.calculate_ambiguity(rec(raw["scores"], raw["weighted_score"], a), rec(raw["scores"], raw["weighted_score"], b)), (name, a, b)


# ---- the bucket gate: one 33-site PSM decides the kernel of its whole class ------------------------------------------------
def _records_of(gpu, batch):
    res = gpu.score_batch(batch, keep=True)
    return res, gpu.batch_pep_scores()


def _slice_records(ps, i):
    a, e = int(ps["rec_off"][i]), int(ps["rec_off"][i + 1])
    return {k: np.ascontiguousarray(v[a:e]) for k, v in ps.items() if k != "rec_off"}


@pytest.mark.parametrize("no_cnt", [False, True])
@pytest.mark.parametrize("name", list(ms.MIXED))
def test_a_33_site_psm_does_not_change_its_neighbours(name, no_cnt, monkeypatch):
    """the PSMs of up to 32 sites of a mixed batch: results and retained records byte-equal to the same PSMs scored without
    the 33-site ones (where the count-node tables take their classes), and both equal to the reference; the same with the
    tables switched off for everybody (PYA_NO_CNT=1)"""
    _three_kernels(monkeypatch)
    if no_cnt:
        monkeypatch.setenv("PYA_NO_CNT", "1")
    else:
        monkeypatch.delenv("PYA_NO_CNT", raising=False)
    settings, batch, want = _case(name)
    _, _, shape = ms.case(name)
    small = [i for i, sh in enumerate(shape) if sh[1] <= 32]
    assert any(sh[1] == 32 for sh in shape) and any(sh[1] == 33 for sh in shape)
    gpu, chk = _gpu(settings), ms.checker(settings, checker_kind())
    sub = ms.take(batch, small)
    _same_results(gpu.score_batch(batch), want, ms.KEYS, name + " mixed")
    _same_results(gpu.score_batch(sub), ms.take_rows(want, small), ms.KEYS, name + " alone")
    mixed, mixed_ps = _records_of(gpu, batch)
    _same_results(mixed, want, ms.KEYS, name + " mixed, keep")
    alone, alone_ps = _records_of(gpu, sub)
    _same_results(alone, ms.take_rows(want, small), ms.KEYS, name + " alone, keep")
    for j, i in enumerate(small):
        a, b = _slice_records(mixed_ps, i), _slice_records(alone_ps, j)
        for key in a:
            assert a[key].tobytes() == b[key].tobytes(), (name, i, key)
    for i in range(int(batch["n_psm"])):                         # ... and every PSM's records are the reference's, in its order
        chk.score(**synth.unpack_psm(batch, i))
        raw, mine = chk.raw_pep_scores(), _slice_records(mixed_ps, i)
        assert np.array_equal(mine["sig_bits"], _bits(raw)), (name, i)
        for key in ("counts", "scores", "weighted_score", "total_fragments"):
            assert mine[key].tobytes() == np.ascontiguousarray(raw[key], mine[key].dtype).tobytes(), (name, i, key)


# ---- the count-node modes on the last shapes the tables take ---------------------------------------------------------------
COUNT_NODE_CASES = ["p_40_31_2", "p_40_32_2", "p_34_32_3", "p_33_32_30", "g_33_32_2", "g_34_32_2"]


@pytest.mark.parametrize("name", COUNT_NODE_CASES + ["p_33_32_31", "p_40_33_2", "g_34_33_2"])
def test_count_node_modes_agree_record_by_record(name, monkeypatch):
    """the table, no table (PYA_DEBUG=0x8000) and every node marked (0x40000000): every field of batch_pep_scores equal, and
    the records of the first three PSMs the reference's own.  (The three shapes behind the gates run too: there the modes
    must not matter.)"""
    _three_kernels(monkeypatch)
    settings, batch, want = _case(name)
    chk = ms.checker(settings, checker_kind())
    recs = {}
    for mode, dbg in (("table", None), ("no_table", str(0x8000)), ("all_marked", str(0x40000000))):
        if dbg is None:
            monkeypatch.delenv("PYA_DEBUG", raising=False)
        else:
            monkeypatch.setenv("PYA_DEBUG", dbg)
        gpu = _gpu(settings)
        _same_results(gpu.score_batch(batch), want, ms.KEYS, "%s %s" % (name, mode))
        _same_results(gpu.score_batch(batch, keep=True), want, ms.KEYS, "%s %s, keep" % (name, mode))
        recs[mode] = gpu.batch_pep_scores()
    for mode in ("table", "all_marked"):
        assert sorted(recs[mode]) == sorted(recs["no_table"])
        for key in recs["no_table"]:
            assert np.array_equal(recs[mode][key], recs["no_table"][key]), (name, mode, key)
    for i in range(3):
        chk.score(**synth.unpack_psm(batch, i))
        raw, mine = chk.raw_pep_scores(), _slice_records(recs["table"], i)
        assert np.array_equal(mine["sig_bits"], _bits(raw)), (name, i)
        for key in ("counts", "scores", "weighted_score", "total_fragments"):
            assert mine[key].tobytes() == np.ascontiguousarray(raw[key], mine[key].dtype).tobytes(), (name, i, key)


# ---- the later stages ------------------------------------------------------------------------------------------------------
STAGE_CASES = ["p_40_32_2", "p_40_33_2", "p_64_63_2", "p_64_63_61", "g_40_36_2"]
N_STAGE = 6                                                       # PSMs per case: two of every planted kind


def _peptides(batch):
    return [synth.unpack_psm(batch, i)["peptide"] for i in range(int(batch["n_psm"]))]


@pytest.mark.parametrize("stage", list(t_edges.STAGES))
@pytest.mark.parametrize("name", STAGE_CASES)
def test_later_stages_equal_their_yardsticks(name, stage, monkeypatch):
    _three_kernels(monkeypatch)
    settings, batch, _ = _case(name)
    t_edges.STAGES[stage](settings, synth.slice_batch(batch, 0, N_STAGE), "%s (%s)" % (name, stage))


@pytest.mark.parametrize("name", STAGE_CASES)
def test_rollup_with_a_slot_per_site(name, monkeypatch):
    """one slot per (peptide, site): a 63-site PSM fills 63 of them; every peptide twice, so that slots add up"""
    _three_kernels(monkeypatch)
    settings, batch, want = _case(name)
    idx = list(range(N_STAGE))
    kws = [synth.unpack_psm(batch, i) for i in idx]
    psms = ms.psm_dicts(batch, idx) + [dict(mz=kws[(j + 1) % N_STAGE]["mz_arr"], intensity=kws[(j + 1) % N_STAGE]["int_arr"], peptide=kws[j]["peptide"],
                                            n_of_mod=kws[j]["n_of_mod"], max_charge=kws[j]["max_fragment_charge"]) for j in range(N_STAGE)]
    both = synth.pack_batch(psms)
    _, got, plain, (slot, n_slots, _) = t_rollup._against_yardstick(settings, both, _peptides(both), name)
    n_sites = ms.CASES[name][1]
    assert n_slots == N_STAGE * n_sites and np.array_equal(np.sort(slot[:N_STAGE * n_sites]), np.arange(n_slots))
    t = got["rollup"].reshape(N_STAGE, n_sites)
    assert (t["n_psm"] == 2).all() and t["n_in_best"][:, 32:].any() == (n_sites > 32)
    _same_results({k: plain[k][:N_STAGE] for k in _keys(both)}, ms.take_rows(want, idx, _keys(both)), _keys(both), name)


def test_peptidoforms_that_differ_in_the_high_word():
    """four 63-site peptides, each against four spectra whose planted assignments share the low site: isomers of one group
    whose sig_bits differ only in the high word -- in the reference's winners, and in the list"""
    batch, group, _ = ms.isomer_batch()
    settings = ms.BASE_SETTINGS
    want_res = ms.checker(settings, checker_kind()).score_batch(batch, 2)
    groups = ms.high_word_isomers(group, want_res["best_sig"])
    assert len(groups) >= 2
    _, plain, want = t_peptidoforms._against_yardstick(settings, batch, group, "high-word isomers")
    _same_results(plain, want_res, ms.KEYS, "high-word isomers")
    assert ms.high_word_isomers(want["group"], want["sig_bits"]) == groups
    for g in groups:
        assert (want["n_isomers"][want["group"] == g] >= 2).all()
    assert (want["n_psm"] >= 2).any()                              # ... and a repeat: two PSMs on one key above bit 31
    assert np.all(np.diff(want["sig_bits"][want["group"] == groups[0]].astype(np.uint64)) > 0)      # sorted by the whole key


def test_ranked_lists_63_rows_of_64(monkeypatch):
    """K = 64 on 63-site PSMs with one modification: exactly 63 rows, the 64th empty"""
    _three_kernels(monkeypatch)
    settings, batch, _ = _case("p_64_63_1")
    _, got = t_ranked._against_yardstick(settings, synth.slice_batch(batch, 0, N_STAGE), "63 rows", top_k=64)
    rows = got["ranked"]
    assert rows.shape == (N_STAGE, 64) and (rows["kind"][:, :63] == rk.SCORED).all() and rows[:, 63].tobytes() == b"\0" * 16 * N_STAGE
    for r in rows:
        assert sorted(r["sig_bits"][:63].tolist()) == [1 << s for s in range(63)]


# ---- the front end of the probability and ranked stages --------------------------------------------------------------------
@pytest.mark.parametrize("name,front", [("p_40_32_2", 1), ("p_33_32_30", 1), ("p_40_33_2", 2), ("p_33_32_31", 2), ("mixed_plain", 3)])
def test_front_end_of_probs_and_ranked(name, front, monkeypatch):
    """32-site PSMs (k + 1 <= 31): the count-node tables alone; 33 sites, or k + 1 = 32: the general front end alone; the
    mixed list: both -- read back from the launches, and the records equal the yardsticks in all three"""
    _three_kernels(monkeypatch)
    settings, batch, want = _case(name)
    gpu, got = t_probs._against_yardstick(settings, batch, name)
    _same_results(got, want, ms.KEYS, name)
    assert (got["psm_probs"]["kind"] == pb.SCORED).all()
    gpu.score_batch(batch, probs=True, site_sig_cap=0)
    sw, lds = t_probs._front_ends(gpu)
    assert sw == (front, 0), (name, sw)
    assert 1024 < lds[0] <= 160 * 1024 and (front != 1 or lds[0] <= 64 * 1024)
    gpu, got = t_ranked._against_yardstick(settings, batch, name)
    gpu.score_batch(batch, ranked=t_ranked.K, site_sig_cap=0)
    sw, _ = t_ranked._front_ends(gpu)
    assert sw == (front, 0), (name, sw)


# ---- typed and shared forms ------------------------------------------------------------------------------------------------
def _three_hits(batch):
    """every spectrum with three hits: its own PSM, then the peptides of the next two"""
    n = int(batch["n_psm"])
    spectra, psms = [], []
    for i in range(n):
        kw = synth.unpack_psm(batch, i)
        spectra.append(dict(mz=kw["mz_arr"], intensity=kw["int_arr"]))
        for j in (i, (i + 1) % n, (i + 2) % n):
            other = synth.unpack_psm(batch, j)
            psms.append(dict(spectrum=i, peptide=other["peptide"], n_of_mod=other["n_of_mod"], max_charge=other["max_fragment_charge"]))
    return synth.pack_shared_batch(spectra, psms)


@pytest.mark.parametrize("route", ["single_launch", "three_kernels"])
def test_typed_and_shared_forms_give_the_same_bytes(route, monkeypatch):
    """the (64, 63, 2) case as float32 spectra: the bytes of the widened batch, which the reference scores; as three hits per
    spectrum: the bytes of the expanded batch"""
    if route == "three_kernels":
        _three_kernels(monkeypatch)
    else:
        for v in ("PYA_NO_TINY", "PYA_PLAIN_MIN", "PYA_DEBUG"):
            monkeypatch.delenv(v, raising=False)
    settings, batch, _ = _case("p_64_63_2")
    batch = synth.slice_batch(batch, 0, 8)
    gpu, chk = _gpu(settings), ms.checker(settings, checker_kind())
    narrow = synth.narrow_batch(batch)
    wide = synth.widen_batch(narrow)
    want = chk.score_batch(wide, 2)
    assert (want["best_sig"] >> np.uint64(32)).any()
    _same_results(gpu.score_batch(wide), want, ms.KEYS, "widened")
    _same_results(gpu.score_batch(narrow), want, ms.KEYS, "float32")
    shared = _three_hits(wide)
    expanded = synth.expand_shared_batch(shared)
    want3 = chk.score_batch(expanded, 2)
    got = gpu.score_batch(shared)
    _same_results(got, want3, ms.KEYS, "shared")
    _same_results({k: got[k][::3] for k in ms.KEYS}, want, ms.KEYS, "own hits of shared spectra")
    _same_results(gpu.score_batch(expanded), want3, ms.KEYS, "expanded")
    _same_results(gpu.score_batch(synth.narrow_batch(shared)), got, ms.KEYS, "shared float32")


# ---- 64 modifiable residues are refused ------------------------------------------------------------------------------------
def _with_a_64_site_psm():
    settings, batch, want = _case("p_64_63_2")
    psms = ms.psm_dicts(batch, range(4))
    rng = np.random.default_rng(64)
    psms.insert(2, dict(psms[1], peptide="".join(rng.choice(list("STY"), size=64)), n_of_mod=2))
    return settings, synth.pack_batch(psms), ms.take_rows(want, range(4)), [0, 1, 3, 4]


PYA_PSM_OVER_LIMIT = 17                                          # include/pyascore_hip.h


def test_64_sites_are_refused_by_name():
    settings, batch, want, keep = _with_a_64_site_psm()
    gpu = _gpu(settings)
    with pytest.raises(ValueError, match=r"PSM 2: 64 modifiable residues exceed 63"):
        gpu.score_batch(batch)
    assert gpu._lib.pya_error_index(gpu._h) == 2
    kw = synth.unpack_psm(batch, 2)
    with pytest.raises(ValueError, match=r"PSM 0: 64 modifiable residues exceed 63"):
        gpu.score(**kw)
    gpu.score(**synth.unpack_psm(batch, 1))                         # still usable, and on 63 sites
    chk = ms.checker(settings, checker_kind())
    chk.score(**synth.unpack_psm(batch, 1))
    assert gpu.best_sequence == chk.best_sequence and np.array_equal(gpu.ascores, chk.ascores)
    got = gpu.score_batch(batch, skip_invalid=True)
    assert got["status"].tolist() == [0, 0, PYA_PSM_OVER_LIMIT, 0, 0] and "PSM 2" in got["status_message"] and "63" in got["status_message"]
    assert got["best_score"][2] == -1.0 and got["n_sig"][2] == -1 and got["best_sig"][2] == 0
    assert not got["ascores"][2].any() and not got["alt_mask"][2].any()
    _same_results({k: got[k][keep] for k in ms.KEYS}, want, ms.KEYS, "the 63-site PSMs on either side")


@pytest.mark.parametrize("stage", ["evidence", "ions", "named", "sites", "probs", "ranked"])
def test_later_stages_set_a_64_site_psm_aside(stage, monkeypatch):
    """every stage against its yardstick with skip_invalid: the yardsticks give a set-aside PSM zeroed or empty records"""
    import test_gpu_evidence as t_evidence
    import test_gpu_ions as t_ions
    import test_gpu_named as t_named
    import test_gpu_sites as t_sites
    _three_kernels(monkeypatch)
    settings, batch, _, _ = _with_a_64_site_psm()
    run = dict(evidence=t_evidence, ions=t_ions, named=t_named, sites=t_sites, probs=t_probs, ranked=t_ranked)[stage]._against_yardstick
    # (named: one query per PSM -- a single move of the winner, and for the PSM without a winner the signature 0)
    out = run(settings, batch, "64 sites (%s)" % stage, skip_invalid=True, **(dict(mode="one") if stage == "named" else {}))
    got = out if isinstance(out, dict) else out[1]
    assert got["status"][2] == PYA_PSM_OVER_LIMIT and got["n_sig"][2] == -1
    if stage == "named":
        a, e = got["named_off"][2], got["named_off"][3]
        assert e - a == 1 and got["named"]["kind"][a] == 0 and got["named"][a].tobytes()[8:] == b"\0" * 24
    if stage == "evidence":
        assert got["evidence"][2].tobytes() == b"\0" * got["evidence"][2].nbytes
    if stage == "ions":
        assert got["ion_off"][3] == got["ion_off"][2]
    if stage == "sites":
        a, e = got["site_off"][2], got["site_off"][3]
        assert not got["sites"]["kind"][a:e].any()
    if stage == "probs":
        assert got["psm_probs"]["kind"][2] == pb.NONE
    if stage == "ranked":
        assert got["ranked"][2].tobytes() == b"\0" * got["ranked"][2].nbytes


def test_rollup_and_peptidoforms_set_a_64_site_psm_aside(monkeypatch):
    _three_kernels(monkeypatch)
    settings, batch, _, _ = _with_a_64_site_psm()
    _, got, _, (slot, n_slots, _) = t_rollup._against_yardstick(settings, batch, _peptides(batch), "64 sites (rollup)", skip_invalid=True)
    assert got["status"][2] == PYA_PSM_OVER_LIMIT
    group = np.arange(5, dtype=np.int32)
    _, _, want = t_peptidoforms._against_yardstick(settings, batch, group, "64 sites (peptidoforms)", skip_invalid=True)
    assert 2 not in want["group"].tolist() and sorted(want["group"].tolist()) == [0, 1, 3, 4]
