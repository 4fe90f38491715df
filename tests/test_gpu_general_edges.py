"""The match window under GENERAL settings -- fragment charges (the FMA division of charge_mz for charges other than 1, 2, 4),
neutral-loss variants, several ion types per direction, tolerances above 0.49 where the reference's `f >= peak - 0.5` cut takes
part -- on spectra whose peaks sit on the window ends of the reference's own fragments (tests/edgespectra.py: ends, the
`f + 0.5` cut, pairs inside one window with a third peak just outside).  tests/test_edgespectra_host.py holds these inputs to
"most PSMs change when every peak moves by one float32 ulp"; here every route of the `path` fixture, the single-launch
kernel, the count-node modes, score(), the typed and the shared forms, and the later stages that match peaks themselves
(evidence, ions, named, sites, probabilities, ranked, mass-error profile) are held to the reference's own core on them, bit
for bit (probabilities: probs_ref.RTOL, as everywhere)."""
import numpy as np
import pytest

import edgespectra as es
import test_gpu_evidence as t_evidence
import test_gpu_ions as t_ions
import test_gpu_mz_profile as t_mz_profile
import test_gpu_named as t_named
import test_gpu_probs as t_probs
import test_gpu_ranked as t_ranked
import test_gpu_sites as t_sites
from conftest import checker_kind
from oracle import harness
from pyascore_amd import synth
from test_gpu_parity import _same_psm_by_psm, path  # noqa: F401  (the route fixture)

pytestmark = pytest.mark.gpu

FAST = [n for n in es.CASES if not n.startswith("gk_")]
GENERAL_KERNEL = [n for n in es.CASES if n.startswith("gk_")]
_want = {}


def _gpu(settings):
    from pyascore_amd import PyAscore
    return harness.make_scorer(PyAscore, settings)


def _case(name):
    """(settings, {placement: batch}, {placement: the checker's results}); made once"""
    if name not in _want:
        settings, batches = es.case_batches(name, checker_kind())
        chk = es.checker(settings, checker_kind())
        _want[name] = (settings, batches, {p: chk.score_batch(b, int(b["n_of_mod"].max())) for p, b in batches.items()})
    return _want[name]


def _keys(batch):
    """the checker's batch form packs alternative sites into residue bits: peptides above 64 residues are compared through
    score() (test_general_kernel_psm_by_psm)"""
    return es.KEYS if int(np.diff(batch["pep_off"]).max()) <= 64 else tuple(k for k in es.KEYS if k != "alt_mask")


def _same_results(got, want, keys, what):
    for key in keys:
        g, w = np.ascontiguousarray(got[key]), np.ascontiguousarray(want[key])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, key)
        bad = np.flatnonzero((g.view(np.uint8).reshape(g.shape[0], -1) != w.view(np.uint8).reshape(w.shape[0], -1)).any(axis=1))
        assert bad.size == 0, "%s: %s differs for PSMs %s: got %s, want %s" % (what, key, bad[:8].tolist(), g[bad[:3]].tolist(), w[bad[:3]].tolist())


def _three_kernels(monkeypatch):
    for v in ("PYA_NO_PLAIN", "PYA_NO_LOC_HASH", "PYA_HASH_PP", "PYA_NO_NODES", "PYA_NODE_CAP", "PYA_NO_FUSED", "PYA_DEBUG", "PYA_NO_BIG_INLINE"):
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("PYA_NO_TINY", "1")
    monkeypatch.setenv("PYA_PLAIN_MIN", "0")


# ---- 3a: the five result arrays on every route -------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(es.CASES))
def test_every_route_matches_the_reference(name, path):
    settings, batches, want = _case(name)
    gpu = _gpu(settings)
    for placement, batch in batches.items():
        _same_results(gpu.score_batch(batch), want[placement], _keys(batch), "%s %s on %s" % (name, placement, path))


@pytest.mark.parametrize("name", list(es.CASES))
def test_single_launch_kernel_matches_the_reference(name, monkeypatch):
    """no switch at all: a batch of up to 64 PSMs takes the single-launch kernel"""
    for v in ("PYA_NO_TINY", "PYA_PLAIN_MIN", "PYA_DEBUG"):
        monkeypatch.delenv(v, raising=False)
    settings, batches, want = _case(name)
    gpu = _gpu(settings)
    for placement, batch in batches.items():
        _same_results(gpu.score_batch(batch), want[placement], _keys(batch), "%s %s" % (name, placement))


@pytest.mark.parametrize("name", FAST)
def test_count_node_modes_agree_record_by_record(name, monkeypatch):
    """the table, no table (PYA_DEBUG=0x8000) and every node marked (0x40000000): every field of batch_pep_scores equal, and the
    records of the first three PSMs against the reference's own"""
    _three_kernels(monkeypatch)
    settings, batches, want = _case(name)
    chk = es.checker(settings, checker_kind())
    scorers = {}
    for mode, dbg in (("table", None), ("no_table", str(0x8000)), ("all_marked", str(0x40000000))):
        if dbg is None:
            monkeypatch.delenv("PYA_DEBUG", raising=False)
        else:
            monkeypatch.setenv("PYA_DEBUG", dbg)
        scorers[mode] = _gpu(settings)
    for placement, batch in batches.items():
        recs = {}
        for mode, gpu in scorers.items():
            _same_results(gpu.score_batch(batch), want[placement], es.KEYS, "%s %s %s" % (name, placement, mode))
            gpu.score_batch(batch, keep=True)
            recs[mode] = gpu.batch_pep_scores()
        for mode in ("table", "all_marked"):
            assert sorted(recs[mode]) == sorted(recs["no_table"])
            for key in recs["no_table"]:
                assert np.array_equal(recs[mode][key], recs["no_table"][key]), (name, placement, mode, key)
        for i in range(3):
            chk.score(**synth.unpack_psm(batch, i))
            raw = chk.raw_pep_scores()
            a, e = recs["table"]["rec_off"][i], recs["table"]["rec_off"][i + 1]
            bits = (raw["signature"].astype(np.uint64) << np.arange(raw["signature"].shape[1], dtype=np.uint64)).sum(axis=1).astype(np.uint64)
            assert np.array_equal(recs["table"]["sig_bits"][a:e], bits), (name, placement, i)
            for key in ("counts", "scores", "weighted_score", "total_fragments"):
                assert recs["table"][key][a:e].tobytes() == np.ascontiguousarray(raw[key], recs["table"][key].dtype).tobytes(), (name, placement, i, key)


@pytest.mark.parametrize("name", GENERAL_KERNEL)
def test_general_kernel_psm_by_psm(name):
    """score() + every property and every per-assignment record of all four PSMs (alternative sites as positions: any length)"""
    settings, batches, _ = _case(name)
    gpu, chk = _gpu(settings), es.checker(settings, checker_kind())
    for placement, batch in batches.items():
        _same_psm_by_psm(gpu, chk, batch)


# ---- 3b: score() per PSM -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cfg4", "z7", "z3_sty_err075"])
def test_score_psm_by_psm(name):
    settings, batches, _ = _case(name)
    gpu, chk = _gpu(settings), es.checker(settings, checker_kind())
    for placement, batch in batches.items():
        sub = synth.slice_batch(batch, 0, 4)
        got, want = harness.collect(gpu, sub, synth.unpack_psm), harness.collect(chk, sub, synth.unpack_psm)
        assert harness.compare(got, want, exact_float=True) == [], (name, placement)


# ---- 3c: typed and shared forms ----------------------------------------------------------------------------------------
def _two_hits(batch):
    """every spectrum with two hits: its own PSM, then the peptide of the next PSM"""
    n = int(batch["n_psm"])
    spectra, psms = [], []
    for i in range(n):
        kw = synth.unpack_psm(batch, i)
        spectra.append(dict(mz=kw["mz_arr"], intensity=kw["int_arr"]))
        for j in (i, (i + 1) % n):
            other = synth.unpack_psm(batch, j)
            psms.append(dict(spectrum=i, peptide=other["peptide"], n_of_mod=other["n_of_mod"], max_charge=other["max_fragment_charge"]))
    return synth.pack_shared_batch(spectra, psms)


@pytest.mark.parametrize("route", ["single_launch", "three_kernels"])
@pytest.mark.parametrize("name", list(es.CASES))
def test_typed_and_shared_forms_give_the_same_bytes(name, route, monkeypatch):
    if route == "three_kernels":
        _three_kernels(monkeypatch)
    else:
        for v in ("PYA_NO_TINY", "PYA_PLAIN_MIN", "PYA_DEBUG"):
            monkeypatch.delenv(v, raising=False)
    settings, batches, want = _case(name)
    gpu, chk = _gpu(settings), es.checker(settings, checker_kind())
    for placement, batch in batches.items():
        keys, what = _keys(batch), "%s %s" % (name, placement)
        narrow = synth.narrow_batch(batch)
        assert narrow["mz"].dtype == np.float32 and np.array_equal(narrow["mz"].astype(np.float64), batch["mz"])   # (nothing is lost)
        _same_results(gpu.score_batch(narrow), want[placement], keys, what + " float32")
        _same_results(gpu.score_batch(synth.narrow_batch(batch, np.float32, np.float64)), want[placement], keys, what + " float32 m/z")
        shared = _two_hits(batch)
        got = gpu.score_batch(shared)
        _same_results({k: got[k][::2] for k in keys}, want[placement], keys, what + " own hits of shared spectra")
        expanded = synth.expand_shared_batch(shared)
        _same_results(got, chk.score_batch(expanded, int(expanded["n_of_mod"].max())), keys, what + " shared spectra")
        _same_results(gpu.score_batch(synth.narrow_batch(shared)), got, keys, what + " shared float32")


# ---- 3d: the later stages, which match peaks themselves ------------------------------------------------------------------
STAGES = {
    "evidence": lambda st, b, what: t_evidence._general_case(st, b, what),
    "ions": lambda st, b, what: t_ions._general_case(st, b, what),             # matched m/z, rank and counted flag of every ion record
    "named": lambda st, b, what: t_named._against_yardstick(st, b, what),
    "sites": lambda st, b, what: t_sites._against_yardstick(st, b, what),
    "probs": lambda st, b, what: t_probs._against_yardstick(st, b, what),
    "ranked": lambda st, b, what: t_ranked._against_yardstick(st, b, what),
    "mz_profile": lambda st, b, what: t_mz_profile._against_yardstick(st, b, what),
}


@pytest.mark.parametrize("stage", list(STAGES))
@pytest.mark.parametrize("name", ["cfg4", "L30_210_z3", "cfg4_err05", "z3_sty_err075"])
def test_later_stages_equal_their_yardsticks(name, stage, monkeypatch):
    _three_kernels(monkeypatch)
    settings, batches, want = _case(name)
    for placement, batch in batches.items():
        sub = synth.slice_batch(batch, 0, 8)
        STAGES[stage](settings, sub, "%s %s (%s)" % (name, placement, stage))
