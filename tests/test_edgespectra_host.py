"""The edge spectra of tests/edgespectra.py, without a GPU: a condition on the INPUTS of tests/test_gpu_general_edges.py (a batch
whose results do not move when every peak moves by one float32 ulp cannot tell a window end one ulp off), and the CPU
restatement against the reference's own core on exactly these batches."""
import numpy as np
import pytest

import edgespectra as es
from oracle import harness, orc
from pyascore_amd import synth

needs_ref = pytest.mark.skipif(not orc.available("ref"), reason="oracle/_ref not built")
KIND = "ref" if orc.available("ref") else "oracle"


@pytest.mark.parametrize("name", list(es.CASES))
def test_most_psms_notice_one_ulp(name):
    """every case x placement the GPU tests use: at least half of the PSMs change some result under nudge(+1), the checker
    alone (measured: the table in edgespectra's docstring).  A case that falls short gets another draw, not another bar."""
    settings, batches = es.case_batches(name, KIND)
    assert tuple(batches) == es.placements(settings)
    for placement, batch in batches.items():
        n = es.sharpness(settings, batch, KIND)
        print("%s %s: %d of %d PSMs notice +1 ulp" % (name, placement, n, batch["n_psm"]))
        assert 2 * n >= batch["n_psm"], (name, placement, n)


@needs_ref
@pytest.mark.parametrize("name", list(es.CASES))
def test_restatement_equals_the_reference(name):
    settings, batches = es.case_batches(name, "ref")
    ref, port = es.checker(settings, "ref"), es.checker(settings, "oracle")
    for placement, batch in batches.items():
        k = int(batch["n_of_mod"].max())
        bad = es.changed(ref.score_batch(batch, k), port.score_batch(batch, k))
        assert bad.size == 0, (name, placement, bad[:10].tolist())
    for i in range(2):                                                              # ... and every per-assignment record of two PSMs
        kw = synth.unpack_psm(batches["ends"], i)
        ref.score(**kw)
        port.score(**kw)
        a, b = ref.raw_pep_scores(), port.raw_pep_scores()
        for key in a:
            assert a[key].tobytes() == b[key].tobytes(), (name, i, key)
        assert ref.best_sequence == port.best_sequence and ref.ascores.tobytes() == port.ascores.tobytes(), (name, i)
        assert [s.tolist() for s in ref.alt_sites] == [s.tolist() for s in port.alt_sites], (name, i)   # (positions: any peptide length)


@needs_ref
def test_the_generator_does_not_depend_on_the_checker():
    """the ions come from the checker: either kind draws the same spectra"""
    for name in ("cfg4", "z7", "z2_err4"):
        a, b = es.case_batches(name, "ref")[1], es.case_batches(name, "oracle")[1]
        for placement in a:
            for key in ("mz", "intensity", "peak_off"):
                assert np.array_equal(a[placement][key], b[placement][key]), (name, placement, key)


def test_the_batches_are_what_the_docstring_says():
    settings, batches = es.case_batches("cfg4_err05", KIND)
    for placement, batch in batches.items():
        for key in ("mz", "intensity"):
            assert batch[key].dtype == np.float64 and np.array_equal(batch[key], batch[key].astype(np.float32)), (placement, key)
        n = np.diff(batch["peak_off"])
        assert n.min() > 100 and n.max() <= es.MAX_PEAKS, placement
        for i in range(batch["n_psm"]):
            m = batch["mz"][batch["peak_off"][i]:batch["peak_off"][i + 1]]
            assert np.all(np.diff(m) >= 0) and m[0] > es.MIN_MZ, (placement, i)
        narrow = synth.narrow_batch(batch)
        assert narrow["mz"].dtype == np.float32 and np.array_equal(synth.widen_batch(narrow)["mz"], batch["mz"])
    # an end peak moved by 0 ulps IS f32(f - err) / f32(f + err) of a fragment the checker lists: the largest share of exact hits
    chk = es.checker(settings, KIND)
    kw = synth.unpack_psm(batches["ends"], 0)
    chk.consume_peptide(kw["peptide"], kw["n_of_mod"], kw["max_fragment_charge"])
    ions = np.unique(np.concatenate([chk.fragments(t, z, sig, cap=8192)[0] for t in settings["fragment_types"]
                                     for z in range(1, kw["max_fragment_charge"] + 1) for sig in chk.signature_order("b")]))
    err = np.float32(settings["mz_error"])
    ends = np.concatenate([ions - err, ions + err]).astype(np.float32)
    peaks = kw["mz_arr"].astype(np.float32)
    assert np.isin(peaks, ends).mean() > 0.04          # 1/2 by ulps x 1/7 at j = 0, diluted by the batch's own peaks


def test_nudge_moves_every_peak_by_whole_ulps():
    batch = dict(mz=np.array([100.0, 1024.0, 1999.9999], np.float32).astype(np.float64), n_psm=1)
    up, down = es.nudge(batch, 1)["mz"], es.nudge(batch, -3)["mz"]
    assert up.dtype == np.float64
    assert np.array_equal(up, np.nextafter(batch["mz"].astype(np.float32), np.float32(np.inf)).astype(np.float64))
    x = batch["mz"].astype(np.float32)
    for _ in range(3):
        x = np.nextafter(x, np.float32(0))
    assert np.array_equal(down, x.astype(np.float64))
    assert np.array_equal(es.nudge(es.nudge(batch, 5), -5)["mz"], batch["mz"])
    typed = es.nudge(dict(batch, mz=batch["mz"].astype(np.float32)), 2)["mz"]
    assert typed.dtype == np.float32 and np.array_equal(typed.astype(np.float64), es.nudge(batch, 2)["mz"])
