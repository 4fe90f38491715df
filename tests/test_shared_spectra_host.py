"""Shared spectra, the host side (no GPU): several PSMs scored against ONE copy of a spectrum -- the hits of a scan in the
reference's command line (`pyascore/__main__.py`, the groupby(psms, scan) / hit_depth loop).  The C ABI has the two entry
points, the packing helpers turn a shared batch into the repeated-spectrum batch it must score like, the ingest path packs
the hits of a scan onto one spectrum, and a batch in any PSM order is put into the order the library wants and back."""
import ctypes as C
import os
import re

import numpy as np

from pyascore_amd import _lib, ingest, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "ingest")
PHOSPHO = 79.966331
CSR = ("mz", "intensity", "peak_off", "pep", "pep_off", "n_of_mod", "max_charge", "aux_pos", "aux_mass", "aux_off")


def test_the_header_declares_and_the_library_exports_the_shared_entry_points():
    header = open(os.path.join(ROOT, "include", "pyascore_hip.h")).read()
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("pya_score_batch_shared", "pya_plan_create_shared"):
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert decl, name + " is not declared in include/pyascore_hip.h"
        assert "const uint32_t *spec_of" in decl.group(1) and "uint64_t n_spectra" in decl.group(1)
        assert hasattr(lib, name), name + " is not exported by the built library"
        assert name in _lib.SYMBOLS
    assert "__main__.py" in header[header.index("Several PSMs against one spectrum"):header.index("int pya_score_batch_shared")]


def _shared_case(seed=3, n_spec=7):
    """n_spec cfg2 spectra, 1 .. 4 PSMs on each with peptides, charges and fixed modifications of their own."""
    base, _ = synth.make_batch("cfg2", n_psm=4 * n_spec, seed=seed)
    rng = np.random.default_rng(seed)
    spectra = []
    for s in range(n_spec):
        kw = synth.unpack_psm(base, s)
        spectra.append(dict(mz=kw["mz_arr"], intensity=kw["int_arr"]))
    psms = []
    for s in range(n_spec):
        for _ in range(int(rng.integers(1, 5))):
            kw = synth.unpack_psm(base, int(rng.integers(0, base["n_psm"])))
            aux = int(rng.integers(0, 3))
            psms.append(dict(spectrum=s, peptide=kw["peptide"], n_of_mod=kw["n_of_mod"], max_charge=int(rng.integers(1, 4)),
                             aux_pos=rng.integers(0, len(kw["peptide"]) + 1, aux).astype(np.uint32),
                             aux_mass=rng.uniform(1., 80., aux).astype(np.float32)))
    return spectra, psms


def test_pack_then_expand_is_the_repeated_spectrum_batch():
    spectra, psms = _shared_case()
    shared = synth.pack_shared_batch(spectra, psms)
    assert shared["n_spectra"] == len(spectra) and shared["peak_off"].size == len(spectra) + 1
    assert shared["spec_of"].dtype == np.uint32 and shared["spec_of"].tolist() == [p["spectrum"] for p in psms]
    assert shared["mz"].size == sum(len(sp["mz"]) for sp in spectra)              # every spectrum once
    want = synth.pack_batch([dict(p, mz=spectra[p["spectrum"]]["mz"], intensity=spectra[p["spectrum"]]["intensity"]) for p in psms])
    got = synth.expand_shared_batch(shared)
    assert got["n_psm"] == want["n_psm"] == len(psms) and "spec_of" not in got and "n_spectra" not in got
    for key in CSR:
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), key
    # a spectrum nobody refers to stays in the shared arrays and out of the expanded ones
    lonely = synth.pack_shared_batch(spectra + [dict(mz=[100.5, 200.5], intensity=[1., 2.])], psms)
    assert lonely["n_spectra"] == len(spectra) + 1 and lonely["mz"].size == shared["mz"].size + 2
    again = synth.expand_shared_batch(lonely)
    for key in CSR:
        assert np.array_equal(again[key], want[key]), key


def test_the_hits_of_a_scan_share_its_spectrum_in_to_batch():
    spectra = ingest.SpectraParser(os.path.join(DATA, "test_spectra.mzML"), "mzML").to_dict()
    psms = ingest.IdentificationParser(os.path.join(DATA, "test_psms.pep.xml"), "pepXML", score_string="xcorr_score").to_list()
    one, scans1 = ingest.to_batch(psms, spectra, "STY", PHOSPHO, hit_depth=1)
    assert "spec_of" not in one and one["peak_off"].size == one["n_psm"] + 1 == 11      # one hit per scan: today's batch
    batch, scans = ingest.to_batch(psms, spectra, "STY", PHOSPHO, hit_depth=2)
    assert batch["n_psm"] == len(scans) == 19 and batch["n_spectra"] == 10 and batch["peak_off"].size == 11
    so = batch["spec_of"].astype(np.int64)
    assert np.all(np.diff(so) >= 0) and so[0] == 0 and so[-1] == 9
    assert [scans[i] for i in np.flatnonzero(np.diff(np.concatenate([[-1], so])))] == scans1       # one spectrum per scan, in order
    assert np.array_equal(batch["peak_off"], one["peak_off"])
    assert np.array_equal(batch["mz"], one["mz"]) and np.array_equal(batch["intensity"], one["intensity"])
    for i, scan in enumerate(scans):                                # every PSM reads its own scan's peaks
        s = so[i]
        assert np.array_equal(batch["mz"][batch["peak_off"][s]:batch["peak_off"][s + 1]], spectra[scan]["mz_values"])
    # ... and expands to what the per-PSM packing of the same hits gives
    from pyascore_amd.batch_cli import select_psms
    picked, _ = select_psms(sorted(psms, key=lambda p: p["scan"]), spectra, "STY", PHOSPHO, 2)
    want = synth.pack_batch(picked)
    got = synth.expand_shared_batch(batch)
    for key in CSR:
        assert np.array_equal(got[key], want[key]), key


def test_a_batch_in_any_order_is_sorted_by_spectrum_and_put_back():
    assert synth.spectrum_order([0, 0, 1, 3, 3]) == (None, None)
    assert synth.spectrum_order([]) == (None, None) and synth.spectrum_order([5]) == (None, None)
    spec_of = np.array([2, 0, 2, 1, 0, 2], np.uint32)
    perm, inv = synth.spectrum_order(spec_of)
    assert perm.tolist() == [1, 4, 3, 0, 2, 5]                      # stable: the PSMs of a spectrum keep their order
    assert np.all(np.diff(spec_of[perm].astype(np.int64)) >= 0)
    rows = np.arange(6) * 10
    assert np.array_equal(rows[perm][inv], rows)                    # sorted rows back in input order
    spectra, psms = _shared_case(seed=11, n_spec=5)
    order = np.random.default_rng(1).permutation(len(psms))
    shuffled = synth.pack_shared_batch(spectra, [psms[i] for i in order])
    perm, inv = synth.spectrum_order(shuffled["spec_of"])
    ordered = synth.take_psms(shuffled, perm)
    assert np.all(np.diff(ordered["spec_of"].astype(np.int64)) >= 0) and ordered["n_psm"] == len(psms)
    want = synth.pack_shared_batch(spectra, [psms[i] for i in order[perm]])
    for key in CSR + ("spec_of",):
        assert np.array_equal(ordered[key], want[key]), key
