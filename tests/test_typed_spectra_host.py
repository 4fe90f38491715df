"""Typed spectra, the parts that need no GPU: the C structure and the two prototypes as header and ctypes table have them,
synth's narrowing / widening and the packs that keep a spectrum's dtype, the parsers' native precision, and the command
line's packing of typed spectra."""
import base64
import ctypes as C
import os
import re
import zlib

import numpy as np
import pytest

from conftest import ROOT
from pyascore_amd import _lib, batch_cli, ingest, synth

GOLDEN = os.path.join(ROOT, "tests", "golden", "ingest")


def _header():
    text = open(os.path.join(ROOT, "include", "pyascore_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_and_ctypes_agree_on_the_structure_and_the_prototypes():
    text = _header()
    body = re.search(r"typedef struct pya_typed_spectra \{(.*?)\} pya_typed_spectra;", text, flags=re.S).group(1)
    fields = [f.strip() for f in body.replace("\n", " ").split(";") if f.strip()]
    assert fields == ["const void *mz, *intensity", "uint32_t mz_type, intensity_type"]
    assert [n for n, _ in _lib.TypedSpectra._fields_] == ["mz", "intensity", "mz_type", "intensity_type"]
    assert [t for _, t in _lib.TypedSpectra._fields_] == [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
    assert C.sizeof(_lib.TypedSpectra) == 24 and _lib.TypedSpectra.mz_type.offset == 16
    assert re.search(r"#define PYA_F64 0u", text) and re.search(r"#define PYA_F32 1u", text)
    assert (_lib.PYA_F64, _lib.PYA_F32) == (0, 1)
    assert _lib.spectrum_type(np.dtype(np.float64)) == 0 and _lib.spectrum_type(np.dtype(np.float32)) == 1
    with pytest.raises(ValueError):
        _lib.spectrum_type(np.dtype(np.float16))

    def params(name):
        m = re.search(r"int %s\((.*?)\);" % name, text, flags=re.S)
        return [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]

    assert params("pya_score_batch_typed") == ["pya_handle *h", "const pya_batch *batch", "const uint32_t *spec_of", "uint64_t n_spectra",
                                               "const pya_typed_spectra *spectra", "uint32_t flags", "const pya_results *out"]
    assert params("pya_plan_run_typed") == ["pya_plan *plan", "const pya_typed_spectra *d_spectra", "void *hip_stream",
                                            "const pya_results *d_out"]
    res, args = _lib.SYMBOLS["pya_score_batch_typed"]
    assert res is C.c_int and args == [C.c_void_p, C.POINTER(_lib.Batch), C.c_void_p, C.c_uint64, C.POINTER(_lib.TypedSpectra),
                                       C.c_uint32, C.POINTER(_lib.Results)]
    res, args = _lib.SYMBOLS["pya_plan_run_typed"]
    assert res is C.c_int and args == [C.c_void_p, C.POINTER(_lib.TypedSpectra), C.c_void_p, C.POINTER(_lib.Results)]


def test_narrow_and_widen_keep_values_and_offsets():
    batch, _ = synth.make_batch("cfg2", n_psm=40, seed=3)
    for mz_t, it_t in ((np.float64, np.float32), (np.float32, np.float32), (np.float64, np.float64)):
        nb = synth.narrow_batch(batch, mz=mz_t, intensity=it_t)
        assert nb["mz"].dtype == mz_t and nb["intensity"].dtype == it_t
        assert np.array_equal(nb["mz"], batch["mz"].astype(mz_t)) and np.array_equal(nb["intensity"], batch["intensity"].astype(it_t))
        wb = synth.widen_batch(nb)
        assert wb["mz"].dtype == np.float64 and wb["intensity"].dtype == np.float64
        assert np.array_equal(wb["mz"], nb["mz"]) and np.array_equal(wb["intensity"], nb["intensity"])
        for k in ("peak_off", "pep", "pep_off", "n_of_mod", "max_charge", "aux_pos", "aux_mass", "aux_off"):
            assert nb[k] is batch[k] and wb[k] is batch[k]
    assert synth.narrow_batch(batch)["mz"].dtype == np.float32                  # (the defaults)
    assert not np.array_equal(synth.widen_batch(synth.narrow_batch(batch))["mz"], batch["mz"])   # (rounded, not reinterpreted)


def _psms(batch, n):
    out = []
    for i in range(n):
        kw = synth.unpack_psm(batch, i)
        out.append(dict(mz=kw["mz_arr"], intensity=kw["int_arr"], peptide=kw["peptide"], n_of_mod=kw["n_of_mod"],
                        max_charge=kw["max_fragment_charge"]))
    return out


def test_packs_keep_the_dtype_of_the_spectra_they_are_given():
    batch, _ = synth.make_batch("cfg2", n_psm=12, seed=5)
    typed = synth.narrow_batch(batch, mz=np.float64, intensity=np.float32)
    packed = synth.pack_batch(_psms(typed, 12))
    assert packed["mz"].dtype == np.float64 and packed["intensity"].dtype == np.float32
    assert np.array_equal(packed["intensity"], typed["intensity"]) and np.array_equal(packed["peak_off"], typed["peak_off"])
    both = synth.pack_batch(_psms(synth.narrow_batch(batch), 12))
    assert both["mz"].dtype == np.float32 and both["intensity"].dtype == np.float32
    mixed = _psms(typed, 6) + _psms(batch, 12)[6:]                              # float32 and float64 intensities: widened
    m = synth.pack_batch(mixed)
    assert m["intensity"].dtype == np.float64 and np.array_equal(m["intensity"][:typed["peak_off"][6]], typed["intensity"][:typed["peak_off"][6]])
    assert synth.pack_batch(_psms(batch, 3))["mz"].dtype == np.float64           # (float64 stays float64)
    spectra = [dict(mz=p["mz"], intensity=p["intensity"]) for p in _psms(typed, 4)]
    hits = [dict(spectrum=i // 2, peptide=p["peptide"], n_of_mod=p["n_of_mod"]) for i, p in enumerate(_psms(typed, 8))]
    shared = synth.pack_shared_batch(spectra, hits)
    assert shared["mz"].dtype == np.float64 and shared["intensity"].dtype == np.float32 and shared["n_spectra"] == 4
    ex = synth.expand_shared_batch(shared)
    assert ex["intensity"].dtype == np.float32 and ex["mz"].dtype == np.float64 and ex["peak_off"].size == 9
    assert np.array_equal(ex["intensity"][:ex["peak_off"][2]], np.tile(spectra[0]["intensity"], 2))
    taken = synth.take_psms(shared, np.array([7, 0, 3]))
    assert taken["intensity"].dtype == np.float32 and taken["intensity"] is shared["intensity"]
    cut = synth.slice_batch(typed, 2, 7)
    assert cut["intensity"].dtype == np.float32 and cut["mz"].dtype == np.float64
    assert np.array_equal(cut["intensity"], typed["intensity"][typed["peak_off"][2]:typed["peak_off"][7]])


def _by_scan(path, fmt, **kw):
    return ingest.SpectraParser(path, fmt, **kw).to_dict()


def test_native_precision_on_the_committed_example_files():
    """the mzML declares 64-bit m/z and 32-bit intensities for every scan, the mzXML precision="64"; the default reader
    gives float64 for both, as before"""
    mzml = os.path.join(GOLDEN, "test_spectra.mzML")
    plain, native = _by_scan(mzml, "mzML"), _by_scan(mzml, "mzML", native_precision=True)
    assert plain.keys() == native.keys() and len(plain) > 0
    for scan, rec in native.items():
        assert rec["mz_values"].dtype == np.float64 and rec["intensity_values"].dtype == np.float32
        assert plain[scan]["mz_values"].dtype == np.float64 and plain[scan]["intensity_values"].dtype == np.float64
        assert np.array_equal(rec["mz_values"], plain[scan]["mz_values"])
        assert np.array_equal(rec["intensity_values"].astype(np.float64), plain[scan]["intensity_values"])
        assert rec["intensity_values"].flags.writeable and rec["intensity_values"].dtype.isnative
    mzxml = os.path.join(GOLDEN, "test_spectra.mzXML")
    plain, native = _by_scan(mzxml, "mzXML"), _by_scan(mzxml, "mzXML", native_precision=True)
    for scan, rec in native.items():
        assert rec["mz_values"].dtype == np.float64 and rec["intensity_values"].dtype == np.float64
        assert np.array_equal(rec["mz_values"], plain[scan]["mz_values"])
        assert np.array_equal(rec["intensity_values"], plain[scan]["intensity_values"])


def _b64(values, dtype, compress):
    raw = np.asarray(values).astype(dtype).tobytes()
    return base64.b64encode(zlib.compress(raw) if compress else raw).decode()


def test_native_precision_on_32_bit_compressed_files(tmp_path):
    mz = np.array([110.5, 220.25, 330.125, 440.0625], np.float64)
    it = np.array([10.0, 2000.5, 30.25, 4.0], np.float64)
    mzml = tmp_path / "c.mzML"
    mzml.write_text(
        '<?xml version="1.0"?><mzML xmlns="http://psi.hupo.org/ms/mzml"><run><spectrumList count="1">'
        '<spectrum index="0" id="controllerType=0 controllerNumber=1 scan=9" defaultArrayLength="4">'
        '<cvParam name="ms level" value="2"/><binaryDataArrayList count="2">'
        '<binaryDataArray><cvParam name="32-bit float"/><cvParam name="zlib compression"/><cvParam name="m/z array"/>'
        '<binary>%s</binary></binaryDataArray>'
        '<binaryDataArray><cvParam name="32-bit float"/><cvParam name="zlib compression"/><cvParam name="intensity array"/>'
        '<binary>%s</binary></binaryDataArray></binaryDataArrayList></spectrum></spectrumList></run></mzML>'
        % (_b64(mz, "<f4", True), _b64(it, "<f4", True)))
    pairs = np.empty(8)
    pairs[0::2], pairs[1::2] = mz, it
    mzxml = tmp_path / "c.mzXML"
    mzxml.write_text(
        '<?xml version="1.0"?><mzXML xmlns="http://sashimi.sourceforge.net/schema_revision/mzXML_3.2"><msRun>'
        '<scan num="9" msLevel="2" peaksCount="4"><peaks precision="32" byteOrder="network" compressionType="zlib" '
        'contentType="m/z-int">%s</peaks></scan></msRun></mzXML>' % _b64(pairs, ">f4", True))
    for path, fmt in ((mzml, "mzML"), (mzxml, "mzXML")):
        plain, native = _by_scan(str(path), fmt)[9], _by_scan(str(path), fmt, native_precision=True)[9]
        for key, want in (("mz_values", mz), ("intensity_values", it)):
            assert plain[key].dtype == np.float64 and native[key].dtype == np.float32, (fmt, key)
            assert native[key].dtype.isnative and native[key].flags.c_contiguous
            assert np.array_equal(native[key].astype(np.float64), plain[key]) and np.array_equal(plain[key], want.astype(np.float32))
    with pytest.raises(TypeError):
        ingest.SpectraParser(str(mzml), "mzML", 2, None, False, True)            # (one new parameter, no more)


def test_the_command_lines_packing_keeps_typed_spectra():
    """two hits of a scan share its float32 intensities (shared batch), one hit per scan gives pack_batch's arrays"""
    spectra = _by_scan(os.path.join(GOLDEN, "test_spectra.mzML"), "mzML", native_precision=True)
    scans = sorted(spectra)[:3]
    picked = [dict(mz=spectra[s]["mz_values"], intensity=spectra[s]["intensity_values"], peptide="ASTK", n_of_mod=1, max_charge=1,
                   aux_pos=np.zeros(0, np.uint32), aux_mass=np.zeros(0, np.float32)) for s in scans]
    one = batch_cli.pack_hits(picked, scans)
    assert one["mz"].dtype == np.float64 and one["intensity"].dtype == np.float32 and "spec_of" not in one
    assert np.array_equal(one["intensity"], np.concatenate([spectra[s]["intensity_values"] for s in scans]))
    twice = [picked[0], dict(picked[0], peptide="ATSK"), picked[1]]
    shared = batch_cli.pack_hits(twice, [scans[0], scans[0], scans[1]])
    assert shared["spec_of"].tolist() == [0, 0, 1] and shared["intensity"].dtype == np.float32 and shared["mz"].dtype == np.float64
    assert shared["intensity"].size == spectra[scans[0]]["intensity_values"].size + spectra[scans[1]]["intensity_values"].size
