"""The host side of the marker-ion stage (pya_marker_params): the numpy restatement pyascore_amd.rollup.markers on hand-made
spectra whose records are written out by hand (tests/markers_cases.py), its independence of the order of the peaks, the
parameters and their 544-byte layout, planted reporter and precursor-loss peaks recovered from synthetic spectra, and the
public surface (header, bindings, argument checks, command line).  No GPU."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import markers_cases as mc
from pyascore_amd import _lib, rollup as ru, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = mc.hand_cases()
NAN, INF = float("nan"), float("inf")


def _run(case):
    x, y = case["mz"], case["intensity"]
    return ru.markers(x, y, [0, x.size], case["params"], [case["prec_mz"]], [case["prec_z"]])


# ---- the rule, one case each ----

@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hand_made_spectrum(case):
    rec, spec = _run(case)
    assert rec.dtype == ru.MARKER_DTYPE and rec.shape == (1, len(case["params"]["value"]))
    assert spec.dtype == ru.MARKER_SPECTRUM_DTYPE and spec.shape == (1,)
    assert rec[0].tolist() == case["markers"].tolist() and spec.tolist() == case["spectrum"].tolist()
    assert rec.tobytes() == case["markers"].tobytes(), "the bytes: no -0.0 reaches a record"
    assert spec.tobytes() == case["spectrum"].tobytes()


def test_the_cases_cover_what_the_rule_names():
    names = " | ".join(c["name"] for c in CASES)
    for word in ("edges of target 0, float64", "edges of target 0, float32", "larger intensity", "nearer the centre", "the smaller m/z",
                 "duplicate", "two overlapping windows", "NaN m/z", "NaN intensity", "-0.0", "no usable precursor", "target 63 of 64",
                 "no peaks"):
        assert word in names, word


def test_windows_against_the_numbers_of_the_header():
    cen, lo, hi, active = ru.marker_windows(400.0, 2, mc.P_BASE)
    assert cen.tolist() == [126.125, 384.0] and lo.tolist() == [126.1171875, 383.9921875] and hi.tolist() == [126.1328125, 384.0078125]
    assert active.tolist() == [True, True]
    cen, lo, hi, active = ru.marker_windows([400.0, 300.0, 400.0], [2, 3, 0], mc.P_BASE)
    assert cen.shape == (3, 2) and active.tolist() == [[True, True], [True, True], [True, False]]
    assert cen[1, 1] == (300.0 * 3.0 - 32.0) / 3.0 and np.isnan(cen[2, 1]) and np.isnan(lo[2, 1]) and np.isnan(hi[2, 1])
    # ppm of the centre on top of tol, in the header's order
    p = ru.marker_params(mz=(500.0,), losses=(97.976896,), tol=0.003, tol_ppm=15.0)
    cen, lo, hi, active = ru.marker_windows(650.3, 3, p)
    c1 = (650.3 * 3.0 - 97.976896) / 3.0
    for t, c in enumerate((500.0, c1)):
        w = 0.003 + (15.0 * 1e-6) * c
        assert (cen[t], lo[t], hi[t]) == (c, c - w, c + w)
    for pm, pz in ((400.0, 0), (400.0, -1), (400.0, 9), (NAN, 2), (INF, 2), (0.0, 2), (-1.0, 2)):
        assert ru.marker_windows(pm, pz, mc.P_BASE)[3].tolist() == [True, False]
    assert ru.marker_windows(400.0, 2, mc.P_BIG_LOSS)[3].tolist() == [True, False, False, True]
    assert ru.marker_windows(400.0, 2, mc.P_64)[3].all() and ru.marker_windows(400.0, 2, mc.P_64)[0][63] == 384.0


# ---- the definition is order-free ----

def _random_spectra(seed, n_spec=40):
    """spectra of 0 .. 200 peaks with many peaks in the windows of P_BASE, few distinct intensities, NaN among both arrays"""
    rng = np.random.default_rng(seed)
    spots = np.array([mc.C + k * mc.D for k in range(-5, 6)] + [mc.L + k * mc.D for k in range(-5, 6)])
    spectra = []
    for n in rng.integers(0, 201, n_spec):
        x = rng.uniform(100.0, 1000.0, size=n)
        x = np.where(rng.random(n) < 0.3, rng.choice(spots, size=n), x)
        y = rng.choice([-0.0, 0.0, 1.0, 2.0, 3.0, 3.0, NAN], size=n)
        x[rng.random(n) < 0.02] = NAN
        spectra.append((x, y))
    return spectra


def test_the_records_do_not_depend_on_the_order_of_the_peaks():
    rng = np.random.default_rng(5)
    spectra = _random_spectra(9)
    n = len(spectra)
    pm, pz = np.full(n, 400.0), np.full(n, 2, np.int32)
    mz, it, off = mc.pack(spectra, gaps=False)
    rec, spec = ru.markers(mz, it, off, mc.P_BASE, pm, pz)
    assert (rec["n_peaks"] > 3).any() and (spec["hit"] == 3).any() and ((rec["flags"] & ru.MARKER_PICKED) == 0).any()
    shuffled = []
    for x, y in spectra:
        perm = rng.permutation(x.size)
        shuffled.append((x[perm], y[perm]))
    mz2, it2, off2 = mc.pack(shuffled, gaps=False)
    assert mz2.tobytes() != mz.tobytes() and off2.tobytes() == off.tobytes()
    rec2, spec2 = ru.markers(mz2, it2, off2, mc.P_BASE, pm, pz)
    assert rec2.tobytes() == rec.tobytes()
    for name in ("base_peak", "hit", "n_peaks", "n_active"):
        assert spec2[name].tobytes() == spec[name].tobytes(), name
    # tic is a float sum: its order is pinned instead -- 64 partials by peak index modulo 64, added in lane order
    for (x, y), got in list(zip(spectra, spec["tic"])) + list(zip(shuffled, spec2["tic"])):
        want = ru._lane_sum([v if v == v else 0.0 for v in y.tolist()])
        assert np.float64(want).tobytes() == np.float64(got).tobytes()


def test_tic_is_the_lane_sum_and_not_another_order():
    """values whose sum depends on the order: 1e16 in lane 0, then 64 ones in lanes 1 .. 63 and 0 -- the one of lane 0 is lost
    against 1e16, the 63 others add up among themselves first"""
    y = np.array([1e16] + [1.0] * 64)
    x = np.full(y.size, 500.0)
    _, spec = ru.markers(x, y, [0, y.size], mc.P_FIXED)
    part0 = (1e16 + 1.0)                                                   # lane 0: peaks 0 and 64
    want = part0
    for _ in range(63):
        want = want + 1.0
    assert spec["tic"][0] == want == ru._lane_sum(y.tolist())
    assert want != sum(sorted(y.tolist())) == 1e16 + 64.0                  # (an ascending sum keeps every one)
    assert spec["base_peak"][0] == 1e16 and spec["n_peaks"][0] == 65


# ---- parameters ----

def test_marker_params_and_their_faults():
    p = ru.marker_params(mz=(126.1277, 127.1248), losses=(97.976896,), tol=0.003, tol_ppm=10.0)
    assert p == dict(tol=0.003, tol_ppm=10.0, value=(126.1277, 127.1248, 97.976896), loss_mask=0b100)
    assert ru.check_marker_params(p) == p
    assert ru.marker_params(mz=[1.0])["loss_mask"] == 0 and ru.marker_params(losses=[0.0])["loss_mask"] == 1
    assert ru.marker_params(mz=np.arange(1.0, 33.0), losses=np.arange(32.0))["loss_mask"] == 0xFFFFFFFF00000000
    bad = [dict(), dict(mz=(1.0,) * 65), dict(mz=(1.0,) * 33, losses=(1.0,) * 32), dict(mz=(0.0,)), dict(mz=(-1.0,)), dict(mz=(NAN,)),
           dict(mz=(INF,)), dict(losses=(-1.0,)), dict(losses=(NAN,)), dict(losses=(INF,)), dict(mz=(1.0,), tol=-0.1), dict(mz=(1.0,), tol=NAN),
           dict(mz=(1.0,), tol=INF), dict(mz=(1.0,), tol_ppm=-1.0), dict(mz=(1.0,), tol_ppm=NAN), dict(mz=(1.0,), tol_ppm=INF), dict(mz=1.0),
           dict(mz=("x",)), dict(mz=(1.0,), tol=None)]
    for kw in bad:
        with pytest.raises(ValueError):
            ru.marker_params(**kw)
    for change in (dict(loss_mask=0b1000), dict(loss_mask=-1), dict(loss_mask=0.5), dict(loss_mask=None), dict(value=()), dict(value=None),
                   dict(value=(1.0, 0.0, 1.0), loss_mask=0b100), dict(tol="a")):
        with pytest.raises(ValueError):
            ru.check_marker_params(dict(p, **change))
    with pytest.raises(ValueError):
        ru.check_marker_params({k: v for k, v in p.items() if k != "tol_ppm"})
    # a loss of 0.0 is the precursor itself; a fixed target of 0.0 is refused
    assert ru.check_marker_params(dict(p, value=(1.0, 1.0, 0.0)))["value"][2] == 0.0


def test_the_c_structure_is_the_544_byte_record():
    assert C.sizeof(_lib.MarkerParams) == 544 and C.sizeof(_lib.Marker) == 24 == ru.MARKER_DTYPE.itemsize
    assert C.sizeof(_lib.MarkerSpectrum) == 32 == ru.MARKER_SPECTRUM_DTYPE.itemsize
    offsets = {name: getattr(_lib.MarkerParams, name).offset for name, _ in _lib.MarkerParams._fields_}
    assert offsets == dict(tol=0, tol_ppm=8, value=16, loss_mask=528, n_targets=536, reserved=540)
    for struct, dtype in ((_lib.Marker, ru.MARKER_DTYPE), (_lib.MarkerSpectrum, ru.MARKER_SPECTRUM_DTYPE)):
        assert [f[0] for f in struct._fields_] == list(dtype.names)
        for name, _ in struct._fields_:
            assert getattr(struct, name).offset == dtype.fields[name][1], name
    c = ru.marker_c_params(ru.marker_params(mz=(126.5, 127.5), losses=(18.0,), tol=0.25, tol_ppm=2.0))
    assert (c.tol, c.tol_ppm, c.loss_mask, c.n_targets, c.reserved) == (0.25, 2.0, 0b100, 3, 0)
    assert list(c.value) == [126.5, 127.5, 18.0] + [0.0] * 61
    raw = bytes(c)
    assert len(raw) == 544 and np.frombuffer(raw, "<f8", 66).tolist() == [0.25, 2.0, 126.5, 127.5, 18.0] + [0.0] * 61
    assert np.frombuffer(raw, "<u8", 1, 528)[0] == 0b100 and np.frombuffer(raw, "<u4", 2, 536).tolist() == [3, 0]
    c64 = ru.marker_c_params(mc.P_64)
    assert c64.n_targets == 64 and c64.loss_mask == 1 << 63 and c64.value[63] == 32.0
    with pytest.raises(ValueError):
        ru.marker_c_params(dict(mc.P_BASE, tol=-1.0))
    assert ru.MARKER_MAX_TARGETS == _lib.PYA_MARKER_MAX_TARGETS == 64


def test_what_the_restatement_refuses():
    x, y = np.array([mc.C, mc.L]), np.array([1.0, 2.0])
    ok = ru.markers(x, y, [0, 2], mc.P_FIXED)                               # no loss target: no precursors needed
    assert ok[0]["intensity"].tolist() == [[1.0]]
    with_prec = ru.markers(x, y, [0, 2], mc.P_FIXED, [400.0], [2])
    assert with_prec[0].tobytes() == ok[0].tobytes() and with_prec[1].tobytes() == ok[1].tobytes()
    for args in ((x, y, [0, 2], mc.P_BASE), (x, y, [0, 2], mc.P_BASE, [400.0], None), (x, y, [0, 2], mc.P_BASE, [400.0, 1.0], [2, 2]),
                 (x, y, [0, 2], mc.P_BASE, [400.0], [2.0]), (x, y, [0, 3], mc.P_FIXED), (x, y, [2, 0], mc.P_FIXED), (x, y, [-1, 2], mc.P_FIXED),
                 (x.astype(np.int64), y, [0, 2], mc.P_FIXED), (x, y, [0, 2], dict(mc.P_FIXED, tol=NAN))):
        with pytest.raises(ValueError):
            ru.markers(*args)
    # peak_off[0] > 0: the elements in front are not looked at
    rec, spec = ru.markers(np.concatenate([[mc.C], x]), np.concatenate([[99.0], y]), [1, 3], mc.P_FIXED)
    assert rec.tobytes() == ok[0].tobytes() and spec.tobytes() == ok[1].tobytes()
    # no spectra
    rec, spec = ru.markers(x[:0], y[:0], [0], mc.P_BASE, [], np.zeros(0, np.int32))
    assert rec.shape == (0, 2) and spec.shape == (0,)


def test_marker_matrix():
    rec, _ = ru.markers(np.array([mc.C, mc.L, 300.0]), np.array([5.0, NAN, 1.0]), [0, 2, 3], mc.P_BASE, [400.0, 400.0], [2, 0])
    m = ru.marker_matrix(rec)
    assert m.dtype == np.float64 and m.shape == (2, 2)
    assert m[0, 0] == 5.0 and np.isnan(m[0, 1]) and np.isnan(m[1]).all()      # a NaN intensity is not picked; no peak; inactive
    assert ru.marker_matrix(rec, "mz")[0, 0] == mc.C and ru.marker_matrix(rec, "n_peaks")[0].tolist()[0] == 1.0
    assert np.isnan(ru.marker_matrix(rec, "n_peaks")[0, 1])                  # counted (1), not picked
    with pytest.raises(ValueError):
        ru.marker_matrix(rec, "flags")


# ---- planted recovery ----

def test_planted_reporters_and_a_precursor_loss_come_back_bit_for_bit():
    batch = synth.make_batch("cfg2", 120, seed=3)[0]
    tol = 0.05
    clean_keep = np.asarray(batch["mz"]) >= mc.MZ_LO
    assert 700 < int((~clean_keep).sum()) < 1100                            # (about 900 noise peaks below m/z 140)
    planted, pm, pz, want = mc.with_markers(batch, tol)
    assert planted["mz"].size == batch["mz"].size + 11 * 120
    rec, spec = ru.markers(planted["mz"], planted["intensity"], planted["peak_off"], mc.planted_params(tol), pm, pz)
    assert rec.shape == (120, 11) and (rec["flags"] == 3).all() and (spec["hit"] == 0x7FF).all() and (spec["n_active"] == 11).all()
    assert rec["intensity"].tobytes() == want.tobytes()                     # whatever n_peaks says:
    assert (rec["n_peaks"][:, :10] > 1).any() and (rec["n_peaks"] >= 1).all() and (rec["n_peaks"][:, 10] == 1).all()
    assert rec["mz"][:, :10].tobytes() == np.tile(np.asarray(mc.REPORTERS), (120, 1)).tobytes()
    assert rec["mz"][:, 10].tolist() == [(m * 2.0 - mc.LOSS_H3PO4) / 2.0 for m in pm.tolist()]
    assert spec["base_peak"].tolist() == want[:, 10].tolist()
    assert ru.marker_matrix(rec).tobytes() == want.tobytes()
    # float32 holds the reporters exactly: the same reporter records from narrowed arrays
    rec32, _ = ru.markers(planted["mz"].astype(np.float32), planted["intensity"].astype(np.float32), planted["peak_off"],
                          mc.planted_params(tol), pm, pz)
    assert rec32["mz"][:, :10].tobytes() == rec["mz"][:, :10].tobytes()
    assert rec32["intensity"][:, :10].tolist() == want[:, :10].astype(np.float32).astype(np.float64).tolist()
    # ... and strip, with the reporter region and the loss, gives the clean arrays back: the stage reads what strip removes
    s_mz, s_it, s_off, report = ru.strip(planted["mz"], planted["intensity"], planted["peak_off"], pm, pz,
                                         ru.strip_params(tol, losses=(mc.LOSS_H3PO4,), mz_lo=mc.MZ_LO))
    assert s_mz.tobytes() == np.asarray(batch["mz"])[clean_keep].tobytes()
    assert s_it.tobytes() == np.asarray(batch["intensity"])[clean_keep].tobytes()
    kept = np.add.reduceat(clean_keep.astype(np.int64), np.asarray(batch["peak_off"][:-1], np.int64))
    assert np.diff(s_off).tolist() == kept.tolist() and (report["hit"] == 0b10).all()


# ---- the public surface ----

def test_header_and_bindings_declare_the_interface():
    text = open(os.path.join(ROOT, "include", "pyascore_hip.h")).read()
    assert re.search(r"#define\s+PYA_MARKER_MAX_TARGETS\s+64\b", text)
    for name in ("pya_marker_params", "pya_marker", "pya_marker_spectrum"):
        assert re.search(r"typedef struct %s \{" % name, text), name
    assert re.search(r"int\s+pya_marker_spectra\s*\(\s*pya_handle\s*\*h,\s*const pya_typed_spectra\s*\*d_in", text)
    assert re.search(r"int\s+pya_marker_spectra_host\s*\(\s*pya_handle\s*\*h,\s*const pya_typed_spectra\s*\*in", text)
    from pyascore_amd import build
    build.build()
    lib = _lib.load()
    for name in ("pya_marker_spectra", "pya_marker_spectra_host"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert " T pya_marker_spectra\n" in out and " T pya_marker_spectra_host\n" in out and " T pya_launch_markers\n" in out
    from pyascore_amd import device
    raw = np.arange(2 * 3 * 24, dtype=np.uint8).reshape(2, 3, 24)
    rec = device.marker_records(raw)
    assert rec.shape == (2, 3) and rec.dtype == ru.MARKER_DTYPE and rec["n_peaks"][1, 2] == int.from_bytes(bytes(range(136, 140)), "little")
    spec = device.marker_spectrum_records(np.arange(64, dtype=np.uint8).reshape(2, 32))
    assert spec.shape == (2,) and spec["n_active"][1] == int.from_bytes(bytes(range(60, 64)), "little")
    for bad in (raw.reshape(6, 24), raw[:, :, :23]):
        with pytest.raises(ValueError):
            device.marker_records(bad)
    with pytest.raises(ValueError):
        device.marker_spectrum_records(raw)


def test_the_host_form_fails_loudly_without_a_device():
    """no handle, no call: pya_marker_spectra_host refuses a NULL handle, and without a device no handle can be made (no CPU
    path)"""
    import torch
    from pyascore_amd import PyAscore, build
    build.build()
    lib = _lib.load()
    x, y, off = np.array([mc.C]), np.array([1.0]), np.array([0, 1], np.int64)
    rec, spec, over = np.zeros(1, ru.MARKER_DTYPE), np.zeros(1, ru.MARKER_SPECTRUM_DTYPE), np.zeros(2, np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)                           # noqa: E731
    t_in = _lib.TypedSpectra(vp(x), vp(y), _lib.PYA_F64, _lib.PYA_F64)
    params = ru.marker_c_params(mc.P_FIXED)
    assert lib.pya_marker_spectra_host(None, C.byref(t_in), vp(off), 1, None, None, C.byref(params), vp(rec), vp(spec), vp(over)) == _lib.PYA_ERR_ARG
    assert lib.pya_marker_spectra(None, C.byref(t_in), vp(off), 1, 1, None, None, C.byref(params), None, vp(rec), vp(spec), vp(over)) == _lib.PYA_ERR_ARG
    assert not rec["flags"].any() and not spec["n_peaks"].any()
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU path"):
            PyAscore(100.0, 10, "STY", 79.966331).marker_spectra(x, y, off, mc.P_FIXED)


def test_score_batch_request_is_checked_before_anything_runs():
    from pyascore_amd.ascore import _markers_request
    p, pm, pz = _markers_request(dict(mz=(126.5,), losses=(18.0,), precursor_mz=[400.0, 500.0], precursor_charge=[2, 300]), 0.05, 2)
    assert p == ru.marker_params(mz=(126.5,), losses=(18.0,), tol=0.05) and pm.dtype == np.float64 and pz.tolist() == [2, 300]
    assert _markers_request(dict(mz=(126.5,), tol=0.01, tol_ppm=5.0), 0.05, 7) == (ru.marker_params(mz=(126.5,), tol=0.01, tol_ppm=5.0), None, None)
    for bad in (True, dict(), dict(mz=(1.0,), window=3), dict(losses=(18.0,)), dict(mz=(1.0,), precursor_mz=[1.0]),
                dict(mz=(1.0,), precursor_mz=[1.0], precursor_charge=[2]), dict(mz=(1.0,), precursor_mz=[1.0, 2.0], precursor_charge=[2.0, 2.0]),
                dict(mz=(1.0,), tol=-1.0), dict(mz=(-1.0,)), dict(mz=1.0), dict(mz=(1.0,) * 65), dict(mz=(1.0,), tol_ppm="x")):
        with pytest.raises(ValueError):
            _markers_request(bad, 0.05, 2)


def test_command_line_options_and_fields():
    from pyascore_amd import batch_cli
    from pyascore_amd.__main__ import markers_request, parse_args
    files = ["spec.mzML", "ident.pepXML", "out.tsv"]
    args = parse_args(files)
    assert (args.markers, args.marker_mz, args.marker_losses, args.marker_tol, args.marker_tol_ppm) == ("", "", "", None, 0.0)
    assert markers_request(args) is None
    args = parse_args(["--markers", "m.tsv", "--marker_mz", "126.1277,127.1248", "--marker_losses", "97.976896", "--marker_tol", "0.003",
                       "--marker_tol_ppm", "10"] + files)
    assert markers_request(args) == dict(mz=(126.1277, 127.1248), losses=(97.976896,), tol=0.003, tol_ppm=10.0)
    assert markers_request(parse_args(["--markers", "m.tsv", "--marker_mz", "216.0426"] + files))["tol"] is None   # (the scorer's mz_error)
    for bad in ([], ["--marker_mz", "126.1,x"], ["--marker_mz", "-1"], ["--marker_losses", "-18.0"], ["--marker_mz", "1", "--marker_tol", "nan"],
                ["--marker_mz", "1", "--marker_tol_ppm", "-1"], ["--marker_mz", ",".join(["100"] * 65)]):
        with pytest.raises(ValueError):
            parse_args(["--markers", "m.tsv"] + bad + files)
        parse_args(bad + files)                                            # (without --markers the values are not looked at)
    parse_args(["--markers", "m.tsv", "--marker_mz", "126.1", "--strip_precursor", "--centroid", "--centroid_gap", "0.01", "--deisotope"] + files)
    out = subprocess.run([sys.executable, "-m", "pyascore_amd", "--help"], cwd=ROOT, capture_output=True, text=True, check=True).stdout
    for opt in ("--markers", "--marker_mz", "--marker_losses", "--marker_tol", "--marker_tol_ppm"):
        assert opt in out
    assert batch_cli.marker_columns((126.5,), (18.0,)) == ("Scan", "TIC", "BasePeak", "mz126.5_Mz", "mz126.5_Intensity", "mz126.5_Peaks",
                                                          "loss18.0_Mz", "loss18.0_Intensity", "loss18.0_Peaks")
    rec, spec = ru.markers(np.array([126.5, 300.0]), np.array([2.5, 1.0]), [0, 2], ru.marker_params(mz=(126.5,), losses=(18.0,), tol=0.01),
                           [400.0], [2])
    assert batch_cli.marker_fields(rec[0], spec[0]) == ["3.5", "2.5", "126.5", "2.5", "1", "", "", "0"]
    with pytest.raises(ValueError):                                        # refused before anything is read: there is no scorer here
        batch_cli.localize(None, [], {}, "STY", 79.9, markers=dict(mz=(-1.0,)), marker_rows=[])
    with pytest.raises(ValueError):
        batch_cli.localize(None, [], {}, "STY", 79.9, markers=dict(mz=(1.0,), precursor_mz=[1.0], precursor_charge=[2]), marker_rows=[])
    with pytest.raises(ValueError):
        batch_cli.localize(None, [], {}, "STY", 79.9, markers=dict(mz=(1.0,)))
    with pytest.raises(TypeError):
        batch_cli.localize(None, [], {}, "STY", 79.9, markers=dict(mz=(1.0,)), marker_rows=[])
