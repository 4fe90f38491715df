"""The spectrum families of tests/binedges.py on the CPU: the reference's own BinnedSpectra (oracle/_ref) against the two
CPU copies of its window arithmetic -- oracle/ascore_oracle.cpp and PyBinnedSpectra (csrc/aux_api.cpp) -- window by window:
bounds, window count, every retained peak's window and rank.  It also pins the families themselves: they hold the edge
they claim to hold (a float window count one below the exact one with peaks in the stretch that is cut off, extremes on
multiples of 100, peaks on both sides of every border), so that tests/test_gpu_binning_table.py, which runs the same
spectra through the kernels, is aimed at what it says."""
import ctypes as C

import numpy as np
import pytest

import binedges
from oracle import orc
from pyascore_amd import _lib

ALL = list(binedges.FAMILIES) + ["window_counts_large", "too_many_windows"]


def _need_ref():
    if not orc.available("ref"):
        pytest.fail("oracle/_ref/libascore_ref.so is missing: build it with `make -C oracle ref`", pytrace=False)


def _aux_binned(settings, mz, intensity):
    """PyBinnedSpectra's windows through the C ABI of include/pyascore_aux.h, in orc_binned's form"""
    lib = _lib.load()
    s = C.c_void_p(lib.pya_spectra_create(settings["bin_size"], settings["n_top"]))
    try:
        mz, intensity = np.ascontiguousarray(mz, np.float64), np.ascontiguousarray(intensity, np.float64)
        rc = lib.pya_spectra_consume(s, mz.ctypes.data, intensity.ctypes.data, mz.size)
        if rc:
            return None
        lo, hi, bs = C.c_float(), C.c_float(), C.c_float()
        nb, nt = C.c_uint64(), C.c_uint64()
        lib.pya_spectra_info(s, C.byref(lo), C.byref(hi), C.byref(bs), C.byref(nb), C.byref(nt))
        out = dict(mz=[], intensity=[], bin=[], rank=[], min_mz=lo.value, max_mz=hi.value, n_bins=nb.value)
        m, t = C.c_double(), C.c_double()
        for w in range(nb.value):
            for r in range(lib.pya_spectra_window_size(s, w)):
                assert lib.pya_spectra_peak(s, w, r, C.byref(m), C.byref(t)) == 0
                out["mz"].append(m.value); out["intensity"].append(t.value); out["bin"].append(w); out["rank"].append(r)
        return out
    finally:
        lib.pya_spectra_destroy(s)


def _same_binned(got, want, what):
    for key in ("min_mz", "max_mz", "n_bins"):
        assert got[key] == want[key], "%s: %s is %r, the reference has %r" % (what, key, got[key], want[key])
    for key in ("bin", "rank", "mz", "intensity"):
        assert np.array_equal(np.asarray(got[key], np.float64), np.asarray(want[key], np.float64)), "%s: %s differs" % (what, key)


@pytest.mark.parametrize("family", ALL)
def test_cpu_copies_bin_like_the_reference(family):
    _need_ref()
    n = 0
    for cid, settings, psms, note in binedges.cases(family):
        for i, p in enumerate(psms):
            what = "%s PSM %d (%s)" % (cid, i, note)
            assert binedges.expected_status(settings, p["mz"]) == p.get("expect_status", 0), what
            if p.get("expect_status") == 1:                  # (the reference writes out of bounds here: nobody asks it)
                assert _aux_binned(settings, p["mz"], p["intensity"]) is None, what
                with pytest.raises(RuntimeError):
                    binedges.reference_binned(settings, p["mz"], p["intensity"], kind="oracle")
                continue
            want = binedges.reference_binned(settings, p["mz"], p["intensity"], kind="ref")
            assert len(want["mz"]) > 0 and np.all(want["rank"] < settings["n_top"]), what
            _same_binned(binedges.reference_binned(settings, p["mz"], p["intensity"], kind="oracle"), want, what + " / oracle port")
            _same_binned(_aux_binned(settings, p["mz"], p["intensity"]), want, what + " / PyBinnedSpectra")
            n += 1
    assert n >= 8 or family == "too_many_windows"


def _ref(settings, p):
    return binedges.reference_binned(settings, p["mz"], p["intensity"], kind="ref")


def test_float_window_count_cuts_the_top_of_the_span_off():
    """bin_size float32(100 / 3) over a span of 100: three windows in float where the exact quotient gives four, and the peaks
    of the last 1e-6 of the span sit in window 2; likewise float32(0.7) over 700 (1 000, not 1 001) and every searched pair."""
    _need_ref()
    assert binedges.n_bins_float(100, np.float32(100 / 3)) == 3 and binedges.n_bins_exact(100, np.float32(100 / 3)) == 4
    assert binedges.n_bins_float(700, np.float32(0.7)) == 1000 and binedges.n_bins_exact(700, np.float32(0.7)) == 1001
    assert list(binedges.NBINS_PAIRS_SMALL) == binedges.search_nbins_pairs(2, 64)
    assert list(binedges.NBINS_PAIRS_LARGE) == binedges.search_nbins_pairs(65, 400)
    cut, hit, short = 0, set(), set()
    for cid, settings, psms, note in binedges.cases("bin_sizes"):
        bsd = settings["bin_size"]
        for p in psms:
            b = _ref(settings, p)
            span = b["max_mz"] - b["min_mz"]
            assert b["n_bins"] == binedges.n_bins_float(span, bsd), note
            if b["n_bins"] == binedges.n_bins_exact(span, bsd):
                continue
            assert b["n_bins"] + 1 == binedges.n_bins_exact(span, bsd), note
            short.add(cid)
            # raw peaks beyond the last float border exist, the reference has them in its last window, and a table built with
            # the exact window count (the stretch a window of its own) would hold other peaks
            beyond = p["mz"] >= b["min_mz"] + b["n_bins"] * bsd
            if beyond.sum() < 3:      # (the variant whose highest peak is a few m/z inside; a stretch narrower than a float32 ulp)
                continue
            cut += 1
            hit.add(cid)
            w = np.minimum(np.floor((p["mz"] - b["min_mz"]) / bsd), b["n_bins"]).astype(int)
            other = []
            for k in np.unique(w):
                sel = np.flatnonzero(w == k)
                other.extend(p["mz"][sel[np.argsort(-p["intensity"][sel], kind="stable")[:settings["n_top"]]]])
            assert sorted(other) != sorted(b["mz"]), note
    assert not (short - hit) and len(hit) >= len(binedges.NBINS_PAIRS_SMALL) + len(binedges.NBINS_PAIRS_LARGE) + 4 and cut >= 2 * len(hit)
    s33 = [c for c in binedges.cases("bin_sizes") if c[1]["bin_size"] == binedges.f32(np.float32(100 / 3)) and "[400, 500]" in c[3]]
    assert s33 and all(_ref(s33[0][1], p)["n_bins"] == 3 for p in s33[0][2])


def test_families_hold_their_edges():
    _need_ref()
    # borders: the bounds are the intended ones, both neighbours of a border are populated beyond n_top, and a peak sits on
    # the border, below it and above it
    for cid, settings, psms, note in binedges.cases("borders"):
        lo, hi = [float(v) for v in note[note.index("[") + 1: note.index("]")].split(",")]
        bsd = settings["bin_size"]
        for p in psms:
            b = _ref(settings, p)
            assert (b["min_mz"], b["max_mz"]) == (lo, hi), note
            assert p["mz"][0] == lo and p["mz"][-1] == hi, note        # (the highest peak's quotient equals n_bins: clamped)
            raw = np.minimum(np.floor((p["mz"] - lo) / bsd), b["n_bins"] - 1)
            assert np.all(np.bincount(raw.astype(int), minlength=b["n_bins"]) > settings["n_top"]), note
            for k in range(1, b["n_bins"]):
                c = lo + k * bsd
                near = p["mz"][np.abs(p["mz"] - c) < 1e-3 * bsd]
                assert (near < c).any() and (near >= c).any(), (note, k)
            assert len(np.unique(b["bin"])) == b["n_bins"]
    # extremes: one ulp below a multiple of 100 opens a window of its own below, one ulp above the top one above
    cid, settings, psms, note = binedges.cases("extremes")[0]
    bounds = {(_ref(settings, p)["min_mz"], _ref(settings, p)["max_mz"]) for p in psms}
    assert bounds == {(400.0, 1200.0), (300.0, 1200.0), (400.0, 1300.0), (300.0, 1300.0)}
    assert any(p["mz"][0] == binedges.step(400.0, 1) for p in psms) and any(p["mz"][-1] == binedges.step(1200.0, -1) for p in psms)
    assert any(p["mz"][0] == binedges.step(400.0, 1, True) for p in psms)
    # window counts: the counts asked for, the fast kernels' 64 and the 16-bit limit among them
    small = {_ref(s, p)["n_bins"] for _, s, ps, _ in binedges.cases("window_counts") for p in ps}
    assert {1, 2, 63, 64, 65, 255, 256, 257} <= small
    large = {_ref(s, p)["n_bins"] for _, s, ps, _ in binedges.cases("window_counts_large") for p in ps}
    assert {4096, 65534, 65535} <= large and max(large) == 65535 and min(large) >= 4096
    for _, s, ps, _ in binedges.cases("too_many_windows"):
        assert [p.get("expect_status", 0) for p in ps] == [0, 2, 0]
        assert _ref(s, ps[1])["n_bins"] > 65535 and all(_ref(s, ps[i])["n_bins"] <= 65535 for i in (0, 2))
    # order: the ends of the third arrangement are in order and are not the extremes; the bounds come from the extremes
    for _, s, ps, _ in binedges.cases("order"):
        for p in ps:
            assert (_ref(s, p)["min_mz"], _ref(s, p)["max_mz"]) == (300.0, 1300.0)
        for p in (ps[2], ps[6]):
            m = p["mz"]
            assert m[0] < m[-1] and m[0] > m.min() and m[-1] < m.max() and np.floor(m[0] / 100) != np.floor(m.min() / 100)
        assert np.all(np.diff(ps[0]["mz"]) >= 0) and np.all(np.diff(ps[1]["mz"]) <= 0) and np.any(np.diff(ps[3]["mz"]) < 0)
        assert len(np.unique(ps[4]["intensity"])) <= 3 < len(np.unique(ps[0]["intensity"]))
