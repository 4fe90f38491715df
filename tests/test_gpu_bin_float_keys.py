"""The float keys of the common-case binning bodies (csrc/bin_key.h: window in the exponent, 23 intensity bits in the mantissa,
"more intense" as a clamped float difference) seen through the retained tables: pya_debug_retained_table against the
reference's BinnedSpectra, entry by entry (the machinery of tests/test_gpu_binning_table.py), on spectra aimed at what the
keys changed -- intensities that collide in 23 key bits and differ in 25, equal intensities inside and outside a top n_top, a
later window louder than an earlier one, peaks beyond the keys' 2^32 of dynamic range, 64 and 65 windows, windows longer than
the per-chunk trip counts reach, zeros and denormals.  Every batch runs on the routes tiny, fast, all_pairs, select_forced and
through score(), with float64, float64 + float32 and float32 spectra.  The reference alone says what is right."""
import ctypes as C

import numpy as np
import pytest

import binedges
from pyascore_amd import _lib
from test_gpu_binning_table import _case

pytestmark = pytest.mark.gpu

ROUTES = ("tiny", "fast", "all_pairs", "select_forced")
SETTINGS = binedges._settings(100.0)                        # n_top 10


def _keys(intensity, window=None):
    it = np.ascontiguousarray(intensity, np.float64)
    w = np.zeros(it.size, np.uint32) if window is None else np.ascontiguousarray(window, np.uint32)
    keys, base = np.zeros(it.size, np.uint32), C.c_uint32()
    assert _lib.load().pya_debug_bin_keys(it.ctypes.data, w.ctypes.data, it.size, keys.ctypes.data, C.byref(base)) == 0
    return keys, base.value


def _spectrum(rng, lo, hi, intensity):
    """peaks at sorted random m/z inside (lo, hi), intensities in the given (shuffled) order"""
    mz = np.sort(lo + 1.0 + (hi - lo - 2.0) * rng.random(len(intensity)))
    assert np.all(np.diff(mz) > 0)
    return mz, np.asarray(intensity, np.float64)


def near_ties():
    """one window of 14 peaks, a (1 + j 2^-20): neighbours one or two units of the high word apart.  a = 2^10 (1 + r 2^-20), so
    the most intense peak's high word takes every residue mod 4 as r does, and with it the alignment of the groups of four
    high words that share a 23-bit key"""
    psms, residues = [], set()
    for r in range(4):
        a = 1024.0 * (1.0 + r * 2.0 ** -20)
        ladder = a * (1.0 + np.arange(14) * 2.0 ** -20)
        hw = (ladder.view(np.uint64) >> np.uint64(32)).astype(np.int64)
        assert np.array_equal(np.diff(hw), np.ones(13)), "one high word per step"
        residues.add(int(hw.max() % 4))
        keys, base = _keys(ladder)
        assert np.unique(keys).size < 14, "the ladder collides in 23-bit keys"
        assert np.unique(hw - base).size == 14, "and is distinct in 25-bit keys"
        top = ladder.copy()
        top[8] = top[9]                                       # ranks 4 and 5: two equal intensities inside the top 10
        out = ladder.copy()
        out[1] = out[2]                                       # ranks 11 and 12: outside it
        for k, it in enumerate((ladder, top, out)):
            rng = np.random.default_rng(8100 + 10 * r + k)
            psms.append(binedges.psm(*_spectrum(rng, 400.0, 500.0, rng.permutation(it)), len(psms)))
    assert residues == {0, 1, 2, 3}
    return psms


def louder_later_window():
    """12 peaks near 1, then 30 at 1e6, then 5 at 1e-3 and two (1e-6, 2e-6) more than 2^32 below the loudest: both get key 0,
    inside a window of seven"""
    rng = np.random.default_rng(8200)
    parts = [_spectrum(rng, 400.0, 500.0, 1.0 + 0.1 * rng.random(12)), _spectrum(rng, 500.0, 600.0, 1e6 * (1.0 + 0.1 * rng.random(30))),
             _spectrum(rng, 600.0, 700.0, rng.permutation(np.concatenate([1e-3 * (1.0 + 0.1 * rng.random(5)), [1e-6, 2e-6]])))]
    mz, it = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    keys, _ = _keys(it)
    assert np.all(keys[it < 1e-5] == keys.min()) and keys.min() == _keys([1e6, 0.0])[0][1], "the two faint peaks have key 0"
    assert np.all(keys[(it > 1e-5) & (it < 1.0)] > keys.min())
    return [binedges.psm(mz, it, 0)]


def window_counts():
    """exactly 64 windows of 3 peaks (the most the keys have room for), and 65 (handed over)"""
    psms = []
    for j, n in enumerate((64, 65)):
        rng = np.random.default_rng(8300 + n)
        parts = [_spectrum(rng, 400.0 + 100.0 * w, 500.0 + 100.0 * w, 10.0 ** rng.uniform(0, 5, 3)) for w in range(n)]
        mz = np.concatenate([p[0] for p in parts])
        assert binedges.n_bins_float(np.ceil(mz.max() / 100) * 100 - 400, 100.0) == n
        psms.append(binedges.psm(mz, np.concatenate([p[1] for p in parts]), j))
    return psms


def long_windows():
    """one window of 200 peaks; one of 1 000, beyond the 960 peaks up to which every chunk has a trip count of its own"""
    psms = []
    for j, n in enumerate((200, 1000)):
        rng = np.random.default_rng(8400 + n)
        psms.append(binedges.psm(*_spectrum(rng, 400.0, 500.0, 10.0 ** rng.uniform(0, 6, n)), j))
    return psms


def small_intensities():
    """0.0, 5e-324 and 1e-310 among normal values: retained in a window of eight, dropped from a window of fourteen (as float32
    the three are equal)"""
    rng = np.random.default_rng(8500)
    tiny = [0.0, 5e-324, 1e-310]
    parts = [_spectrum(rng, 400.0, 500.0, rng.permutation(np.concatenate([tiny, 50.0 + 100.0 * rng.random(5)]))),
             _spectrum(rng, 500.0, 600.0, rng.permutation(np.concatenate([tiny, 1e-3 * (1.0 + rng.random(11))])))]
    return [binedges.psm(np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), 0)]


FAMILIES = {"near_ties": near_ties, "louder_later_window": louder_later_window, "window_counts": window_counts,
            "long_windows": long_windows, "small_intensities": small_intensities}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_tables_of_float_keys_equal_the_reference(family, monkeypatch):
    _case(monkeypatch, "float_keys/" + family, SETTINGS, FAMILIES[family](), family, routes=ROUTES)
