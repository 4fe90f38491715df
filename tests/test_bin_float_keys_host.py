"""The composite keys of the common-case binning bodies (csrc/bin_key.h), through their host restatement pya_debug_bin_keys:
a float32 with the window in its exponent and 23 intensity bits in its mantissa.  What the kernels lean on is checked here in
numpy's float32 arithmetic (IEEE round-to-nearest, as v_sub_f32 / v_pk_add_f32 compute):
  - read as integers the keys order like (window descending, then intensity);
  - within a window clip(o - me, 0, 1) is exactly 1.0 when o's key is larger and 0.0 otherwise;
  - it is 0.0 for every key of a later window and for the zero padding;
  - the extremes of the fields, and the key base for every residue mod 4 of the most intense peak's high word.
No device is needed."""
import ctypes as C

import numpy as np
import pytest

from pyascore_amd import _lib

EXP0, WINDOWS, BITS, RANGE = 150, 64, 23, (1 << 25) - 1


def keys_of(intensity, window):
    it, w = np.ascontiguousarray(intensity, np.float64), np.ascontiguousarray(window, np.uint32)
    keys, base = np.zeros(it.size, np.uint32), C.c_uint32()
    rc = _lib.load().pya_debug_bin_keys(it.ctypes.data, w.ctypes.data, it.size, keys.ctypes.data, C.byref(base))
    assert rc == 0
    return keys, base.value


def high_words(intensity):
    return (np.ascontiguousarray(intensity, np.float64).view(np.uint64) >> np.uint64(32)).astype(np.int64)


def from_high_words(hw):
    return (np.asarray(hw, np.uint64) << np.uint64(32)).view(np.float64)


def expected_keys(intensity, window):
    """the definition, restated: base = max high word - (2^25 - 1) or 0; k23 = (max(hw, base) - base) >> 2"""
    hw = high_words(intensity)
    base = max(int(hw.max()) - RANGE, 0)
    k = (np.maximum(hw, base) - base) >> 2
    return (((EXP0 + WINDOWS - 1 - np.asarray(window, np.int64)) << BITS) | k).astype(np.uint32), base


def count(o, me):
    """the rank count's term: clamp(o - me) in float32"""
    with np.errstate(all="raise"):
        d = o.view(np.float32) - me.view(np.float32)
    assert d.dtype == np.float32
    return np.clip(d, np.float32(0), np.float32(1))


def spectra():
    """(intensity, window) arrays: random magnitudes over 40 binades, ladders one high word apart, equal values, the ends"""
    rng = np.random.default_rng(2301)
    out = []
    for n in (1, 2, 50, 4000):
        out.append((2.0 ** rng.uniform(-20, 20, n) * (1 + rng.random(n)), rng.integers(0, WINDOWS, n)))
    top = int(high_words([3.7e4])[0])
    for r in range(4):                                        # ladders of neighbouring high words, every alignment of the base
        hw = np.concatenate([top + r - np.arange(300), [top + r - RANGE - 2, top + r - RANGE, top + r - RANGE + 3, top + r - RANGE + 4]])
        for w in (np.zeros(hw.size, int), rng.integers(0, WINDOWS, hw.size), np.full(hw.size, 63)):
            out.append((from_high_words(hw), w))
    out.append((np.asarray([5.0, 5.0, 0.0, 5e-324, 1e-310, 5.0 * (1 + 2.0 ** -52), 1e300, 1e300]), np.asarray([0, 0, 0, 0, 63, 63, 5, 63])))
    out.append((np.zeros(7), np.arange(7)))                   # (a spectrum of zeros: base 0, every key 0)
    return out


@pytest.mark.parametrize("case", range(len(spectra())))
def test_keys_are_the_definition_and_order_like_window_then_intensity(case):
    it, w = spectra()[case]
    keys, base = keys_of(it, w)
    want, want_base = expected_keys(it, w)
    assert base == want_base and np.array_equal(keys, want)
    # fields back out of the bits
    assert np.array_equal(EXP0 + WINDOWS - 1 - (keys >> BITS), w)
    k = (keys & ((1 << BITS) - 1)).astype(np.int64)
    # integer order of the bits = (window descending, then intensity field); the field is monotone in the intensity
    a, b = np.meshgrid(np.arange(it.size)[:400], np.arange(it.size)[-400:], indexing="ij")
    wa, wb, ka, kb = w[a].astype(np.int64), w[b].astype(np.int64), k[a], k[b]
    assert np.array_equal(keys[a] > keys[b], (wa < wb) | ((wa == wb) & (ka > kb)))
    assert np.all(ka[it[a] >= it[b]] >= kb[it[a] >= it[b]])
    # every key is a finite positive float of at least 2^23: one mantissa step is at least 1.0
    f = keys.view(np.float32)
    assert np.all(np.isfinite(f)) and np.all(f >= 2.0 ** 23) and np.all(np.spacing(f) >= 1.0)


@pytest.mark.parametrize("case", range(len(spectra())))
def test_clamped_difference_is_the_integer_compare(case):
    it, w = spectra()[case]
    keys, _ = keys_of(it, w)
    a, b = np.meshgrid(np.arange(it.size)[:600], np.arange(it.size)[-600:], indexing="ij")
    o, me = keys[a], keys[b]
    c = count(o, me)
    same = w[a] == w[b]
    assert np.array_equal(c[same], (o[same] > me[same]).astype(np.float32)), "within a window: exactly the integer compare"
    later = w[a] > w[b]
    assert np.all(c[later] == 0), "a key of a later window never counts"
    assert np.all(count(np.zeros_like(me), me) == 0), "the zero padding never counts"


def test_adversarial_pairs_in_every_window():
    """keys one step apart, equal keys, and the two ends of the mantissa, in every window: built from bits"""
    k = np.asarray([0, 1, 2, 3, (1 << 22) - 1, 1 << 22, (1 << 22) + 1, (1 << BITS) - 2, (1 << BITS) - 1], np.uint32)
    for w in range(WINDOWS):
        keys = (np.uint32(EXP0 + WINDOWS - 1 - w) << np.uint32(BITS)) | k
        o, me = np.meshgrid(keys, keys, indexing="ij")
        assert np.array_equal(count(o, me), (o > me).astype(np.float32)), w
        if w + 1 < WINDOWS:
            nxt = (np.uint32(EXP0 + WINDOWS - 2 - w) << np.uint32(BITS)) | k
            o, me = np.meshgrid(nxt, keys, indexing="ij")
            assert np.all(count(o, me) == 0), w
    # counts add up exactly in float32 far beyond any window length
    assert np.float32(2 ** 24 - 1) + np.float32(1) == np.float32(2 ** 24)


def test_extremes_of_the_fields_and_every_residue_of_the_key_base():
    top = int(high_words([1.0e6])[0]) & ~3
    for r in range(4):
        hw = np.asarray([top + r, top + r - 1, top + r - 4, top + r - RANGE + 3, top + r - RANGE, top + r - RANGE - 1, 0], np.int64)
        for w in (0, 63):
            keys, base = keys_of(from_high_words(hw), np.full(hw.size, w))
            assert base == top + r - RANGE and base % 4 == (r + 1) % 4
            k = keys & ((1 << BITS) - 1)
            # the loudest and the high word below it share the largest field; four below it is the next one; three above the
            # base, the base, below it and zero all have field 0
            assert list(k) == [(1 << BITS) - 1, (1 << BITS) - 1, (1 << BITS) - 2, 0, 0, 0, 0]
            assert np.all(keys >> BITS == EXP0 + WINDOWS - 1 - w)
    # the key keeps the upper 23 of the 25 bits: the bucket bits of the selection route are the same six
    hw = top - np.arange(0, RANGE, 997)
    keys, base = keys_of(from_high_words(hw), np.zeros(hw.size, int))
    assert np.array_equal((keys & ((1 << BITS) - 1)) >> 17, (hw - base) >> 19)


def test_refuses_what_no_fast_path_sees():
    lib = _lib.load()
    it, w, k = np.asarray([1.0, 2.0]), np.asarray([0, 1], np.uint32), np.zeros(2, np.uint32)
    call = lambda it, w, n: lib.pya_debug_bin_keys(it.ctypes.data, w.ctypes.data, n, k.ctypes.data, None)
    assert call(it, w, 2) == 0
    assert call(it, w, 0) == -1
    assert call(it, np.asarray([0, 64], np.uint32), 2) == -1
    for bad in (-1.0, -0.0, np.inf, np.nan):
        assert call(np.asarray([1.0, bad]), w, 2) == -1
    assert lib.pya_debug_bin_keys(None, w.ctypes.data, 2, k.ctypes.data, None) == -1
