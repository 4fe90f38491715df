"""Roll-up tables for the site FLR tests, built directly as records (the stage takes any table: no scoring is needed).
SIZES straddle the sort's tile (T slots per workgroup and pass) and the levels of its scans: 256 * tiles histogram entries
are one scan level for one tile, two from the second tile and three from the 257th (about 300 tiles)."""
import math

import numpy as np

from pyascore_amd import _lib

T = _lib.PYA_FLR_TILE
TABLE_DTYPE = np.dtype(_lib.ROLLUP_DTYPE)
SIZES = (0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, 300 * T + 37)
KINDS = ("same", "distinct", "eight") + tuple("byte%d" % b for b in range(8)) + ("special", "third_empty", "reported")
HALF = 0x3FE0000000000000            # the bits of 0.5


def _classes(rng, n):
    return rng.choice(np.array([0, 0, 0, 1, 2], np.uint8), n)


def make(n, kind, seed=0):
    """(table, cls or None, reported_only) of `kind` with n slots"""
    rng = np.random.default_rng([seed, n, KINDS.index(kind)])
    t = np.zeros(n, TABLE_DTYPE)
    t["best_psm"] = rng.integers(0, 1000, n)
    t["n_psm"] = rng.integers(1, 5, n)
    t["n_in_best"] = 1
    cls, reported_only = None, False
    if kind == "same":                                       # one tie group
        t["best_prob"] = 0.75
    elif kind in ("distinct", "third_empty"):
        t["best_prob"] = (rng.permutation(n) + 1.0) / (n + 2.0)
        if kind == "distinct":
            cls = _classes(rng, n)
        else:
            t["n_psm"][::3] = 0                              # (an empty slot keeps whatever best_prob says: it is not ranked)
    elif kind in ("eight", "reported"):                      # long tie groups that straddle tile borders
        t["best_prob"] = rng.choice(np.array([1.0, 0.999, 0.99, 0.9, 0.75, 0.5, 0.1, 0.0]), n)
        cls = _classes(rng, n)
        if kind == "eight":
            t["n_psm"][::3] = 0
        else:
            t["n_in_best"] = rng.integers(0, 2, n)
            reported_only = True
    elif kind.startswith("byte"):                            # bit patterns that differ in exactly one byte: one digit decides
        b = int(kind[4:])
        v = rng.integers(0, 0x40 if b == 7 else 0x100, n).astype(np.uint64)      # (byte 7: sign clear, exponent below 2^0)
        mask = np.uint64(~(0xFF << (8 * b)) & 0xFFFFFFFFFFFFFFFF)
        t["best_prob"] = ((np.uint64(HALF) & mask) | (v << np.uint64(8 * b))).view(np.float64)
        cls = _classes(rng, n) if b % 2 else None
    elif kind == "special":
        t["best_prob"] = rng.choice(np.array([0.0, 1.0, 5e-324, math.nextafter(1.0, 0.0), 0.5, 2.0 ** -1022, 1.0000000000000002]), n)
        cls = _classes(rng, n)
    else:
        raise ValueError(kind)
    return t, cls, reported_only
