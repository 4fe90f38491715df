"""Record arrays for the peptidoform reduce tests, built directly (the reduce takes any records: no scoring is needed).
SIZES straddle the sort's tile (T entries per workgroup and pass) and the levels of its scans: 256 * tiles histogram entries
are two scan levels from the second tile, and the tile totals of the segmented reduction get a second level above 256 tiles."""
import numpy as np

from pyascore_amd import _lib

T = _lib.PYA_PFORM_TILE
DTYPE = np.dtype(_lib.PEPTIDOFORM_DTYPE)
SIZES = (0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1)
BIG = 256 * T + 1
# 258 tiles: 257 whole ones and a tail of 19 entries, so that the last two tile totals of the segmented reduction lie in the second
# block of the level above -- for the kinds whose runs cross tile borders (KINDS_PAST_256_TILES)
PAST_256_TILES = 257 * T + 19
KINDS_PAST_256_TILES = ("runs", "group_ends")
KINDS = ("one_key", "distinct", "sig_top") + tuple("group_byte%d" % b for b in range(4)) + ("group_ends", "runs", "ties", "ascores", "zeros")
SPECIAL_ASCORES = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0xBF800000,
                            0xC2C80000, 0x3F800000, 0x00000001, 0x80000001], np.uint32)       # +-0, +-inf, NaNs, -1, -100, 1, denormals
PROBS = np.array([1.0, 0.999, 0.75, 0.7499999999999999, 0.5, 0.0, 5e-324])


def make(n, kind, seed=0):
    """n records of `kind`"""
    rng = np.random.default_rng([seed, n, KINDS.index(kind)])
    r = np.zeros(n, DTYPE)
    r["n_psm"] = rng.integers(1, 5, n)
    r["n_confident"] = rng.integers(0, 5, n) % (r["n_psm"] + 1)
    r["best_psm"] = rng.integers(0, 1 << 20, n)
    r["best_min_prob"] = rng.choice(PROBS, n)
    r["best_z"] = 1.0 + rng.integers(0, 8, n) / 4.0
    r["best_min_ascore"] = rng.choice(np.array([np.inf, 19.5, 3.25, 0.0, -2.5], np.float32), n)
    r["n_isomers"] = rng.integers(0, 9, n)                    # (ignored and recomputed)
    r["group"] = 5
    r["sig_bits"] = 0x0000010000000003
    if kind == "one_key":
        pass
    elif kind == "distinct":
        r["group"] = rng.permutation(n) // 3
        r["sig_bits"] = (rng.permutation(n).astype(np.uint64) << np.uint64(20)) | np.uint64(1)
    elif kind == "sig_top":                                  # keys that differ only in the top byte of sig_bits
        r["sig_bits"] = np.uint64(0x0000123456789ABC) | (rng.integers(0, 256, n).astype(np.uint64) << np.uint64(56))
    elif kind.startswith("group_byte"):                      # keys that differ only in one byte of group
        b = int(kind[10:])
        v = rng.integers(0, 0x80 if b == 3 else 0x100, n).astype(np.uint32)
        r["group"] = (np.uint32(0x12345678) & np.uint32(~(0xFF << (8 * b)) & 0xFFFFFFFF)) | (v << np.uint32(8 * b))
    elif kind == "group_ends":
        r["group"] = rng.choice(np.array([0, 0x7FFFFFFF], np.uint32), n)
        r["sig_bits"] = rng.choice(np.array([0, 1, 0x8000000000000000, 0xFFFFFFFFFFFFFFFF], np.uint64), n)
    elif kind == "runs":                                     # runs of equal keys that straddle the tile borders, shuffled
        run = np.arange(n) // 700
        r["group"] = run // 2
        r["sig_bits"] = (run % 2 + 1).astype(np.uint64) << np.uint64(33)
        r = r[rng.permutation(n)]
    elif kind == "ties":                                     # equal best_min_prob bits, different ids
        r["group"] = rng.integers(0, 3, n)
        r["best_min_prob"] = 0.75
        r["best_psm"] = rng.permutation(n) + 17
    elif kind == "ascores":
        r["group"] = rng.integers(0, 4, n)
        r["best_min_ascore"] = rng.choice(SPECIAL_ASCORES, n).view(np.float32)
    elif kind == "zeros":                                    # records without PSMs mixed in
        r["group"] = rng.integers(0, 50, n)
        r["sig_bits"] = rng.integers(0, 4, n).astype(np.uint64)
        r["n_psm"][rng.random(n) < 0.4] = 0
    else:
        raise ValueError(kind)
    return r
