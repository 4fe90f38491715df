"""CPU yardstick for the channel correction (include/pyascore_hip.h: channel correction): apply, sums and factors written for
clarity rather than speed -- Python loops over rows and channels, one float operation per line, Python integers for every sum.
Nothing here needs a device, and nothing is shared with the vectorised ``pyascore_amd.rollup.correct_channels`` /
``channel_sums`` / ``channel_factors``.

A value v is usable when ``v == v and v > 0.0``.  A reading that is not usable is copied, bits and all.  A usable one becomes
the chain ``x = x + m[c][j] * u[j]`` over j ascending from ``x = +0.0`` (u: the row with 0.0 in place of what is not usable),
then ``x * f[c]``, and 0.0 unless the result is a positive number.
"""
import numpy as np

from site_quant_ref import CELL, quantum


def usable(v):
    return v == v and v > 0.0


def apply(values, matrix=None, factor=None):
    """the corrected matrix, float64 ``[n_rows, n_channels]``"""
    values = np.ascontiguousarray(values, np.float64)
    n_rows, n_ch = values.shape
    assert matrix is not None or factor is not None
    m = None if matrix is None else [[float(x) for x in row] for row in np.asarray(matrix, np.float64)]
    f = None if factor is None else [float(x) for x in np.asarray(factor, np.float64)]
    out = values.copy()                                 # (what is not usable stays as it is, bits and all)
    for r in range(n_rows):
        v = [float(x) for x in values[r]]
        u = [x if usable(x) else 0.0 for x in v]
        for c in range(n_ch):
            if not usable(v[c]):
                continue
            if m is not None:
                x = 0.0
                for j in range(n_ch):
                    t = m[c][j] * u[j]
                    x = x + t
            else:
                x = v[c]
            if f is not None:
                x = x * f[c]
            out[r, c] = x if (x == x and x > 0.0) else 0.0
    return out


def sums(values, select=None, scale_log2=10, into=None):
    """the table row CELL[n_channels], or ``into`` (a copy of it) with the rows added"""
    values = np.asarray(values, np.float64)
    n_rows, n_ch = values.shape
    acc = [[0, 0, 0] for _ in range(n_ch)]
    for r in range(n_rows):
        if select is not None and not int(select[r]):
            continue
        for c in range(n_ch):
            v = float(values[r, c])
            if usable(v):
                q, sat = quantum(v, scale_log2)
                acc[c][0] += q
                acc[c][1] += 1
                acc[c][2] += 1 if sat else 0
    cell = np.zeros(n_ch, CELL) if into is None else np.array(into, CELL)
    for c in range(n_ch):
        cell["sum"][c] = (int(cell["sum"][c]) + acc[c][0]) & 0xFFFFFFFFFFFFFFFF
        cell["n"][c] = (int(cell["n"][c]) + acc[c][1]) & 0xFFFFFFFF
        cell["n_saturated"][c] = (int(cell["n_saturated"][c]) + acc[c][2]) & 0xFFFFFFFF
    return cell


def factors(cell):
    """float64 [n_channels]: the largest sum over each sum, 1.0 for an empty column"""
    s = [int(x) for x in cell["sum"]]
    top = float(max(s))                                 # (int -> float rounds to nearest)
    out = np.ones(len(s), np.float64)
    for c, x in enumerate(s):
        if x != 0:
            d = float(x)
            out[c] = top / d
    return out


def special_matrix(rng, n_rows, n_ch):
    """a seeded channel matrix of positive readings with every special value among them"""
    v = rng.uniform(1.0, 1e5, (n_rows, n_ch))
    specials = [float("nan"), 0.0, -0.0, -3.5, float("inf"), 5e-324, 2.5e-310, 1e300, -float("inf")]
    n = n_rows * n_ch
    flat = v.reshape(-1)
    if n:
        at = rng.choice(n, size=min(n, max(len(specials), n // 5)), replace=False)
        for k, i in enumerate(at):
            flat[i] = specials[k % len(specials)]
    return v


def mixing_matrix(rng, n_ch, negative=True):
    """a seeded correction matrix: near the identity, with negative entries off the diagonal as an inverted spill has them"""
    m = np.eye(n_ch) * rng.uniform(1.0, 1.2, n_ch)
    off = rng.uniform(-0.08 if negative else 0.0, 0.01, (n_ch, n_ch))
    off[np.abs(np.subtract.outer(np.arange(n_ch), np.arange(n_ch))) > 2] = 0.0
    np.fill_diagonal(off, 0.0)
    return m + off
