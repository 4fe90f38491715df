"""The yardstick of the precursor-purity stage: THE RULE of pya_purity_params (include/pyascore_hip.h) in plain Python -- loops
over lists of floats, one operation per line where the header has one, no numpy arithmetic.  Python's float is IEEE double and
every operation below rounds once, as the header asks.  tests/purity_cases.py pins it by hand; pyascore_amd.rollup.purity and
the kernel are compared with it byte for byte."""
import math
import struct

MAX_CHARGE = 8                      # PYA_STRIP_MAX_CHARGE
ACTIVE, SEEN = 1, 2
NO_READING = 0x7FF8000000000000     # the NaN pya_marker_values writes
ZERO = (0.0, 0.0, 0.0, 0.0, 0, 0, 0, 0)
RECORD = struct.Struct("<ddddIIII")


def centres(prec_mz, prec_z, params):
    """[(lo_i, hi_i)] for i = -below .. isotopes"""
    d = params["step"] / float(prec_z)
    ppm = params["tol_ppm"] * 1e-6
    out = []
    for i in range(-params["below"], params["isotopes"] + 1):
        c = prec_mz + float(i) * d
        w = params["tol"] + ppm * c
        out.append((c - w, c + w))
    return out


def one(peaks, prec_mz, prec_z, win_lo, win_hi, params):
    """the record of an ACTIVE query over ``peaks`` = [(x, y)] in index order"""
    bounds = centres(prec_mz, prec_z, params)
    window = 0.0
    precursor = 0.0
    n_window = n_precursor = iso_hit = 0
    other = None
    for x, y in peaks:
        inside = win_lo <= x and x <= win_hi
        eligible = inside and y > 0.0
        if not eligible:
            continue
        window = window + y
        n_window += 1
        hit = 0
        for k, (lo, hi) in enumerate(bounds):
            if lo <= x and x <= hi:
                hit |= 1 << k
        if hit:
            precursor = precursor + y
            n_precursor += 1
            iso_hit |= hit
        elif other is None or y > other[1] or (y == other[1] and x < other[0]):
            other = (x, y)
    other_mz, other_intensity = (0.0, 0.0) if other is None else (other[0] + 0.0, other[1] + 0.0)
    return (window, precursor, other_mz, other_intensity, n_window, n_precursor, iso_hit, ACTIVE | (SEEN if n_precursor else 0))


def is_active(survey, prec_mz, prec_z, win_lo, win_hi):
    if survey < 0:
        return False
    if not (1 <= prec_z <= MAX_CHARGE and math.isfinite(prec_mz) and prec_mz > 0.0):
        return False
    return win_lo <= win_hi and math.isfinite(win_lo) and math.isfinite(win_hi)


def purity(spectra, queries, params):
    """``spectra``: [[(x, y), ...]] the survey spectra; ``queries``: [(survey, prec_mz, prec_z, win_lo, win_hi)].  Returns
    (records, (count, first)): one 8-tuple in the field order of pya_purity per query, and the queries whose survey lies beyond
    the spectra."""
    records, beyond = [], []
    for q, (survey, prec_mz, prec_z, win_lo, win_hi) in enumerate(queries):
        if not is_active(survey, prec_mz, prec_z, win_lo, win_hi):
            records.append(ZERO)
        elif survey >= len(spectra):
            records.append(ZERO)
            beyond.append(q)
        else:
            records.append(one(spectra[survey], prec_mz, prec_z, win_lo, win_hi, params))
    return records, (len(beyond), beyond[0] if beyond else None)


def to_bytes(records):
    return b"".join(RECORD.pack(*r) for r in records)


def ratio(record):
    return record[1] / record[0] if record[0] > 0.0 else float("nan")


def gate(records, threshold, keep_unknown, rows=None):
    """``rows``: the matrix as lists of 64-bit patterns, or None.  Returns (select, rows)"""
    select, out = [], []
    for r, rec in enumerate(records):
        known = bool(rec[7] & ACTIVE) and rec[0] > 0.0
        if known:
            passes = rec[1] >= threshold * rec[0]
        else:
            passes = bool(keep_unknown)
        select.append(1 if passes else 0)
        if rows is not None:
            out.append(list(rows[r]) if passes else [NO_READING] * len(rows[r]))
    return select, (out if rows is not None else None)
