"""A plain-Python yardstick of the precursor-XIC rule (include/pyascore_hip.h: pya_xic_params): loops over Python floats, no
numpy arithmetic and no code shared with pyascore_amd.rollup.xic.  It is written the other way round where the rule allows
it: the trace walks every peak, the region grows scan by scan from a list of absent runs, the valleys are found by testing
every scan against the definition, the peak is cut afterwards.

    records, over = xic(scans, rt, queries, params)

``scans``: a list of lists of (x, y) Python floats (float32 inputs are widened by the caller: float(np.float32) is exact);
``rt``: a list of floats; ``queries``: a list of (seed, scan_lo, scan_hi, prec_mz, prec_z); ``params``: a dict with tol, tol_ppm,
step, rise, isotopes, max_gap.  ``records``: a list of 12-tuples in the field order of pya_xic; ``over``: (count, first | None)."""
import math

MAX_SCANS, MAX_CHARGE = 64, 8
ACTIVE, SEEN, SEED_PRESENT, LEFT_VALLEY, RIGHT_VALLEY, UNSORTED, LEFT_OPEN, RIGHT_OPEN = 1, 2, 4, 8, 16, 32, 64, 128
ZERO = (0.0, 0.0, 0.0, 0.0, 0, 0, 0, 0, 0, 0, 0, 0)


def ascending(scan):
    for j in range(len(scan) - 1):
        if not scan[j][0] <= scan[j + 1][0]:
            return False
    return True


def _trace_point(scan, lo, hi):
    best = 0.0
    for x, y in scan:
        if lo <= x and x <= hi and y > 0.0 and y > best:
            best = y
    return best


def _one(scans, rt, query, prm):
    """(record, out_of_range)"""
    seed, s_lo, s_hi, pm, pz = query
    if seed < 0:
        return ZERO, False
    if not (0 <= s_lo and s_lo <= seed and seed < s_hi and s_hi <= len(scans) and s_hi - s_lo <= MAX_SCANS):
        return ZERO, True
    if not (1 <= pz <= MAX_CHARGE and not math.isnan(pm) and not math.isinf(pm) and pm > 0.0):
        return ZERO, False
    window = list(range(s_lo, s_hi))
    flags = ACTIVE
    d = prm["step"] / float(pz)
    p = {}
    for s in window:
        good = ascending(scans[s])
        if not good:
            flags |= UNSORTED
        for i in range(prm["isotopes"] + 1):
            c = pm + float(i) * d
            w = prm["tol"] + (prm["tol_ppm"] * 1e-6) * c
            p[s, i] = _trace_point(scans[s], c - w, c + w) if good else 0.0
    present = {s: p[s, 0] > 0.0 for s in window}
    t = {}
    for s in window:
        t[s] = 0.0
        if present[s]:
            acc = p[s, 0]
            for i in range(1, prm["isotopes"] + 1):
                acc = acc + p[s, i]
            t[s] = acc
    n_present = len([s for s in window if present[s]])
    # start: candidates by (distance, scan), the nearest, the earlier on a tie
    near = sorted((abs(s - seed), s) for s in window if present[s] and abs(s - seed) <= prm["max_gap"] + 1)
    if not near:
        return (0.0, 0.0, 0.0, 0.0, 0, 0, 0, 0, 0, n_present, 0, flags), False
    a0 = near[0][1]
    # region: every interval [l, h] around a0 with present ends and no long absent run; the largest
    def allowed(l, h):
        if not (present[l] and present[h]):
            return False
        run = 0
        for s in range(l, h + 1):
            run = 0 if present[s] else run + 1
            if run > prm["max_gap"]:
                return False
        return True
    r_lo = min(l for l in range(s_lo, a0 + 1) if allowed(l, a0))
    r_hi = max(h for h in range(a0, s_hi) if allowed(a0, h))
    region = [s for s in range(r_lo, r_hi + 1) if present[s]]

    def is_valley(v):
        step = 1 if v > a0 else -1
        beyond = [s for s in region if (s - v) * step > 0]
        if not beyond:
            return False
        nxt = min(beyond, key=lambda s: abs(s - v))
        between = [s for s in region if min(a0, v) <= s <= max(a0, v)]
        big_l = max(t[s] for s in between)
        big_f = max(t[s] for s in beyond)
        low = prm["rise"] * t[v]
        return t[v] <= t[nxt] and low < big_l and low < big_f

    right = [v for v in region if v > a0 and is_valley(v)]
    left = [v for v in region if v < a0 and is_valley(v)]
    e_r = min(right) if right else r_hi
    e_l = max(left) if left else r_lo
    peak = [s for s in region if e_l <= s <= e_r]
    apex = peak[0]
    for s in peak[1:]:
        if t[s] > t[apex]:
            apex = s
    total, area = 0.0, 0.0
    for s in peak:
        total = total + t[s]
    for u, v in zip(peak[:-1], peak[1:]):
        area = area + (0.5 * (t[u] + t[v])) * (rt[v] - rt[u])
    flags |= SEEN
    if a0 == seed:
        flags |= SEED_PRESENT
    if left:
        flags |= LEFT_VALLEY
    elif e_l == s_lo:
        flags |= LEFT_OPEN
    if right:
        flags |= RIGHT_VALLEY
    elif e_r == s_hi - 1:
        flags |= RIGHT_OPEN
    iso_hit = 0
    for i in range(prm["isotopes"] + 1):
        if p[apex, i] > 0.0:
            iso_hit |= 1 << i
    return (area, t[apex], t[seed], total, apex, e_l, e_r, a0, len(peak), n_present, iso_hit, flags), False


def xic(scans, rt, queries, params):
    records, outside = [], []
    for q, query in enumerate(queries):
        rec, out = _one(scans, rt, query, params)
        records.append(rec)
        if out:
            outside.append(q)
    return records, (len(outside), outside[0] if outside else None)
