/* span_guard.h -- when the fused score-localize body may COUNT the site-determining ions of a span instead of comparing
 * fragment m/z lists (fused_core.hip.h, `no_cross`).  One restatement for the kernel and for the host
 * (pya_debug_span_guard, host_abi.cpp), in the same float32 / float64 operations, so a test can place a PSM on a chosen side.
 *
 * The question.  The winner W and a single-move competitor C differ in the modification state of two residues p < q (in the
 * direction of travel).  The fused body examines the steps i of the span, the fragments that contain p and not q, in both
 * lists; an ion is site-determining when the OTHER list holds no ion within mz_error of it, at any step j (the pairing of
 * fused_core.hip.h finds every such ion: it probes the neighbours and falls back to a search of the whole list).
 *
 * The argument.  Write a_i(X) for the exact, real-number sum of the float32 residue masses of X's first i + 1 residues, each
 * in X's state (m0 or m1).  For a span step i and any step j of the other list
 *     j = i          a_i(W) - a_i(C) = +-delta(p)                       delta(r) = m1(r) - m0(r)
 *     j > i          a_j(C) - a_i(W) = R -+ delta(p)                    R = C's residues i + 1 .. j, a non-empty run; for j >= q
 *                                                                        the run holds q in C's state, nothing else changes
 *     lo <= j < i    a_i(W) - a_j(C) = R +- delta(p)                    R = W's residues j + 1 .. i
 *     j < lo         a_i(W) - a_j(C) = R                                R = W's residues j + 1 .. i, it holds p
 * and the same with W and C exchanged for the competitor's ions.  So every difference is +-delta, R, or R +- delta with R a
 * non-empty run of residue masses in some state.  With E = mz_error + margin and u = ulp_f32(M) (below), the guard asks:
 *   (a) mod_mass > E, and every modifiable residue's delta, taken from its two floats, lies in [mod_mass - u, mod_mass + u]
 *       (m1 = m0 + mod_mass in float32, and the fixed modifications added to both, round a delta away from mod_mass by a few
 *       ulp of a residue mass: this is CHECKED per residue, not assumed)                      -> delta > E - u, R + delta > E
 *   (b) 2 min(m0, m1) > mod_mass + E for every residue: a run of two or more residues exceeds every delta by more than
 *       E - u; with (a), min(m0, m1) > E                                                       -> R > E, R - delta > E - u
 *   (c) no m0(r), m1(r), r < L, lies inside (mod_mass - E, mod_mass + E): a run of one residue is at least E - u from
 *       every delta.
 * So every exact difference is at least E - u in absolute value.
 *
 * The margin.  The kernel does not compare real sums.  An ion is float32((double)s + A - B + 1.007825), s the float32 running
 * sum: at most L - 1 additions, each off by half an ulp of a value no larger than the largest fragment m/z, then one
 * narrowing, half an ulp again (the float64 steps in between are exact to 2^-29 of that ulp).  Two lists: L ulp together.  The
 * test itself, float32(me - o), is exact when the two are within a factor of two (Sterbenz) and off by half an ulp of the
 * larger otherwise.  That is (L + 1/2) u, with u = ulp_f32(M) and M >= every fragment m/z and running sum of the PSM:
 * M = L x (heaviest residue state, rounded up to an integer) + 32, the 32 covering the ion-type offsets (at most 18.02) and
 * the proton.  margin = (L + 2) u: one u for the deltas of (a), L + 1/2 for the rounding, half a u to spare.  Per PSM: cfg2's
 * 20 residues give 22 x 2^-11 = 0.011, a peptide of 60 residues (fragments above 4096) 62 x 2^-10 = 0.061.
 * With |exact difference| >= mz_error + (L + 1) u and |computed - exact| <= (L + 1/2) u, no computed |me - o| is below
 * mz_error: the pairing would find `total == 0` for every item of every task, count the ion (c_tr) and test its recorded rank
 * against the depth (c_cnt).  Counting without building the lists gives the same integers: bit-identical, not approximately
 * equal.
 * Arithmetic: every comparison is made in float64 on float32 inputs, exactly -- the residue masses are required below 2^20
 * so that the difference of two of them is a float64.
 *
 * What the guard does not cover takes the pairing as before: negative or tiny deltas, a delta equal to a residue mass
 * (114.04293 = N = G + G), a fixed modification that moves a residue onto the delta, mz_error > 0.49, fragment charges
 * above 1 (the caller: another instantiation). */
#ifndef PYA_SPAN_GUARD_H
#define PYA_SPAN_GUARD_H
#include <stdint.h>

#if defined(__HIPCC__)
#define PYA_SPAN_HD __host__ __device__ static inline
#else
#define PYA_SPAN_HD static inline
#endif

struct SpanGuard {
    double E, d_min, d_max;   /* mz_error + margin; the interval every modifiable residue's delta must lie in */
    double mod;               /* mod_mass */
    bool ok;                  /* the conditions that do not depend on a residue */
};

/* heaviest: the largest m0 / m1 of the peptide's L residues (fixed modifications included) */
PYA_SPAN_HD SpanGuard span_guard_make(float mz_error, float mod_mass, int L, float heaviest) {
    SpanGuard g;
    g.ok = heaviest > 0.f && heaviest <= 1048576.f && L >= 1 && L <= 64 && !(mz_error > 0.49f) && mz_error >= 0.f;
    const uint32_t up = g.ok ? (uint32_t)heaviest + 1u : 1u;
    const uint32_t M = (uint32_t)L * up + 32u;                              /* < 2^27 */
    const int e = 31 - __builtin_clz(M);                                    /* 2^e <= M < 2^(e + 1) */
    const double u = __builtin_ldexp(1.0, e - 23);                          /* ulp_f32(M) */
    g.mod = (double)mod_mass;
    g.E = (double)mz_error + (double)(L + 2) * u;
    g.d_min = g.mod - u;
    g.d_max = g.mod + u;
    g.ok = g.ok && g.mod > g.E;
    return g;
}

/* residue r of the peptide, its two states: true when (a), (b) or (c) fails for it */
PYA_SPAN_HD bool span_guard_residue_fails(const SpanGuard &g, float m0, float m1, bool modifiable) {
    const double v0 = (double)m0, v1 = (double)m1, d = v1 - v0, lo = g.mod - g.E, hi = g.mod + g.E;
    const double least = v0 < v1 ? v0 : v1;
    const bool a = !modifiable || (d >= g.d_min && d <= g.d_max);
    const bool b = 2.0 * least > hi;
    const bool c = !(v0 > lo && v0 < hi) && !(v1 > lo && v1 < hi);
    return !(a && b && c);
}

#endif
