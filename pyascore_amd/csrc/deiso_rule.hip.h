/* deiso_rule.hip.h -- what deisotope.hip and decharge.hip share: the relation R of THE RULE (include/pyascore_hip.h:
 * pya_deisotope_params) as the walk that decides whether a peak is removed, the clipping of a spectrum's offsets, and the launch
 * shape (one wavefront per spectrum, four per workgroup, a capped grid). */
#pragma once
#include "device_common.hip.h"
#include "../../include/pyascore_hip.h"

#define DEISO_WAVES 4
#define DEISO_MAX_BLOCKS 2048u

/* the capped grid that strides over n_spectra spectra, DEISO_WAVES of them per workgroup */
static inline uint32_t deiso_blocks(uint64_t n_spectra) {
    const uint64_t want = (n_spectra + DEISO_WAVES - 1) / DEISO_WAVES;
    return (uint32_t)(want < DEISO_MAX_BLOCKS ? want : DEISO_MAX_BLOCKS);
}

DEV double deiso_widen(double x) { return x; }
DEV double deiso_widen(float x) { return (double)x; }

/* whether peak j (m/z xj, intensity yj) of the spectrum that starts at p0 has a parent: the rule, operation for operation.  The
 * candidates of every charge lie in one window below j: the walk goes down from j - 1 and ends at the first i whose
 * e = (xj - x[i]) - spacing[0] exceeds tol -- e rises as i falls, and the e of a higher charge (a smaller spacing) is no smaller,
 * rounding included, so nothing below that i can match at any charge.  The exact predicate decides; there is no slack term. */
template <typename TM, typename TI>
DEV bool deiso_removed(const TM *mz, const TI *in, int64_t p0, int64_t j, double xj, double yj, const pya_deisotope_params &prm) {
    for (int64_t i = j - 1; i >= p0; i--) {
        const double xi = deiso_widen(mz[i]);
        const double d = xj - xi;
        const double e0 = d - prm.spacing[0];
        if (e0 > prm.tol) break;
        for (uint32_t z = 1; z <= prm.max_charge; z++) {
            const double e = d - prm.spacing[z - 1];
            if (__builtin_fabs(e) <= prm.tol) {
                const double m = xi * (double)z;
                const double b = prm.ratio0 + prm.ratio_per_mz * m;
                if (yj <= deiso_widen(in[i]) * b) return true;
            }
        }
    }
    return false;
}

/* the offsets of spectrum s clipped to [0, total] */
DEV void deiso_range(const int64_t *peak_off, uint64_t s, int64_t total, int64_t *p0, int64_t *p1, bool *clipped) {
    const int64_t a = peak_off[s], b = peak_off[s + 1];
    int64_t lo = a < 0 ? 0 : (a > total ? total : a);
    int64_t hi = b < lo ? lo : (b > total ? total : b);
    *clipped = lo != a || hi != b;
    *p0 = lo;
    *p1 = hi;
}

DEV int64_t deiso_total(const int64_t *peak_off, uint64_t n_spectra, int64_t cap_peaks) {
    const int64_t t = peak_off[n_spectra];
    return t < 0 ? 0 : (t > cap_peaks ? cap_peaks : t);
}
