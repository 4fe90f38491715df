/* ion_match.hip.h -- the match of one theoretical fragment with the peak that stands for it: what the ion stage (ions.hip)
 * and the mass-error profile (mz_profile.hip) share beyond the general route's device functions. */
#ifndef PYA_ION_MATCH_H
#define PYA_ION_MATCH_H
#include "general_core.hip.h"

/* gen_match_rank with the table index of the peak: the lowest rank inside the open window and, among equal ranks, the
 * lowest m/z (the table is in m/z order; the reference consumes windows in that order and replaces a match only by a
 * lower rank).  -1: none */
DEV int ion_match_index(const PeakEntry *e, int n, float f, float err, bool half_check, int *rank) {
    const float lo = f - err, hi = f + err;
    int a = 0, b = n;
    while (a < b) {                                           /* first entry above lo */
        const int m = (a + b) >> 1;
        if (e[m].mz > lo) b = m;
        else a = m + 1;
    }
    int best = GEN_NO_MATCH, at = -1;
    for (int i = a; i < n; i++) {
        const PeakEntry x = e[i];
        if (!(x.mz < hi)) break;
        if ((!half_check || (double)f >= (double)x.mz - 0.5) && (int)x.rank < best) {
            best = (int)x.rank;
            at = i;
        }
    }
    *rank = best;
    return at;
}

#endif
