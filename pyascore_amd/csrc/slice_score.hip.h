/* slice_score.hip.h -- what a stage behind a run needs to score a slice of 64 site assignments, one per lane, with either
 * of the two front ends that give the float32 bits of the pep_scores records (probs.hip, ranked.hip; sites.hip takes the
 * general one alone):
 *   count nodes   probs_cnt.hip.h (pc_fits, pc_setup, pc_score): the tables once per PSM in LDS, then k table reads per
 *                 assignment, for a PSM under score_cnt.hip's conditions;
 *   general       pb_gen_score below: the lane-per-signature walk and PepScore chain of general_core.hip.h (a binary search
 *                 per fragment), for everything else.
 * and the LDS both are carved from: the front ends share the bytes at the start of the launch's dynamic LDS, whatever a stage
 * keeps for itself lies behind pb_front_bytes. */
#ifndef PYA_SLICE_SCORE_H
#define PYA_SLICE_SCORE_H
#include "probs_cnt.hip.h"
#include "general_core.hip.h"

/* launch switches */
#define PB_CNT 1u                     /* the count-node front end is carved (caps are valid) */
#define PB_GEN 2u                     /* the general front end is carved */

/* the general front end's LDS: the general route's without its lists, then hist[PYA_NTOP_MAX][64], a column per lane */
__host__ __device__ static inline size_t pb_gen_bytes(uint32_t l_cap) {
    return gen_own_off(l_cap, 0) + PYA_NTOP_MAX * 64 * 4;
}
/* whichever front end is larger: a stage's own LDS lies behind it */
__host__ __device__ static inline size_t pb_front_bytes(uint32_t l_cap, const PcCaps &caps, uint32_t sw) {
    const size_t a = (sw & PB_CNT) ? (pc_lds_bytes(caps) + 15) & ~(size_t)15 : 0;
    const size_t g = (sw & PB_GEN) ? (pb_gen_bytes(l_cap) + 15) & ~(size_t)15 : 0;
    return a > g ? a : g;
}

/* the general front end: the PepScore of the lane's site assignment (Ascore.cpp:53-139), counted by gen_walk_assignment into
 * the lane's column of hist and scored by gen_pep_score; -1 and *bad when the score table has no row for its fragment count */
DEV float pb_gen_score(const BatchDev &b, const DevConfig *cfg, const GenLds &g, uint32_t *hist, const PeakEntry *tab, int R, int L, int zmax,
                       uint64_t bits, bool active, bool *bad) {
    const int lane = lane_id();
    const int ntop = cfg->n_top;
    for (int d = 0; d < PYA_NTOP_MAX; d++) hist[d * 64 + lane] = 0u;
    float ws = -1.f;
    bool in_table = true;
    if (active) {
        const uint32_t nfrag = gen_walk_assignment(g, cfg, bits, L, zmax, tab, R, [&](int rk) {
            if (rk < ntop) hist[rk * 64 + lane]++;
        });
        in_table = gen_pep_score(b, cfg, hist + lane, 64, nfrag, &ws);
    }
    *bad = *bad || __any(!in_table);                            /* (the run would have rejected the PSM: not reached) */
    return ws;
}

#endif
