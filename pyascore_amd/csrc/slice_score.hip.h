/* slice_score.hip.h -- what a stage behind a run needs to score a slice of 64 site assignments, one per lane, with either
 * of the two front ends that give the float32 bits of the pep_scores records (probs.hip, ranked.hip):
 *   count nodes   probs_cnt.hip.h (pc_fits, pc_setup, pc_score): the tables once per PSM in LDS, then k table reads per
 *                 assignment, for a PSM under score_cnt.hip's conditions;
 *   general       pb_gen_score below: the lane-per-signature count loop of sites.hip on general_core.hip.h (a binary search
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
    return ((gen_lds_bytes(l_cap, 0) + 15) & ~(size_t)15) + PYA_NTOP_MAX * 64 * 4;
}
/* whichever front end is larger: a stage's own LDS lies behind it */
__host__ __device__ static inline size_t pb_front_bytes(uint32_t l_cap, const PcCaps &caps, uint32_t sw) {
    const size_t a = (sw & PB_CNT) ? (pc_lds_bytes(caps) + 15) & ~(size_t)15 : 0;
    const size_t g = (sw & PB_GEN) ? (pb_gen_bytes(l_cap) + 15) & ~(size_t)15 : 0;
    return a > g ? a : g;
}

/* the general front end: the PepScore of the lane's site assignment as sites.hip counts it (Ascore.cpp:53-139); -1 and
 * *bad when the score table has no row for its fragment count */
DEV float pb_gen_score(const BatchDev &b, const DevConfig *cfg, const GenLds &g, uint32_t *hist, const PeakEntry *tab, int R, int L, int zmax,
                       uint64_t bits, bool active, bool *bad) {
    const int lane = lane_id();
    const float err = cfg->mz_error;
    const bool half_check = err > 0.49f;
    const int T = cfg->n_types, n_fwd = cfg->n_fwd;
    const uint64_t types64 = load_types64(cfg);
    const int ntop = cfg->n_top;
    for (int d = 0; d < PYA_NTOP_MAX; d++) hist[d * 64 + lane] = 0u;
    uint32_t nfrag = 0;
    if (active) {
        for (int dir = 0; dir < 2; dir++) {
            const int t0 = dir ? n_fwd : 0, t1 = dir ? T : n_fwd;
            if (t0 == t1) continue;
            float running = 0.f;
            uint32_t st = 0;
            uint64_t pm_now = 1ull;
            for (int step = 0; step + 1 < L; step++) {
                const int ri = dir ? L - 1 - step : step;
                const bool mod = gen_modified(g, bits, ri);
                running = (mod ? g.m1[ri] : g.m0[ri]) + running;
                if (cfg->n_nl) {
                    const uint32_t cls = mod ? g.nl1[ri] : g.nl0[ri];
                    if (cls) {
                        const uint32_t st2 = nl_bump(st, cls);
                        if (st2 != st) pm_now = gen_present(g, cfg->n_cand, st2);
                        st = st2;
                    }
                }
                uint64_t pm = pm_now;
                while (pm) {
                    const int v = __builtin_ctzll(pm);
                    pm &= pm - 1;
                    const float x = running - (cfg->n_nl ? g.uniq[v] : 0.f);
                    for (int t = t0; t < t1; t++) {
                        double A, B;
                        type_constants(type_at(types64, t), &A, &B);
                        const double m = ((double)x + A) - B;
                        for (int z = 1; z <= zmax; z++) {
                            const int rk = gen_match_rank(tab, R, charge_mz(m, z), err, half_check);
                            if (rk < ntop) hist[rk * 64 + lane]++;
                            nfrag++;
                        }
                    }
                }
            }
        }
    }
    const bool in_table = nfrag <= b.lut_n_max;
    float ws = -1.f;
    if (active && in_table) {
        double sum = 0.;
        uint32_t acc = 0;
        const float *row = b.lut + b.lut_off[nfrag];
        for (int d = 0; d < ntop; d++) {
            acc += hist[d * 64 + lane];
            const float sc = row[(uint32_t)d * (nfrag + 1) + acc];
            if (d < PYA_NTOP) {
                const float prod = cfg->weights[d] * sc;      /* float product ... */
                sum = sum + (double)prod;                     /* ... double sum    */
            }
        }
        ws = (float)sum;
    }
    *bad = *bad || __any(active && !in_table);                  /* (the run would have rejected the PSM: not reached) */
    return ws;
}

#endif
