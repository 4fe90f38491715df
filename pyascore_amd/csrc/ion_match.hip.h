/* ion_match.hip.h -- the matched fragments of a reported localisation: what the ion stage (ions.hip, its section 1), the
 * mass-error profile (mz_profile.hip) and the explained ion current (coverage.hip) share beyond the general route's device
 * functions. */
#ifndef PYA_ION_MATCH_H
#define PYA_ION_MATCH_H
#include "general_core.hip.h"

/* Every fragment Ascore::accumulateCounts visits for the signature `bits` (cpp/Ascore.cpp:53-121), by the whole wavefront:
 * both prefix tables staged (slot 0 forward, slot 1 backward), then direction, block of 64 consecutive prefixes (one per
 * lane), loss variant, ion type of the direction, charge -- the order the ion stage's records are in.  Every lane calls
 * visit(direction, prefix, loss variant, ion type, charge, theoretical m/z, table index, rank) together, so it may ballot;
 * a lane without that fragment (prefix at or beyond L - 1, loss sum not present) has table index -1, as a fragment without
 * a retained peak in its window has (gen_match_index) */
template <typename F>
DEV void ion_walk_winner(const GenLds &g, const DevConfig *cfg, uint64_t bits, int L, int zmax, uint32_t lc, const PeakEntry *tab, int R,
                         F &&visit) {
    const int lane = lane_id();
    const float err = cfg->mz_error;
    const bool half_check = err > 0.49f;
    const int T = cfg->n_types, n_fwd = cfg->n_fwd;
    const uint64_t types64 = load_types64(cfg);
    const int n_uniq = cfg->n_nl ? cfg->n_uniq : 1;
    if (lane < 2) gen_prefix_table(g, cfg, bits, L, lane, lane, lc);
    gen_sync();
    for (int dir = 0; dir < 2; dir++) {
        const int t0 = dir ? n_fwd : 0, t1 = dir ? T : n_fwd;
        for (int s0 = 0; s0 + 1 < L && t0 < t1; s0 += 64) {
            const int step = s0 + lane;
            const bool live = step + 1 < L;
            const float running = live ? g.run[dir * lc + step] : 0.f;
            const uint64_t pm = live ? g.pm[dir * lc + step] : 0ull;
            for (int v = 0; v < n_uniq; v++) {
                const bool has = (pm >> v) & 1ull;
                if (!__ballot(has)) continue;
                const float x = running - (cfg->n_nl ? g.uniq[v] : 0.f);
                for (int t = t0; t < t1; t++) {
                    const uint32_t type = type_at(types64, t);
                    double A, B;
                    type_constants((uint8_t)type, &A, &B);
                    const double m = ((double)x + A) - B;
                    for (int z = 1; z <= zmax; z++) {
                        const float f = charge_mz(m, z);
                        int rk = GEN_NO_MATCH;
                        const int at = has ? gen_match_index(tab, R, f, err, half_check, &rk) : -1;
                        visit(dir, step, v, type, z, f, at, rk);
                    }
                }
            }
        }
    }
}

#endif
