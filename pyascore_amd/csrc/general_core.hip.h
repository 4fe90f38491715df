/* general_core.hip.h -- the device functions of the general route (general_psm.hip has the notes): residues and loss
 * classes in LDS, one signature's prefix tables, fragment lists ranked by counting, the greedy walk for the
 * site-determining ions of a pair.  The arithmetic that fixes the float32 bits of a PepScore exists here once, for
 * general_psm.hip and every stage behind a run: the window search (gen_match_index), the walk of a site assignment on one
 * lane (gen_walk_assignment), the PepScore chain (gen_pep_score), the depth of a pair (gen_pair_depth), the pair routine's
 * steps (gen_pair_tables, gen_fill_list, gen_rank_sort, gen_greedy_walk). */
#ifndef PYA_GENERAL_CORE_H
#define PYA_GENERAL_CORE_H
#include "localize_core.hip.h"

#define GEN_NO_MATCH 255
#define GEN_MAX_SITES 64

/* the table index of the peak that stands for fragment f: among the retained peaks p with f32(f - err) < p < f32(f + err)
 * and f >= p - 0.5 (ModifiedPeptide.cpp:126-150) the lowest rank and, among equal ranks, the lowest m/z (the table is in
 * m/z order; the reference consumes windows in that order and replaces a match only by a lower rank).  -1: none, and
 * *rank = GEN_NO_MATCH */
DEV int gen_match_index(const PeakEntry *e, int n, float f, float err, bool half_check, int *rank) {
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
/* its rank alone */
DEV int gen_match_rank(const PeakEntry *e, int n, float f, float err, bool half_check) {
    int rank;
    (void)gen_match_index(e, n, f, err, half_check, &rank);
    return rank;
}

/* LDS of one wavefront (l_cap residues, list_cap ions per list) */
struct GenLds {
    float *m0, *m1;              /* [l_cap] */
    float *run;                  /* [2][l_cap] running sums of the two signatures being compared, current direction */
    uint32_t *cpre;              /* [2][l_cap] ions (x charges) before the prefix */
    uint64_t *pm;                /* [2][l_cap] loss sums present (bit v = uniq[v]) */
    uint8_t *nl0, *nl1, *sor;    /* [l_cap] loss class unmodified / modified, site index of the residue (255: none) */
    uint8_t *site_pos;           /* [64] residue of the j-th modifiable one */
    float *uniq;                 /* [PYA_MAX_UNIQ_WIDE] the distinct sums of <= 2 neutral losses, [0] = none */
    uint8_t *cand;               /* [3][PYA_MAX_NL_CANDS] classes a, b (255: a alone) and sum number of every candidate */
    uint32_t *site_max, *site_tie;   /* [64] */
    unsigned long long *site_alt;    /* [64] */
    float *site_asc;             /* [64] */
    uint32_t *misc;              /* [16] counters */
    float *sc;                   /* [2][PYA_NTOP_MAX] depth scores of the two signatures */
    float *la, *lb, *sa, *sb;    /* [list_cap] each: the two lists, unsorted and sorted */
    uint8_t *ha, *hb;            /* [list_cap] the sorted ion matched a peak of rank <= depth */
};
__host__ __device__ static inline size_t gen_lds_bytes(uint32_t l_cap, uint32_t list_cap) {
    const size_t lc = (l_cap + 3u) & ~3u;
    return lc * (4 + 4 + 2 * 4 + 2 * 4 + 2 * 8 + 3) + 64 + 3 * PYA_MAX_NL_CANDS + 4 + PYA_MAX_UNIQ_WIDE * 4 + 64 * (4 + 4 + 8 + 4) + 64 +
           2 * PYA_NTOP_MAX * 4 + 8 + (size_t)list_cap * (4 * 4 + 2) + 64;
}
/* where a stage's own LDS begins behind this carve: lds_raw + gen_own_off(...), 16-byte aligned */
__host__ __device__ static inline size_t gen_own_off(uint32_t l_cap, uint32_t list_cap) {
    return (gen_lds_bytes(l_cap, list_cap) + 15) & ~(size_t)15;
}
DEV GenLds gen_carve(unsigned char *raw, uint32_t l_cap, uint32_t list_cap) {
    const size_t lc = (l_cap + 3u) & ~3u;
    GenLds g;
    g.site_alt = (unsigned long long *)raw;
    g.pm = (uint64_t *)(g.site_alt + 64);
    g.m0 = (float *)(g.pm + 2 * lc);
    g.m1 = g.m0 + lc;
    g.run = g.m1 + lc;
    g.cpre = (uint32_t *)(g.run + 2 * lc);
    g.uniq = (float *)(g.cpre + 2 * lc);
    g.site_max = (uint32_t *)(g.uniq + PYA_MAX_UNIQ_WIDE);
    g.site_tie = g.site_max + 64;
    g.site_asc = (float *)(g.site_tie + 64);
    g.misc = (uint32_t *)(g.site_asc + 64);
    g.sc = (float *)(g.misc + 16);
    g.la = g.sc + 2 * PYA_NTOP_MAX + 2;
    g.lb = g.la + list_cap;
    g.sa = g.lb + list_cap;
    g.sb = g.sa + list_cap;
    g.nl0 = (uint8_t *)(g.sb + list_cap);
    g.nl1 = g.nl0 + lc;
    g.sor = g.nl1 + lc;
    g.site_pos = g.sor + lc;
    g.cand = g.site_pos + 64;
    g.ha = g.cand + 3 * PYA_MAX_NL_CANDS + 4;
    g.hb = g.ha + list_cap;
    return g;
}

DEV void gen_sync() {           /* lanes hand data over through LDS and through the workspace */
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

/* is residue ri modified in the signature `bits` (bit j = j-th modifiable residue)? */
DEV bool gen_modified(const GenLds &g, uint64_t bits, int ri) {
    const uint32_t j = g.sor[ri];
    return j != 255u && ((bits >> j) & 1ull);
}

/* which loss sums exist for a fragment whose residues carried the loss classes counted in `st` (2 bits per class,
 * saturating at 2): none, every class seen, every pair of classes seen, a class twice when it was seen twice --
 * PowerSetSum(stack, 2), cpp/Util.cpp:95-141, as the set of distinct values (host_tables.cpp: build_dev_config) */
DEV uint64_t gen_present(const GenLds &g, int n_cand, uint32_t st) {
    uint64_t m = 1ull;
    for (int i = 0; i < n_cand; i++) {
        const uint32_t a = g.cand[i], b2 = g.cand[PYA_MAX_NL_CANDS + i];
        const uint32_t ca = (st >> (2u * a)) & 3u;
        const bool ok = b2 == 255u ? ca >= 1u : (b2 == a ? ca >= 2u : (ca >= 1u && ((st >> (2u * b2)) & 3u) >= 1u));
        if (ok) m |= 1ull << g.cand[2 * PYA_MAX_NL_CANDS + i];
    }
    return m;
}

/* The prefixes of one signature along one direction, on the calling lane (ModifiedPeptide.cpp:385-408): the float32
 * running sum -- (mod ? m1 : m0) + running, the order that fixes the bits -- and the neutral-loss state.
 * per_prefix(step, running, loss sums present) */
template <typename F>
DEV void gen_walk_prefixes(const GenLds &g, const DevConfig *cfg, uint64_t bits, int L, int dir, F &&per_prefix) {
    float running = 0.f;
    uint32_t st = 0;
    uint64_t pm = 1ull;
    for (int step = 0; step + 1 < L; step++) {
        const int ri = dir ? L - 1 - step : step;
        const bool mod = gen_modified(g, bits, ri);
        running = (mod ? g.m1[ri] : g.m0[ri]) + running;
        if (cfg->n_nl) {
            const uint32_t cls = mod ? g.nl1[ri] : g.nl0[ri];
            if (cls) {
                const uint32_t st2 = nl_bump(st, cls);
                if (st2 != st) pm = gen_present(g, cfg->n_cand, st2);
                st = st2;
            }
        }
        per_prefix(step, running, pm);
    }
}

/* Running sums, loss sums present and ion offsets of one signature along one direction into slot `slot` (one lane).
 * Returns the number of (prefix, loss variant) pairs. */
DEV uint32_t gen_prefix_table(const GenLds &g, const DevConfig *cfg, uint64_t bits, int L, int dir, int slot, uint32_t lc) {
    uint32_t cnt = 0;
    gen_walk_prefixes(g, cfg, bits, L, dir, [&](int step, float running, uint64_t pm) {
        g.run[slot * lc + step] = running;
        g.pm[slot * lc + step] = pm;
        g.cpre[slot * lc + step] = cnt;
        cnt += (uint32_t)__popcll(pm);
    });
    return cnt;
}

/* One whole site assignment on the calling lane, as Ascore::accumulateCounts visits it (Ascore.cpp:53-121): both
 * directions, every prefix, loss variant, ion type of the direction and charge; per_rank(rank of the fragment's match,
 * GEN_NO_MATCH when it has none).  Returns the number of fragments. */
template <typename F>
DEV uint32_t gen_walk_assignment(const GenLds &g, const DevConfig *cfg, uint64_t bits, int L, int zmax, const PeakEntry *tab, int R,
                                 F &&per_rank) {
    const float err = cfg->mz_error;
    const bool half_check = err > 0.49f;
    const int T = cfg->n_types, n_fwd = cfg->n_fwd;
    const uint64_t types64 = load_types64(cfg);
    uint32_t nfrag = 0;
    for (int dir = 0; dir < 2; dir++) {
        const int t0 = dir ? n_fwd : 0, t1 = dir ? T : n_fwd;
        if (t0 == t1) continue;
        gen_walk_prefixes(g, cfg, bits, L, dir, [&](int, float running, uint64_t pm) {
            while (pm) {
                const int v = __builtin_ctzll(pm);
                pm &= pm - 1;
                const float x = running - (cfg->n_nl ? g.uniq[v] : 0.f);
                for (int t = t0; t < t1; t++) {
                    double A, B;
                    type_constants(type_at(types64, t), &A, &B);
                    const double m = ((double)x + A) - B;
                    for (int z = 1; z <= zmax; z++) {
                        per_rank(gen_match_rank(tab, R, charge_mz(m, z), err, half_check));
                        nfrag++;
                    }
                }
            }
        });
    }
    return nfrag;
}

/* From a lane's counts per depth (cnt[d * stride], d < n_top) and its fragment count to the float32 PepScore
 * (Ascore.cpp:123-139): cumulative counts, the score table's row, float product, double sum over the first PYA_NTOP
 * depths, (float).  cum / sc (optional, same stride; either may be cnt itself): the cumulative counts and the depth
 * scores of all n_top depths.  false, and *ws = -1, when the score table has no row for nfrag. */
DEV bool gen_pep_score(const BatchDev &b, const DevConfig *cfg, const uint32_t *cnt, int stride, uint32_t nfrag, float *ws,
                       uint32_t *cum = nullptr, float *sc = nullptr) {
    *ws = -1.f;
    if (nfrag > b.lut_n_max) return false;
    const int ntop = cfg->n_top;
    const float *row = b.lut + b.lut_off[nfrag];
    double sum = 0.;
    uint32_t acc = 0;
    for (int d = 0; d < ntop; d++) {
        acc += cnt[d * stride];
        if (cum) cum[d * stride] = acc;
        const float s = row[(uint32_t)d * (nfrag + 1) + acc];
        if (sc) sc[d * stride] = s;
        if (d < PYA_NTOP) {
            const float prod = cfg->weights[d] * s;       /* float product ... */
            sum = sum + (double)prod;                     /* ... double sum    */
        }
    }
    *ws = (float)sum;
    return true;
}

/* the depth of a pair (Ascore.cpp:164-172): the first depth with the largest gap between the depth scores of the
 * reference and the other (ref[d * stride], oth[d * stride], d < n); 0 when no gap is positive */
DEV int gen_pair_depth(const float *ref, const float *oth, int stride, int n) {
    int depth = 0;
    float bestd = 0.f;
    for (int d = 0; d < n; d++) {
        const float diff = ref[d * stride] - oth[d * stride];
        if (diff > bestd) {
            bestd = diff;
            depth = d;
        }
    }
    return depth;
}

/* the ions of one (signature slot, ion type), every charge and loss variant, into `out`: one prefix per lane and trip.
 * ident (optional): the identity of every ion beside its m/z -- size | charge << 16 | (a loss sum) << 24 (ions.hip) */
DEV void gen_fill_list(const GenLds &g, const DevConfig *cfg, int L, int zmax, int slot, uint32_t lc, double A, double B, float *out,
                       uint32_t *ident = nullptr) {
    for (int step = lane_id(); step + 1 < L; step += 64) {
        const float running = g.run[slot * lc + step];
        uint64_t pm = g.pm[slot * lc + step];
        uint32_t at = g.cpre[slot * lc + step] * (uint32_t)zmax;
        while (pm) {
            const int v = __builtin_ctzll(pm);
            pm &= pm - 1;
            const float x = running - (cfg->n_nl ? g.uniq[v] : 0.f);
            const double m = ((double)x + A) - B;
            for (int z = 1; z <= zmax; z++) {
                if (ident) ident[at] = (uint32_t)(step + 1) | (uint32_t)z << 16 | (v ? 1u << 24 : 0u);
                out[at++] = charge_mz(m, z);
            }
        }
    }
}

/* ascending order by counting: position = ions below + equal ions before (any correct sort leaves the same values).
 * ident (optional): moved with the values, so equal m/z keep the order of the fill: size, loss sum, charge */
DEV void gen_rank_sort(const float *in, float *out, int n, const uint32_t *ident = nullptr, uint32_t *ident_out = nullptr) {
    for (int i = lane_id(); i < n; i += 64) {
        const float x = in[i];
        int pos = 0;
        for (int j = 0; j < n; j++) {
            const float y = in[j];
            pos += (y < x || (y == x && j < i)) ? 1 : 0;
        }
        out[pos] = x;
        if (ident) ident_out[pos] = ident[i];
    }
}

/* the prefix tables of a pair along one direction, slot 0 `ref_bits` and slot 1 `oth_bits` (lanes 0 and 1); their numbers
 * of (prefix, loss variant) pairs, wave-uniform */
DEV void gen_pair_tables(const GenLds &g, const DevConfig *cfg, uint64_t ref_bits, uint64_t oth_bits, int L, int dir, uint32_t lc,
                         uint32_t *npairs_a, uint32_t *npairs_b) {
    const int lane = lane_id();
    gen_sync();
    uint32_t n = 0;
    if (lane < 2) n = gen_prefix_table(g, cfg, lane ? oth_bits : ref_bits, L, dir, lane, lc);
    *npairs_a = (uint32_t)__shfl((int)n, 0, 64);
    *npairs_b = (uint32_t)__shfl((int)n, 1, 64);
    gen_sync();
}

/* the greedy walk over two sorted lists (ModifiedPeptide.cpp:291-316), one lane's: ions of the two lists closer than err
 * cancel in pairs, every other ion is site-determining; survives(1 for list b, its index) */
template <typename F>
DEV void gen_greedy_walk(const float *sa, int na, const float *sb, int nb, float err, F &&survives) {
    int ia = 0, ib = 0;
    while (ia < na || ib < nb) {
        if (ib == nb) {
            survives(0, ia++);
        } else if (ia == na) {
            survives(1, ib++);
        } else {
            const float xa = sa[ia], xb = sb[ib];
            if (__builtin_fabsf(xa - xb) < err) {
                ia++;
                ib++;
            } else if (xa < xb) {
                survives(0, ia++);
            } else {
                survives(1, ib++);
            }
        }
    }
}

/* residues, fixed modifications, neutral-loss classes, the list of modifiable residues (ModifiedPeptide.cpp:24-79);
 * zeroes the per-site work areas.  Returns the number of modifiable residues. */
DEV int gen_setup_residues(const BatchDev &b, const DevConfig *cfg, const GenLds &g, uint32_t psm, int64_t pep0, int L) {
    const int lane = lane_id();
    for (int i = lane; i < L; i += 64) {
        const uint32_t li = ((uint32_t)b.pep[pep0 + i] - 'A') & 31u;
        const float m0 = cfg->res_mass[li];
        const bool modifiable = cfg->res_modifiable[li] || (cfg->allow_n && i == 0) || (cfg->allow_c && i == L - 1);
        g.m0[i] = m0;
        g.m1[i] = m0 + cfg->mod_mass;
        g.nl0[i] = cfg->nl_upper[li];
        g.nl1[i] = modifiable ? cfg->nl_lower[li] : 0;
        g.sor[i] = modifiable ? 0 : 255;
    }
    if (lane < PYA_MAX_UNIQ_WIDE) g.uniq[lane] = cfg->uniq_w[lane];
    if (lane < PYA_MAX_NL_CANDS) {
        g.cand[lane] = cfg->cand_a[lane];
        g.cand[PYA_MAX_NL_CANDS + lane] = cfg->cand_b[lane];
        g.cand[2 * PYA_MAX_NL_CANDS + lane] = cfg->cand_u[lane];
    }
    if (lane < GEN_MAX_SITES) {
        g.site_max[lane] = 0;
        g.site_tie[lane] = 0;
        g.site_alt[lane] = 0ull;
        g.site_asc[lane] = __builtin_huge_valf();
    }
    if (lane < 16) g.misc[lane] = 0;
    gen_sync();
    if (lane == 0) {
        for (int64_t a = b.aux_off[psm]; a < b.aux_off[psm + 1]; a++) {       /* fixed modifications, in their order */
            const uint32_t pos = b.aux_pos[a];
            const float am = b.aux_mass[a];
            const int idx = pos > 0 ? (int)pos - 1 : 0;
            if (idx < L) {
                const uint32_t li = ((uint32_t)b.pep[pep0 + idx] - 'A') & 31u;
                g.m0[idx] += am;
                g.m1[idx] += am;
                if (cfg->nl_lower[li]) g.nl0[idx] = cfg->nl_lower[li];
            }
        }
        int j = 0;
        for (int i = 0; i < L; i++)
            if (g.sor[i] != 255) {
                /* (8 bits: read only where L <= 64, for the residue bits of alt_mask in general_psm.hip; above that
                 * length alt_mask holds site bits, and evidence.hip / sites.hip keep 16-bit residues of their own.
                 * tests/test_gpu_stage_limits.py runs modifiable residues at 256 and above through every stage) */
                if (j < GEN_MAX_SITES) g.site_pos[j] = (uint8_t)i;
                g.sor[i] = (uint8_t)j;
                j++;
            }
        g.misc[0] = (uint32_t)j;
    }
    gen_sync();
    return (int)g.misc[0];
}

/* Ascore of `ref` against `oth` at `depth` (Ascore.cpp:177-209): per ion type both fragment lists, sorted, the greedy
 * walk for the site-determining ions (ModifiedPeptide.cpp:259-320), their matches of rank <= depth, the two binomial
 * scores from the table.  The value is lane 0's; returns non-zero (wave-uniform) when a list or a trial count is
 * beyond what the launch / the score table was sized for.  tally (optional, lane 0's): the site-determining ions of `ref`,
 * those of them matched, the same for `oth` -- ion_trials / ion_counts of Ascore.cpp:177-197. */
DEV int gen_ascore_pair(const BatchDev &b, const DevConfig *cfg, const GenLds &g, uint64_t ref_bits, uint64_t oth_bits, int depth,
                        int L, int zmax, uint32_t lc, uint32_t list_cap, const PeakEntry *tab, int R, float *asc_out,
                        uint32_t *tally = nullptr) {
    const int lane = lane_id();
    const float err = cfg->mz_error;
    const bool half_check = err > 0.49f;
    const int T = cfg->n_types, n_fwd = cfg->n_fwd;
    const uint64_t types64 = load_types64(cfg);
    int fail = 0;
    uint32_t tr0 = 0, tr1 = 0, c0 = 0, c1 = 0;              /* (lane 0 keeps the tallies) */
    int tables_dir = -1;
    uint32_t npairs_a = 0, npairs_b = 0;
    for (int t = 0; t < T; t++) {
        const int dir = t < n_fwd ? 0 : 1;
        if (dir != tables_dir) {
            gen_pair_tables(g, cfg, ref_bits, oth_bits, L, dir, lc, &npairs_a, &npairs_b);
            tables_dir = dir;
        }
        const int na = (int)npairs_a * zmax, nb = (int)npairs_b * zmax;
        if ((uint32_t)na > list_cap || (uint32_t)nb > list_cap) {
            fail = 1;                                       /* (the host sized list_cap for the longest list: not reached) */
            break;
        }
        double A, B;
        type_constants(type_at(types64, t), &A, &B);
        gen_fill_list(g, cfg, L, zmax, 0, lc, A, B, g.la);
        gen_fill_list(g, cfg, L, zmax, 1, lc, A, B, g.lb);
        gen_sync();
        gen_rank_sort(g.la, g.sa, na);
        gen_rank_sort(g.lb, g.sb, nb);
        gen_sync();
        for (int i = lane; i < na; i += 64) g.ha[i] = gen_match_rank(tab, R, g.sa[i], err, half_check) <= depth ? 1 : 0;
        for (int i = lane; i < nb; i += 64) g.hb[i] = gen_match_rank(tab, R, g.sb[i], err, half_check) <= depth ? 1 : 0;
        gen_sync();
        if (lane == 0)
            gen_greedy_walk(g.sa, na, g.sb, nb, err, [&](int side, int i) {
                if (side) {
                    tr1++;
                    c1 += g.hb[i];
                } else {
                    tr0++;
                    c0 += g.ha[i];
                }
            });
        gen_sync();
    }
    if (lane == 0 && !fail) {
        if (tr0 > b.lut_n_max || tr1 > b.lut_n_max) {
            fail = 1;
        } else {
            const float sc0 = b.lut[b.lut_off[tr0] + (uint32_t)depth * (tr0 + 1) + c0];
            const float sc1 = b.lut[b.lut_off[tr1] + (uint32_t)depth * (tr1 + 1) + c1];
            *asc_out = sc0 - sc1;
            if (tally) {                                    /* (evidence.hip: what the two scores were made of) */
                tally[0] = tr0;
                tally[1] = c0;
                tally[2] = tr1;
                tally[3] = c1;
            }
        }
    }
    gen_sync();
    return __any(fail) ? 1 : 0;
}

#endif
