/* general_psm.hip -- the whole Ascore path of ONE PSM by one wavefront, without the size limits the fast kernels
 * buy their speed with: peptides up to 255 residues (a 64-bit residue mask and one residue per lane are the data
 * layout of every other kernel), any number of site assignments the workspace holds (the others keep their sort
 * room and pre-sort tables in LDS), fragment lists of up to 8 192 ions per ion type.
 *
 * It is the reference's algorithm in the reference's own shape, laid out for a wavefront only where that is free:
 *   residues, fixed modifications, neutral-loss classes        cpp/ModifiedPeptide.cpp:24-79
 *   counts per site assignment (one assignment per lane)       cpp/Ascore.cpp:53-121, cpp/ModifiedPeptide.cpp:326-609
 *   PepScores from the host-built score table                  cpp/Ascore.cpp:123-139, cpp/Util.cpp:16-83
 *   the front of std::sort (wave emulation in global memory)   cpp/Ascore.cpp:141-146
 *   single-move competitors, the best of every modified site   cpp/Ascore.cpp:212-254
 *   site-determining ions: both lists, sorted, greedy walk     cpp/ModifiedPeptide.cpp:259-320
 *   Ascores                                                    cpp/Ascore.cpp:157-210
 * n_top (peaks retained per window = depths scored) is a run-time value here, 10 to 16: such depths are counted and
 * scored, the first ten weighted, all of them searched for the depth of an Ascore (Ascore.cpp:15-36, :123-139, :164-172);
 * a scorer created with n_top > 10 sends every PSM here.
 * Binning is not repeated: the PSM's spectrum goes through bin_spectra like every other one.  The host sends a PSM
 * here only when it exceeds a limit of the fast kernels (host_plan.cpp: plan_create_impl); a batch of ordinary PSMs never
 * launches this kernel.  Speed is not a goal: the lookups are binary searches in the workspace table, the lists are
 * ranked by counting, the walk is one lane's.
 */
#include "general_core.hip.h"

/* scratch_off[i]: where the i-th PSM of the list has its slice of `scratch` -- sized for ITS OWN number of site assignments
 * and competitors (pya_general_scratch_bytes), not for the launch's largest (r04 advisor finding: one PSM with millions
 * of site assignments made every general PSM of the batch reserve as much) */
__global__ __launch_bounds__(64) void pya_general_psm_kernel(BatchDev b, const uint32_t *ids, uint32_t n_ids, unsigned char *scratch,
                                                              const uint64_t *scratch_off, uint32_t l_cap, uint32_t list_cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    if (blockIdx.x >= n_ids) return;
    const uint32_t psm = ids[blockIdx.x];
    const int lane = lane_id();
    const DevConfig *cfg = b.cfg;
    const GenLds g = gen_carve(lds_raw, l_cap, list_cap);
    const uint32_t lc = (l_cap + 3u) & ~3u;
    unsigned char *my = scratch + scratch_off[blockIdx.x];

    const uint32_t max_k = b.max_k;
    float *out_asc = b.ascores + (size_t)psm * max_k;
    uint64_t *out_alt = b.alt_mask + (size_t)psm * max_k;
    for (uint32_t a = lane; a < max_k; a += 64) {
        out_asc[a] = 0.f;
        out_alt[a] = 0ull;
    }
    if (b.status[psm] != PYA_ST_OK) {
        if (lane == 0) {
            b.best_score[psm] = -1.f;
            b.best_sig[psm] = 0ull;
            b.n_sig_out[psm] = -1;
        }
        return;
    }
    const int64_t pep0 = b.pep_off[psm];
    const int L = (int)(b.pep_off[psm + 1] - pep0);
    const int k = b.n_of_mod[psm];
    const int zmax = b.max_charge[psm];
    const int N = (int)b.n_sig[psm];
    PushedEntry *pushed = (PushedEntry *)(my + ((sort_global_bytes((size_t)N) + 15) & ~(size_t)15));
    const uint64_t *order = b.order_tab + b.order_off[psm];
    const uint32_t *inv = b.inv_tab + b.order_off[psm];
    const int64_t s0 = b.sig_off[psm];
    const PeakEntry *tab = b.ret + b.ret_off[psm];
    const int R = (int)b.ret_n[psm];
    const int ntop = cfg->n_top;                               /* 10..PYA_NTOP_MAX */
    const uint32_t rec_words = (uint32_t)(ntop + 1) / 2u + 1u;    /* count record: ntop 16-bit counts + the fragment total (host_internal.h: rec_words) */

    const int n_sites = gen_setup_residues(b, cfg, g, psm, pep0, L);
    /* (its own competitors: k (n - k) single moves -- what the host sized the slice for) */
    const uint32_t push_cap = k >= 0 && k <= n_sites ? (((uint32_t)k * (uint32_t)(n_sites - k)) + 3u) & ~3u : 0u;

    /* ---- counts and PepScores, one site assignment per lane and trip (Ascore.cpp:53-139) ---- */
    int fail = 0;
    for (int s = lane; s < N; s += 64) {
        const uint64_t bits = order[s];
        uint32_t cnt[PYA_NTOP_MAX];
#pragma unroll
        for (int d = 0; d < PYA_NTOP_MAX; d++) cnt[d] = 0;
        const uint32_t nfrag = gen_walk_assignment(g, cfg, bits, L, zmax, tab, R, [&](int rk) {
            if (rk < ntop) cnt[rk]++;
        });
        float ws;                                              /* (the counts turn cumulative where they stand, in registers) */
        if (!gen_pep_score(b, cfg, cnt, 1, nfrag, &ws, cnt)) fail = 1;
        b.ws[s0 + s] = ws;
        uint32_t *r6 = b.rec + (size_t)(s0 + s) * rec_words;
#pragma unroll
        for (int d = 0; d < PYA_NTOP_MAX; d += 2)
            if (d < ntop) r6[d >> 1] = cnt[d] | ((d + 1 < ntop ? cnt[d + 1] : 0u) << 16);
        r6[rec_words - 1] = nfrag;
    }
    if (__any(fail)) {
        if (lane == 0) {
            b.status[psm] = PYA_ST_LUT_RANGE;
            b.best_score[psm] = -1.f;
            b.best_sig[psm] = 0ull;
            b.n_sig_out[psm] = -1;
        }
        return;
    }
    gen_sync();
    const float *ws = b.ws + s0;

    /* ---- Ascore::isUnambiguous (Ascore.cpp:38-51) ---- */
    if (k >= n_sites) {
        for (int a = lane; a < k && a < (int)max_k; a += 64) out_asc[a] = __builtin_huge_valf();
        if (lane == 0) {
            b.best_score[psm] = N > 0 ? ws[0] : -1.f;
            b.best_sig[psm] = N > 0 ? order[0] : 0ull;
            b.n_sig_out[psm] = N;
            if (b.keep && N > 0) b.sorted_idx[s0] = 0;
        }
        return;
    }

    /* ---- the winner: the front of std::sort (Ascore.cpp:141-146) ---- */
    uint32_t kmax = 0, first_max = 0xffffffffu;
    int n_max = 0;
    for (int i = lane; i < N; i += 64) {
        const uint32_t u = __float_as_uint(ws[i]);             /* scores are >= 0: bit order = value order */
        kmax = u > kmax ? u : kmax;
    }
    kmax = wave_max_u32(kmax);
    for (int i = lane; i < N; i += 64)
        if (__float_as_uint(ws[i]) == kmax) {
            n_max++;
            first_max = first_max < (uint32_t)i ? first_max : (uint32_t)i;
        }
    n_max = wave_sum_i32(n_max);
    first_max = wave_min_u32(first_max);
    uint32_t best_i = first_max;
    if (n_max != 1 || b.keep || (b.debug & 1024)) {
        const SortGlobal srt = sort_carve_global(my, N);
        for (int i = lane; i < N; i += 64) {
            srt.key[i] = ws[i];
            srt.idx[i] = (uint32_t)i;
        }
        srt.sync();
        int front_len = N;
        sort_introsort_loop<false>(srt, N, b.keep == 0, &front_len);
        uint32_t first_pos = 0xffffffffu;
        for (int i = lane; i < front_len; i += 64)
            if (__float_as_uint(srt.key[i]) == kmax) first_pos = first_pos < (uint32_t)i ? first_pos : (uint32_t)i;
        first_pos = wave_min_u32(first_pos);
        best_i = srt.idx[first_pos];
        if (b.keep)
            for (int i = lane; i < N; i += 64) b.sorted_idx[s0 + sort_final_pos(srt, i, N)] = srt.idx[i];
        srt.sync();
    }
    const float best_ws = __uint_as_float(kmax);
    const uint64_t best_bits = order[best_i];

    /* ---- single-move competitors (Ascore.cpp:212-254): the k (n - k) signatures one move away, enumerated through
     * their combination rank; the best of every modified site and its exact ties are kept ---- */
    const uint64_t all_sites = n_sites >= 64 ? ~0ull : ((1ull << n_sites) - 1ull);
    const uint64_t free_bits = all_sites & ~best_bits;
    const int n_free = n_sites - k, items = k * n_free;
    for (int pass = 0; pass < 2; pass++) {
        for (int e = lane; e < items; e += 64) {
            const int a = e / n_free, fb = e - a * n_free;
            const int pos_a = nth_set_bit(best_bits, a), pos_b = nth_set_bit(free_bits, fb);
            const uint64_t c = (best_bits & ~(1ull << pos_a)) | (1ull << pos_b);
            uint32_t rank = 0;
            uint64_t m = c;
            for (int t = 1; m; t++) {                              /* colexicographic rank of the combination */
                const int pos = __builtin_ctzll(m);
                m &= m - 1;
                rank += b.binom[pos * 64 + t];
            }
            const uint32_t idx = inv[rank];
            const uint32_t u = __float_as_uint(ws[idx]);
            if (pass == 0) {
                atomicMax(&g.site_max[a], u);
            } else if (u == g.site_max[a]) {
                if ((double)__builtin_fabsf(best_ws - __uint_as_float(u)) < 1e-6) {
                    g.site_tie[a] = 1u;                            /* ties the winner: Ascore 0 (Ascore.cpp:159-161) */
                    atomicOr(&g.site_alt[a], 1ull << (L <= 64 ? (int)g.site_pos[pos_b] : pos_b));
                } else {
                    const uint32_t slot = atomicAdd(&g.misc[1], 1u);
                    if (slot < push_cap) {
                        PushedEntry pe;
                        pe.bits = c;
                        pe.ws = __uint_as_float(u);
                        pe.idx = idx;
                        pushed[slot] = pe;
                    }
                }
            }
        }
        gen_sync();
    }
    uint32_t np = g.misc[1];
    if (np > push_cap) {                                       /* cannot happen: push_cap >= k (n - k) */
        np = push_cap;
        fail = 2;
    }

    /* ---- Ascores (Ascore.cpp:157-210), one competitor after the other ---- */
    for (uint32_t e = 0; e < np; e++) {
        const PushedEntry pe = pushed[e];
        const uint64_t gone = best_bits & ~pe.bits, came = pe.bits & ~best_bits;
        const int a = __popcll(best_bits & (gone - 1));
        const int came_j = __builtin_ctzll(came);
        if (lane == 0) g.site_alt[a] |= 1ull << (L <= 64 ? (int)g.site_pos[came_j] : came_j);
        /* depth scores of the two from the recorded counts; depth of the largest gap (first one, 0 when none is positive) */
        if (lane < 2 * PYA_NTOP_MAX) {
            const int which = lane / PYA_NTOP_MAX, d = lane - which * PYA_NTOP_MAX;
            if (d < ntop) {
                const uint32_t *r6 = b.rec + (size_t)(s0 + (which ? pe.idx : best_i)) * rec_words;
                const uint32_t cumd = (r6[d >> 1] >> ((d & 1) * 16)) & 0xffffu, nf = r6[rec_words - 1];
                g.sc[lane] = b.lut[b.lut_off[nf] + (uint32_t)d * (nf + 1) + cumd];
            }
        }
        gen_sync();
        const int depth = gen_pair_depth(g.sc, g.sc + PYA_NTOP_MAX, 1, ntop);
        float asc = 0.f;
        if (gen_ascore_pair(b, cfg, g, best_bits, pe.bits, depth, L, zmax, lc, list_cap, tab, R, &asc)) fail = 1;
        else if (lane == 0) g.site_asc[a] = asc < g.site_asc[a] ? asc : g.site_asc[a];
        gen_sync();
    }
    if (lane < k && lane < GEN_MAX_SITES) {
        float asc = g.site_asc[lane];
        if (g.site_tie[lane]) asc = 0.f < asc ? 0.f : asc;
        if (lane < (int)max_k) {
            out_asc[lane] = asc;
            out_alt[lane] = g.site_alt[lane];
        }
    }
    const bool any_fail = __any(fail != 0), overflow = __any(fail == 2);
    if (lane == 0) {
        b.best_score[psm] = best_ws;
        b.best_sig[psm] = best_bits;
        b.n_sig_out[psm] = N;
        if (any_fail) b.status[psm] = overflow ? PYA_ST_PUSHED_OVERFLOW : PYA_ST_LUT_RANGE;
    }
}

/* PyAscore.calculate_ambiguity (Ascore.pyx:208-230, Ascore.cpp:157-210) for PSM `psm` of a retained batch with the
 * caller's two score containers, without the fast kernels' limits: any peptide the general kernel takes, n_top up to
 * PYA_NTOP_MAX (`scores` = n_scores depth scores of the reference container, then n_scores of the other), a retained
 * table of any size (looked up where it lies in the workspace).  out[0] = the value, out[1] != 0: a list or a trial
 * count beyond the launch / the score table. */
__global__ __launch_bounds__(64) void pya_general_ambiguity_kernel(BatchDev b, uint32_t psm, uint32_t l_cap, uint32_t list_cap,
                                                                    uint64_t ref_bits, uint64_t oth_bits, const float *scores,
                                                                    uint32_t n_scores, float ref_ws, float oth_ws, float *out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int lane = lane_id();
    const DevConfig *cfg = b.cfg;
    const GenLds g = gen_carve(lds_raw, l_cap, list_cap);
    const uint32_t lc = (l_cap + 3u) & ~3u;
    if ((double)__builtin_fabsf(ref_ws - oth_ws) < 1e-6) {          /* Ascore.cpp:159-161 */
        if (lane == 0) {
            out[0] = 0.f;
            out[1] = 0.f;
        }
        return;
    }
    const int64_t pep0 = b.pep_off[psm];
    const int L = (int)(b.pep_off[psm + 1] - pep0);
    (void)gen_setup_residues(b, cfg, g, psm, pep0, L);
    const int depth = gen_pair_depth(scores, scores + n_scores, 1, (int)n_scores);
    float asc = 0.f;
    const int fail = gen_ascore_pair(b, cfg, g, ref_bits, oth_bits, depth, L, b.max_charge[psm], lc, list_cap,
                                     b.ret + b.ret_off[psm], (int)b.ret_n[psm], &asc);
    if (lane == 0) {
        out[0] = asc;
        out[1] = fail ? 1.f : 0.f;
    }
}

extern "C" size_t pya_general_lds_bytes(uint32_t l_cap, uint32_t list_cap) { return gen_lds_bytes(l_cap, list_cap); }
extern "C" size_t pya_general_scratch_bytes(uint32_t n_cap, uint32_t push_cap) {
    return ((sort_global_bytes(n_cap) + 15) & ~(size_t)15) + (size_t)push_cap * sizeof(PushedEntry) + 64;
}

/* d_scratch_off[n_ids]: the PSMs' slices of d_scratch, each pya_general_scratch_bytes(its site assignments, its k (n - k)
 * rounded up to a multiple of 4) long */
extern "C" int pya_launch_general(const BatchDev *b, const uint32_t *d_ids, uint32_t n_ids, unsigned char *d_scratch,
                                  const uint64_t *d_scratch_off, uint32_t l_cap, uint32_t list_cap, hipStream_t stream) {
    if (n_ids == 0) return 0;
    const size_t lds = gen_lds_bytes(l_cap, list_cap);
    hipError_t e = PYA_ENSURE_MAX_LDS(pya_general_psm_kernel);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(pya_general_psm_kernel, dim3(n_ids), dim3(64), lds, stream, *b, d_ids, n_ids, d_scratch, d_scratch_off,
                       l_cap, list_cap);
    return (int)hipGetLastError();
}

extern "C" int pya_launch_general_ambiguity(const BatchDev *b, uint32_t psm, uint32_t l_cap, uint32_t list_cap, uint64_t ref_bits,
                                            uint64_t oth_bits, const float *d_scores, uint32_t n_scores, float ref_ws, float oth_ws,
                                            float *d_out, hipStream_t stream) {
    const size_t lds = gen_lds_bytes(l_cap, list_cap);
    hipError_t e = PYA_ENSURE_MAX_LDS(pya_general_ambiguity_kernel);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(pya_general_ambiguity_kernel, dim3(1), dim3(64), lds, stream, *b, psm, l_cap, list_cap, ref_bits, oth_bits,
                       d_scores, n_scores, ref_ws, oth_ws, d_out);
    return (int)hipGetLastError();
}
