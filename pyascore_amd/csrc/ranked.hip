/* ranked.hip -- ranked localisations: the K best site assignments of a PSM by PepScore, the reported localisation first, one
 * PSM per wavefront, launched BEHIND a run like evidence.hip, named.hip, sites.hip and probs.hip.  The definition is in
 * include/pyascore_hip.h (pya_ranked); the reference has no counterpart but a sort of its pep_scores records.
 *
 * Nothing here is read by a kernel of a run and no launch of a run changes: the kernel reads what the run left -- the
 * retained peak tables, best_score, best_sig, n_sig, status, the host-built score table, the shape's signature list
 * (order_tab + order_off[psm]) -- and, per slice of 64 site assignments (one per lane, in list order):
 *   1. scores the slice            the two front ends of probs.hip (slice_score.hip.h), the float32 bits of the pep_scores
 *                                  records either way;
 *   2. selects                     the wave holds the list so far SORTED, lane j the j-th best (PepScore, bits) in registers;
 *                                  lane 0 is the reported localisation, seeded from best_sig / best_score and never moved
 *                                  (best_sig is skipped where the list names it).  The order of the others: PepScore
 *                                  descending as float32, equal floats by ascending bits -- a strict total order, so the
 *                                  list does not depend on the order the assignments arrive in.  One ballot finds the lanes
 *                                  whose assignment comes before lane K - 1's entry (an empty entry comes after everything);
 *                                  per set bit a wave-uniform insertion: the candidate is read from its lane (v_readlane),
 *                                  every lane compares it with its own entry, a ballot and a popcount give the position,
 *                                  the lanes behind it take their left neighbour's entry (__shfl_up) and lane K - 1's old
 *                                  entry falls off.  After the first slices the ballot is almost always empty.
 *   3. after the last slice        lane r < K writes row r, flags from a compare with the left neighbour: one 16-byte store.
 * The insertion runs in wave-uniform control flow with all 64 lanes active (the ballot mask is an SGPR pair).
 * A PSM writes exactly its K rows out[psm * K .. psm * K + K - 1], whatever it finds. */
#include "slice_score.hip.h"

#define RK_NONE 0u
#define RK_SCORED 1u
#define RK_OVER 2u
#define RK_TIED_PREV 1u
#define RK_IN_BEST_TIE 2u
#define RK_MAX 64u                    /* PYA_MAX_RANKED: a row per lane */

/* the stage keeps nothing of its own in LDS: the list lives in registers */
__host__ __device__ static inline size_t rk_lds_bytes(uint32_t l_cap, const PcCaps &caps, uint32_t sw) { return pb_front_bytes(l_cap, caps, sw); }

DEV void rk_store(uint4 *rec, uint64_t bits, float score, uint32_t rank, uint32_t kind, uint32_t flags) {
    *rec = make_uint4((uint32_t)bits, (uint32_t)(bits >> 32), __float_as_uint(score), (rank & 0xffffu) | kind << 16 | flags << 24);
}
DEV void rk_store_zero(uint4 *rec) { *rec = make_uint4(0u, 0u, 0u, 0u); }

/* does (sa, ba) come before (sb, bb)?  PepScore descending, equal floats by ascending bits */
DEV bool rk_before(float sa, uint64_t ba, float sb, uint64_t bb) { return sa > sb || (sa == sb && ba < bb); }

/* lane `src`'s value, src wave-uniform: v_readlane, no trip through the LDS crossbar */
DEV float rk_readlane_f32(float v, int src) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src)); }
DEV uint64_t rk_readlane64(uint64_t v, int src) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, src);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), src);
    return (uint64_t)hi << 32 | lo;
}

/* ids == NULL: block i takes PSM i */
__global__ __launch_bounds__(64) void pya_ranked_kernel(BatchDev b, const uint32_t *ids, uint32_t n_ids, const int64_t *site_off, uint32_t top_k,
                                                         uint32_t sig_cap, uint4 *out, uint32_t l_cap, PcCaps caps, uint32_t sw) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    if (blockIdx.x >= n_ids || top_k == 0u || top_k > RK_MAX) return;
    const uint32_t psm = ids ? ids[blockIdx.x] : blockIdx.x;
    const int lane = lane_id();
    const int K = (int)top_k;
    const bool row = lane < K;
    uint4 *my_out = out + (size_t)psm * top_k + (row ? lane : 0);
    const int64_t n_rec64 = site_off[psm + 1] - site_off[psm];       /* modifiable residues (the site stage's offsets) */
    const int n_rec = (int)(n_rec64 < 0 ? 0 : (n_rec64 < 64 ? n_rec64 : 64));
    const DevConfig *cfg = b.cfg;

    const int64_t pep0 = b.pep_off[psm];
    const int L = (int)(b.pep_off[psm + 1] - pep0);
    /* PYA_RANK_NONE: not scored (set aside, rejected by a kernel, no site assignment); PYA_RANK_OVER: more than asked for */
    const int N_out = b.status[psm] == PYA_ST_OK ? b.n_sig_out[psm] : -1;
    const uint32_t N = b.n_sig[psm];
    const int k = b.n_of_mod[psm];
    const bool scored = n_rec64 >= 0 && n_rec64 < GEN_MAX_SITES && N_out > 0 && (uint32_t)N_out == N && k >= 0 && k <= n_rec && L >= 1 &&
                        (uint32_t)L <= l_cap;
    if (!scored) {
        if (row) rk_store_zero(my_out);
        return;
    }
    const uint64_t best_bits = b.best_sig[psm];
    const float best = b.best_score[psm];
    if (sig_cap && N > sig_cap) {
        if (row) {
            if (lane == 0) rk_store(my_out, best_bits, best, 0u, RK_OVER, 0u);
            else rk_store_zero(my_out);
        }
        return;
    }
    const int zmax = b.max_charge[psm];
    const int64_t ret0 = b.ret_off[psm];
    const int R = (int)b.ret_n[psm];
    const bool use_cnt = (sw & PB_CNT) && pc_fits(cfg, caps, L, k, n_rec, zmax, R);

    bool ok = use_cnt || (sw & PB_GEN);
    PcPsm pc;
    GenLds g = {};
    uint32_t *hist = nullptr;
    if (use_cnt) {
        ok = pc_setup(b, psm, lds_raw, caps, ret0, R, k, n_rec, pc);
    } else if (ok) {
        g = gen_carve(lds_raw, l_cap, 0);
        hist = (uint32_t *)(lds_raw + gen_own_off(l_cap, 0));
        ok = gen_setup_residues(b, cfg, g, psm, pep0, L) == n_rec;
    }
    /* (the host launches the tables alone only where its own copy of pc_fits passed every scored PSM of the list --
     * host_run.cpp: prob_lists --: not reached) */
    if (!ok) {
        if (row) rk_store_zero(my_out);
        return;
    }

    const uint64_t *order = b.order_tab + b.order_off[psm];
    const PeakEntry *tab = b.ret + ret0;
    /* the list: lane 0 the reported localisation, every other lane empty (-inf comes after every PepScore) */
    float e_score = lane == 0 ? best : -INFINITY;
    uint64_t e_bits = lane == 0 ? best_bits : ~0ull;
    uint32_t n_list = 1u;                                            /* entries so far, the pinned one among them */
    bool bad = false, seen_best = false;
    for (uint32_t base = 0; base < N; base += 64u) {
        const uint32_t left = N - base;
        const int n_slice = (int)(left < 64u ? left : 64u);
        const bool active = lane < n_slice;
        const uint64_t bits = active ? order[base + (uint32_t)lane] : 0ull;
        /* ---- 1: the PepScore of the lane's assignment ---- */
        float ws;
        if (use_cnt) {
            ws = pc_score(b, pc, bits, active);
            bad = bad || __any(active && ws < 0.f);
        } else {
            ws = pb_gen_score(b, cfg, g, hist, tab, R, L, zmax, bits, active, &bad);   /* (a lane reads its own column only) */
        }
        const bool is_best = active && bits == best_bits;
        seen_best = seen_best || __any(is_best);
        /* ---- 2: the lanes that come before the K-th entry, and their insertions ---- */
        PYA_FULL_WAVE();                                             /* (readlane, ballot and __shfl_up below run through all 64 lanes) */
        float thr_s = rk_readlane_f32(e_score, K - 1);
        uint64_t thr_b = rk_readlane64(e_bits, K - 1);
        uint64_t todo = __ballot(active && !is_best && rk_before(ws, bits, thr_s, thr_b));
        while (todo) {
            const int c = __builtin_ctzll(todo);
            todo &= todo - 1ull;
            const float cs = rk_readlane_f32(ws, c);
            const uint64_t cb = rk_readlane64(bits, c);
            if (!rk_before(cs, cb, thr_s, thr_b)) continue;          /* (an earlier insertion of this slice moved the K-th entry) */
            /* the entries that stay in front of the candidate are a prefix of the lanes: lane 0 always */
            const int at = __popcll(__ballot(lane == 0 || rk_before(e_score, e_bits, cs, cb)));
            const float l_score = __shfl_up(e_score, 1, 64);
            const uint64_t l_bits = __shfl_up(e_bits, 1, 64);
            if (lane == at) {
                e_score = cs;
                e_bits = cb;
            } else if (lane > at) {
                e_score = l_score;
                e_bits = l_bits;
            }
            n_list += n_list < RK_MAX ? 1u : 0u;
            thr_s = rk_readlane_f32(e_score, K - 1);
            thr_b = rk_readlane64(e_bits, K - 1);
        }
    }
    /* ---- 3: the records ---- */
    /* (a list without best_sig, a fragment count without a row of the score table: the run would not have reported the PSM) */
    const float l_score = __shfl_up(e_score, 1, 64);
    if (bad || !seen_best) {
        if (row) rk_store_zero(my_out);
        return;
    }
    if (row) {
        if ((uint32_t)lane < n_list) {
            const uint32_t flags = (lane > 0 && e_score == l_score ? RK_TIED_PREV : 0u) | (e_score == best ? RK_IN_BEST_TIE : 0u);
            rk_store(my_out, e_bits, e_score, (uint32_t)lane, RK_SCORED, flags);
        } else {
            rk_store_zero(my_out);
        }
    }
}

extern "C" size_t pya_ranked_lds_bytes(uint32_t l_cap, const PcCaps *caps, uint32_t sw) { return rk_lds_bytes(l_cap, *caps, sw); }

/* d_ids (n_ids PSM numbers) or NULL: the PSMs 0 .. n_ids - 1; d_site_off: [n_psm + 1] offsets of the site stage (their
 * differences: the modifiable residues of a PSM); d_out: n_psm * top_k records of 16 bytes; sig_cap 0: no cap; sw: PB_CNT |
 * PB_GEN */
extern "C" int pya_launch_ranked(const BatchDev *b, const uint32_t *d_ids, uint32_t n_ids, const int64_t *d_site_off, uint32_t top_k,
                                 uint32_t sig_cap, void *d_out, uint32_t l_cap, const PcCaps *caps, uint32_t sw, hipStream_t stream) {
    if (n_ids == 0) return 0;
    if (top_k == 0u || top_k > RK_MAX) return (int)hipErrorInvalidValue;
    const size_t lds = rk_lds_bytes(l_cap, *caps, sw);
    hipError_t e = PYA_ENSURE_MAX_LDS(pya_ranked_kernel);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(pya_ranked_kernel, dim3(n_ids), dim3(64), lds, stream, *b, d_ids, n_ids, d_site_off, top_k, sig_cap, (uint4 *)d_out, l_cap,
                       *caps, sw);
    return (int)hipGetLastError();
}
