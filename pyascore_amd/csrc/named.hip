/* named.hip -- localisations the CALLER names: one 32-byte record (pya_named, include/pyascore_hip.h) per (PSM, queried
 * signature), the queries a CSR list per PSM, one PSM per wavefront, launched BEHIND a run like evidence.hip.
 *
 * Nothing here is read by a kernel of a run and no launch of a run changes: the kernel reads what the run left -- the
 * retained peak tables where they lie, best_sig, n_sig, status, the host-built score table -- and the query arrays, and
 * repeats the reference's own steps for the winner and the signatures asked for:
 *   the score container of a signature         cpp/Ascore.cpp:53-139.  The only sequential piece of a signature's count is
 *                                              the float32 running sum (whose order fixes the bits) and the neutral-loss
 *                                              state: gen_prefix_table (general_core.hip.h) makes both for TWO signatures
 *                                              at a time, one per lane, into the two slots of the general route's LDS; the
 *                                              independent lookups -- slot x prefix x ion type x charge, the loss variants
 *                                              inside -- are then spread over the 64 lanes, LDS atomic adds into the
 *                                              signature's column of a histogram [depth][64].  Counts are integers and the
 *                                              m/z arithmetic of a fragment is the general kernel's, so the order of the
 *                                              lookups changes no bit.
 *   a tie with the winner                      cpp/Ascore.cpp:159-161: PYA_NAMED_TIED, no ion is looked at
 *   the depth of the pair                      gen_pair_depth (cpp/Ascore.cpp:164-172), every lane its own column against column 0
 *   site-determining ions, their matches       gen_ascore_pair as it is, for any number of moved modifications
 * Queries go through in slices: column 0 is the winner, counted once per PSM, columns 1 .. 63 the slice's queries.
 * The code is the general route's, so one body serves the PSMs inside the fast kernels' limits and the plan's general list,
 * each launched with its own l_cap / list_cap (evidence.hip does the same).
 * No write lies at or past out + n_q: a PSM whose query range is not inside [0, n_q] writes nothing and is reported through
 * over[] (count, 0xffffffff - the smallest such PSM), as the ion fill reports a PSM that passes its cap.
 */
#include "general_core.hip.h"

#define NM_NONE 0u
#define NM_INVALID 1u
#define NM_WINNER 2u
#define NM_TIED 3u
#define NM_COUNTED 4u
#define NM_NO_COL 255u

/* behind the general route's LDS: hist[PYA_NTOP_MAX][64] counts per depth, a column per signature (cumulative once the
 * column is scored), scf[PYA_NTOP_MAX][64] the columns' depth scores, col_of[64] the column a slice's record reads */
__host__ __device__ static inline size_t nm_lds_bytes(uint32_t l_cap, uint32_t list_cap) {
    return gen_own_off(l_cap, list_cap) + 2 * PYA_NTOP_MAX * 64 * 4 + 64;
}

/* ids == NULL: block i takes PSM i */
__global__ __launch_bounds__(64) void pya_named_kernel(BatchDev b, const uint32_t *ids, uint32_t n_ids, const int64_t *q_off,
                                                        const uint64_t *q_bits, uint64_t n_q, uint4 *out, int32_t *counts_out,
                                                        float *scores_out, uint32_t *over, uint32_t l_cap, uint32_t list_cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    if (blockIdx.x >= n_ids) return;
    const uint32_t psm = ids ? ids[blockIdx.x] : blockIdx.x;
    const int64_t q0 = q_off[psm], q1 = q_off[psm + 1];
    if (q1 == q0) return;                                            /* (the common PSM of a sparse query list) */
    const int lane = lane_id();
    if (q0 < 0 || q1 < q0 || (uint64_t)q1 > n_q) {                   /* nothing of the PSM is written */
        if (lane == 0) report_over(over, psm);
        return;
    }
    const DevConfig *cfg = b.cfg;
    const GenLds g = gen_carve(lds_raw, l_cap, list_cap);
    const uint32_t lc = (l_cap + 3u) & ~3u;
    uint32_t *hist = (uint32_t *)(lds_raw + gen_own_off(l_cap, list_cap));
    float *scf = (float *)(hist + PYA_NTOP_MAX * 64);
    uint8_t *col_of = (uint8_t *)(scf + PYA_NTOP_MAX * 64);
    const int ntop = cfg->n_top;

    /* PYA_NAMED_NONE for every query of the PSM: not scored (set aside, rejected by a kernel, no site assignment) */
    const int N = b.status[psm] == PYA_ST_OK ? b.n_sig_out[psm] : -1;
    const int64_t pep0 = b.pep_off[psm];
    const int L = (int)(b.pep_off[psm + 1] - pep0);
    int n_sites = -1;
    if (N > 0 && L >= 1 && (uint32_t)L <= l_cap) n_sites = gen_setup_residues(b, cfg, g, psm, pep0, L);
    const bool scored = n_sites >= 0 && n_sites <= GEN_MAX_SITES;

    const int k = b.n_of_mod[psm];
    const int zmax = b.max_charge[psm];
    const uint64_t best_bits = b.best_sig[psm];
    const PeakEntry *tab = b.ret + b.ret_off[psm];
    const int R = scored ? (int)b.ret_n[psm] : 0;
    const float err = cfg->mz_error;
    const bool half_check = err > 0.49f;
    const int T = cfg->n_types, n_fwd = cfg->n_fwd;
    const uint64_t types64 = load_types64(cfg);

    uint32_t win_nfrag = 0;
    float win_ws = -1.f;
    bool win_ok = false;
    for (int64_t base = q0; base < q1; base += 63) {
        const int n_slice = (int)(q1 - base < 63 ? q1 - base : 63);
        const bool first = base == q0;
        const bool mine = lane >= 1 && lane <= n_slice;
        const uint64_t bits = mine ? q_bits[base + lane - 1] : best_bits;
        uint32_t kind = NM_NONE;
        if (mine && scored) {
            const bool in_range = n_sites >= 64 || (bits >> n_sites) == 0ull;
            kind = bits == best_bits ? NM_WINNER : (__popcll(bits) == k && in_range ? NM_COUNTED : NM_INVALID);
        }
        /* the columns to count: the slice's valid queries, and the winner once */
        const bool count_me = kind == NM_COUNTED || (lane == 0 && first && scored);
        for (int d = 0; d < PYA_NTOP_MAX; d++)
            if (lane != 0 || first) hist[d * 64 + lane] = 0u;
        uint32_t nfrag = 0;

        /* ---- counts (Ascore.cpp:53-121): two signatures' prefix tables, then every lane its share of the lookups ---- */
        uint64_t todo = __ballot(count_me);
        while (todo) {
            const int ca = __builtin_ctzll(todo);
            todo &= todo - 1;
            const int cb = todo ? __builtin_ctzll(todo) : -1;
            if (todo) todo &= todo - 1;
            const uint64_t bits_a = (uint64_t)__shfl((long long)bits, ca, 64);
            const uint64_t bits_b = (uint64_t)__shfl((long long)bits, cb < 0 ? ca : cb, 64);
            const int n_slots = cb < 0 ? 1 : 2;
            uint32_t nf_a = 0, nf_b = 0;
            for (int dir = 0; dir < 2; dir++) {
                const int t0 = dir ? n_fwd : 0, t1 = dir ? T : n_fwd;
                if (t0 == t1) continue;
                gen_sync();
                uint32_t n = 0;
                if (lane < n_slots) n = gen_prefix_table(g, cfg, lane ? bits_b : bits_a, L, dir, lane, lc);
                gen_sync();
                const uint32_t per_pair = (uint32_t)(t1 - t0) * (uint32_t)zmax;
                nf_a += (uint32_t)__shfl((int)n, 0, 64) * per_pair;
                nf_b += (uint32_t)__shfl((int)n, 1, 64) * per_pair;
                const int per_slot = (L - 1) * (int)per_pair;
                for (int i = lane; i < n_slots * per_slot; i += 64) {
                    const int slot = i >= per_slot ? 1 : 0;
                    int r = i - slot * per_slot;
                    const int step = r / (int)per_pair;
                    r -= step * (int)per_pair;
                    const int t = t0 + r / zmax, z = 1 + r % zmax;
                    const int col = slot ? cb : ca;
                    const float running = g.run[slot * lc + step];
                    uint64_t pm = g.pm[slot * lc + step];
                    double A, B;
                    type_constants(type_at(types64, t), &A, &B);
                    while (pm) {
                        const int v = __builtin_ctzll(pm);
                        pm &= pm - 1;
                        const float x = running - (cfg->n_nl ? g.uniq[v] : 0.f);
                        const double m = ((double)x + A) - B;
                        const int rk = gen_match_rank(tab, R, charge_mz(m, z), err, half_check);
                        if (rk < ntop) atomicAdd(&hist[rk * 64 + col], 1u);
                    }
                }
            }
            if (lane == ca) nfrag = nf_a;
            if (lane == cb) nfrag = nf_b;
        }
        gen_sync();
        /* ---- depth scores and PepScore (gen_pep_score): the column's counts become cumulative, scf takes the scores ---- */
        float ws = -1.f;
        const bool in_table = !count_me || gen_pep_score(b, cfg, hist + lane, 64, nfrag, &ws, hist + lane, scf + lane);
        if (first) {
            win_nfrag = (uint32_t)__shfl((int)nfrag, 0, 64);
            win_ws = __shfl(ws, 0, 64);
            win_ok = __shfl((int)(count_me && in_table), 0, 64) != 0;
        }
        gen_sync();
        /* (a container the score table does not reach, the winner's or the query's: the run would have rejected the PSM) */
        if (kind == NM_WINNER && !win_ok) kind = NM_NONE;
        if (kind == NM_COUNTED && !(in_table && win_ok)) kind = NM_NONE;
        if (kind == NM_WINNER) {
            nfrag = win_nfrag;
            ws = win_ws;
        }
        /* ---- the depth of every pair (Ascore.cpp:164-172), the tie (:159-161) ---- */
        int depth = 0;
        if (kind == NM_COUNTED) {
            depth = gen_pair_depth(scf, scf + lane, 64, ntop);
            if ((double)__builtin_fabsf(win_ws - ws) < 1e-6) {
                kind = NM_TIED;
                depth = 0;
            }
        }
        /* ---- Ascore::calculateAmbiguity's second half, one counted query after the other; the values are lane 0's ---- */
        float amb = 0.f;
        uint32_t tl0 = 0, tl1 = 0, tl2 = 0, tl3 = 0;
        uint64_t pairs = __ballot(kind == NM_COUNTED);
        while (pairs) {
            const int c = __builtin_ctzll(pairs);
            pairs &= pairs - 1;
            const uint64_t oth = (uint64_t)__shfl((long long)bits, c, 64);
            const int dep = __shfl(depth, c, 64);
            float asc = 0.f;
            uint32_t tally[4] = {0u, 0u, 0u, 0u};
            const int fail = gen_ascore_pair(b, cfg, g, best_bits, oth, dep, L, zmax, lc, list_cap, tab, R, &asc, tally);
            const float asc0 = __shfl(asc, 0, 64);
            const uint32_t a0 = (uint32_t)__shfl((int)tally[0], 0, 64), a1 = (uint32_t)__shfl((int)tally[1], 0, 64);
            const uint32_t a2 = (uint32_t)__shfl((int)tally[2], 0, 64), a3 = (uint32_t)__shfl((int)tally[3], 0, 64);
            if (lane == c) {
                if (fail) {
                    kind = NM_NONE;                                 /* (a list beyond the launch's caps: not reached) */
                } else {
                    amb = asc0;
                    tl0 = a0;
                    tl1 = a1;
                    tl2 = a2;
                    tl3 = a3;
                }
            }
        }
        /* ---- the records: two 16-byte stores each, then the rows of the two optional arrays ---- */
        const bool has_container = kind >= NM_WINNER;
        col_of[lane] = (uint8_t)(has_container ? (kind == NM_WINNER ? 0u : (uint32_t)lane) : NM_NO_COL);
        if (mine) {
            const uint32_t moved = has_container ? (uint32_t)(k - __popcll(bits & best_bits)) : 0u;
            const uint32_t dep8 = kind == NM_COUNTED ? (uint32_t)depth & 0xffu : 0u;
            uint4 *rec = out + 2 * (size_t)(base + lane - 1);
            rec[0] = make_uint4((uint32_t)bits, (uint32_t)(bits >> 32), has_container ? __float_as_uint(ws) : 0u,
                                kind == NM_COUNTED ? __float_as_uint(amb) : 0u);
            rec[1] = make_uint4(has_container ? nfrag : 0u, kind | dep8 << 8 | (moved & 0xffu) << 16, (tl1 & 0xffffu) | tl0 << 16,
                                (tl3 & 0xffffu) | tl2 << 16);
        }
        gen_sync();
        if (counts_out || scores_out) {
            for (int i = lane; i < n_slice * ntop; i += 64) {
                const int q = i / ntop, d = i - q * ntop;
                const uint32_t col = col_of[q + 1];
                const size_t at = (size_t)(base + q) * (size_t)ntop + (size_t)d;
                if (counts_out) counts_out[at] = col == NM_NO_COL ? 0 : (int32_t)hist[d * 64 + col];
                if (scores_out) scores_out[at] = col == NM_NO_COL ? 0.f : scf[d * 64 + col];
            }
        }
        gen_sync();
    }
}

extern "C" size_t pya_named_lds_bytes(uint32_t l_cap, uint32_t list_cap) { return nm_lds_bytes(l_cap, list_cap); }

/* d_ids (n_ids PSM numbers) or NULL: the PSMs 0 .. n_ids - 1; d_out: n_q records of 32 bytes; d_counts / d_scores: NULL or
 * n_q rows of n_top; d_over: two words, zeroed by the caller */
extern "C" int pya_launch_named(const BatchDev *b, const uint32_t *d_ids, uint32_t n_ids, const int64_t *d_q_off, const uint64_t *d_q_bits,
                                uint64_t n_q, void *d_out, int32_t *d_counts, float *d_scores, uint32_t *d_over, uint32_t l_cap,
                                uint32_t list_cap, hipStream_t stream) {
    if (n_ids == 0) return 0;
    const size_t lds = nm_lds_bytes(l_cap, list_cap);
    hipError_t e = PYA_ENSURE_MAX_LDS(pya_named_kernel);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(pya_named_kernel, dim3(n_ids), dim3(64), lds, stream, *b, d_ids, n_ids, d_q_off, d_q_bits, n_q, (uint4 *)d_out,
                       d_counts, d_scores, d_over, l_cap, list_cap);
    return (int)hipGetLastError();
}
