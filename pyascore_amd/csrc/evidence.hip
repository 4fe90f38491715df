/* evidence.hip -- what stands behind every Ascore of a scored plan: one 16-byte record (pya_evidence,
 * include/pyascore_hip.h) per (PSM, modified site of the winner), one PSM per wavefront, launched BEHIND a run.
 *
 * Nothing here is read by the scoring or localize kernels and no launch of a run changes: the kernel reads what the run
 * left -- the retained peak tables where they lie, the results (best_sig, alt_mask, ascores) -- and repeats, for the
 * handful of site assignments that matter, the reference's own steps:
 *   the competitors of site j                  alt_mask[j]: the single-move competitors that share the best PepScore
 *                                              of the site (cpp/Ascore.cpp:212-250, the test at :240)
 *   depth scores and PepScore of the winner    cpp/Ascore.cpp:53-139: one site assignment per lane -- lane 0 the winner,
 *   and of every competitor of the site        lane i the i-th competitor in position order -- counted into an LDS
 *                                              histogram (a column per lane) by gen_walk_assignment, scored from the
 *                                              host-built table by gen_pep_score (general_core.hip.h)
 *   a tie with the winner                      cpp/Ascore.cpp:159-161: PYA_EV_TIED, no ion is looked at
 *   the depth of the pair                      gen_pair_depth (cpp/Ascore.cpp:164-172), every lane its own
 *   site-determining ions, their matches       gen_ascore_pair (general_core.hip.h): both lists, ranked, the greedy walk
 *                                              of cpp/ModifiedPeptide.cpp:259-320 -- it ends with the four tallies on
 *                                              lane 0, one competitor after the other; the smallest Ascore, and among
 *                                              equal ones the smallest position, is the row (getAscores takes the minimum)
 * The code is the general route's (a peptide of any length the library takes, n_top up to 16, eight loss masses, a
 * retained table of any size): the same body serves the PSMs inside the fast kernels' limits, launched with the LDS
 * their own longest peptide and fragment list need, and the PSMs of the plan's general list with theirs.
 */
#include "general_core.hip.h"

#define EV_NONE 0u
#define EV_COUNTED 1u
#define EV_TIED 2u

/* behind the general route's LDS: hist[PYA_NTOP_MAX][64] counts per depth, a column per lane (later the lanes' depth
 * scores), rows[64] the records of the PSM, site_res[64] the residue of the j-th modifiable one */
__host__ __device__ static inline size_t ev_lds_bytes(uint32_t l_cap, uint32_t list_cap) {
    return gen_own_off(l_cap, list_cap) + PYA_NTOP_MAX * 64 * 4 + 64 * 16 + 64 * 2;
}

DEV uint4 ev_row(float comp_score, uint32_t comp_pos, uint32_t depth, uint32_t kind, uint32_t ref_m, uint32_t ref_p,
                 uint32_t comp_m, uint32_t comp_p) {
    return make_uint4(__float_as_uint(comp_score), (comp_pos & 0xffffu) | (depth & 0xffu) << 16 | kind << 24,
                      (ref_m & 0xffffu) | ref_p << 16, (comp_m & 0xffffu) | comp_p << 16);
}

/* ids == NULL: block i takes PSM i */
__global__ __launch_bounds__(64) void pya_evidence_kernel(BatchDev b, const uint32_t *ids, uint32_t n_ids, uint4 *out, uint32_t l_cap,
                                                           uint32_t list_cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    if (blockIdx.x >= n_ids) return;
    const uint32_t psm = ids ? ids[blockIdx.x] : blockIdx.x;
    const int lane = lane_id();
    const DevConfig *cfg = b.cfg;
    const GenLds g = gen_carve(lds_raw, l_cap, list_cap);
    const uint32_t lc = (l_cap + 3u) & ~3u;
    uint32_t *hist = (uint32_t *)(lds_raw + gen_own_off(l_cap, list_cap));
    float *scf = (float *)hist;
    uint4 *rows = (uint4 *)(hist + PYA_NTOP_MAX * 64);
    uint16_t *site_res = (uint16_t *)(rows + 64);

    const uint32_t max_k = b.max_k;
    uint4 *my_out = out + (size_t)psm * max_k;
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    rows[lane] = zero;

    /* PYA_EV_NONE for the whole PSM: not scored (set aside, rejected by a kernel, no site assignment) or unambiguous */
    const int N = b.status[psm] == PYA_ST_OK ? b.n_sig_out[psm] : -1;
    int L = 0, k = 0, n_sites = 0;
    if (N > 0) {
        const int64_t pep0 = b.pep_off[psm];
        L = (int)(b.pep_off[psm + 1] - pep0);
        k = b.n_of_mod[psm];
        if (L >= 1 && (uint32_t)L <= l_cap) n_sites = gen_setup_residues(b, cfg, g, psm, pep0, L);
    }
    if (!(N > 0 && k > 0 && k < n_sites && n_sites <= GEN_MAX_SITES)) {
        for (uint32_t a = lane; a < max_k; a += 64) my_out[a] = zero;
        return;
    }
    for (int i = lane; i < L; i += 64)
        if (g.sor[i] != 255) site_res[g.sor[i]] = (uint16_t)i;
    gen_sync();

    const int zmax = b.max_charge[psm];
    const uint64_t best_bits = b.best_sig[psm];
    const PeakEntry *tab = b.ret + b.ret_off[psm];
    const int R = (int)b.ret_n[psm];
    const int ntop = cfg->n_top;

    for (int a = 0; a < k && a < (int)max_k && a < 64; a++) {
        const float asc_out = b.ascores[(size_t)psm * max_k + a];
        const uint64_t alt = b.alt_mask[(size_t)psm * max_k + a];
        if (asc_out == __builtin_huge_valf() || alt == 0ull) continue;
        const int pos_a = nth_set_bit(best_bits, a);
        if (pos_a >= 64) continue;
        int nc = __popcll(alt);
        nc = nc > 63 ? 63 : nc;
        /* lane 0: the winner; lane i in 1 .. nc: the modification of site `a` moved to the i-th alternative position */
        const bool active = lane <= nc;
        uint64_t bits = best_bits;
        if (lane >= 1 && active) {
            const int bit = nth_set_bit(alt, lane - 1);
            const int sj = L <= 64 ? (int)g.sor[bit < L ? bit : 0] : bit;
            bits = (best_bits & ~(1ull << pos_a)) | (1ull << (sj & 63));
        }
        for (int d = 0; d < PYA_NTOP_MAX; d++) hist[d * 64 + lane] = 0u;

        /* ---- counts (gen_walk_assignment), then depth scores and PepScore (gen_pep_score): the lane's column turns from
         * counts into scores ---- */
        float ws = -1.f;
        bool in_table = true;
        if (active) {
            const uint32_t nfrag = gen_walk_assignment(g, cfg, bits, L, zmax, tab, R, [&](int rk) {
                if (rk < ntop) hist[rk * 64 + lane]++;
            });
            in_table = gen_pep_score(b, cfg, hist + lane, 64, nfrag, &ws, nullptr, scf + lane);
        }
        gen_sync();
        if (__any(!in_table)) continue;                             /* (the run would have rejected the PSM: not reached) */
        /* ---- the depth of every pair, every lane its own against the winner's column ---- */
        const int depth = gen_pair_depth(scf, scf + lane, 64, ntop);
        const float best_ws = __shfl(ws, 0, 64), comp_ws = __shfl(ws, 1, 64);
        const int first_bit = __builtin_ctzll(alt);
        if ((double)__builtin_fabsf(best_ws - comp_ws) < 1e-6) {   /* Ascore.cpp:159-161 */
            const uint32_t pos = (L <= 64 ? (uint32_t)first_bit : (uint32_t)site_res[first_bit]) + 1u;
            if (lane == 0) rows[a] = ev_row(comp_ws, pos, 0u, EV_TIED, 0u, 0u, 0u, 0u);
            continue;
        }
        uint4 best_row = zero;
        float best_asc = 0.f;
        bool have = false;
        for (int i = 1; i <= nc; i++) {
            const int bit = nth_set_bit(alt, i - 1);
            const int sj = (L <= 64 ? (int)g.sor[bit < L ? bit : 0] : bit) & 63;
            const uint64_t oth = (best_bits & ~(1ull << pos_a)) | (1ull << sj);
            const int dep = __shfl(depth, i, 64);
            float asc = 0.f;
            uint32_t tally[4] = {0u, 0u, 0u, 0u};
            const int fail = gen_ascore_pair(b, cfg, g, best_bits, oth, dep, L, zmax, lc, list_cap, tab, R, &asc, tally);
            if (!fail && lane == 0 && (!have || asc < best_asc)) {
                have = true;
                best_asc = asc;
                best_row = ev_row(comp_ws, (uint32_t)site_res[sj] + 1u, (uint32_t)dep, EV_COUNTED, tally[1], tally[0], tally[3], tally[2]);
            }
        }
        if (lane == 0) rows[a] = best_row;
    }
    gen_sync();
    for (uint32_t a = lane; a < max_k; a += 64) my_out[a] = a < 64u ? rows[a] : zero;
}

extern "C" size_t pya_evidence_lds_bytes(uint32_t l_cap, uint32_t list_cap) { return ev_lds_bytes(l_cap, list_cap); }

/* d_ids (n_ids PSM numbers) or NULL: the PSMs 0 .. n_ids - 1; d_out: [n_psm * b->max_k] records of 16 bytes */
extern "C" int pya_launch_evidence(const BatchDev *b, const uint32_t *d_ids, uint32_t n_ids, void *d_out, uint32_t l_cap, uint32_t list_cap,
                                   hipStream_t stream) {
    if (n_ids == 0) return 0;
    const size_t lds = ev_lds_bytes(l_cap, list_cap);
    hipError_t e = PYA_ENSURE_MAX_LDS(pya_evidence_kernel);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(pya_evidence_kernel, dim3(n_ids), dim3(64), lds, stream, *b, d_ids, n_ids, (uint4 *)d_out, l_cap, list_cap);
    return (int)hipGetLastError();
}
