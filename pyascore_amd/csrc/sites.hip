/* sites.hip -- the site table of a PSM: one 32-byte record (pya_site, include/pyascore_hip.h) per modifiable residue, the
 * best PepScore among the site assignments that modify the residue and the best among those that leave it alone (the two
 * max-marginals), one PSM per wavefront, launched BEHIND a run like evidence.hip and named.hip.
 *
 * Nothing here is read by a kernel of a run and no launch of a run changes: the kernel reads what the run left -- the
 * retained peak tables where they lie, best_sig, n_sig, status, the host-built score table, the shape's signature list
 * (order_tab + order_off[psm], the list every route scores from) -- and repeats the reference's own steps for EVERY site
 * assignment of the PSM:
 *   the score container of a signature         cpp/Ascore.cpp:53-139, pb_gen_score (slice_score.hip.h) on the one walk and
 *                                              PepScore chain of general_core.hip.h:
 *                                              lane c of a slice owns signature base + c whole -- the float32 running sum
 *                                              (whose order fixes the bits), the neutral-loss state, every lookup of its
 *                                              fragments, its own column of a histogram [depth][64] in LDS.  All 64 lanes
 *                                              have a signature (the last slice apart), so no prefix table has to be handed
 *                                              from a lane that walks to lanes that look up, and no add is atomic.  Counts
 *                                              are integers and the m/z arithmetic of a fragment is the general kernel's,
 *                                              so the PepScore has the bits of the signature's pep_scores record.
 *   the reduction                              lane s owns residue s (at most 63 sites): after a slice the 64 (PepScore,
 *                                              bits) pairs lie in LDS, and the lane walks them with broadcast reads, keeping
 *                                              (max, smallest bits that attain it, whether best_sig attains it, whether more
 *                                              than one does) for the assignments with bit s and for those without, in
 *                                              registers across slices.  max and min do not depend on the order of the
 *                                              list, so nothing of the reference's std::sort is emulated.
 * There is no winner column, no tie test against the winner and no site-determining ion: gen_ascore_pair is not called, and
 * the lists of the general route's LDS are not carved (list_cap 0).
 * One body serves the PSMs inside the fast kernels' limits and the plan's general list, each launched with its own l_cap.
 * The records of a PSM lie at site_off[psm] .. site_off[psm + 1], offsets the host made from its pre-pass: a PSM writes
 * exactly that range, whatever it finds.
 */
#include "slice_score.hip.h"

#define ST_NONE 0u
#define ST_SCORED 1u
#define ST_OVER 2u
#define ST_IN_BEST 1u
#define ST_WITH_TIED 2u
#define ST_WITHOUT_TIED 4u
#define ST_NO_WITHOUT 8u

/* behind the general route's LDS without its lists: hist[PYA_NTOP_MAX][64] counts per depth, a column per lane, s_bits[64] /
 * s_score[64] the slice's signatures and PepScores, site_res[64] the residue of the j-th modifiable one */
__host__ __device__ static inline size_t st_lds_bytes(uint32_t l_cap) {
    return pb_gen_bytes(l_cap) + 64 * 8 + 64 * 4 + 64 * 2;
}

/* (max, arg, ties) of one of a residue's two sets, a register each */
struct StBest {
    float score;             /* -1: the set is empty so far (a PepScore is never negative) */
    uint64_t bits;           /* the smallest signature bits that attain `score` */
    uint32_t n;              /* how many attain it, saturating at 2 */
    bool has_best;           /* best_sig is one of them */
};
DEV void st_take(StBest &m, float sc, uint64_t bits, bool is_best) {
    if (sc > m.score) {
        m.score = sc;
        m.bits = bits;
        m.n = 1u;
        m.has_best = is_best;
    } else if (sc == m.score) {
        m.bits = bits < m.bits ? bits : m.bits;
        m.n = 2u;
        m.has_best = m.has_best || is_best;
    }
}

DEV void st_store(uint4 *rec, uint64_t with_sig, uint64_t without_sig, float with_score, float without_score, uint32_t pos,
                  uint32_t kind, uint32_t flags) {
    rec[0] = make_uint4((uint32_t)with_sig, (uint32_t)(with_sig >> 32), (uint32_t)without_sig, (uint32_t)(without_sig >> 32));
    rec[1] = make_uint4(__float_as_uint(with_score), __float_as_uint(without_score), (pos & 0xffffu) | kind << 16 | flags << 24, 0u);
}

/* ids == NULL: block i takes PSM i */
__global__ __launch_bounds__(64) void pya_sites_kernel(BatchDev b, const uint32_t *ids, uint32_t n_ids, const int64_t *site_off,
                                                        uint64_t n_out, uint32_t sig_cap, uint4 *out, uint32_t l_cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    if (blockIdx.x >= n_ids) return;
    const uint32_t psm = ids ? ids[blockIdx.x] : blockIdx.x;
    const int64_t o0 = site_off[psm];
    const int64_t n_rec64 = site_off[psm + 1] - o0;
    if (n_rec64 <= 0) return;                                        /* set aside, or no modifiable residue */
    if (o0 < 0 || (uint64_t)o0 > n_out || (uint64_t)n_rec64 > n_out - (uint64_t)o0) return;   /* (no write at or past out + n_out) */
    const int lane = lane_id();
    const int n_rec = (int)(n_rec64 < 64 ? n_rec64 : 64);
    const DevConfig *cfg = b.cfg;
    const GenLds g = gen_carve(lds_raw, l_cap, 0);
    uint32_t *hist = (uint32_t *)(lds_raw + gen_own_off(l_cap, 0));
    uint64_t *s_bits = (uint64_t *)(hist + PYA_NTOP_MAX * 64);
    float *s_score = (float *)(s_bits + 64);
    uint16_t *site_res = (uint16_t *)(s_score + 64);
    uint4 *my_out = out + 2 * (size_t)o0;
    const bool mine = lane < n_rec;

    const int64_t pep0 = b.pep_off[psm];
    const int L = (int)(b.pep_off[psm + 1] - pep0);
    int n_sites = -1;
    if (L >= 1 && (uint32_t)L <= l_cap) n_sites = gen_setup_residues(b, cfg, g, psm, pep0, L);
    /* (the host's offsets are made of the same count: anything else is not reached, and leaves zeroed records) */
    if (n_sites != (int)n_rec64 || n_sites >= GEN_MAX_SITES) {        /* (63 at most: a signature is keyed by a long) */
        for (int64_t s = lane; s < n_rec64; s += 64) st_store(out + 2 * (size_t)(o0 + s), 0ull, 0ull, 0.f, 0.f, 0u, ST_NONE, 0u);
        return;
    }
    for (int i = lane; i < L; i += 64)
        if (g.sor[i] != 255) site_res[g.sor[i]] = (uint16_t)i;
    gen_sync();
    const uint32_t pos = mine ? (uint32_t)site_res[lane] + 1u : 0u;

    /* PYA_SITE_NONE: not scored (rejected by a kernel, no site assignment); PYA_SITE_OVER: more assignments than asked for */
    const int N_out = b.status[psm] == PYA_ST_OK ? b.n_sig_out[psm] : -1;
    const uint32_t N = b.n_sig[psm];
    const int k = b.n_of_mod[psm];
    const uint64_t best_bits = b.best_sig[psm];
    const bool scored = N_out > 0 && (uint32_t)N_out == N && k >= 0 && k <= n_sites;
    const uint32_t in_best = scored && ((best_bits >> lane) & 1ull) ? ST_IN_BEST : 0u;
    if (!scored || (sig_cap && N > sig_cap)) {
        if (mine) st_store(my_out + 2 * lane, 0ull, 0ull, 0.f, 0.f, pos, scored ? ST_OVER : ST_NONE, in_best);
        return;
    }

    const int zmax = b.max_charge[psm];
    const uint64_t *order = b.order_tab + b.order_off[psm];
    const PeakEntry *tab = b.ret + b.ret_off[psm];
    const int R = (int)b.ret_n[psm];

    StBest with = {-1.f, 0ull, 0u, false}, without = {-1.f, 0ull, 0u, false};
    bool bad = false;
    for (uint32_t base = 0; base < N; base += 64u) {
        const uint32_t left = N - base;
        const int n_slice = (int)(left < 64u ? left : 64u);
        const bool active = lane < n_slice;
        const uint64_t bits = active ? order[base + (uint32_t)lane] : 0ull;
        /* ---- counts and PepScore (Ascore.cpp:53-139): the lane's signature, its own column; the chain that fills
         * pya_named.pep_score ---- */
        const float ws = pb_gen_score(b, cfg, g, hist, tab, R, L, zmax, bits, active, &bad);
        s_bits[lane] = bits;
        s_score[lane] = ws;
        gen_sync();
        /* ---- the reduction: lane s and the slice's pairs, each read by every lane at once ---- */
        if (mine) {
            for (int c = 0; c < n_slice; c++) {
                const uint64_t cb = s_bits[c];
                const float cs = s_score[c];
                if ((cb >> lane) & 1ull) st_take(with, cs, cb, cb == best_bits);
                else st_take(without, cs, cb, cb == best_bits);
            }
        }
        gen_sync();
    }
    /* ---- the records: two 16-byte stores each ---- */
    if (mine) {
        if (bad) {
            st_store(my_out + 2 * lane, 0ull, 0ull, 0.f, 0.f, pos, ST_NONE, 0u);
        } else {
            uint32_t flags = in_best;
            if (with.n > 1u) flags |= ST_WITH_TIED;
            if (without.n > 1u) flags |= ST_WITHOUT_TIED;
            if (without.n == 0u) flags |= ST_NO_WITHOUT;
            const uint64_t with_sig = with.n == 0u ? 0ull : (with.has_best ? best_bits : with.bits);
            const uint64_t without_sig = without.n == 0u ? 0ull : (without.has_best ? best_bits : without.bits);
            st_store(my_out + 2 * lane, with_sig, without_sig, with.score, without.score, pos, ST_SCORED, flags);
        }
    }
}

extern "C" size_t pya_sites_lds_bytes(uint32_t l_cap, uint32_t list_cap) {
    (void)list_cap;                                                  /* (no fragment list is kept: the stage sorts nothing) */
    return st_lds_bytes(l_cap);
}

/* d_ids (n_ids PSM numbers) or NULL: the PSMs 0 .. n_ids - 1; d_site_off: [n_psm + 1] record offsets; d_out: n_out =
 * d_site_off[n_psm] records of 32 bytes; sig_cap 0: no cap */
extern "C" int pya_launch_sites(const BatchDev *b, const uint32_t *d_ids, uint32_t n_ids, const int64_t *d_site_off, uint64_t n_out,
                                uint32_t sig_cap, void *d_out, uint32_t l_cap, hipStream_t stream) {
    if (n_ids == 0) return 0;
    const size_t lds = st_lds_bytes(l_cap);
    hipError_t e = PYA_ENSURE_MAX_LDS(pya_sites_kernel);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(pya_sites_kernel, dim3(n_ids), dim3(64), lds, stream, *b, d_ids, n_ids, d_site_off, n_out, sig_cap, (uint4 *)d_out,
                       l_cap);
    return (int)hipGetLastError();
}
