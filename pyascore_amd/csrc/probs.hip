/* probs.hip -- site probabilities: the posterior over the site assignments of a PSM that their PepScores imply, summed per
 * modifiable residue (the two SUM-marginals where sites.hip takes the two max-marginals), one PSM per wavefront, launched
 * BEHIND a run like evidence.hip, named.hip and sites.hip.  The definition is in include/pyascore_hip.h (pya_site_prob,
 * pya_psm_prob); this is a PepScore-based posterior, MaxQuant's construction, and no part of the Ascore publication.
 *
 * Nothing here is read by a kernel of a run and no launch of a run changes: the kernel reads what the run left -- the
 * retained peak tables, best_score, n_sig, status, the host-built score table, the shape's signature list (order_tab +
 * order_off[psm]) -- and, per slice of 64 site assignments (one per lane, in list order):
 *   1. scores the slice            two front ends with the same float32 PepScores (the bits of the pep_scores records):
 *        count nodes                 probs_cnt.hip.h: the tables once per PSM, then k table reads per assignment, for a PSM
 *                                    under score_cnt.hip's conditions;
 *        general                     the lane-per-signature walk (gen_walk_assignment, general_core.hip.h: a binary search
 *                                    per fragment), for everything else and for every PSM under PYA_NO_PROB_CNT;
 *   2. weights                     w = exp2(((double)s - (double)best_score) * C) per lane, (w, bits) into LDS;
 *   3. reduces                     lane r owns residue r and walks the slice's 64 pairs IN INDEX ORDER with broadcast LDS
 *                                  reads, adding w to its with- or its without-accumulator (two doubles in registers,
 *                                  carried across the slices); lane 63, which owns no residue (at most 63 sites), takes
 *                                  every pair and so carries Z.  The sums are therefore sequential in list order: a host
 *                                  loop over the same w reproduces them bit for bit, whatever the route or the batch.
 *   4. after the last slice        divides; one 16-byte store per residue lane, one for the PSM's record.
 * The reduction issues two double adds per pair and wave (a quarter-rate class): 128 per slice beside
 * the slice's scoring -- DESIGN.md section 8 has the measured share.
 * The records of a PSM lie at site_off[psm] .. site_off[psm + 1], the offsets of the site stage; a PSM writes exactly that
 * range and its own pya_psm_prob, whatever it finds. */
#include "slice_score.hip.h"

#define PB_NONE 0u
#define PB_SCORED 1u
#define PB_OVER 2u
#define PB_C 0.33219280948873623      /* log2(10) / 10 */

/* behind whichever front end is larger (slice_score.hip.h): the slice's 64 (w, bits) pairs */
__host__ __device__ static inline size_t pb_lds_bytes(uint32_t l_cap, const PcCaps &caps, uint32_t sw) {
    return pb_front_bytes(l_cap, caps, sw) + 64 * (8 + 8);
}

DEV void pb_store_site(double2 *rec, double with_p, double without_p) { *rec = make_double2(with_p, without_p); }
DEV void pb_store_psm(uint4 *rec, double z, uint32_t n_summed, uint32_t kind) {
    const uint64_t zb = (uint64_t)__double_as_longlong(z);
    *rec = make_uint4((uint32_t)zb, (uint32_t)(zb >> 32), n_summed, kind);
}

/* ids == NULL: block i takes PSM i */
__global__ __launch_bounds__(64) void pya_probs_kernel(BatchDev b, const uint32_t *ids, uint32_t n_ids, const int64_t *site_off, uint64_t n_out,
                                                        uint32_t sig_cap, double2 *out, uint4 *psm_out, uint32_t l_cap, PcCaps caps, uint32_t sw) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    if (blockIdx.x >= n_ids) return;
    const uint32_t psm = ids ? ids[blockIdx.x] : blockIdx.x;
    const int lane = lane_id();
    uint4 *my_psm = psm_out + psm;
    const int64_t o0 = site_off[psm];
    int64_t n_rec64 = site_off[psm + 1] - o0;
    /* (no write at or past out + n_out: a range that does not lie inside is not written at all) */
    if (n_rec64 < 0 || o0 < 0 || (uint64_t)o0 > n_out || (uint64_t)n_rec64 > n_out - (uint64_t)o0) n_rec64 = -1;
    const int n_rec = (int)(n_rec64 < 0 ? 0 : (n_rec64 < 64 ? n_rec64 : 64));
    const bool mine = lane < n_rec;
    double2 *my_out = out + (n_rec64 > 0 ? o0 : 0) + lane;
    const DevConfig *cfg = b.cfg;

    const int64_t pep0 = b.pep_off[psm];
    const int L = (int)(b.pep_off[psm + 1] - pep0);
    /* PYA_SITE_NONE: not scored (set aside, rejected by a kernel, no site assignment); PYA_SITE_OVER: more than asked for */
    const int N_out = b.status[psm] == PYA_ST_OK ? b.n_sig_out[psm] : -1;
    const uint32_t N = b.n_sig[psm];
    const int k = b.n_of_mod[psm];
    const bool scored = n_rec64 >= 0 && n_rec64 < GEN_MAX_SITES && N_out > 0 && (uint32_t)N_out == N && k >= 0 && k <= n_rec && L >= 1 &&
                        (uint32_t)L <= l_cap;
    if (!scored) {
        for (int64_t s = lane; s < n_rec64; s += 64) pb_store_site(out + o0 + s, 0., 0.);
        if (lane == 0) pb_store_psm(my_psm, 0., 0u, PB_NONE);
        return;
    }
    if (sig_cap && N > sig_cap) {
        if (mine) pb_store_site(my_out, -1., -1.);
        if (lane == 0) pb_store_psm(my_psm, 0., 0u, PB_OVER);
        return;
    }
    const int zmax = b.max_charge[psm];
    const int64_t ret0 = b.ret_off[psm];
    const int R = (int)b.ret_n[psm];
    const bool use_cnt = (sw & PB_CNT) && pc_fits(cfg, caps, L, k, n_rec, zmax, R);
    unsigned char *tail = lds_raw + pb_front_bytes(l_cap, caps, sw);
    double *s_w = (double *)tail;
    uint64_t *s_bits = (uint64_t *)(tail + 64 * 8);

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
    /* (the host's offsets are made of the same count, and it launches the tables alone only where its own copy of pc_fits
     * passed every scored PSM of the list -- host_run.cpp: prob_lists --: not reached) */
    if (!ok) {
        if (mine) pb_store_site(my_out, 0., 0.);
        if (lane == 0) pb_store_psm(my_psm, 0., 0u, PB_NONE);
        return;
    }

    const uint64_t *order = b.order_tab + b.order_off[psm];
    const PeakEntry *tab = b.ret + ret0;
    const double best = (double)b.best_score[psm];
    const bool z_lane = lane == 63;                                  /* (owns no residue: n_rec <= 63) */
    double with = 0., without = 0.;
    bool bad = false;
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
            ws = pb_gen_score(b, cfg, g, hist, tab, R, L, zmax, bits, active, &bad);
        }
        /* ---- 2: its weight, the likelihood ratio 10^((s - s*) / 10) ---- */
        s_w[lane] = active ? exp2(((double)ws - best) * PB_C) : 0.;
        s_bits[lane] = bits;
        gen_sync();
        /* ---- 3: the reduction, sequential in list order; every pair is read by all lanes at once ---- */
        if (mine || z_lane) {
            for (int c = 0; c < n_slice; c++) {
                const double cw = s_w[c];
                const uint64_t cb = s_bits[c];
                if (z_lane || ((cb >> lane) & 1ull)) with += cw;
                else without += cw;
            }
        }
        gen_sync();
    }
    /* ---- 4: the records ---- */
    const double z = __shfl(with, 63, 64);
    if (bad || !(z > 0.)) {
        if (mine) pb_store_site(my_out, 0., 0.);
        if (lane == 0) pb_store_psm(my_psm, 0., 0u, PB_NONE);
        return;
    }
    if (mine) pb_store_site(my_out, with / z, without / z);
    if (lane == 0) pb_store_psm(my_psm, z, N, PB_SCORED);
}

extern "C" size_t pya_probs_lds_bytes(uint32_t l_cap, const PcCaps *caps, uint32_t sw) { return pb_lds_bytes(l_cap, *caps, sw); }
/* what score_cnt.hip needs for the same caps (the bound the count-node path keeps: that plus the 64 pairs) */
extern "C" size_t pya_probs_cnt_bytes(const PcCaps *caps) { return pc_lds_bytes(*caps); }

/* d_ids (n_ids PSM numbers) or NULL: the PSMs 0 .. n_ids - 1; d_site_off: [n_psm + 1] record offsets; d_out: n_out =
 * d_site_off[n_psm] records of 16 bytes; d_psms: [n_psm] records of 16 bytes; sig_cap 0: no cap; sw: PB_CNT | PB_GEN */
extern "C" int pya_launch_probs(const BatchDev *b, const uint32_t *d_ids, uint32_t n_ids, const int64_t *d_site_off, uint64_t n_out,
                                uint32_t sig_cap, void *d_out, void *d_psms, uint32_t l_cap, const PcCaps *caps, uint32_t sw, hipStream_t stream) {
    if (n_ids == 0) return 0;
    const size_t lds = pb_lds_bytes(l_cap, *caps, sw);
    hipError_t e = PYA_ENSURE_MAX_LDS(pya_probs_kernel);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(pya_probs_kernel, dim3(n_ids), dim3(64), lds, stream, *b, d_ids, n_ids, d_site_off, n_out, sig_cap, (double2 *)d_out,
                       (uint4 *)d_psms, l_cap, *caps, sw);
    return (int)hipGetLastError();
}
