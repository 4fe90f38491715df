/* mz_profile.hip -- fragment mass-error profile: the m/z errors of the matched fragments of the reported localisations,
 * binned in Da and in ppm over bands of m/z, into one table per caller-named run slot (pya_mz_profile, include/pyascore_hip.h).
 * Launched BEHIND a run like evidence.hip; no kernel of a run reads anything written here.  The reference has no counterpart.
 *
 * The ions are those of the ion stage's section 1 (ions.hip), without the emission: gen_setup_residues, then
 * ion_walk_winner (ion_match.hip.h).  Neither evidence rows nor fragment lists are needed, so the LDS is the general carve
 * with list_cap 0 plus ONE slot's table.
 *
 * A workgroup is one wavefront and takes PYA_MZP_CHUNK consecutive PSMs of its list, one after the other.  A matched ion is
 * two LDS atomic adds (its Da cell, its ppm cell).  The table in LDS belongs to the slot of the PSMs since the last flush:
 * when the next contributing PSM names another slot, and at the end of the chunk, every NON-ZERO word goes to the slot's
 * record in device memory with a device-scope atomicAdd and is cleared.  Word i of the record is lane i & 63's in trip
 * i >> 6, so a flush instruction covers 256 contiguous bytes with the zero words masked out.  A chunk of one run costs at
 * most 1 032 global atomics however many ions it had.  Every word is an integer count: the table is a function of the
 * multiset of matched ions, whatever order the atomics arrive in and however the PSMs were spread over chunks and calls.
 *
 * The arithmetic of a bin is the definition's, operation for operation, in double: one subtraction, one multiplication and
 * one division for ppm, one multiplication and a floor per axis; the three inverse widths are the caller's doubles.  This
 * file is compiled with -ffp-contract=off and without fast-math, so a host restatement does the same IEEE operations.
 * No write lies outside table[0 .. n_slots): a slot at or above n_slots is counted in over[0] (the smallest such PSM in
 * over[1] as 0xffffffff - psm) and nothing of it is written; a band below 0 (not reached: m/z is positive) is band 0. */
#include "ion_match.hip.h"
#include "../../include/pyascore_hip.h"

#define MZP_WORDS ((uint32_t)(sizeof(pya_mz_profile) / 4))
#define MZP_W_NPSM 0
#define MZP_W_NIONS 1
#define MZP_W_SKIPPED 2
#define MZP_W_OUT_DA 3
#define MZP_W_OUT_PPM 5
#define MZP_W_DA 8
#define MZP_W_PPM (MZP_W_DA + PYA_MZP_BANDS * PYA_MZP_BINS)
static_assert(sizeof(pya_mz_profile) == 4128 && MZP_W_PPM + PYA_MZP_BANDS * PYA_MZP_BINS == MZP_WORDS, "the record as words");

struct MzpArgs {
    const uint32_t *ids;              /* [n_ids] PSM numbers, or NULL: 0 .. n_ids - 1 */
    const int32_t *run;               /* [n_psm] or NULL: slot 0 */
    uint32_t *table;                  /* n_slots records of MZP_WORDS words */
    uint32_t *over;
    uint64_t n_slots;
    double inv_da, inv_ppm, inv_band;
    uint32_t n_ids, max_rank, l_cap;
};

__host__ __device__ static inline size_t mzp_lds_bytes(uint32_t l_cap) {
    return gen_own_off(l_cap, 0) + sizeof(pya_mz_profile);
}

/* the cell of x on an axis of PYA_MZP_BINS half-open bins around 0: floor(x) + BINS / 2, -1 below the axis, BINS at or above it */
DEV int mzp_bin(double x) {
    const double fl = __builtin_floor(x);
    if (!(fl >= -(double)(PYA_MZP_BINS / 2))) return -1;
    if (!(fl < (double)(PYA_MZP_BINS / 2))) return PYA_MZP_BINS;
    return (int)fl + PYA_MZP_BINS / 2;
}

DEV void mzp_count(uint32_t *hist, const MzpArgs &a, float theo, float peak) {
    const double t = (double)theo;
    const double d = (double)peak - t;
    const double scaled = d * 1e6;
    const double p = scaled / t;
    const double fb = __builtin_floor(t * a.inv_band);
    const int band = !(fb >= 0.) ? 0 : (!(fb < (double)(PYA_MZP_BANDS - 1)) ? PYA_MZP_BANDS - 1 : (int)fb);
    const int qd = mzp_bin(d * a.inv_da), qp = mzp_bin(p * a.inv_ppm);
    if (qd < 0) atomicAdd(&hist[MZP_W_OUT_DA], 1u);
    else if (qd >= PYA_MZP_BINS) atomicAdd(&hist[MZP_W_OUT_DA + 1], 1u);
    else atomicAdd(&hist[MZP_W_DA + band * PYA_MZP_BINS + qd], 1u);
    if (qp < 0) atomicAdd(&hist[MZP_W_OUT_PPM], 1u);
    else if (qp >= PYA_MZP_BINS) atomicAdd(&hist[MZP_W_OUT_PPM + 1], 1u);
    else atomicAdd(&hist[MZP_W_PPM + band * PYA_MZP_BINS + qp], 1u);
}

/* the non-zero words of the LDS table into the record of `slot` (inside the table: the caller has checked), cleared behind */
DEV void mzp_flush(uint32_t *hist, uint32_t *table, uint64_t slot) {
    gen_sync();
    uint32_t *rec = table + slot * MZP_WORDS;
    for (uint32_t i = (uint32_t)lane_id(); i < MZP_WORDS; i += 64) {
        const uint32_t v = hist[i];
        if (v) {
            atomicAdd(&rec[i], v);
            hist[i] = 0u;
        }
    }
    gen_sync();
}

__global__ __launch_bounds__(64) void pya_mz_profile_kernel(BatchDev b, const MzpArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int lane = lane_id();
    const DevConfig *cfg = b.cfg;
    const uint32_t l_cap = a.l_cap;
    const GenLds g = gen_carve(lds_raw, l_cap, 0);
    const uint32_t lc = (l_cap + 3u) & ~3u;
    uint32_t *hist = (uint32_t *)(lds_raw + gen_own_off(l_cap, 0));
    for (uint32_t i = (uint32_t)lane; i < MZP_WORDS; i += 64) hist[i] = 0u;
    gen_sync();

    const uint64_t first = (uint64_t)blockIdx.x * PYA_MZP_CHUNK;
    const uint64_t last = first + PYA_MZP_CHUNK < a.n_ids ? first + PYA_MZP_CHUNK : a.n_ids;
    int64_t held = -1;                                              /* the slot the LDS table belongs to; -1: it is empty */
    for (uint64_t at_id = first; at_id < last; at_id++) {
        const uint32_t psm = a.ids ? a.ids[at_id] : (uint32_t)at_id;
        const int N = b.status[psm] == PYA_ST_OK ? b.n_sig_out[psm] : -1;
        const int32_t slot = a.run ? a.run[psm] : 0;
        if (N <= 0 || slot < 0) continue;
        if ((uint64_t)slot >= a.n_slots) {
            if (lane == 0) report_over(a.over, psm);
            continue;
        }
        if (held >= 0 && held != (int64_t)slot) mzp_flush(hist, a.table, (uint64_t)held);
        held = (int64_t)slot;

        uint32_t n_ions = 0, n_skipped = 0;
        const int64_t pep0 = b.pep_off[psm];
        const int L = (int)(b.pep_off[psm + 1] - pep0);
        int n_sites = -1;
        if (L >= 1 && (uint32_t)L <= l_cap) n_sites = gen_setup_residues(b, cfg, g, psm, pep0, L);
        if (n_sites >= 0 && n_sites <= GEN_MAX_SITES) {
            const int zmax = b.max_charge[psm];
            const uint64_t best_bits = b.best_sig[psm];
            const PeakEntry *tab = b.ret + b.ret_off[psm];
            const int R = (int)b.ret_n[psm];
            ion_walk_winner(g, cfg, best_bits, L, zmax, lc, tab, R, [&](int, int, int, uint32_t, int, float f, int at, int rk) {
                const bool counted = at >= 0 && (uint32_t)rk <= a.max_rank;
                if (counted) mzp_count(hist, a, f, tab[at].mz);
                n_ions += (uint32_t)__popcll(__ballot(counted));
                n_skipped += (uint32_t)__popcll(__ballot(at >= 0 && !counted));
            });
            gen_sync();                                             /* (the next PSM's set-up overwrites the tables) */
        }
        if (lane == 0) {                                            /* (one wavefront: nobody else adds to these words) */
            hist[MZP_W_NPSM] += 1u;
            hist[MZP_W_NIONS] += n_ions;
            hist[MZP_W_SKIPPED] += n_skipped;
        }
    }
    if (held >= 0) mzp_flush(hist, a.table, (uint64_t)held);
}

extern "C" size_t pya_mz_profile_lds_bytes(uint32_t l_cap) { return mzp_lds_bytes(l_cap); }

/* d_ids (n_ids PSM numbers) or NULL: the PSMs 0 .. n_ids - 1; d_run: [n_psm] slots or NULL (slot 0); d_table: n_slots records
 * of pya_mz_profile, accumulated into; d_over: two words, zeroed by the caller */
extern "C" int pya_launch_mz_profile(const BatchDev *b, const uint32_t *d_ids, uint32_t n_ids, const int32_t *d_run, uint64_t n_slots,
                                     const pya_mz_profile_params *prm, void *d_table, uint32_t *d_over, uint32_t l_cap, hipStream_t stream) {
    if (n_ids == 0) return 0;
    hipError_t e = PYA_ENSURE_MAX_LDS(pya_mz_profile_kernel);
    if (e != hipSuccess) return (int)e;
    const MzpArgs a = {d_ids, d_run, (uint32_t *)d_table, d_over, n_slots, prm->inv_da, prm->inv_ppm, prm->inv_band, n_ids, prm->max_rank, l_cap};
    const uint32_t blocks = (n_ids + PYA_MZP_CHUNK - 1) / PYA_MZP_CHUNK;
    hipLaunchKernelGGL(pya_mz_profile_kernel, dim3(blocks), dim3(64), mzp_lds_bytes(l_cap), stream, *b, a);
    return (int)hipGetLastError();
}
