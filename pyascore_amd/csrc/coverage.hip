/* coverage.hip -- explained ion current: per PSM, how much of its spectrum the reported localisation explains, one 64-byte
 * record (pya_coverage, include/pyascore_hip.h).  Launched BEHIND a run like evidence.hip and mz_profile.hip; no kernel of a
 * run reads anything written here.  The reference has no counterpart.
 *
 * A workgroup is one wavefront and takes one PSM.  Three phases:
 *   1  the winner's matched fragments, the walk the ion stage's section 1 and mz_profile.hip take: gen_setup_residues, then
 *      ion_walk_winner (ion_match.hip.h).  A match ORs bit `at` (the table index of its peak) into one of two bit planes over the retained
 *      table -- forward types, backward types -- and bit `size` into one of two size planes, all in LDS (ds_or).
 *   2  the lanes stride the RAW peaks of the PSM's spectrum: (float)mz is looked up in the retained table (lower bound, then
 *      the run of equal entries), the plane bits of those entries say explained / N-terminal / C-terminal, and the intensity
 *      goes into four double accumulators by select -- + 0.0 where the peak is outside the set.
 *   3  the 64 partials of each sum go through LDS and are added in lane order by one lane per sum; lane 0 turns the size
 *      planes into the five 16-bit fields; the record goes out as four 16-byte stores.
 * The sums are in the order of the definition and nothing else: no float atomics, no butterfly.  This file is compiled with
 * -ffp-contract=off and without fast-math.  Every LDS index is bounded: a table index at or above the plane's room and a
 * size above PYA_MAX_PEPTIDE_LEN set no bit (neither is reached: retained <= raw <= peak_cap, size < L <= l_cap). */
#include "ion_match.hip.h"
#include "../../include/pyascore_hip.h"

#define COV_SIZE_WORDS 16u                                  /* bits 0 .. 511: sizes 1 .. L - 1, L <= PYA_MAX_PEPTIDE_LEN */
static_assert(PYA_MAX_PEPTIDE_LEN <= 32 * COV_SIZE_WORDS - 1, "a size plane holds every fragment size");
static_assert(sizeof(pya_coverage) == 64 && offsetof(pya_coverage, explained_current) == 8 && offsetof(pya_coverage, nterm_current) == 16 &&
                  offsetof(pya_coverage, cterm_current) == 24 && offsetof(pya_coverage, n_peaks) == 32 && offsetof(pya_coverage, n_retained) == 36 &&
                  offsetof(pya_coverage, n_explained) == 40 && offsetof(pya_coverage, n_fragments) == 44 && offsetof(pya_coverage, nterm_sizes) == 48 &&
                  offsetof(pya_coverage, cterm_sizes) == 50 && offsetof(pya_coverage, nterm_run) == 52 && offsetof(pya_coverage, cterm_run) == 54 &&
                  offsetof(pya_coverage, bonds) == 56 && offsetof(pya_coverage, kind) == 58 && offsetof(pya_coverage, pad) == 59,
              "pya_coverage is the four 16-byte stores of this kernel");

struct CovArgs {
    const uint32_t *ids;              /* [n_ids] PSM numbers, or NULL: 0 .. n_ids - 1 */
    const uint32_t *spec_of;          /* [n_psm] the spectrum of every PSM (~0u: set aside), or NULL: its own */
    uint4 *out;                       /* [n_psm] records of four 16-byte words */
    uint32_t n_ids, l_cap, peak_cap;
};

/* words of one bit plane over a retained table of at most peak_cap peaks */
__host__ __device__ static inline uint32_t cov_plane_words(uint32_t peak_cap) { return (peak_cap + 31u) >> 5; }

/* the general carve without lists | two size planes | 4 x 64 partial sums | two planes over the retained table */
__host__ __device__ static inline size_t cov_lds_bytes(uint32_t l_cap, uint32_t peak_cap) {
    return gen_own_off(l_cap, 0) + 2 * COV_SIZE_WORDS * 4 + 4 * 64 * 8 + 2 * (size_t)cov_plane_words(peak_cap) * 4;
}

/* the longest run of consecutive set bits among bits 1 .. hi of a size plane, and how many are set (one lane) */
DEV uint32_t cov_sizes(const uint32_t *plane, int hi, uint32_t *longest) {
    uint32_t n = 0, run = 0, best = 0;
    for (int s = 1; s <= hi; s++) {
        const bool set = (plane[s >> 5] >> (s & 31)) & 1u;
        run = set ? run + 1u : 0u;
        best = run > best ? run : best;
        n += set ? 1u : 0u;
    }
    *longest = best;
    return n;
}

template <typename MZ, typename IT>
__global__ __launch_bounds__(64) void pya_coverage_kernel(BatchDev b, const CovArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    if (blockIdx.x >= a.n_ids) return;
    const uint32_t psm = a.ids ? a.ids[blockIdx.x] : blockIdx.x;
    const int lane = lane_id();
    const DevConfig *cfg = b.cfg;
    const uint32_t l_cap = a.l_cap;
    const GenLds g = gen_carve(lds_raw, l_cap, 0);
    const uint32_t lc = (l_cap + 3u) & ~3u;
    uint32_t *size_pl = (uint32_t *)(lds_raw + gen_own_off(l_cap, 0));    /* [2][COV_SIZE_WORDS] */
    double *part = (double *)(size_pl + 2 * COV_SIZE_WORDS);                                        /* [4][64] */
    uint32_t *peak_pl = (uint32_t *)(part + 4 * 64);                                                /* [2][pw] */
    const uint32_t pw = cov_plane_words(a.peak_cap);
    uint4 *rec = a.out + (size_t)psm * 4;

    /* PYA_COV_NONE: not scored (set aside, rejected by a kernel, no site assignment) */
    const int N = b.status[psm] == PYA_ST_OK ? b.n_sig_out[psm] : -1;
    const uint32_t spec = a.spec_of ? a.spec_of[psm] : psm;
    if (N <= 0 || spec == 0xffffffffu) {
        if (lane < 4) rec[lane] = make_uint4(0u, 0u, 0u, 0u);
        return;
    }
    const PeakEntry *tab = b.ret + b.ret_off[psm];
    const int R = (int)b.ret_n[psm];
    const uint32_t r_words = ((uint32_t)R + 31u) >> 5 < pw ? ((uint32_t)R + 31u) >> 5 : pw;
    for (uint32_t i = (uint32_t)lane; i < 2 * COV_SIZE_WORDS; i += 64) size_pl[i] = 0u;
    for (uint32_t i = (uint32_t)lane; i < r_words; i += 64) {
        peak_pl[i] = 0u;
        peak_pl[pw + i] = 0u;
    }
    gen_sync();

    /* ---- phase 1: the winner's matched fragments into the planes ---- */
    const int64_t pep0 = b.pep_off[psm];
    const int L = (int)(b.pep_off[psm + 1] - pep0);
    uint32_t n_frag = 0;
    int n_sites = -1;
    if (L >= 1 && (uint32_t)L <= l_cap && L <= PYA_MAX_PEPTIDE_LEN) n_sites = gen_setup_residues(b, cfg, g, psm, pep0, L);
    const bool walked = n_sites >= 0 && n_sites <= GEN_MAX_SITES;   /* (otherwise: not reached by a scored PSM; no fragments) */
    if (walked) {
        ion_walk_winner(g, cfg, b.best_sig[psm], L, b.max_charge[psm], lc, tab, R, [&](int dir, int step, int, uint32_t, int, float, int at, int) {
            const uint32_t size = (uint32_t)(step + 1);
            if (at >= 0) {
                if (((uint32_t)at >> 5) < r_words) atomicOr(&peak_pl[dir * pw + ((uint32_t)at >> 5)], 1u << ((uint32_t)at & 31u));
                if (size < 32u * COV_SIZE_WORDS) atomicOr(&size_pl[dir * COV_SIZE_WORDS + (size >> 5)], 1u << (size & 31u));
            }
            n_frag += (uint32_t)__popcll(__ballot(at >= 0));
        });
    }
    gen_sync();

    /* ---- phase 2: the raw peaks against the planes ---- */
    const int64_t p0 = b.peak_off[spec];
    const int64_t np64 = b.peak_off[spec + 1] - p0;
    const uint32_t n_peaks = np64 > 0 ? (uint32_t)np64 : 0u;
    const MZ *mz = (const MZ *)b.mz + p0;
    const IT *inten = (const IT *)b.inten + p0;
    double s_tot = 0.0, s_exp = 0.0, s_fwd = 0.0, s_bwd = 0.0;
    uint32_t n_expl = 0;
    for (uint32_t i0 = 0; i0 < n_peaks; i0 += 64) {
        const uint32_t i = i0 + (uint32_t)lane;
        const bool live = i < n_peaks;
        bool fwd = false, bwd = false;
        double y = 0.0;
        if (live) {
            const float x = (float)mz[i];
            y = (double)inten[i];
            int lo = 0, hi = R;
            while (lo < hi) {                                       /* first entry not below x (a NaN x: entry 0, which is not equal) */
                const int m = (lo + hi) >> 1;
                if (tab[m].mz < x) lo = m + 1;
                else hi = m;
            }
            for (int j = lo; j < R && tab[j].mz == x; j++) {
                const uint32_t w = (uint32_t)j >> 5, bit = 1u << ((uint32_t)j & 31u);
                if (w < r_words) {
                    fwd = fwd || (peak_pl[w] & bit);
                    bwd = bwd || (peak_pl[pw + w] & bit);
                }
            }
            s_tot = s_tot + y;
            s_exp = s_exp + ((fwd || bwd) ? y : 0.0);
            s_fwd = s_fwd + (fwd ? y : 0.0);
            s_bwd = s_bwd + (bwd ? y : 0.0);
        }
        n_expl += (uint32_t)__popcll(__ballot(live && (fwd || bwd)));
    }

    /* ---- phase 3: the partials in lane order, the sizes, the record ---- */
    part[lane] = s_tot;
    part[64 + lane] = s_exp;
    part[128 + lane] = s_fwd;
    part[192 + lane] = s_bwd;
    gen_sync();
    double s = 0.0;
    if (lane < 4)
        for (int l = 0; l < 64; l++) s = s + part[lane * 64 + l];
    const unsigned long long bits = (unsigned long long)__double_as_longlong(s);
    const uint32_t s_lo = (uint32_t)bits, s_hi = (uint32_t)(bits >> 32);
    const uint32_t lo1 = (uint32_t)__shfl((int)s_lo, 1, 64), hi1 = (uint32_t)__shfl((int)s_hi, 1, 64);
    const uint32_t lo3 = (uint32_t)__shfl((int)s_lo, 3, 64), hi3 = (uint32_t)__shfl((int)s_hi, 3, 64);
    if (lane == 0) {
        rec[0] = make_uint4(s_lo, s_hi, lo1, hi1);
        uint32_t f_run = 0, b_run = 0, bonds = 0;
        const int Lw = walked ? L : 1;                              /* (the planes hold sizes below PYA_MAX_PEPTIDE_LEN only) */
        const uint32_t f_n = cov_sizes(size_pl, Lw - 1, &f_run), b_n = cov_sizes(size_pl + COV_SIZE_WORDS, Lw - 1, &b_run);
        for (int bond = 1; bond < Lw; bond++) {
            const int bs = Lw - bond;                               /* the backward size that covers this bond */
            const bool cf = (size_pl[bond >> 5] >> (bond & 31)) & 1u, cb = (size_pl[COV_SIZE_WORDS + (bs >> 5)] >> (bs & 31)) & 1u;
            bonds += (cf || cb) ? 1u : 0u;
        }
        rec[2] = make_uint4(n_peaks, (uint32_t)R, n_expl, n_frag);
        rec[3] = make_uint4(f_n | b_n << 16, f_run | b_run << 16, bonds | (uint32_t)PYA_COV_SCORED << 16, 0u);
    }
    if (lane == 2) rec[1] = make_uint4(s_lo, s_hi, lo3, hi3);
}

extern "C" size_t pya_coverage_lds_bytes(uint32_t l_cap, uint32_t peak_cap) { return cov_lds_bytes(l_cap, peak_cap); }

template <typename MZ, typename IT>
static int cov_launch(const BatchDev *b, const CovArgs &a, hipStream_t stream) {
    hipError_t e = PYA_ENSURE_MAX_LDS((pya_coverage_kernel<MZ, IT>));
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL((pya_coverage_kernel<MZ, IT>), dim3(a.n_ids), dim3(64), cov_lds_bytes(a.l_cap, a.peak_cap), stream, *b, a);
    return (int)hipGetLastError();
}

/* d_ids (n_ids PSM numbers) or NULL: the PSMs 0 .. n_ids - 1; d_spec_of: [n_psm] or NULL (PSM i has spectrum i); b->mz and
 * b->inten: the raw arrays of element types `types` (PYA_SPEC_*); peak_cap: no listed PSM's spectrum has more raw peaks */
extern "C" int pya_launch_coverage(const BatchDev *b, const uint32_t *d_ids, uint32_t n_ids, const uint32_t *d_spec_of, uint32_t types,
                                   void *d_out, uint32_t l_cap, uint32_t peak_cap, hipStream_t stream) {
    if (n_ids == 0) return 0;
    const CovArgs a = {d_ids, d_spec_of, (uint4 *)d_out, n_ids, l_cap, peak_cap};
    switch (types) {
        case PYA_SPEC_F64_F64: return cov_launch<double, double>(b, a, stream);
        case PYA_SPEC_F64_F32: return cov_launch<double, float>(b, a, stream);
        case PYA_SPEC_F32_F32: return cov_launch<float, float>(b, a, stream);
        default: return (int)hipErrorInvalidValue;
    }
}
