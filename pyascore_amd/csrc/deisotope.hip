/* deisotope.hip -- deisotoping of spectra in front of a run (include/pyascore_hip.h: pya_deisotope_params has THE RULE).  Not
 * part of a run: it changes how many peaks a spectrum has, and a plan reads the peak counts on the host, so it is a transform
 * of spectra that runs before a plan exists.  The reference has no counterpart.
 *
 * Three stream-ordered passes, no float atomics, no LDS:
 * MARK   one wavefront per spectrum striding over its peaks 64 at a time, four wavefronts per workgroup, a capped grid that
 *        strides over the spectra (as the recalibration's apply kernel).  Each lane decides its own peak: it walks down from its
 *        predecessor through the one window that holds the candidate parents of every charge, bounded by the exact predicate
 *        (xj - x[i]) - spacing[0] > tol, and tests every charge on each peak it meets.  A ballot per stride gives 64 keep
 *        bits, written as one word of the workspace; their popcounts add up to the spectrum's kept count, written to new_off[s].  The ascending check (the lane's peak
 *        against its predecessor) runs in the same pass; a spectrum that fails it gets all of its keep bits set again.
 * SCAN   the ion stage's exclusive scan (ions.hip, pya_launch_ions_scan) over new_off, in place.
 * FILL   one wavefront per spectrum: the keep word of a stride is a uniform load, the position of a kept peak inside the stride
 *        is mbcnt of the word below the lane, m/z and intensity are moved as integers of their width (bits copied).
 * The keep words of spectrum s start at word (p0 >> 6) + s of the workspace: ceil(n / 64) words never reach the next
 * spectrum's first word, and no two spectra share a word.  Both kernels clip the offsets of a spectrum to [0, total], total
 * being peak_off[n_spectra] or the peaks the lent workspace has bits for, whichever is smaller, and FILL writes no element at or
 * beyond total: no write lies outside the arrays whatever the offsets say. */
#include "deiso_rule.hip.h"

template <typename TM, typename TI>
__global__ __launch_bounds__(64 * DEISO_WAVES) void pya_deiso_mark_kernel(const TM *mz, const TI *in, const int64_t *peak_off, uint64_t n_spectra,
                                                                          pya_deisotope_params prm, int64_t cap_peaks, uint64_t *keep,
                                                                          int64_t *new_off, uint32_t *over) {
    const int lane = lane_id();
    /* (the wavefront's number through readfirstlane: the spectrum and its offsets are wave-uniform) */
    const uint64_t wave = (uint64_t)blockIdx.x * DEISO_WAVES + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t n_waves = (uint64_t)gridDim.x * DEISO_WAVES;
    const int64_t total = deiso_total(peak_off, n_spectra, cap_peaks);
    for (uint64_t s = wave; s < n_spectra; s += n_waves) {
        int64_t p0, p1;
        bool clipped;
        deiso_range(peak_off, s, total, &p0, &p1, &clipped);
        uint64_t *words = keep + ((uint64_t)p0 >> 6) + s;
        uint64_t kept = 0;
        bool bad = false;
        for (int64_t k0 = p0; k0 < p1; k0 += 64) {                     /* (wave-uniform trip count) */
            const int64_t j = k0 + lane;
            bool stay = false, unordered = false;
            if (j < p1) {
                const double xj = deiso_widen(mz[j]);
                if (j > p0 && !(deiso_widen(mz[j - 1]) <= xj)) unordered = true;
                stay = !deiso_removed(mz, in, p0, j, xj, deiso_widen(in[j]), prm);
            }
            const uint64_t mask = __ballot(stay);
            if (__ballot(unordered) != 0ull) bad = true;
            if (lane == 0) words[(k0 - p0) >> 6] = mask;
            kept += (uint64_t)__builtin_popcountll(mask);
        }
        if (bad) {                                                     /* not ascending: every peak stays */
            for (int64_t k0 = p0; k0 < p1; k0 += 64) {
                const int64_t left = p1 - k0;
                if (lane == 0) words[(k0 - p0) >> 6] = left >= 64 ? ~0ull : (1ull << left) - 1ull;
            }
            kept = (uint64_t)(p1 - p0);
        }
        if (lane == 0) {
            new_off[s] = (int64_t)kept;
            if (bad || clipped) report_over(over, (uint32_t)s);
        }
    }
}

/* TM / TI: unsigned integers of the width of the m/z and intensity elements */
template <typename TM, typename TI>
__global__ __launch_bounds__(64 * DEISO_WAVES) void pya_deiso_fill_kernel(const TM *mz, const TI *in, const int64_t *peak_off, uint64_t n_spectra,
                                                                          int64_t cap_peaks, const uint64_t *keep, const int64_t *new_off,
                                                                          TM *out_mz, TI *out_in) {
    const int lane = lane_id();
    const uint64_t wave = (uint64_t)blockIdx.x * DEISO_WAVES + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t n_waves = (uint64_t)gridDim.x * DEISO_WAVES;
    const int64_t total = deiso_total(peak_off, n_spectra, cap_peaks);
    for (uint64_t s = wave; s < n_spectra; s += n_waves) {
        int64_t p0, p1;
        bool clipped;
        deiso_range(peak_off, s, total, &p0, &p1, &clipped);
        const uint64_t *words = keep + ((uint64_t)p0 >> 6) + s;
        int64_t dst = new_off[s];
        for (int64_t k0 = p0; k0 < p1; k0 += 64) {
            const uint64_t mask = words[(k0 - p0) >> 6];
            const int64_t j = k0 + lane;
            if ((mask >> lane) & 1ull) {
                const int64_t at = dst + mask_rank(mask);
                if (j < p1 && at >= 0 && at < total) {                 /* (offsets that overlap cannot push a write past the array) */
                    out_mz[at] = mz[j];
                    out_in[at] = in[j];
                }
            }
            dst += (int64_t)__builtin_popcountll(mask);
        }
    }
}

extern "C" int pya_launch_ions_scan(int64_t *d_off, uint32_t n, uint64_t *d_tiles, hipStream_t stream);

template <typename TM, typename TI>
static void deiso_mark(uint32_t blocks, hipStream_t stream, const void *mz, const void *in, const int64_t *peak_off, uint64_t n_spectra,
                       const pya_deisotope_params *prm, int64_t cap_peaks, uint64_t *keep, int64_t *new_off, uint32_t *over) {
    hipLaunchKernelGGL((pya_deiso_mark_kernel<TM, TI>), dim3(blocks), dim3(64 * DEISO_WAVES), 0, stream, (const TM *)mz, (const TI *)in, peak_off,
                       n_spectra, *prm, cap_peaks, keep, new_off, over);
}

template <typename TM, typename TI>
static void deiso_fill(uint32_t blocks, hipStream_t stream, const void *mz, const void *in, const int64_t *peak_off, uint64_t n_spectra,
                       int64_t cap_peaks, const uint64_t *keep, const int64_t *new_off, void *out_mz, void *out_in) {
    hipLaunchKernelGGL((pya_deiso_fill_kernel<TM, TI>), dim3(blocks), dim3(64 * DEISO_WAVES), 0, stream, (const TM *)mz, (const TI *)in, peak_off,
                       n_spectra, cap_peaks, keep, new_off, (TM *)out_mz, (TI *)out_in);
}

/* FILL alone, for a caller with keep words and scanned offsets of its own (strip.hip): the launch pya_launch_deisotope ends
 * with.  d_keep and cap_peaks as there. */
extern "C" int pya_launch_deiso_fill(const void *d_mz, const void *d_in, uint32_t mz_type, uint32_t in_type, const int64_t *d_peak_off,
                                     uint64_t n_spectra, int64_t cap_peaks, const uint64_t *d_keep, const int64_t *d_new_off, void *d_out_mz,
                                     void *d_out_in, hipStream_t stream) {
    if (n_spectra == 0) return 0;
    const uint32_t blocks = deiso_blocks(n_spectra);
    if (mz_type == PYA_F32)
        deiso_fill<uint32_t, uint32_t>(blocks, stream, d_mz, d_in, d_peak_off, n_spectra, cap_peaks, d_keep, d_new_off, d_out_mz, d_out_in);
    else if (in_type == PYA_F32)
        deiso_fill<uint64_t, uint32_t>(blocks, stream, d_mz, d_in, d_peak_off, n_spectra, cap_peaks, d_keep, d_new_off, d_out_mz, d_out_in);
    else
        deiso_fill<uint64_t, uint64_t>(blocks, stream, d_mz, d_in, d_peak_off, n_spectra, cap_peaks, d_keep, d_new_off, d_out_mz, d_out_in);
    return (int)hipGetLastError();
}

/* d_tiles: room for pya_ions_scan_tiles(n_spectra) words; d_keep: the keep words; cap_peaks: the peaks d_keep has bits for.
 * The types are checked by the caller: (F64, F64), (F64, F32) or (F32, F32).  n_spectra in 1 .. 2^32 - 2. */
extern "C" int pya_launch_deisotope(const void *d_mz, const void *d_in, uint32_t mz_type, uint32_t in_type, const int64_t *d_peak_off,
                                    uint64_t n_spectra, const pya_deisotope_params *prm, int64_t cap_peaks, uint64_t *d_tiles, uint64_t *d_keep,
                                    void *d_out_mz, void *d_out_in, int64_t *d_new_off, uint32_t *d_over, hipStream_t stream) {
    if (n_spectra == 0) return 0;
    const uint32_t blocks = deiso_blocks(n_spectra);
    if (mz_type == PYA_F32)
        deiso_mark<float, float>(blocks, stream, d_mz, d_in, d_peak_off, n_spectra, prm, cap_peaks, d_keep, d_new_off, d_over);
    else if (in_type == PYA_F32)
        deiso_mark<double, float>(blocks, stream, d_mz, d_in, d_peak_off, n_spectra, prm, cap_peaks, d_keep, d_new_off, d_over);
    else
        deiso_mark<double, double>(blocks, stream, d_mz, d_in, d_peak_off, n_spectra, prm, cap_peaks, d_keep, d_new_off, d_over);
    int e = (int)hipGetLastError();
    if (e) return e;
    e = pya_launch_ions_scan(d_new_off, (uint32_t)n_spectra, d_tiles, stream);
    if (e) return e;
    return pya_launch_deiso_fill(d_mz, d_in, mz_type, in_type, d_peak_off, n_spectra, cap_peaks, d_keep, d_new_off, d_out_mz, d_out_in, stream);
}
