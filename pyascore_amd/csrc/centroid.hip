/* centroid.hip -- peak picking in front of a run (include/pyascore_hip.h: pya_centroid_params has THE RULE): a profile-mode
 * spectrum, 10 to 20 samples per real peak, becomes one (centroid, height or area) pair per local maximum.  The first of the
 * transforms in front of a plan, for deisotope.hip's reason: the peak counts change and a plan reads them on the host.  The
 * reference has no counterpart.
 *
 * Three stream-ordered passes, no float atomics, no LDS, the launch shape of deisotope.hip (one wavefront per spectrum striding
 * over its points 64 at a time, four wavefronts per workgroup, a capped grid that strides over the spectra):
 * MARK   a lane holds one point and loads its two neighbours (shifted loads: the lines are the stride's own but for the two
 *        edge lanes), decides CONNECTED on either side and APEX; a ballot per stride gives the 64 keep bits, written as one
 *        word of the workspace; their popcounts add up to the spectrum's apex count, written to new_off[s].  The ascending
 *        check is deisotoping's and runs in the same pass.  A spectrum that fails it, or that d_select leaves out, gets all of
 *        its keep bits set: its count is its length.  Nothing else is stored: no centroid, no footprint.
 * SCAN   the ion stage's exclusive scan (ions.hip, pya_launch_ions_scan) over new_off, in place.
 * PLACE  the keep word of a stride is a uniform load; a kept lane's output position is the spectrum's offset, the popcounts of
 *        the strides before it and mbcnt of the word below the lane.  A spectrum whose count is its length is copied, bits
 *        moved: it is not ascending, not selected, or all of its points are isolated apexes, whose output is themselves
 *        (PASS-THROUGH).  Otherwise every kept lane walks down to l (a wave-uniform loop of at most half_width steps, left as
 *        soon as no lane goes on), then up from l to r, adding the CENTROID sums in the rule's order and finding r on the way
 *        (at most 2 half_width + 1 steps); both walks advance by selects.  It then computes c and writes the pair.
 * The keep words, the clipping of the offsets to [0, total] and the guard of every write are deisotope.hip's: no write lies
 * outside the arrays whatever the offsets say. */
#include "deiso_rule.hip.h"

/* CONNECTED for the step from a point at xa to the next at xb, operation for operation */
DEV bool cen_connected(double xa, double xb, const pya_centroid_params &prm) {
    const double g = xb - xa;
    const double lim = prm.gap0 + prm.gap_per_mz * xa;
    return g <= lim;
}

template <typename TM, typename TI>
__global__ __launch_bounds__(64 * DEISO_WAVES) void pya_centroid_mark_kernel(const TM *mz, const TI *in, const int64_t *peak_off, uint64_t n_spectra,
                                                                             const uint8_t *select, pya_centroid_params prm, int64_t cap_peaks,
                                                                             uint64_t *keep, int64_t *new_off, uint32_t *over) {
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
        const bool chosen = select == nullptr || select[s] != 0;
        uint64_t kept = 0;
        bool bad = false;
        if (chosen) {
            for (int64_t k0 = p0; k0 < p1; k0 += 64) {                 /* (wave-uniform trip count) */
                const int64_t j = k0 + lane;
                bool apex = false, unordered = false;
                if (j < p1) {
                    const double xj = deiso_widen(mz[j]), yj = deiso_widen(in[j]);
                    apex = yj > 0. && yj >= prm.min_height;
                    if (j > p0) {
                        const double xa = deiso_widen(mz[j - 1]);
                        if (!(xa <= xj)) unordered = true;
                        if (cen_connected(xa, xj, prm)) apex = apex && deiso_widen(in[j - 1]) < yj;
                    }
                    if (j + 1 < p1 && cen_connected(xj, deiso_widen(mz[j + 1]), prm)) apex = apex && deiso_widen(in[j + 1]) <= yj;
                }
                const uint64_t mask = __ballot(apex);
                if (__ballot(unordered) != 0ull) bad = true;
                if (lane == 0) words[(k0 - p0) >> 6] = mask;
                kept += (uint64_t)__builtin_popcountll(mask);
            }
        }
        if (bad || !chosen) {                                          /* copied unchanged: every point stays */
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

template <typename TM, typename TI>
__global__ __launch_bounds__(64 * DEISO_WAVES) void pya_centroid_place_kernel(const TM *mz, const TI *in, const int64_t *peak_off, uint64_t n_spectra,
                                                                              pya_centroid_params prm, int64_t cap_peaks, const uint64_t *keep,
                                                                              const int64_t *new_off, TM *out_mz, TI *out_in) {
    const int lane = lane_id();
    const uint64_t wave = (uint64_t)blockIdx.x * DEISO_WAVES + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t n_waves = (uint64_t)gridDim.x * DEISO_WAVES;
    const int64_t total = deiso_total(peak_off, n_spectra, cap_peaks);
    const int64_t hw = (int64_t)prm.half_width;
    for (uint64_t s = wave; s < n_spectra; s += n_waves) {
        int64_t p0, p1;
        bool clipped;
        deiso_range(peak_off, s, total, &p0, &p1, &clipped);
        const uint64_t *words = keep + ((uint64_t)p0 >> 6) + s;
        int64_t dst = new_off[s];
        const bool copy = new_off[s + 1] - dst == p1 - p0;             /* (wave-uniform) */
        for (int64_t k0 = p0; k0 < p1; k0 += 64) {
            const uint64_t mask = words[(k0 - p0) >> 6];
            if (mask == 0ull) continue;                                /* (uniform: a stride of flanks) */
            const int64_t i = k0 + lane;
            const int64_t at = dst + mask_rank(mask);
            dst += (int64_t)__builtin_popcountll(mask);
            /* (offsets that overlap cannot push a write past the array) */
            const bool mine = ((mask >> lane) & 1ull) && i < p1 && at >= 0 && at < total;
            if (copy) {
                if (mine) {
                    out_mz[at] = mz[i];
                    out_in[at] = in[i];
                }
                continue;
            }
            const TM xi_raw = mine ? mz[i] : (TM)0;
            const TI yi_raw = mine ? in[i] : (TI)0;
            const double xi = deiso_widen(xi_raw);
            /* FOOTPRINT, left: down from i while the step is connected and rises strictly towards i */
            int64_t l = i;
            double xl = xi, yl = deiso_widen(yi_raw);
            bool go = mine;
            for (int64_t t = 1; t <= hw; t++) {
                const int64_t k = i - t;
                go = go && k >= p0;
                if (__ballot(go) == 0ull) break;
                const double xk = go ? deiso_widen(mz[k]) : 0., yk = go ? deiso_widen(in[k]) : 0.;
                go = go && cen_connected(xk, xl, prm) && yk < yl;
                l = go ? k : l;
                xl = go ? xk : xl;
                yl = go ? yk : yl;
            }
            /* CENTROID from l upwards, and r on the way: below i every step belongs to the footprint, above i a step does while
             * it is connected, does not rise and stays within half_width */
            const double x_lo = xl;
            double sw = 0., sum = 0., xr = xl, yr = yl;
            int64_t r = l;
            go = mine;
            for (int64_t t = 0; t <= 2 * hw; t++) {
                const int64_t k = l + t;
                if (t) {
                    go = go && k < p1 && k - i <= hw;
                    if (__ballot(go) == 0ull) break;
                }
                const double xk = go ? deiso_widen(mz[k]) : 0., yk = go ? deiso_widen(in[k]) : 0.;
                if (t) go = go && (k <= i || (cen_connected(xr, xk, prm) && yk <= yr));
                const double w2 = sw + yk;
                const double d = xk - xi;
                const double p = d * yk;
                const double s2 = sum + p;
                sw = go ? w2 : sw;
                sum = go ? s2 : sum;
                r = go ? k : r;
                xr = go ? xk : xr;
                yr = go ? yk : yr;
            }
            if (mine) {
                const double q = sum / sw;
                double c = xi + q;
                c = c >= x_lo ? c : x_lo;
                c = c <= xr ? c : xr;
                out_mz[at] = l == r ? xi_raw : (TM)c;
                out_in[at] = prm.area ? (TI)sw : yi_raw;
            }
        }
    }
}

extern "C" int pya_launch_ions_scan(int64_t *d_off, uint32_t n, uint64_t *d_tiles, hipStream_t stream);

template <typename TM, typename TI>
static void centroid_launch(uint32_t blocks, hipStream_t stream, const void *mz, const void *in, const int64_t *peak_off,
                            uint64_t n_spectra, const uint8_t *select, const pya_centroid_params *prm, int64_t cap_peaks, uint64_t *keep,
                            int64_t *new_off, uint32_t *over, void *out_mz, void *out_in, bool place) {
    if (!place)
        hipLaunchKernelGGL((pya_centroid_mark_kernel<TM, TI>), dim3(blocks), dim3(64 * DEISO_WAVES), 0, stream, (const TM *)mz, (const TI *)in,
                           peak_off, n_spectra, select, *prm, cap_peaks, keep, new_off, over);
    else
        hipLaunchKernelGGL((pya_centroid_place_kernel<TM, TI>), dim3(blocks), dim3(64 * DEISO_WAVES), 0, stream, (const TM *)mz, (const TI *)in,
                           peak_off, n_spectra, *prm, cap_peaks, keep, new_off, (TM *)out_mz, (TI *)out_in);
}

/* d_tiles: room for pya_ions_scan_tiles(n_spectra) words; d_keep: the keep words; cap_peaks: the peaks d_keep has bits for.
 * The types are checked by the caller: (F64, F64), (F64, F32) or (F32, F32).  n_spectra in 1 .. 2^32 - 2.  d_select may be
 * NULL.  passes: bit 0 mark, bit 1 scan, bit 2 place (7 but for a probe that times them apart). */
extern "C" int pya_launch_centroid(const void *d_mz, const void *d_in, uint32_t mz_type, uint32_t in_type, const int64_t *d_peak_off,
                                   uint64_t n_spectra, const uint8_t *d_select, const pya_centroid_params *prm, int64_t cap_peaks,
                                   uint64_t *d_tiles, uint64_t *d_keep, void *d_out_mz, void *d_out_in, int64_t *d_new_off, uint32_t *d_over,
                                   uint32_t passes, hipStream_t stream) {
    if (n_spectra == 0) return 0;
    const uint32_t blocks = deiso_blocks(n_spectra);
    for (int place = 0; place < 2; place++) {
        if (passes & (place ? 4u : 1u)) {
            if (mz_type == PYA_F32)
                centroid_launch<float, float>(blocks, stream, d_mz, d_in, d_peak_off, n_spectra, d_select, prm, cap_peaks, d_keep, d_new_off,
                                              d_over, d_out_mz, d_out_in, place != 0);
            else if (in_type == PYA_F32)
                centroid_launch<double, float>(blocks, stream, d_mz, d_in, d_peak_off, n_spectra, d_select, prm, cap_peaks, d_keep,
                                               d_new_off, d_over, d_out_mz, d_out_in, place != 0);
            else
                centroid_launch<double, double>(blocks, stream, d_mz, d_in, d_peak_off, n_spectra, d_select, prm, cap_peaks, d_keep,
                                                d_new_off, d_over, d_out_mz, d_out_in, place != 0);
            const int e = (int)hipGetLastError();
            if (e) return e;
        }
        if (!place && (passes & 2u)) {
            const int e = pya_launch_ions_scan(d_new_off, (uint32_t)n_spectra, d_tiles, stream);
            if (e) return e;
        }
    }
    return 0;
}
