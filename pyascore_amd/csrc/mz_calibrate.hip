/* mz_calibrate.hip -- fragment m/z recalibration: the step between "read the profile" and "re-run narrow".  Two kernels
 * (include/pyascore_hip.h: pya_mz_calibration): FIT turns the ppm axis of a mass-error profile (pya_mz_profile, mz_profile.hip)
 * into one systematic error per band of m/z, APPLY corrects the m/z array of spectra with it where they lie.  Neither is part
 * of a run; no kernel of a run reads anything but the corrected array.  The reference has no counterpart.
 *
 * FIT: one wavefront per slot, lane = bin of the 64-bin ppm axis, the eight bands one after the other.  Per band the flat
 * floor of random matches (the four outermost bins) is taken off every bin, the excess is scanned (a 64-bit inclusive scan
 * over the wave) and the 16 %, 50 % and 84 % points are found with a ballot and a find-first and interpolated inside their
 * bin.  Integer sums throughout, one double division per quantile and one per scaling, so a host restatement does the same
 * IEEE operations (the file is compiled with -ffp-contract=off and without fast-math) and gives EQUAL bytes.  A band that has
 * too little above the floor copies the nearest fitted one (the lower on a tie).  Every byte of a record is written.
 *
 * APPLY: a streaming kernel, 8 or 16 bytes of traffic per peak.  One wavefront per spectrum striding over its peaks, four
 * wavefronts per workgroup, a capped grid that strides over the spectra.  The slot is wave-uniform, so the eight knots are
 * uniform loads and the piecewise-linear error between band centres is a chain of selects.  The arithmetic is the header's,
 * operation for operation in double; float32 m/z is widened, corrected and rounded back once.  No write lies outside
 * out[0 .. peak_off[n_spectra]): the offsets of a spectrum are clamped to that range before anything is written.  A spectrum
 * whose slot is at or above n_slots, or whose record has a knot that is not finite or beyond PYA_MZC_MAX_PPM, is copied
 * unchanged and counted in over[0] (the smallest such spectrum in over[1] as 0xffffffff - spectrum). */
#include "device_common.hip.h"
#include "../../include/pyascore_hip.h"

static_assert(PYA_MZP_BINS == 64, "one bin of the ppm axis per lane");
static_assert(sizeof(pya_mz_calibration) == 128, "the record as the fit kernel stores it");

/* inclusive prefix sum of a 64-bit value over the 64 lanes (all active) */
DEV uint64_t mzc_wave_incl_scan_u64(uint64_t v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t y = (uint64_t)__shfl_up((unsigned long long)v, (unsigned)o, 64);
        if (lane_id() >= o) v += y;
    }
    return v;
}

/* where num / 100 of the excess lies, in bins from the lower edge of bin 0 (E > 0) */
DEV double mzc_quantile(uint64_t ex, uint64_t cum, uint64_t E, uint64_t num) {
    const uint64_t want = num * E;
    const uint64_t reached = __ballot(100ull * cum >= want);           /* (lane 63 always: cum == E there) */
    const int j = __builtin_ctzll(reached);
    const uint64_t cum_j = (uint64_t)__shfl((unsigned long long)cum, j, 64);
    const uint64_t ex_j = (uint64_t)__shfl((unsigned long long)ex, j, 64);
    const double frac = (double)(want - 100ull * (cum_j - ex_j)) / (double)(100ull * ex_j);
    return (double)j + frac;
}

__global__ __launch_bounds__(64) void pya_mz_fit_kernel(const pya_mz_profile *table, uint64_t n_slots, double inv_ppm, uint32_t min_ions,
                                                        pya_mz_calibration *cal) {
    __shared__ double s_ppm[PYA_MZP_BANDS];
    __shared__ float s_spread[PYA_MZP_BANDS];
    __shared__ uint32_t s_signal[PYA_MZP_BANDS];
    const uint64_t slot = blockIdx.x;
    if (slot >= n_slots) return;
    const int lane = lane_id();
    const pya_mz_profile *rec = table + slot;
    uint32_t fitted = 0;                                               /* bit b: band b has enough above the floor */
    for (int b = 0; b < PYA_MZP_BANDS; b++) {
        const uint64_t hcount = (uint64_t)rec->ppm[b][lane];
        const uint64_t floor4 = (uint64_t)__shfl((unsigned long long)hcount, 0, 64) + (uint64_t)__shfl((unsigned long long)hcount, 1, 64) +
                                (uint64_t)__shfl((unsigned long long)hcount, 62, 64) + (uint64_t)__shfl((unsigned long long)hcount, 63, 64);
        const uint64_t ex = 4ull * hcount > floor4 ? 4ull * hcount - floor4 : 0ull;
        const uint64_t cum = mzc_wave_incl_scan_u64(ex);
        const uint64_t E = (uint64_t)__shfl((unsigned long long)cum, 63, 64);
        const bool fit = E >= 4ull * (uint64_t)min_ions;               /* (min_ions >= 1: E > 0) */
        double ppm = 0.;
        float spread = 0.f;
        if (fit) {                                                     /* (wave-uniform) */
            const double p16 = mzc_quantile(ex, cum, E, 16ull), p50 = mzc_quantile(ex, cum, E, 50ull), p84 = mzc_quantile(ex, cum, E, 84ull);
            ppm = (p50 - (double)(PYA_MZP_BINS / 2)) / inv_ppm;
            const double half = 0.5 * (p84 - p16);
            spread = (float)(half / inv_ppm);
            fitted |= 1u << b;
        }
        if (lane == 0) {
            const uint64_t sig = E >> 2;
            s_ppm[b] = ppm;
            s_spread[b] = spread;
            s_signal[b] = sig > 0xffffffffull ? 0xffffffffu : (uint32_t)sig;
        }
    }
    __syncthreads();
    if (lane < PYA_MZP_BANDS) {
        /* a band that is not fitted copies the nearest fitted one, the lower index on a tie; none: 0 */
        int from = -1;
        for (int d = 0; d < PYA_MZP_BANDS && from < 0; d++) {
            if (lane - d >= 0 && ((fitted >> (lane - d)) & 1u)) from = lane - d;
            else if (lane + d < PYA_MZP_BANDS && ((fitted >> (lane + d)) & 1u)) from = lane + d;
        }
        pya_mz_calibration *out = cal + slot;
        out->ppm[lane] = from >= 0 ? s_ppm[from] : 0.;
        out->spread_ppm[lane] = s_spread[lane];
        out->n_signal[lane] = s_signal[lane];
    }
}

extern "C" int pya_launch_mz_fit(const void *d_table, uint64_t n_slots, double inv_ppm, uint32_t min_ions, void *d_cal, hipStream_t stream) {
    if (n_slots == 0) return 0;
    hipLaunchKernelGGL(pya_mz_fit_kernel, dim3((uint32_t)n_slots), dim3(64), 0, stream, (const pya_mz_profile *)d_table, n_slots, inv_ppm,
                       min_ions, (pya_mz_calibration *)d_cal);
    return (int)hipGetLastError();
}

#define MZC_WAVES 4
#define MZC_MAX_BLOCKS 2048u

DEV double mzc_widen(double x) { return x; }
DEV double mzc_widen(float x) { return (double)x; }

/* the corrected value of x (finite and positive) under the eight knots k[] at the band centres */
DEV double mzc_correct(double x, const double *k, double inv_band) {
    const double u = x * inv_band - 0.5;
    const double fl = __builtin_floor(u);
    const int j = !(fl >= 0.) ? 0 : (!(fl < (double)(PYA_MZP_BANDS - 2)) ? PYA_MZP_BANDS - 2 : (int)fl);
    const double rel = u - (double)j;
    const double t = !(rel >= 0.) ? 0. : (!(rel < 1.) ? 1. : rel);
    double a = k[0], b = k[1];
#pragma unroll
    for (int q = 1; q < PYA_MZP_BANDS - 1; q++)
        if (j >= q) {
            a = k[q];
            b = k[q + 1];
        }
    const double step = (b - a) * t;
    const double e = a + step;
    const double c = e * 1e-6;
    const double shift = x * c;
    return x - shift;
}

template <typename T>
__global__ __launch_bounds__(64 * MZC_WAVES) void pya_mz_apply_kernel(const T *mz, const int64_t *peak_off, uint64_t n_spectra, const int32_t *run,
                                                                       const pya_mz_calibration *cal, uint64_t n_slots, double inv_band, T *out,
                                                                       uint32_t *over) {
    const int lane = lane_id();
    /* (the wavefront's number through readfirstlane: the compiler then knows that the spectrum, its offsets, its slot and the
     * knots are wave-uniform and fetches them with scalar loads) */
    const uint64_t wave = (uint64_t)blockIdx.x * MZC_WAVES + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t n_waves = (uint64_t)gridDim.x * MZC_WAVES;
    const int64_t total = peak_off[n_spectra];
    for (uint64_t s = wave; s < n_spectra; s += n_waves) {
        int64_t p0 = peak_off[s], p1 = peak_off[s + 1];
        if (p0 < 0) p0 = 0;                                            /* (no write outside out[0 .. total), whatever the offsets say) */
        if (p1 > total) p1 = total;
        const int32_t slot = run ? run[s] : 0;
        bool apply = slot >= 0;
        bool bad = false;
        double k[PYA_MZP_BANDS];
#pragma unroll
        for (int q = 0; q < PYA_MZP_BANDS; q++) k[q] = 0.;
        if (apply) {                                                   /* (wave-uniform: the slot is the spectrum's) */
            if ((uint64_t)slot >= n_slots) {
                bad = true;
            } else {
#pragma unroll
                for (int q = 0; q < PYA_MZP_BANDS; q++) {
                    k[q] = cal[slot].ppm[q];
                    if (!(__builtin_fabs(k[q]) <= (double)PYA_MZC_MAX_PPM)) bad = true;    /* (NaN and inf fail the comparison) */
                }
            }
        }
        if (bad) {
            apply = false;
            if (lane == 0) report_over(over, (uint32_t)s);
        }
        if (!apply && out == mz) continue;                             /* in place: the bytes stay */
        for (int64_t i = p0 + lane; i < p1; i += 64) {
            const T raw = mz[i];
            T res = raw;
            const double x = mzc_widen(raw);
            if (apply && x > 0. && x < (double)__builtin_huge_val()) res = (T)mzc_correct(x, k, inv_band);
            out[i] = res;
        }
    }
}

/* d_mz / d_out: float64 (mz_type PYA_F64) or float32 (PYA_F32) arrays of peak_off[n_spectra] elements, may be the same;
 * d_run: [n_spectra] slots or NULL (slot 0); d_over: two words, zeroed by the caller */
extern "C" int pya_launch_mz_apply(const void *d_mz, uint32_t mz_type, const int64_t *d_peak_off, uint64_t n_spectra, const int32_t *d_run,
                                   const void *d_cal, uint64_t n_slots, double inv_band, void *d_out, uint32_t *d_over, hipStream_t stream) {
    if (n_spectra == 0) return 0;
    const uint64_t want = (n_spectra + MZC_WAVES - 1) / MZC_WAVES;
    const uint32_t blocks = (uint32_t)(want < MZC_MAX_BLOCKS ? want : MZC_MAX_BLOCKS);
    const pya_mz_calibration *cal = (const pya_mz_calibration *)d_cal;
    if (mz_type == PYA_F32)
        hipLaunchKernelGGL(pya_mz_apply_kernel<float>, dim3(blocks), dim3(64 * MZC_WAVES), 0, stream, (const float *)d_mz, d_peak_off, n_spectra,
                           d_run, cal, n_slots, inv_band, (float *)d_out, d_over);
    else
        hipLaunchKernelGGL(pya_mz_apply_kernel<double>, dim3(blocks), dim3(64 * MZC_WAVES), 0, stream, (const double *)d_mz, d_peak_off,
                           n_spectra, d_run, cal, n_slots, inv_band, (double *)d_out, d_over);
    return (int)hipGetLastError();
}
