/* strip.hip -- precursor stripping in front of a run (include/pyascore_hip.h: pya_strip_params has THE RULE): the unfragmented
 * precursor, its neutral-loss forms, the charge-reduced precursors and the peaks outside [mz_lo, mz_hi] leave a spectrum.
 * Not part of a run, for deisotope.hip's reason: the peak counts change and a plan reads them on the host.  The reference has
 * no counterpart.
 *
 * Three stream-ordered passes, no float atomics, no LDS, the launch shape of deisotope.hip (one wavefront per spectrum striding
 * over its peaks 64 at a time, four wavefronts per workgroup, a capped grid that strides over the spectra):
 * MARK   lane w computes window w of the spectrum once -- lo, hi and whether it is active -- and keeps it in registers: at most
 *        8 charges x 8 losses = 64 windows, one per lane.  The wavefront then strides over the peaks; a lane tests its own peak
 *        against every ACTIVE window in a wave-uniform loop over the set bits of the active word, the bounds of window w read
 *        from lane w (v_readlane: w is uniform).  A ballot per window says whether any peak of the stride lies in it (a bit of
 *        hit), a ballot per stride gives the 64 keep bits, written as one word of the workspace; their popcounts add up to the
 *        spectrum's kept count, written to new_off[s].  Lane 0 writes the report.  Intensities are not read.
 * SCAN   the ion stage's exclusive scan (ions.hip, pya_launch_ions_scan) over new_off, in place.
 * FILL   deisotope.hip's fill kernel through pya_launch_deiso_fill: the keep words have its layout (those of spectrum s start
 *        at word (p0 >> 6) + s of the workspace) and the offsets are clipped the same way (deiso_range / deiso_total), so no
 *        write lies outside the arrays whatever the offsets say.
 * Every 64-bit mask is shifted as a 64-bit value: window 63 is a window like any other. */
#include "deiso_rule.hip.h"

/* a double held by lane `src` (wave-uniform), to every lane: two v_readlane */
DEV double strip_lane_f64(double v, int src) {
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, src);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), src);
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | (uint64_t)lo));
}

template <typename TM>
__global__ __launch_bounds__(64 * DEISO_WAVES) void pya_strip_mark_kernel(const TM *mz, const int64_t *peak_off, uint64_t n_spectra,
                                                                          const double *prec_mz, const int32_t *prec_z, pya_strip_params prm,
                                                                          int64_t cap_peaks, uint64_t *keep, int64_t *new_off,
                                                                          pya_strip_report *report, uint32_t *over) {
    const int lane = lane_id();
    /* (the wavefront's number through readfirstlane: the spectrum, its precursor and its offsets are wave-uniform) */
    const uint64_t wave = (uint64_t)blockIdx.x * DEISO_WAVES + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t n_waves = (uint64_t)gridDim.x * DEISO_WAVES;
    const int64_t total = deiso_total(peak_off, n_spectra, cap_peaks);
    /* what of window `lane` does not depend on the spectrum: its charge and loss index (n_loss <= 7: 1 .. 8 windows a charge),
     * and its loss -- picked by compares, prm lives in scalar registers and has no lane-indexed form */
    const uint32_t per_charge = prm.n_loss + 1u;
    const uint32_t c_idx = (uint32_t)lane / per_charge, l_idx = (uint32_t)lane % per_charge;
    double loss = prm.loss[0];
#pragma unroll
    for (uint32_t l = 1; l <= PYA_STRIP_MAX_LOSS; l++) loss = l_idx == l ? prm.loss[l] : loss;
    for (uint64_t s = wave; s < n_spectra; s += n_waves) {
        int64_t p0, p1;
        bool clipped;
        deiso_range(peak_off, s, total, &p0, &p1, &clipped);
        const double pm = prec_mz[s];
        const int32_t pz = prec_z[s];
        /* THE WINDOWS, operation for operation (pya_strip_params) */
        double lo = 0., hi = 0.;
        bool active = false;
        const bool has = pz >= 1 && pz <= PYA_STRIP_MAX_CHARGE && __builtin_isfinite(pm) && pm > 0.;
        if (has && c_idx < (prm.reduced ? (uint32_t)pz : 1u)) {
            const double zr = (double)(pz - (int32_t)c_idx);
            const double M = pm * (double)pz;
            const double cen = (M - loss) / zr;
            const double span = (double)prm.isotopes * (prm.step / zr);
            lo = cen - prm.tol;
            hi = (cen + span) + prm.tol;
            active = __builtin_isfinite(cen) && cen > 0.;
        }
        const uint64_t act = __ballot(active);
        uint64_t *words = keep + ((uint64_t)p0 >> 6) + s;
        uint64_t kept = 0, hit = 0;
        for (int64_t k0 = p0; k0 < p1; k0 += 64) {                     /* (wave-uniform trip count) */
            const int64_t j = k0 + lane;
            const bool mine = j < p1;
            const double x = mine ? deiso_widen(mz[j]) : 0.;
            bool in_any = false;
            for (uint64_t left = act; left != 0ull; left &= left - 1ull) {   /* (wave-uniform: the active windows, lowest first) */
                const int w = __builtin_ctzll(left);
                const double wlo = strip_lane_f64(lo, w), whi = strip_lane_f64(hi, w);
                const bool in = mine && wlo <= x && x <= whi;
                if (__ballot(in) != 0ull) hit |= 1ull << w;
                in_any = in_any || in;
            }
            const bool stay = mine && !(x < prm.mz_lo) && !(x > prm.mz_hi) && !in_any;
            const uint64_t mask = __ballot(stay);
            if (lane == 0) words[(k0 - p0) >> 6] = mask;
            kept += (uint64_t)__builtin_popcountll(mask);
        }
        if (lane == 0) {
            new_off[s] = (int64_t)kept;
            if (report) {
                pya_strip_report r;
                r.hit = hit;
                r.n_removed = (uint32_t)((uint64_t)(p1 - p0) - kept);
                r.n_windows = (uint32_t)__builtin_popcountll(act);
                report[s] = r;
            }
            if (clipped) report_over(over, (uint32_t)s);
        }
    }
}

extern "C" int pya_launch_ions_scan(int64_t *d_off, uint32_t n, uint64_t *d_tiles, hipStream_t stream);
extern "C" int pya_launch_deiso_fill(const void *d_mz, const void *d_in, uint32_t mz_type, uint32_t in_type, const int64_t *d_peak_off,
                                     uint64_t n_spectra, int64_t cap_peaks, const uint64_t *d_keep, const int64_t *d_new_off, void *d_out_mz,
                                     void *d_out_in, hipStream_t stream);

template <typename TM>
static void strip_mark(uint32_t blocks, hipStream_t stream, const void *mz, const int64_t *peak_off, uint64_t n_spectra, const double *prec_mz,
                       const int32_t *prec_z, const pya_strip_params *prm, int64_t cap_peaks, uint64_t *keep, int64_t *new_off,
                       pya_strip_report *report, uint32_t *over) {
    hipLaunchKernelGGL((pya_strip_mark_kernel<TM>), dim3(blocks), dim3(64 * DEISO_WAVES), 0, stream, (const TM *)mz, peak_off, n_spectra, prec_mz,
                       prec_z, *prm, cap_peaks, keep, new_off, report, over);
}

/* d_tiles: room for pya_ions_scan_tiles(n_spectra) words; d_keep: the keep words; cap_peaks: the peaks d_keep has bits for.
 * The types are checked by the caller: (F64, F64), (F64, F32) or (F32, F32).  n_spectra in 1 .. 2^32 - 2.  d_report may be
 * NULL. */
extern "C" int pya_launch_strip(const void *d_mz, const void *d_in, uint32_t mz_type, uint32_t in_type, const int64_t *d_peak_off,
                                uint64_t n_spectra, const double *d_prec_mz, const int32_t *d_prec_z, const pya_strip_params *prm,
                                int64_t cap_peaks, uint64_t *d_tiles, uint64_t *d_keep, void *d_out_mz, void *d_out_in, int64_t *d_new_off,
                                pya_strip_report *d_report, uint32_t *d_over, hipStream_t stream) {
    if (n_spectra == 0) return 0;
    const uint32_t blocks = deiso_blocks(n_spectra);
    if (mz_type == PYA_F32)
        strip_mark<float>(blocks, stream, d_mz, d_peak_off, n_spectra, d_prec_mz, d_prec_z, prm, cap_peaks, d_keep, d_new_off, d_report, d_over);
    else
        strip_mark<double>(blocks, stream, d_mz, d_peak_off, n_spectra, d_prec_mz, d_prec_z, prm, cap_peaks, d_keep, d_new_off, d_report, d_over);
    int e = (int)hipGetLastError();
    if (e) return e;
    e = pya_launch_ions_scan(d_new_off, (uint32_t)n_spectra, d_tiles, stream);
    if (e) return e;
    return pya_launch_deiso_fill(d_mz, d_in, mz_type, in_type, d_peak_off, n_spectra, cap_peaks, d_keep, d_new_off, d_out_mz, d_out_in, stream);
}
