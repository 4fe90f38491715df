/* markers.hip -- marker ions: reporter and diagnostic ion intensities per spectrum (include/pyascore_hip.h: pya_marker_params
 * has THE RULE).  The read-only sibling of strip.hip: it looks at the peaks strip is there to remove and writes records; the
 * spectra and their counts stay, so there is no workspace, no scan and no fill.  Not part of a run; the reference has no
 * counterpart.
 *
 * One launch, the launch shape of strip.hip (one wavefront per spectrum striding over its peaks 64 at a time, four wavefronts
 * per workgroup, a capped grid that strides over the spectra), no float atomics, no LDS:
 *   lane t computes target t of the spectrum once -- its centre c, lo, hi and whether it is active -- and keeps them in
 *   registers beside its running best (x, y, |x - c|) and its count.  The wavefront strides over the peaks; a wave-uniform loop
 *   runs over the set bits of the active word, the bounds of target t read from lane t (v_readlane: t is uniform), and a
 *   ballot gives the peaks of the stride inside the window.  It is almost always zero.  Where it is not, lane t adds its
 *   popcount and a second wave-uniform loop over its set bits broadcasts each candidate (x, y) by v_readlane; lane t alone
 *   updates its best by selects.  The order of the pick is total up to equal (x, y), so neither the order of the peaks nor the
 *   stride a peak falls in shows in a record.
 *   With more than MARKER_SPAN_FROM active targets the loop is preceded by a test every lane makes for its own target at once:
 *   the smallest and the largest m/z of the stride (two wave reductions, NaN left out) against lo and hi -- a window that misses
 *   [min, max] holds no peak of the stride and is not visited.  Spectra are nearly always ascending, so a stride spans little
 *   and 64 targets cost what a handful do; the test is exact for any order (it only leaves out windows that hold nothing).
 *   Below that many targets the two reductions cost more than the visits they save.
 *   tic: lane l adds the peaks l, l + 64, .. of the spectrum in order, then every lane adds the 64 partials in lane order
 *   (v_readlane: the order of pya_coverage's sum, without its LDS).  base_peak: a wave maximum by butterfly -- a maximum does
 *   not depend on the order once + 0.0 has merged the two zeros.
 * Every 64-bit mask is shifted as a 64-bit value: target 63 is a target like any other.  value[] arrives by value in scalar
 * registers and has no lane-indexed form: lane t picks its entry by an unrolled chain of selects, once per wavefront. */
#include "deiso_rule.hip.h"
#include "lane_f64.hip.h"

/* the largest and the smallest of v over the wavefront, in every lane (v is no NaN) */
DEV double marker_wave_max(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}
DEV double marker_wave_min(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double o = __shfl_xor(v, d, 64);
        v = o < v ? o : v;
    }
    return v;
}

#define MARKER_SPAN_FROM 8     /* active targets above which a stride's m/z span is taken first (two reductions: about 8 visits) */

template <typename TM, typename TI>
__global__ __launch_bounds__(64 * DEISO_WAVES) void pya_markers_kernel(const TM *mz, const TI *in, const int64_t *peak_off, uint64_t n_spectra,
                                                                       int64_t cap_peaks, const double *prec_mz, const int32_t *prec_z,
                                                                       pya_marker_params prm, pya_marker *markers, pya_marker_spectrum *spectra,
                                                                       uint32_t *over) {
    const int lane = lane_id();
    const uint64_t wave = (uint64_t)blockIdx.x * DEISO_WAVES + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t n_waves = (uint64_t)gridDim.x * DEISO_WAVES;
    const int64_t total = deiso_total(peak_off, n_spectra, cap_peaks);
    /* what of target `lane` does not depend on the spectrum: its value -- picked by compares, prm lives in scalar registers --,
     * whether it is a target at all and whether it is relative to the precursor */
    double value = prm.value[0];
#pragma unroll
    for (int t = 1; t < PYA_MARKER_MAX_TARGETS; t++) value = lane == t ? prm.value[t] : value;
    const bool is_target = (uint32_t)lane < prm.n_targets;
    const bool is_loss = (prm.loss_mask >> lane) & 1ull;
    const bool any_loss = prm.loss_mask != 0ull;                        /* (wave-uniform: the precursors may be NULL without it) */
    const double ppm = prm.tol_ppm * 1e-6;
    for (uint64_t s = wave; s < n_spectra; s += n_waves) {
        int64_t p0, p1;
        bool clipped;
        deiso_range(peak_off, s, total, &p0, &p1, &clipped);
        /* THE CENTRE AND THE WINDOW, operation for operation (pya_marker_params) */
        double c = value;
        bool active = is_target;
        if (any_loss) {
            const double pm = prec_mz[s];
            const int32_t pz = prec_z[s];
            const bool has = pz >= 1 && pz <= PYA_STRIP_MAX_CHARGE && __builtin_isfinite(pm) && pm > 0.;
            const double zd = (double)(has ? pz : 1);
            const double rel = (pm * zd - value) / zd;
            c = is_loss ? rel : value;
            active = is_target && (!is_loss || (has && __builtin_isfinite(rel) && rel > 0.));
        }
        const double w = prm.tol + ppm * c;
        const double lo = c - w, hi = c + w;
        const uint64_t act = __ballot(active);
        const bool by_span = __builtin_popcountll(act) > MARKER_SPAN_FROM;          /* (wave-uniform) */
        double bx = 0., by = 0., bd = 0.;                               /* lane t: the best peak of target t so far */
        bool have = false;
        uint32_t count = 0;
        double part = 0., top = 0.;                                     /* lane l: the sum and the maximum of the peaks l, l + 64, .. */
        bool some = false;
        for (int64_t k0 = p0; k0 < p1; k0 += 64) {                      /* (wave-uniform trip count) */
            const int64_t j = k0 + lane;
            const bool mine = j < p1;
            const double x = mine ? deiso_widen(mz[j]) : 0.;
            const double y = mine ? deiso_widen(in[j]) : 0.;
            const bool num = mine && y == y;
            part = part + (num ? y : 0.0);
            top = num && (!some || y > top) ? y : top;
            some = some || num;
            uint64_t visit = act;
            if (by_span) {                                              /* the targets whose window meets the stride's span at all */
                const bool on = mine && x == x;
                const double xmin = marker_wave_min(on ? x : __builtin_inf()), xmax = marker_wave_max(on ? x : -__builtin_inf());
                visit = __ballot(active && lo <= xmax && hi >= xmin);
            }
            for (uint64_t left = visit; left != 0ull; left &= left - 1ull) {   /* (wave-uniform: the targets to visit, lowest first) */
                const int t = __builtin_ctzll(left);
                const double tlo = marker_lane_f64(lo, t), thi = marker_lane_f64(hi, t);
                const uint64_t inside = __ballot(mine && tlo <= x && x <= thi);
                if (inside == 0ull) continue;
                const bool me = lane == t;
                count += me ? (uint32_t)__builtin_popcountll(inside) : 0u;
                for (uint64_t cand = inside; cand != 0ull; cand &= cand - 1ull) {   /* (wave-uniform: the peaks inside, lowest first) */
                    const int src = __builtin_ctzll(cand);
                    const double cx = marker_lane_f64(x, src), cy = marker_lane_f64(y, src);
                    const double cd = __builtin_fabs(cx - c);
                    /* THE PICK: the larger y, then the smaller |x - c|, then the smaller x */
                    const bool better = !have || cy > by || (cy == by && (cd < bd || (cd == bd && cx < bx)));
                    const bool take = me && cy == cy && better;
                    bx = take ? cx : bx;
                    by = take ? cy : by;
                    bd = take ? cd : bd;
                    have = have || take;
                }
            }
        }
        if (is_target) {
            pya_marker r;
            r.mz = active && have ? bx + 0.0 : 0.0;
            r.intensity = active && have ? by + 0.0 : 0.0;
            r.n_peaks = active ? count : 0u;
            r.flags = (active ? PYA_MARKER_ACTIVE : 0u) | (active && have ? PYA_MARKER_PICKED : 0u);
            markers[s * prm.n_targets + (uint32_t)lane] = r;
        }
        const uint64_t hit = __ballot(active && have);
        const bool any_num = __ballot(some) != 0ull;
        const double base = marker_wave_max(some ? top : -__builtin_inf());
        double tic = 0.0;
        if (spectra) {                                                  /* (wave-uniform) */
            for (int l = 0; l < 64; l++) tic = tic + marker_lane_f64(part, l);
        }
        if (lane == 0) {
            if (spectra) {
                pya_marker_spectrum r;
                r.tic = tic;
                r.base_peak = any_num ? base + 0.0 : 0.0;
                r.hit = hit;
                r.n_peaks = (uint32_t)(uint64_t)(p1 - p0);
                r.n_active = (uint32_t)__builtin_popcountll(act);
                spectra[s] = r;
            }
            if (clipped) report_over(over, (uint32_t)s);
        }
    }
}

template <typename TM, typename TI>
static void markers_launch(uint32_t blocks, hipStream_t stream, const void *mz, const void *in, const int64_t *peak_off, uint64_t n_spectra,
                           int64_t cap_peaks, const double *prec_mz, const int32_t *prec_z, const pya_marker_params *prm, pya_marker *markers,
                           pya_marker_spectrum *spectra, uint32_t *over) {
    hipLaunchKernelGGL((pya_markers_kernel<TM, TI>), dim3(blocks), dim3(64 * DEISO_WAVES), 0, stream, (const TM *)mz, (const TI *)in, peak_off,
                       n_spectra, cap_peaks, prec_mz, prec_z, *prm, markers, spectra, over);
}

/* cap_peaks: the elements d_mz and d_in hold.  The types are checked by the caller: (F64, F64), (F64, F32) or (F32, F32).
 * n_spectra in 1 .. 2^32 - 2.  d_prec_mz and d_prec_z may be NULL when prm->loss_mask is 0, d_spectra may be NULL. */
extern "C" int pya_launch_markers(const void *d_mz, const void *d_in, uint32_t mz_type, uint32_t in_type, const int64_t *d_peak_off,
                                  uint64_t n_spectra, int64_t cap_peaks, const double *d_prec_mz, const int32_t *d_prec_z,
                                  const pya_marker_params *prm, pya_marker *d_markers, pya_marker_spectrum *d_spectra, uint32_t *d_over,
                                  hipStream_t stream) {
    if (n_spectra == 0) return 0;
    const uint32_t blocks = deiso_blocks(n_spectra);
    if (mz_type == PYA_F32)
        markers_launch<float, float>(blocks, stream, d_mz, d_in, d_peak_off, n_spectra, cap_peaks, d_prec_mz, d_prec_z, prm, d_markers, d_spectra,
                                     d_over);
    else if (in_type == PYA_F32)
        markers_launch<double, float>(blocks, stream, d_mz, d_in, d_peak_off, n_spectra, cap_peaks, d_prec_mz, d_prec_z, prm, d_markers, d_spectra,
                                      d_over);
    else
        markers_launch<double, double>(blocks, stream, d_mz, d_in, d_peak_off, n_spectra, cap_peaks, d_prec_mz, d_prec_z, prm, d_markers,
                                       d_spectra, d_over);
    return (int)hipGetLastError();
}
