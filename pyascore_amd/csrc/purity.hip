/* purity.hip -- precursor purity: the share of an isolation window that belonged to the identified precursor, read off the
 * survey (MS1) spectra (include/pyascore_hip.h: pya_purity_params has THE RULE), and the gate that takes the failing rows out
 * of a channel matrix.  The read-only sibling of markers.hip one level up: it reads survey spectra and writes records.  Not
 * part of a run; the reference has no counterpart.
 *
 * pya_purity_kernel: the launch shape of markers.hip -- one wavefront per QUERY striding over its survey spectrum 64 m/z at a
 * time, four wavefronts per workgroup, a capped grid that strides over the queries --, no LDS, no float atomics.
 *   Lane i < n_c computes centre i - below of the query once and keeps lo_i, hi_i.  The m/z of PURITY_AHEAD strides are asked
 *   for together; per stride ONE ballot of the isolation window.  It is zero for nearly every stride (a window is a few m/z
 *   wide, a survey spectrum a thousand), and then nothing else happens: the intensities are not loaded.  Otherwise the stride's
 *   intensities are loaded and a wave-uniform loop runs over the set bits, lowest first: (x, y) broadcast by v_readlane,
 *   eligibility wave-uniform, one ballot of the centre test over the lanes < n_c -- "precursor" and the iso_hit bits at once --
 *   and the two running sums, the counts and the other_* pick advance uniformly, the same in every lane.  The strides ascend and
 *   the bits ascend: this order IS the index order the rule gives the sums, so there is nothing to reduce.
 *   A survey spectrum is re-read by every query that names it (about 20 in a top-20 method), out of L2.
 * pya_purity_gate_kernel: streaming, the lane = (row, channel) mapping of channel_correct.hip (R = 64 / C rows per stride, one
 * contiguous run of R * C doubles).  Lane (r, 0) reads the record of its row and computes the verdict ONCE; the lanes of the
 * row read it from there (ds_bpermute).  A lane loads its own reading before it stores it and no two lanes share one: in
 * place is safe.  With no channels the layout is that of one channel without a matrix.
 * No write lies outside purity[0 .. n_query), over[0 .. 2), out[0 .. n_rows * C) and select[0 .. n_rows). */
#include "deiso_rule.hip.h"
#include "lane_f64.hip.h"

#define PURITY_AHEAD 4             /* strides of m/z in flight together */

static_assert(PYA_PURITY_MAX_CENTRES <= 32, "the centre ballot is read as one 32-bit word");

template <typename TM, typename TI>
__global__ __launch_bounds__(64 * DEISO_WAVES) void pya_purity_kernel(const TM *mz, const TI *in, const int64_t *peak_off, uint64_t n_survey,
                                                                      int64_t cap_peaks, const int64_t *survey, const double *prec_mz,
                                                                      const int32_t *prec_z, const double *win_lo, const double *win_hi,
                                                                      uint64_t n_query, pya_purity_params prm, pya_purity *purity,
                                                                      uint32_t *over) {
    const int lane = lane_id();
    const uint64_t wave = (uint64_t)blockIdx.x * DEISO_WAVES + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t n_waves = (uint64_t)gridDim.x * DEISO_WAVES;
    const int64_t total = deiso_total(peak_off, n_survey, cap_peaks);
    const uint32_t n_c = prm.below + 1u + prm.isotopes;
    const bool is_centre = (uint32_t)lane < n_c;
    const double pos = (double)(lane - (int)prm.below);                 /* i of centre `lane` */
    const double ppm = prm.tol_ppm * 1e-6;
    for (uint64_t q = wave; q < n_query; q += n_waves) {                /* (everything about q is wave-uniform) */
        const int64_t sv = survey[q];
        const double pm = prec_mz[q], wl = win_lo[q], wh = win_hi[q];
        const int32_t pz = prec_z[q];
        const bool usable = pz >= 1 && pz <= PYA_STRIP_MAX_CHARGE && __builtin_isfinite(pm) && pm > 0.;
        const bool active = sv >= 0 && usable && wl <= wh && __builtin_isfinite(wl) && __builtin_isfinite(wh);
        const bool beyond = active && (uint64_t)sv >= n_survey;
        double window = 0.0, precursor = 0.0, ox = 0.0, oy = 0.0;
        uint32_t n_window = 0, n_precursor = 0, iso_hit = 0;
        bool have_other = false, clipped = false;
        if (active && !beyond) {
            int64_t p0, p1;
            deiso_range(peak_off, (uint64_t)sv, total, &p0, &p1, &clipped);
            /* THE CENTRES, operation for operation (pya_purity_params) */
            const double d = prm.step / (double)pz;
            const double c = pm + pos * d;
            const double w = prm.tol + ppm * c;
            const double lo = c - w, hi = c + w;
            for (int64_t k0 = p0; k0 < p1; k0 += 64 * PURITY_AHEAD) {   /* (wave-uniform trip count) */
                double x[PURITY_AHEAD];
                bool mine[PURITY_AHEAD];
#pragma unroll
                for (int u = 0; u < PURITY_AHEAD; u++) {
                    const int64_t j = k0 + 64 * u + lane;
                    mine[u] = j < p1;
                    x[u] = mine[u] ? deiso_widen(mz[j]) : 0.;
                }
#pragma unroll
                for (int u = 0; u < PURITY_AHEAD; u++) {
                    const uint64_t inside = __ballot(mine[u] && wl <= x[u] && x[u] <= wh);
                    if (inside == 0ull) continue;
                    const double y = mine[u] ? deiso_widen(in[k0 + 64 * u + lane]) : 0.;
                    for (uint64_t cand = inside; cand != 0ull; cand &= cand - 1ull) {   /* (wave-uniform: the peaks inside, lowest first) */
                        const int src = __builtin_ctzll(cand);
                        const double cx = marker_lane_f64(x[u], src), cy = marker_lane_f64(y, src);
                        const bool eligible = cy > 0.0;
                        const uint32_t at = (uint32_t)__ballot(eligible && is_centre && lo <= cx && cx <= hi);
                        const bool prec = at != 0u;
                        window = eligible ? window + cy : window;
                        n_window += eligible ? 1u : 0u;
                        precursor = prec ? precursor + cy : precursor;
                        n_precursor += prec ? 1u : 0u;
                        iso_hit |= at;
                        /* THE OTHER PEAK: the larger y, then the smaller x */
                        const bool take = eligible && !prec && (!have_other || cy > oy || (cy == oy && cx < ox));
                        ox = take ? cx : ox;
                        oy = take ? cy : oy;
                        have_other = have_other || take;
                    }
                }
            }
        }
        if (lane == 0) {
            pya_purity r;
            r.window = window;
            r.precursor = precursor;
            r.other_mz = have_other ? ox + 0.0 : 0.0;
            r.other_intensity = have_other ? oy + 0.0 : 0.0;
            r.n_window = n_window;
            r.n_precursor = n_precursor;
            r.iso_hit = iso_hit;
            r.flags = active && !beyond ? PYA_PURITY_ACTIVE | (n_precursor ? PYA_PURITY_SEEN : 0u) : 0u;
            purity[q] = r;
            if (beyond || clipped) report_over(over, (uint32_t)q);
        }
    }
}

#define PG_THREADS 256
#define PG_WAVES (PG_THREADS / 64)
#define PG_MAX_BLOCKS 2048u

/* C: the channels of the matrix, or 0 for select alone (values and out are then not looked at) */
__global__ void __launch_bounds__(PG_THREADS) pya_purity_gate_kernel(const pya_purity *purity, uint64_t n_rows, double threshold,
                                                                     uint32_t keep_unknown, const uint64_t *values, uint32_t C, uint64_t *out,
                                                                     uint8_t *select) {
    const uint32_t l = (uint32_t)lane_id();
    const uint32_t Cl = C ? C : 1u;
    const uint32_t R = 64u / Cl, span = R * Cl;
    const bool on = l < span;
    const uint32_t r = on ? l / Cl : 0u;
    const uint32_t c = on ? l - r * Cl : 0u;
    const uint64_t n_strides = (n_rows + R - 1) / R;
    const uint64_t step = (uint64_t)gridDim.x * PG_WAVES;
    /* (wave-uniform: stride s is the rows s * R .. s * R + R - 1, its readings one run from s * R * C) */
    for (uint64_t s = (uint64_t)blockIdx.x * PG_WAVES + (threadIdx.x >> 6); s < n_strides; s += step) {
        const uint64_t row = s * R + r;
        const bool have = on && row < n_rows;
        const uint64_t v = have && C ? values[s * span + l] : 0ull;
        uint32_t pass = 0u;
        if (have && c == 0u) {                                          /* THE GATE, once per row */
            const pya_purity p = purity[row];
            const bool known = (p.flags & PYA_PURITY_ACTIVE) && p.window > 0.0;
            pass = known ? (p.precursor >= threshold * p.window ? 1u : 0u) : keep_unknown;
            if (select) select[row] = (uint8_t)pass;
        }
        pass = (uint32_t)__shfl((int)pass, (int)(r * Cl), 64);          /* (all 64 lanes exchange) */
        if (have && C) out[s * span + l] = pass ? v : 0x7ff8000000000000ull;
    }
}

template <typename TM, typename TI>
static void purity_launch(uint32_t blocks, hipStream_t stream, const void *mz, const void *in, const int64_t *peak_off, uint64_t n_survey,
                          int64_t cap_peaks, const int64_t *survey, const double *prec_mz, const int32_t *prec_z, const double *win_lo,
                          const double *win_hi, uint64_t n_query, const pya_purity_params *prm, pya_purity *purity, uint32_t *over) {
    hipLaunchKernelGGL((pya_purity_kernel<TM, TI>), dim3(blocks), dim3(64 * DEISO_WAVES), 0, stream, (const TM *)mz, (const TI *)in, peak_off,
                       n_survey, cap_peaks, survey, prec_mz, prec_z, win_lo, win_hi, n_query, *prm, purity, over);
}

/* cap_peaks: the elements d_mz and d_in hold.  The types are checked by the caller: (F64, F64), (F64, F32) or (F32, F32).
 * n_query in 1 .. 2^32 - 2, n_survey in 0 .. 2^32 - 2; d_peak_off has n_survey + 1 entries. */
extern "C" int pya_launch_purity(const void *d_mz, const void *d_in, uint32_t mz_type, uint32_t in_type, const int64_t *d_peak_off,
                                 uint64_t n_survey, int64_t cap_peaks, const int64_t *d_survey, const double *d_prec_mz, const int32_t *d_prec_z,
                                 const double *d_win_lo, const double *d_win_hi, uint64_t n_query, const pya_purity_params *prm,
                                 pya_purity *d_purity, uint32_t *d_over, hipStream_t stream) {
    if (n_query == 0) return 0;
    const uint32_t blocks = deiso_blocks(n_query);
    if (mz_type == PYA_F32)
        purity_launch<float, float>(blocks, stream, d_mz, d_in, d_peak_off, n_survey, cap_peaks, d_survey, d_prec_mz, d_prec_z, d_win_lo, d_win_hi,
                                    n_query, prm, d_purity, d_over);
    else if (in_type == PYA_F32)
        purity_launch<double, float>(blocks, stream, d_mz, d_in, d_peak_off, n_survey, cap_peaks, d_survey, d_prec_mz, d_prec_z, d_win_lo, d_win_hi,
                                     n_query, prm, d_purity, d_over);
    else
        purity_launch<double, double>(blocks, stream, d_mz, d_in, d_peak_off, n_survey, cap_peaks, d_survey, d_prec_mz, d_prec_z, d_win_lo,
                                      d_win_hi, n_query, prm, d_purity, d_over);
    return (int)hipGetLastError();
}

/* d_values / d_out: n_rows x n_ch doubles (d_out may be d_values), not looked at when n_ch == 0; d_select: n_rows bytes or
 * NULL.  The arguments have been checked. */
extern "C" int pya_launch_purity_gate(const pya_purity *d_purity, uint64_t n_rows, double threshold, uint32_t keep_unknown, const double *d_values,
                                      uint32_t n_ch, double *d_out, uint8_t *d_select, hipStream_t stream) {
    if (n_rows == 0) return 0;
    const uint32_t R = 64u / (n_ch ? n_ch : 1u);
    const uint64_t strides = (n_rows + R - 1) / R, want = (strides + PG_WAVES - 1) / PG_WAVES;
    const uint32_t blocks = want > PG_MAX_BLOCKS ? PG_MAX_BLOCKS : (uint32_t)want;
    hipLaunchKernelGGL(pya_purity_gate_kernel, dim3(blocks), dim3(PG_THREADS), 0, stream, d_purity, n_rows, threshold, keep_unknown,
                       (const uint64_t *)d_values, n_ch, (uint64_t *)d_out, d_select);
    return (int)hipGetLastError();
}
