/* xic.hip -- precursor XIC: the label-free MS1 intensity of an identified precursor, its chromatographic peak over the survey
 * scans around the identification (include/pyascore_hip.h: pya_xic_params has THE RULE).  The read-only sibling of purity.hip:
 * it reads survey spectra and writes records.  Not part of a run; the reference has no counterpart.
 *
 * pya_xic_check_kernel: one wavefront per survey scan striding it 64 m/z at a time; the neighbour comes from a load shifted by
 * one element, one ballot of "descends" per stride, one byte per scan.
 * pya_xic_kernel: purity's launch shape -- one wavefront per QUERY, DEISO_WAVES per workgroup, a capped grid that strides over
 * the queries --, no LDS, no float atomics.  Lane j IS survey scan scan_lo + j (why a window holds 64 scans at the most).
 *   Each lane with an ok scan searches lo_i in its own scan (a lower bound: one 4- or 8-byte load per step, 64 independent
 *   chains in flight per wavefront) and walks forward while x <= hi_i, taking the maximum by select.  Both loops are
 *   wave-uniform (they run while any lane has work: one ballot per trip) and advance by selects.  Every isotope searches the
 *   whole scan anew: with tol_ppm large the bounds need not ascend with i.
 *   The trace then lives one value per lane, and the rest is wave arithmetic: presence as one 64-bit ballot; start and region
 *   by scalar bit operations on that word (the runs of more than max_gap absent scans are max_gap shifted ANDs of its
 *   complement); L and F as two prefix-max and two suffix-max scans over the lanes (ds_bpermute; a maximum is exact and
 *   order-free); the valleys as two ballots, find-first above and find-last below the start; the apex as a wave maximum and a
 *   ballot of the lanes that hold it.  sum and area are added in LANE ORDER by a wave-uniform loop over the peak's bits that
 *   reads t and rt of each scan through scalar registers (v_readlane): one defined order, no butterfly.
 *   Lane 0 writes the record.
 * pya_xic_values_kernel: one thread per record.
 * No write lies outside scan_ok[0 .. n_survey), xic[0 .. n_query), over[0 .. 2) and out[0 .. n). */
#include "deiso_rule.hip.h"
#include "lane_f64.hip.h"

static_assert(PYA_XIC_MAX_SCANS == 64, "one survey scan per lane, presence as one 64-bit word");
static_assert(PYA_XIC_MAX_ISOTOPES == 3, "p_0 .. p_3 live in four registers");

template <typename TM>
__global__ __launch_bounds__(64 * DEISO_WAVES) void pya_xic_check_kernel(const TM *mz, const int64_t *peak_off, uint64_t n_survey,
                                                                         int64_t cap_peaks, uint8_t *scan_ok) {
    const int lane = lane_id();
    const uint64_t wave = (uint64_t)blockIdx.x * DEISO_WAVES + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t n_waves = (uint64_t)gridDim.x * DEISO_WAVES;
    const int64_t total = deiso_total(peak_off, n_survey, cap_peaks);
    for (uint64_t s = wave; s < n_survey; s += n_waves) {              /* (everything about s is wave-uniform) */
        int64_t p0, p1;
        bool clipped;
        deiso_range(peak_off, s, total, &p0, &p1, &clipped);
        uint64_t bad = 0ull;
        for (int64_t k0 = p0; k0 + 1 < p1; k0 += 64) {                  /* pair (j, j + 1) for j = k0 + lane */
            const int64_t j = k0 + lane;
            const bool pair = j + 1 < p1;
            const double a = pair ? deiso_widen(mz[j]) : 0., b = pair ? deiso_widen(mz[j + 1]) : 0.;
            bad |= __ballot(pair && !(a <= b));
        }
        if (lane == 0) scan_ok[s] = bad ? (uint8_t)0 : (uint8_t)1;
    }
}

/* inclusive maximum over the lanes at and below / at and above this one.  All 64 lanes are active at every call site. */
DEV double xic_prefix_max(double v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double w = __shfl_up(v, o, 64);
        v = lane >= o && w > v ? w : v;
    }
    return v;
}
DEV double xic_suffix_max(double v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double w = __shfl_down(v, o, 64);
        v = lane + o < 64 && w > v ? w : v;
    }
    return v;
}

/* bits a .. b of a 64-bit word, 0 <= a <= b <= 63 */
DEV uint64_t xic_bits(int a, int b) { return (~0ull << a) & (~0ull >> (63 - b)); }

template <typename TM, typename TI>
__global__ __launch_bounds__(64 * DEISO_WAVES) void pya_xic_kernel(const TM *mz, const TI *in, const int64_t *peak_off, uint64_t n_survey,
                                                                   int64_t cap_peaks, const double *rt, const uint8_t *scan_ok,
                                                                   const int64_t *seed, const int64_t *scan_lo, const int64_t *scan_hi,
                                                                   const double *prec_mz, const int32_t *prec_z, uint64_t n_query,
                                                                   pya_xic_params prm, pya_xic *xic, uint32_t *over) {
    const int lane = lane_id();
    const uint64_t wave = (uint64_t)blockIdx.x * DEISO_WAVES + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t n_waves = (uint64_t)gridDim.x * DEISO_WAVES;
    const int64_t total = deiso_total(peak_off, n_survey, cap_peaks);
    const double ppm = prm.tol_ppm * 1e-6;
    const int reach = (int)prm.max_gap + 1;
    for (uint64_t q = wave; q < n_query; q += n_waves) {                /* (everything about q is wave-uniform) */
        const int64_t sd = seed[q], s_lo = scan_lo[q], s_hi = scan_hi[q];
        const double pm = prec_mz[q];
        const int32_t pz = prec_z[q];
        const bool in_range = 0 <= s_lo && s_lo <= sd && sd < s_hi && (uint64_t)s_hi <= n_survey && s_hi - s_lo <= PYA_XIC_MAX_SCANS;
        const bool usable = pz >= 1 && pz <= PYA_STRIP_MAX_CHARGE && __builtin_isfinite(pm) && pm > 0.;
        const bool active = sd >= 0 && in_range && usable;
        pya_xic r;
        r.area = r.apex_intensity = r.seed_intensity = r.sum_intensity = 0.0;
        r.apex_scan = r.left_scan = r.right_scan = r.start_scan = r.n_points = r.n_present = r.iso_hit = r.flags = 0u;
        bool report = sd >= 0 && !in_range;
        if (active) {
            const int W = (int)(s_hi - s_lo), sj = (int)(sd - s_lo);     /* 1 <= W <= 64, 0 <= sj < W */
            const bool mine = lane < W;
            /* ---- the lane's scan ---- */
            int64_t p0 = 0, p1 = 0;
            bool clipped = false, sorted = true;
            double my_rt = 0.0;
            if (mine) {
                const uint64_t s = (uint64_t)s_lo + (uint32_t)lane;      /* < n_survey */
                deiso_range(peak_off, s, total, &p0, &p1, &clipped);
                sorted = scan_ok[s] != 0;
                my_rt = rt[s];
            }
            if (!sorted) p1 = p0;                                        /* no peaks for this purpose */
            report = __ballot(clipped) != 0ull;
            const bool unsorted = __ballot(!sorted) != 0ull;
            /* ---- THE TRACE, operation for operation (pya_xic_params) ---- */
            const double d = prm.step / (double)pz;
            double p[PYA_XIC_MAX_ISOTOPES + 1] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int i = 0; i <= PYA_XIC_MAX_ISOTOPES; i++) {
                if ((uint32_t)i > prm.isotopes) break;                   /* (wave-uniform) */
                const double c = pm + (double)i * d;
                const double w = prm.tol + ppm * c;
                const double lo = c - w, hi = c + w;
                int64_t a = p0, b = p1;                                  /* the first k in [p0, p1) with x[k] >= lo */
                while (__ballot(a < b) != 0ull) {
                    const bool go = a < b;
                    const int64_t mid = a + ((b - a) >> 1);
                    const double x = go ? deiso_widen(mz[mid]) : 0.;
                    const bool below = x < lo;
                    a = go && below ? mid + 1 : a;
                    b = go && !below ? mid : b;
                }
                double best = 0.0;
                int64_t k = a;
                bool go = k < p1;
                while (__ballot(go) != 0ull) {
                    const double x = go ? deiso_widen(mz[k]) : 0.;
                    go = go && x <= hi;
                    const double y = go ? deiso_widen(in[k]) : 0.;
                    best = go && lo <= x && y > best ? y : best;        /* (best >= 0: y > best has y > 0; a NaN never passes) */
                    k++;
                    go = go && k < p1;
                }
                p[i] = best;
            }
            const bool present = mine && p[0] > 0.0;
            double t = p[0];
#pragma unroll
            for (int i = 1; i <= PYA_XIC_MAX_ISOTOPES; i++)
                if ((uint32_t)i <= prm.isotopes) t = t + p[i];
            t = present ? t : 0.0;
            const uint64_t P = __ballot(present);
            r.flags = PYA_XIC_ACTIVE | (unsorted ? PYA_XIC_UNSORTED : 0u);
            r.n_present = (uint32_t)__popcll(P);
            /* ---- START: scalar bit operations on P ---- */
            int a0 = -1;
            if ((P >> sj) & 1ull) {
                a0 = sj;
            } else {
                const uint64_t under = P & ((1ull << sj) - 1ull), above = sj == 63 ? 0ull : P >> (sj + 1);
                const int du = under ? sj - (63 - __builtin_clzll(under)) : 1000;
                const int da = above ? __builtin_ctzll(above) + 1 : 1000;
                if (du <= da && du <= reach) a0 = sj - du;
                else if (da < du && da <= reach) a0 = sj + da;
            }
            if (a0 >= 0) {
                /* ---- REGION: the runs of max_gap + 1 absent scans nearest to a0 bound it ---- */
                const uint64_t A = ~P;
                uint64_t run_up = A, run_dn = A;                         /* bit b: A[b .. b + max_gap] / A[b - max_gap .. b] all absent */
                for (uint32_t g = 1; g <= prm.max_gap; g++) {
                    run_up &= A >> g;
                    run_dn &= A << g;
                }
                const uint64_t block_up = a0 == 63 ? 0ull : run_up & (~0ull << (a0 + 1));
                const uint64_t block_dn = run_dn & ((1ull << a0) - 1ull);
                const uint64_t upto = block_up ? P & ((1ull << __builtin_ctzll(block_up)) - 1ull) : P;
                const int r_hi = 63 - __builtin_clzll(upto);             /* (a0 itself is among the bits) */
                const int top = block_dn ? 63 - __builtin_clzll(block_dn) : -1;
                const uint64_t from = top == 63 ? 0ull : P & (~0ull << (top + 1));
                const int r_lo = __builtin_ctzll(from);
                const uint64_t PR = P & xic_bits(r_lo, r_hi);
                const bool inr = (PR >> lane) & 1ull;
                /* ---- VALLEYS ---- */
                const double tr = inr ? t : 0.0;
                const double L_up = xic_prefix_max(lane >= a0 ? tr : 0.0, lane);       /* max t over [a0, v] for v > a0 */
                const double L_dn = xic_suffix_max(lane <= a0 ? tr : 0.0, lane);       /* ... over [v, a0] for v < a0 */
                const double pre = xic_prefix_max(tr, lane), suf = xic_suffix_max(tr, lane);
                double F_dn = __shfl_up(pre, 1, 64), F_up = __shfl_down(suf, 1, 64);   /* strictly beyond v */
                F_dn = lane == 0 ? 0.0 : F_dn;
                F_up = lane == 63 ? 0.0 : F_up;
                const uint64_t beyond_up = lane == 63 ? 0ull : PR & (~0ull << (lane + 1));
                const uint64_t beyond_dn = PR & lanemask_lt();
                const int n_up = beyond_up ? __builtin_ctzll(beyond_up) : lane, n_dn = beyond_dn ? 63 - __builtin_clzll(beyond_dn) : lane;
                const double t_up = __shfl(t, n_up, 64), t_dn = __shfl(t, n_dn, 64);
                const double low = prm.rise * t;                         /* one rounded product */
                const uint64_t V_up = __ballot(inr && lane > a0 && beyond_up != 0ull && t <= t_up && low < L_up && low < F_up);
                const uint64_t V_dn = __ballot(inr && lane < a0 && beyond_dn != 0ull && t <= t_dn && low < L_dn && low < F_dn);
                const int e_r = V_up ? __builtin_ctzll(V_up) : r_hi;
                const int e_l = V_dn ? 63 - __builtin_clzll(V_dn) : r_lo;
                /* ---- THE PEAK ---- */
                const uint64_t PK = PR & xic_bits(e_l, e_r);
                const bool inp = (PK >> lane) & 1ull;
                const double top_t = wave_max_f64(inp ? t : 0.0);
                const int apex = __builtin_ctzll(__ballot(inp && t == top_t));          /* (t > 0 in the peak: never empty) */
                const uint32_t hits = (p[0] > 0.0 ? 1u : 0u) | (p[1] > 0.0 ? 2u : 0u) | (p[2] > 0.0 ? 4u : 0u) | (p[3] > 0.0 ? 8u : 0u);
                double S = 0.0, Ar = 0.0, t_prev = 0.0, rt_prev = 0.0;
                bool first = true;
                for (uint64_t rest = PK; rest != 0ull; rest &= rest - 1ull) {          /* (wave-uniform: LANE ORDER) */
                    const int u = __builtin_ctzll(rest);
                    const double tu = marker_lane_f64(t, u), ru = marker_lane_f64(my_rt, u);
                    S = S + tu;
                    Ar = first ? Ar : Ar + (0.5 * (t_prev + tu)) * (ru - rt_prev);
                    first = false;
                    t_prev = tu;
                    rt_prev = ru;
                }
                r.area = Ar;
                r.apex_intensity = top_t;
                r.seed_intensity = marker_lane_f64(t, sj);
                r.sum_intensity = S;
                r.apex_scan = (uint32_t)(s_lo + apex);
                r.left_scan = (uint32_t)(s_lo + e_l);
                r.right_scan = (uint32_t)(s_lo + e_r);
                r.start_scan = (uint32_t)(s_lo + a0);
                r.n_points = (uint32_t)__popcll(PK);
                r.iso_hit = (uint32_t)__builtin_amdgcn_readlane((int)hits, apex);
                r.flags |= PYA_XIC_SEEN | (a0 == sj ? PYA_XIC_SEED_PRESENT : 0u) | (V_dn ? PYA_XIC_LEFT_VALLEY : 0u) |
                           (V_up ? PYA_XIC_RIGHT_VALLEY : 0u) | (!V_dn && e_l == 0 ? PYA_XIC_LEFT_OPEN : 0u) |
                           (!V_up && e_r == W - 1 ? PYA_XIC_RIGHT_OPEN : 0u);
            }
        }
        if (lane == 0) {
            xic[q] = r;
            if (report) report_over(over, (uint32_t)q);
        }
    }
}

#define XV_THREADS 256
#define XV_MAX_BLOCKS 2048u

static_assert(sizeof(pya_xic) == 64 && offsetof(pya_xic, area) == 8 * PYA_XIC_AREA && offsetof(pya_xic, apex_intensity) == 8 * PYA_XIC_APEX &&
                  offsetof(pya_xic, seed_intensity) == 8 * PYA_XIC_SEED && offsetof(pya_xic, sum_intensity) == 8 * PYA_XIC_SUM &&
                  offsetof(pya_xic, flags) == 60,
              "a record is eight 64-bit words: column `which` is word `which`, the flags the high half of word 7");

/* A record is read as the words it is: ONE load at a computed index (which & 3: inside the record whatever `which` says; the host
 * has refused anything above 3) and one of the flags, straight-line -- a chain of selects over the four fields compiled to
 * branches, one of which loaded through an address register that was never set. */
__global__ void __launch_bounds__(XV_THREADS) pya_xic_values_kernel(const pya_xic *xic, uint64_t n, uint32_t which, uint64_t *out) {
    const uint64_t step = (uint64_t)gridDim.x * XV_THREADS;
    const uint32_t word = which & 3u;
    const uint64_t *words = (const uint64_t *)xic;
    for (uint64_t i = (uint64_t)blockIdx.x * XV_THREADS + threadIdx.x; i < n; i += step) {
        const uint64_t bits = words[i * 8u + word];
        const uint32_t flags = (uint32_t)(words[i * 8u + 7u] >> 32);
        const double v = __longlong_as_double((long long)bits);
        out[i] = (flags & PYA_XIC_SEEN) && v > 0.0 ? bits : 0x7ff8000000000000ull;
    }
}

/* cap_peaks: the elements d_mz holds.  n_survey in 1 .. 2^32 - 2; the type has been checked. */
extern "C" int pya_launch_xic_check(const void *d_mz, uint32_t mz_type, const int64_t *d_peak_off, uint64_t n_survey, int64_t cap_peaks,
                                    uint8_t *d_scan_ok, hipStream_t stream) {
    if (n_survey == 0) return 0;
    const uint32_t blocks = deiso_blocks(n_survey);
    if (mz_type == PYA_F32)
        hipLaunchKernelGGL((pya_xic_check_kernel<float>), dim3(blocks), dim3(64 * DEISO_WAVES), 0, stream, (const float *)d_mz, d_peak_off, n_survey,
                           cap_peaks, d_scan_ok);
    else
        hipLaunchKernelGGL((pya_xic_check_kernel<double>), dim3(blocks), dim3(64 * DEISO_WAVES), 0, stream, (const double *)d_mz, d_peak_off,
                           n_survey, cap_peaks, d_scan_ok);
    return (int)hipGetLastError();
}

template <typename TM, typename TI>
static void xic_launch(uint32_t blocks, hipStream_t stream, const void *mz, const void *in, const int64_t *peak_off, uint64_t n_survey,
                       int64_t cap_peaks, const double *rt, const uint8_t *scan_ok, const int64_t *seed, const int64_t *scan_lo,
                       const int64_t *scan_hi, const double *prec_mz, const int32_t *prec_z, uint64_t n_query, const pya_xic_params *prm,
                       pya_xic *xic, uint32_t *over) {
    hipLaunchKernelGGL((pya_xic_kernel<TM, TI>), dim3(blocks), dim3(64 * DEISO_WAVES), 0, stream, (const TM *)mz, (const TI *)in, peak_off, n_survey,
                       cap_peaks, rt, scan_ok, seed, scan_lo, scan_hi, prec_mz, prec_z, n_query, *prm, xic, over);
}

/* The types are checked by the caller: (F64, F64), (F64, F32) or (F32, F32).  n_query in 1 .. 2^32 - 2. */
extern "C" int pya_launch_xic(const void *d_mz, const void *d_in, uint32_t mz_type, uint32_t in_type, const int64_t *d_peak_off, uint64_t n_survey,
                              int64_t cap_peaks, const double *d_rt, const uint8_t *d_scan_ok, const int64_t *d_seed, const int64_t *d_scan_lo,
                              const int64_t *d_scan_hi, const double *d_prec_mz, const int32_t *d_prec_z, uint64_t n_query,
                              const pya_xic_params *prm, pya_xic *d_xic, uint32_t *d_over, hipStream_t stream) {
    if (n_query == 0) return 0;
    const uint32_t blocks = deiso_blocks(n_query);
    if (mz_type == PYA_F32)
        xic_launch<float, float>(blocks, stream, d_mz, d_in, d_peak_off, n_survey, cap_peaks, d_rt, d_scan_ok, d_seed, d_scan_lo, d_scan_hi,
                                 d_prec_mz, d_prec_z, n_query, prm, d_xic, d_over);
    else if (in_type == PYA_F32)
        xic_launch<double, float>(blocks, stream, d_mz, d_in, d_peak_off, n_survey, cap_peaks, d_rt, d_scan_ok, d_seed, d_scan_lo, d_scan_hi,
                                  d_prec_mz, d_prec_z, n_query, prm, d_xic, d_over);
    else
        xic_launch<double, double>(blocks, stream, d_mz, d_in, d_peak_off, n_survey, cap_peaks, d_rt, d_scan_ok, d_seed, d_scan_lo, d_scan_hi,
                                   d_prec_mz, d_prec_z, n_query, prm, d_xic, d_over);
    return (int)hipGetLastError();
}

extern "C" int pya_launch_xic_values(const pya_xic *d_xic, uint64_t n, uint32_t which, double *d_out, hipStream_t stream) {
    if (n == 0) return 0;
    const uint64_t want = (n + XV_THREADS - 1) / XV_THREADS;
    const uint32_t blocks = want > XV_MAX_BLOCKS ? XV_MAX_BLOCKS : (uint32_t)want;
    hipLaunchKernelGGL(pya_xic_values_kernel, dim3(blocks), dim3(XV_THREADS), 0, stream, d_xic, n, which, (uint64_t *)d_out);
    return (int)hipGetLastError();
}
