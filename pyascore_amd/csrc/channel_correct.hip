/* channel_correct.hip -- channel correction: the isotope-impurity matrix and the loading factors applied to a channel matrix,
 * its column sums as one row of the quantification table, and the factors of such a row.  The definition is in
 * include/pyascore_hip.h (channel correction); the reference has no counterpart.
 *
 * The stage has ONE order of arithmetic -- per reading a chain x = x + m * u over the channels in ascending order, every
 * product and every sum rounded on its own (the library is built with -ffp-contract=off) --, so its bytes are those of the host
 * restatement.  Hence no matrix instruction, no butterfly over the terms and no atomics in the apply; the sums are integers
 * (quant_rule.hip.h) and may arrive in any order.
 *
 * Both streaming kernels share one lane mapping.  With C channels a wavefront takes R = 64 / C consecutive rows per stride:
 * lane l is (row l / C of the stride, channel l % C), the lanes from R * C on idle (C = 18: 10 of them, C = 63: one), and the
 * stride's readings are ONE contiguous run of R * C doubles.  A lane's channel never changes.  In the apply a workgroup of four
 * wavefronts takes PYA_CHANNEL_TILE consecutive rows, wavefront w the strides w, w + 4, ...
 *   apply  The matrix is staged once per workgroup in LDS, TRANSPOSED: mT[j][c] = m[c * C + j], so that in turn j of the
 *          wave-uniform loop lane c reads mT[j][c] -- consecutive doubles over the lanes of one row, one address for the lanes
 *          of one channel: no bank conflict (the rows are pitched to CC_PITCH doubles, an odd count, so the staging's stores
 *          have none either).  u[j] of the lane's own row comes from lane (row, j) by ds_bpermute -- or by v_readlane when
 *          R == 1, where it is wave-uniform.  Every lane has loaded its reading before any lane of the wavefront stores (each
 *          store depends on the exchange), and no two wavefronts share a row: d_out == d_values is safe.
 *   sums   No tiles: the wavefronts of at most CS_MAX_BLOCKS workgroups of eight walk the strides of the whole matrix by a
 *          grid stride, accumulators in registers; at the end a tree over the rows of the stride (integer adds, log2 R turns)
 *          and the wavefronts onto the first through LDS, then one 64-bit atomic add per (workgroup, channel) for sum and one
 *          for n | n_saturated << 32, as quant_wave.hip.h's qw_flush has them; a part that is zero adds nothing.  Few
 *          workgroups, because the atomics of all of them land on the same few cache lines (C cells of 16 bytes) and are served
 *          one after another there: their number grows with the workgroups, not with the bytes.
 * Both loops ask for the next stride's readings before they work on this one's.
 * No write lies outside out[0 .. n_rows * C), cell[0 .. C) and factor[0 .. C): a lane stores only under row < n_rows and
 * l < R * C, a channel lane only under l < C. */
#include "quant_rule.hip.h"
#include "../../include/pyascore_hip.h"

#define CC_THREADS 256
#define CC_WAVES (CC_THREADS / 64)
#define CS_THREADS 512                /* the sums kernel: eight wavefronts, so that few workgroups keep many loads in flight */
#define CS_WAVES (CS_THREADS / 64)
#define CS_MAX_BLOCKS 256u            /* ... and at most this many of them: every workgroup ends in atomics on the same few cache lines */

static_assert(PYA_QUANT_MAX_CHANNELS == 64, "one channel per lane of a wavefront at the most");

struct CcLane {
    uint32_t R, span;                 /* rows per stride, R * C */
    uint32_t r, c, row_lane;          /* this lane's row of the stride, its channel, lane of (r, 0) */
    bool on;                          /* the lane stands for a reading */
};

DEV CcLane cc_lane(uint32_t C) {
    CcLane k;
    const uint32_t l = (uint32_t)lane_id();
    k.R = 64u / C;
    k.span = k.R * C;
    k.on = l < k.span;
    k.r = k.on ? l / C : 0u;
    k.c = k.on ? l - k.r * C : 0u;
    k.row_lane = k.r * C;
    return k;
}

/* the row stride of the staged matrix in doubles, whatever C is: odd, so that the 8-byte stores of the staging (stride CC_PITCH
 * between neighbouring lanes) spread over the banks as the loads of the loop (stride 1) do, and a constant, so that the terms of
 * an unrolled turn are read at immediate offsets from one address */
#define CC_PITCH 65u

/* THE CHAIN of one reading: x = +0.0, then x = x + mT[j][c] * u[j] for j ascending, one rounded product and one rounded sum per
 * term.  `col` is &mT[0][c], `get(j)` gives u[j] of the lane's row and is called by all 64 lanes with a wave-uniform j.  The
 * terms are fetched CC_UNROLL at a time -- LDS reads and lane exchanges of the next terms in flight while the sums, which depend
 * on one another, wait for nothing else -- and added in order all the same.  (Unrolled by hand: the compiler does not unroll a
 * loop of unknown length around a cross-lane operation.) */
#define CC_UNROLL 8
template <typename Get>
DEV double cc_chain(const double *col, uint32_t C, const Get &get) {
    double x = 0.0;
    uint32_t j = 0;
    for (; j + CC_UNROLL <= C; j += CC_UNROLL) {
        double m[CC_UNROLL], uj[CC_UNROLL];
#pragma unroll
        for (uint32_t t = 0; t < CC_UNROLL; t++) {
            m[t] = col[(j + t) * CC_PITCH];
            uj[t] = get(j + t);
        }
#pragma unroll
        for (uint32_t t = 0; t < CC_UNROLL; t++) x = x + m[t] * uj[t];
    }
    for (; j < C; j++) x = x + col[j * CC_PITCH] * get(j);
    return x;
}

__global__ void __launch_bounds__(CC_THREADS) pya_channel_correct_kernel(const double *values, uint64_t n_rows, uint32_t C, const double *matrix,
                                                                         const double *factor, double *out) {
    extern __shared__ __attribute__((aligned(16))) double cc_mT[];
    if (matrix) {
        for (uint32_t i = threadIdx.x; i < C * C; i += CC_THREADS) {
            const uint32_t c = i / C, j = i - c * C;
            cc_mT[j * CC_PITCH + c] = matrix[i];
        }
        __syncthreads();
    }
    const CcLane k = cc_lane(C);
    const double f = factor && k.on ? factor[k.c] : 1.0;
    const uint64_t tile0 = (uint64_t)blockIdx.x * PYA_CHANNEL_TILE;
    const uint64_t tile1 = tile0 + PYA_CHANNEL_TILE < n_rows ? tile0 + PYA_CHANNEL_TILE : n_rows;
    const uint64_t step = (uint64_t)CC_WAVES * k.R;
    /* (wave-uniform from here: the loop's bounds are, and the exchange below is done by all 64 lanes).  The readings of the
     * next stride are asked for before this one is worked on: other rows, which this wavefront alone writes, later. */
    uint64_t row0 = tile0 + (uint64_t)(threadIdx.x >> 6) * k.R;
    bool have = k.on && row0 + k.r < tile1;
    double v = have ? values[row0 * C + (uint32_t)lane_id()] : 0.0;
    /* vmcnt(0): the first readings are waited for HERE.  Otherwise the compiler takes `v` for pending at the head of the loop --
     * it is, on the way in -- and waits for everything in flight where the loop first touches it: for the readings of the next
     * stride, which have just been asked for.  The fetch-ahead would then hide nothing. */
    __builtin_amdgcn_s_waitcnt(0x0f70);
    while (row0 < tile1) {
        const uint64_t next0 = row0 + step;
        const bool have_next = k.on && next0 + k.r < tile1;
        const double v_next = have_next ? values[next0 * C + (uint32_t)lane_id()] : 0.0;
        const bool usable = qr_usable(v);
        double x = v;
        if (matrix) {
            const double u = usable ? v : 0.0;
            const double *col = cc_mT + k.c;
            if (k.R == 1u) {
                const uint64_t ub = (uint64_t)__double_as_longlong(u);
                x = cc_chain(col, C, [&](uint32_t j) {
                    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)ub, (int)j);
                    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(ub >> 32), (int)j);
                    return __longlong_as_double((long long)((uint64_t)hi << 32 | lo));
                });
            } else {
                x = cc_chain(col, C, [&](uint32_t j) { return __shfl(u, (int)(k.row_lane + j), 64); });
            }
        }
        if (factor) x = x * f;
        x = (x == x && x > 0.0) ? x : 0.0;
        if (have) out[row0 * C + (uint32_t)lane_id()] = usable ? x : v;
        row0 = next0;
        have = have_next;
        v = v_next;
    }
}

__global__ void __launch_bounds__(CS_THREADS) pya_channel_sums_kernel(const double *values, uint64_t n_rows, uint32_t C, const uint8_t *select,
                                                                      double scale, unsigned long long *cell) {
    __shared__ unsigned long long cc_part[CS_WAVES][64][2];
    const CcLane k = cc_lane(C);
    const uint64_t n_strides = (n_rows + k.R - 1) / k.R;
    const uint64_t step = (uint64_t)gridDim.x * CS_WAVES;
    uint64_t sum = 0ull, counts = 0ull;                          /* counts: n | n_saturated << 32 */
    /* (wave-uniform: stride s is the rows s * R .. s * R + R - 1, its readings one run from s * R * C) */
    uint64_t s = (uint64_t)blockIdx.x * CS_WAVES + (threadIdx.x >> 6);
    bool have = k.on && s < n_strides && s * k.R + k.r < n_rows;
    double v = have ? values[s * k.span + (uint32_t)lane_id()] : 0.0;
    uint32_t pick = have && select ? (uint32_t)select[s * k.R + k.r] : 1u;
    __builtin_amdgcn_s_waitcnt(0x0f70);                          /* vmcnt(0), as in the apply: the loop waits for its own loads only */
    while (s < n_strides) {
        const uint64_t next = s + step;
        const bool have_next = k.on && next < n_strides && next * k.R + k.r < n_rows;
        const double v_next = have_next ? values[next * k.span + (uint32_t)lane_id()] : 0.0;
        const uint32_t pick_next = have_next && select ? (uint32_t)select[next * k.R + k.r] : 1u;
        if (have && pick != 0u && qr_usable(v)) {
            bool sat;
            sum += qr_quantum(v, scale, &sat);
            counts += 1ull + (sat ? 1ull << 32 : 0ull);
        }
        s = next;
        have = have_next;
        v = v_next;
        pick = pick_next;
    }
    /* the rows of the stride onto row 0: n rows left, the upper half added onto the lower (all 64 lanes exchange) */
    for (uint32_t n = k.R; n > 1u; n = (n + 1u) >> 1) {
        const uint32_t h = (n + 1u) >> 1;
        const int src = (int)(((uint32_t)lane_id() + h * C) & 63u);
        const uint64_t s2 = __shfl(sum, src, 64), c2 = __shfl(counts, src, 64);
        if (k.on && k.r + h < n) {
            sum += s2;
            counts += c2;
        }
    }
    /* the wavefronts onto the first, then one atomic per (workgroup, channel) and word */
    const uint32_t w = threadIdx.x >> 6, l = (uint32_t)lane_id();
    if (w != 0u && l < C) {
        cc_part[w][l][0] = sum;
        cc_part[w][l][1] = counts;
    }
    __syncthreads();
    if (w == 0u && l < C) {
#pragma unroll
        for (uint32_t o = 1; o < CS_WAVES; o++) {
            sum += cc_part[o][l][0];
            counts += cc_part[o][l][1];
        }
        unsigned long long *p = cell + (size_t)l * 2;
        if (sum) atomicAdd(p, (unsigned long long)sum);
        if (counts) atomicAdd(p + 1, (unsigned long long)counts);
    }
}

/* one wavefront: lane = channel */
__global__ void __launch_bounds__(64) pya_channel_factors_kernel(const unsigned long long *cell, uint32_t C, double *factor) {
    const uint32_t l = (uint32_t)lane_id();
    const uint64_t sum = l < C ? cell[(size_t)l * 2] : 0ull;
    uint64_t top = sum;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t w = __shfl_xor(top, o, 64);
        top = w > top ? w : top;
    }
    if (l < C) factor[l] = sum == 0ull ? 1.0 : (double)top / (double)sum;
}

/* d_values / d_out: n_rows x n_ch doubles (d_out may be d_values); d_matrix: n_ch x n_ch or NULL; d_factor: n_ch or NULL.  The
 * arguments have been checked. */
extern "C" int pya_launch_channel_correct(const double *d_values, uint64_t n_rows, uint32_t n_ch, const double *d_matrix, const double *d_factor,
                                          double *d_out, hipStream_t stream) {
    if (n_rows == 0) return 0;
    const uint64_t blocks = (n_rows + PYA_CHANNEL_TILE - 1) / PYA_CHANNEL_TILE;
    if (blocks > 0x7fffffffull) return (int)hipErrorInvalidValue;
    const size_t lds = d_matrix ? (size_t)n_ch * CC_PITCH * sizeof(double) : 0;
    hipLaunchKernelGGL(pya_channel_correct_kernel, dim3((uint32_t)blocks), dim3(CC_THREADS), lds, stream, d_values, n_rows, n_ch, d_matrix, d_factor,
                       d_out);
    return (int)hipGetLastError();
}

extern "C" int pya_launch_channel_sums(const double *d_values, uint64_t n_rows, uint32_t n_ch, const uint8_t *d_select, double scale, void *d_cell,
                                       hipStream_t stream) {
    if (n_rows == 0) return 0;
    const uint64_t strides = (n_rows + (64u / n_ch) - 1) / (64u / n_ch), want = (strides + CS_WAVES - 1) / CS_WAVES;
    const uint32_t blocks = want > CS_MAX_BLOCKS ? CS_MAX_BLOCKS : (uint32_t)want;
    hipLaunchKernelGGL(pya_channel_sums_kernel, dim3(blocks), dim3(CS_THREADS), 0, stream, d_values, n_rows, n_ch, d_select, scale,
                       (unsigned long long *)d_cell);
    return (int)hipGetLastError();
}

extern "C" int pya_launch_channel_factors(const void *d_cell, uint32_t n_ch, double *d_factor, hipStream_t stream) {
    hipLaunchKernelGGL(pya_channel_factors_kernel, dim3(1), dim3(64), 0, stream, (const unsigned long long *)d_cell, n_ch, d_factor);
    return (int)hipGetLastError();
}
