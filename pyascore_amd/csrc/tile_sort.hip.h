/* tile_sort.hip.h -- what the two stages built as grids over tiles share (flr.hip, peptidoforms.hip): the tile geometry, one
 * block scan, one multi-level scan and one stable radix sort.  Every launch is a grid over tiles of TS_TILE elements and KERNEL
 * BOUNDARIES ARE THE ONLY GRID-WIDE SYNCHRONISATION: no kernel waits on another workgroup.  Everything is launched on the
 * caller's stream into memory the caller lends; nothing is allocated and the host waits for nothing.
 *
 *   scan      reduce-then-scan with three kernels (reduce / scan_block / apply, 256 entries per workgroup) over as many levels
 *             as the length needs: 256 * n_tiles histogram entries are two levels from the second tile and three from the 257th.
 *             What is scanned is a policy S: a type S::T (trivially copyable, whole 32-bit words), S::identity() and S::op(a, b)
 *             with a before b; op is associative and need not commute.
 *   sort      a stable LSD radix sort over a key policy K (below), K::passes passes of 8 bits, none skipped.  A pass is:
 *               histogram  per tile, 256 digit counts in LDS -> hist[digit * n_tiles + tile];
 *               scan       the exclusive prefix sum of that array as it lies (digit-major: every smaller digit of every tile,
 *                          then the same digit of the earlier tiles) is the place of a tile's first element of a digit;
 *               scatter    a wave owns 256 consecutive elements of the tile, 64 at a time; the lanes that hold one digit find
 *                          each other with eight ballots, a lane's rank among them is v_mbcnt of that mask, and the wave's
 *                          running count per digit lives in LDS (one wave touches one row: no atomics).  Ranks are in index
 *                          order, so the pass is stable.  Every store is guarded by its index.
 * The kernels are templates and the library is linked from separate objects, each of which registers its own code object
 * against the host stub's address, so NO KERNEL MAY BE INSTANTIATED OVER THE SAME TYPES IN TWO OBJECTS: a stage instantiates
 * them over policies of its own (the count scan under a sort is TsCount<K>, which carries the stage's key policy). */
#ifndef PYA_TILE_SORT_H
#define PYA_TILE_SORT_H
#include <type_traits>
#include "device_common.hip.h"
#include "../../include/pyascore_hip.h"

#define TS_THREADS 256
#define TS_ITEMS 4
#define TS_TILE (TS_THREADS * TS_ITEMS)
#define TS_WAVE_SPAN (64 * TS_ITEMS)          /* consecutive elements of a tile one wave owns */
#define TS_BINS 256
static_assert(TS_TILE == PYA_FLR_TILE && TS_TILE == PYA_PFORM_TILE, "the tile sizes the header exports");
static_assert(TS_BINS == TS_THREADS, "one digit per thread where a tile's counts are combined");

/* 256-byte parts of a lent workspace */
static inline uint64_t ts_round(uint64_t b) { return (b + 255u) & ~(uint64_t)255u; }
/* records the next phase event of a launcher (its `phase`, NULL for none, `ph`, `st` and `e`) */
#define TS_PHASE()                                                                \
    do {                                                                          \
        if (phase && (e = hipEventRecord(phase[ph++], st)) != hipSuccess) return (int)e; \
    } while (0)

/* ---- the block scan ---- */
template <typename T>
DEV T ts_shfl_up(const T &v, int o) {
    static_assert(std::is_trivially_copyable<T>::value && sizeof(T) % 4 == 0, "shuffled word by word");
    union U {
        T t;
        uint32_t w[sizeof(T) / 4];
        DEV U() {}
    } a, r;
    a.t = v;
#pragma unroll
    for (unsigned k = 0; k < sizeof(T) / 4; k++) r.w[k] = __shfl_up(a.w[k], o, 64);
    return r.t;
}

/* EXCLUSIVE scan over the 256 threads of a workgroup in thread order; every thread takes part.  lds: 4 entries.  *total: the
 * workgroup's. */
template <typename S>
DEV typename S::T ts_block_scan(typename S::T v, typename S::T *lds, typename S::T *total) {
    typedef typename S::T T;
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T y = ts_shfl_up(v, o);
        if (lane >= o) v = S::op(y, v);
    }
    T ex = ts_shfl_up(v, 1);
    if (lane == 0) ex = S::identity();
    __syncthreads();                                      /* (lds may still be read from the call before) */
    if (lane == 63) lds[wave] = v;
    __syncthreads();
    T before = S::identity(), all = S::identity();
#pragma unroll
    for (int w = 0; w < TS_THREADS / 64; w++) {
        const T x = lds[w];
        if (w < wave) before = S::op(before, x);
        all = S::op(all, x);
    }
    *total = all;
    return S::op(before, ex);
}

/* ---- the multi-level scan ---- */
/* sums[b] = the entries b * 256 .. of in[n] combined */
template <typename S>
__global__ void __launch_bounds__(TS_THREADS) pya_ts_reduce_kernel(const typename S::T *in, uint64_t n, typename S::T *sums) {
    typedef typename S::T T;
    __shared__ T lds[TS_THREADS / 64];
    const uint64_t i = (uint64_t)blockIdx.x * TS_THREADS + threadIdx.x;
    T total;
    ts_block_scan<S>(i < n ? in[i] : S::identity(), lds, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}
/* data[n], n <= 256, one workgroup: the exclusive scan in place */
template <typename S>
__global__ void __launch_bounds__(TS_THREADS) pya_ts_scan_block_kernel(typename S::T *data, uint32_t n) {
    typedef typename S::T T;
    __shared__ T lds[TS_THREADS / 64];
    const uint32_t i = threadIdx.x;
    T total;
    const T ex = ts_block_scan<S>(i < n ? data[i] : S::identity(), lds, &total);
    if (i < n) data[i] = ex;
}
/* data[n] in place: the exclusive scan of every run of 256 entries, started from offs[block] (the scanned sums) */
template <typename S>
__global__ void __launch_bounds__(TS_THREADS) pya_ts_apply_kernel(typename S::T *data, uint64_t n, const typename S::T *offs) {
    typedef typename S::T T;
    __shared__ T lds[TS_THREADS / 64];
    const uint64_t i = (uint64_t)blockIdx.x * TS_THREADS + threadIdx.x;
    T total;
    const T ex = ts_block_scan<S>(i < n ? data[i] : S::identity(), lds, &total);
    if (i < n) data[i] = S::op(offs[blockIdx.x], ex);
}

/* the number of entries of level l + 1 over a level of n entries */
static inline uint64_t ts_up(uint64_t n) { return (n + TS_THREADS - 1) / TS_THREADS; }
/* entries of every level of a scan over n entries together: n + ceil(n / 256) + ... down to a level of at most 256 */
static inline uint64_t ts_levels_total(uint64_t n) {
    uint64_t total = n;
    while (n > TS_THREADS) {
        n = ts_up(n);
        total += n;
    }
    return total;
}
/* the exclusive scan of data[n] in place; the levels above it follow it in memory (ts_levels_total entries in all) */
template <typename S>
static hipError_t ts_scan(typename S::T *data, uint64_t n, hipStream_t st) {
    typedef typename S::T T;
    T *level[8];
    uint64_t len[8];
    int top = 0;
    level[0] = data;
    len[0] = n;
    while (len[top] > TS_THREADS) {
        level[top + 1] = level[top] + len[top];
        len[top + 1] = ts_up(len[top]);
        top++;                                            /* (2^39 entries would be five levels) */
    }
    for (int l = 0; l < top; l++)
        hipLaunchKernelGGL(pya_ts_reduce_kernel<S>, dim3((uint32_t)len[l + 1]), dim3(TS_THREADS), 0, st, (const T *)level[l], len[l], level[l + 1]);
    hipLaunchKernelGGL(pya_ts_scan_block_kernel<S>, dim3(1), dim3(TS_THREADS), 0, st, level[top], (uint32_t)len[top]);
    for (int l = top - 1; l >= 0; l--)
        hipLaunchKernelGGL(pya_ts_apply_kernel<S>, dim3((uint32_t)len[l + 1]), dim3(TS_THREADS), 0, st, level[l], len[l], (const T *)level[l + 1]);
    return hipGetLastError();
}

/* ---- the radix sort ----
 * A key policy K:  K::E         an element as a thread holds it, K::none() one that is never stored;
 *                  K::Buf       one of the two buffers the passes go between (pointers; passed to the kernels by value);
 *                  K::passes    how many;
 *                  K::digit(e, pass)            0 .. 255;
 *                  K::load(buf, i), K::store(buf, i, e)   the whole element;
 *                  K::load_digit(buf, i, pass)  as much of it as digit(., pass) reads: the histogram moves nothing else. */
template <typename K>
struct TsCount {
    typedef uint32_t T;
    static DEV T identity() { return 0u; }
    static DEV T op(T a, T b) { return a + b; }
};
/* the lanes of the wave that are `in` and hold digit d (every lane calls this) */
DEV uint64_t ts_same_digit(uint32_t d, bool in) {
    uint64_t m = __ballot(in);
#pragma unroll
    for (int b = 0; b < 8; b++) {
        const bool bit = (d >> b) & 1u;
        const uint64_t v = __ballot(bit);
        m &= bit ? v : ~v;
    }
    return m;
}

template <typename K>
__global__ void __launch_bounds__(TS_THREADS) pya_ts_hist_kernel(const typename K::Buf src, uint32_t n, uint32_t n_tiles, int pass, uint32_t *hist) {
    __shared__ uint32_t cnt[TS_BINS];
    cnt[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t base = blockIdx.x * TS_TILE + (threadIdx.x >> 6) * TS_WAVE_SPAN + (uint32_t)lane_id();
#pragma unroll
    for (int r = 0; r < TS_ITEMS; r++) {
        const uint32_t i = base + r * 64;
        const bool in = i < n;
        const uint32_t d = in ? K::digit(K::load_digit(src, i, pass), pass) : 0u;
        const uint64_t m = ts_same_digit(d, in);
        if (in && mask_rank(m) == 0) atomicAdd(&cnt[d], (uint32_t)__popcll(m));
    }
    __syncthreads();
    hist[(size_t)threadIdx.x * n_tiles + blockIdx.x] = cnt[threadIdx.x];
}

template <typename K>
__global__ void __launch_bounds__(TS_THREADS) pya_ts_scatter_kernel(const typename K::Buf src, uint32_t n, uint32_t n_tiles, int pass,
                                                                    const uint32_t *offs, const typename K::Buf dst) {
    __shared__ uint32_t cnt[TS_THREADS / 64][TS_BINS];    /* a wave's running count of every digit, then the waves' before it */
    __shared__ uint32_t first[TS_BINS];                   /* where the tile's first element of a digit goes */
    const int wave = (int)(threadIdx.x >> 6);
#pragma unroll
    for (int w = 0; w < TS_THREADS / 64; w++) cnt[w][threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t base = blockIdx.x * TS_TILE + (uint32_t)wave * TS_WAVE_SPAN + (uint32_t)lane_id();
    typename K::E k[TS_ITEMS];
    uint32_t d[TS_ITEMS], rk[TS_ITEMS];
#pragma unroll
    for (int r = 0; r < TS_ITEMS; r++) k[r] = base + r * 64 < n ? K::load(src, base + r * 64) : K::none();
#pragma unroll
    for (int r = 0; r < TS_ITEMS; r++) {
        const bool in = base + r * 64 < n;
        d[r] = in ? K::digit(k[r], pass) : 0u;
        const uint64_t m = ts_same_digit(d[r], in);
        const uint32_t mine = (uint32_t)mask_rank(m);
        const uint32_t seen = cnt[wave][d[r]];            /* the row is this wave's alone, and a wave's LDS traffic is in order */
        rk[r] = seen + mine;
        wave_lds_sync();
        if (in && mine == 0u) cnt[wave][d[r]] = seen + (uint32_t)__popcll(m);
        wave_lds_sync();
    }
    __syncthreads();
    {
        uint32_t run = 0u;
#pragma unroll
        for (int w = 0; w < TS_THREADS / 64; w++) {
            const uint32_t c = cnt[w][threadIdx.x];
            cnt[w][threadIdx.x] = run;
            run += c;
        }
        first[threadIdx.x] = offs[(size_t)threadIdx.x * n_tiles + blockIdx.x];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < TS_ITEMS; r++) {
        if (base + r * 64 < n) {
            const uint32_t to = first[d[r]] + cnt[wave][d[r]] + rk[r];
            if (to < n) K::store(dst, to, k[r]);
        }
    }
}

/* Sorts the n elements of buf[0] between buf[0] and buf[1]; *cur: the buffer that holds them afterwards.  hist:
 * ts_levels_total(256 * n_tiles) counts.  before_pass: NULL, or K::passes events, one recorded before every pass. */
template <typename K>
static hipError_t ts_sort(const typename K::Buf *buf, uint32_t n, uint32_t *hist, hipEvent_t *before_pass, hipStream_t st, int *cur) {
    const uint32_t n_tiles = (n + TS_TILE - 1) / TS_TILE;
    hipError_t e;
    *cur = 0;
    for (int pass = 0; pass < K::passes; pass++) {
        if (before_pass && (e = hipEventRecord(before_pass[pass], st)) != hipSuccess) return e;
        hipLaunchKernelGGL(pya_ts_hist_kernel<K>, dim3(n_tiles), dim3(TS_THREADS), 0, st, buf[*cur], n, n_tiles, pass, hist);
        if ((e = ts_scan<TsCount<K>>(hist, (uint64_t)TS_BINS * n_tiles, st)) != hipSuccess) return e;
        hipLaunchKernelGGL(pya_ts_scatter_kernel<K>, dim3(n_tiles), dim3(TS_THREADS), 0, st, buf[*cur], n, n_tiles, pass, (const uint32_t *)hist,
                           buf[*cur ^ 1]);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        *cur ^= 1;
    }
    return hipSuccess;
}

#endif
