/* debug_ops.hip -- TEST-ONLY kernels (include/pyascore_debug.h: pya_debug_lookup, pya_debug_lane_ops, pya_debug_wave64,
 * pya_debug_block_scan, pya_debug_ts_scan): the building blocks every production kernel shares -- the peak lookup and its
 * grid, the per-lane arithmetic, the wavefront helpers and the tile scans -- run directly on inputs a test chooses.  The
 * production headers are included as they are; nothing here is on any production path, and no production kernel is
 * instantiated here (tile_sort.hip.h: the scan templates get policies of this file's own).  tests/test_gpu_device_ops.py. */
#include "device_common.hip.h"
#include "lane_f64.hip.h"
#include "tile_sort.hip.h"
#include "../../include/pyascore_debug.h"

/* ---- the lookup ---- */

/* LDS of one wavefront: the grid, then the staged table (16-byte aligned, as in every production layout) */
static size_t dbg_lookup_lds_bytes(uint32_t n) { return PYA_GRID_CELLS * sizeof(uint16_t) + ((size_t)n + PYA_TABLE_PAD) * sizeof(PeakEntry); }

DEV BatchDev dbg_batch(const PeakEntry *table, const uint16_t *grid, const DevConfig *cfg) {
    BatchDev b;
    __builtin_memset(&b, 0, sizeof b);
    b.ret = const_cast<PeakEntry *>(table);
    b.grid = const_cast<uint16_t *>(grid);
    b.cfg = cfg;
    return b;
}

/* one wavefront: stages the table and builds the grid as the scoring kernels do, and leaves the grid in global memory (what
 * score_signatures does for the kernels that look up through global_peak_table_at); cells_out[0 .. 255] the cells,
 * cells_out[256] last_cell */
__global__ __launch_bounds__(64) void pya_debug_grid_kernel(const PeakEntry *table, uint32_t n, const DevConfig *cfg, uint16_t *grid,
                                                            uint32_t *cells_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dbg_lds[];
    uint16_t *cell = (uint16_t *)dbg_lds;
    PeakEntry *e = (PeakEntry *)(dbg_lds + PYA_GRID_CELLS * sizeof(uint16_t));
    const int lane = lane_id();
    const BatchDev b = dbg_batch(table, grid, cfg);
    PeakTable tab;
    stage_peak_table_at(b, 0, (int)n, e, &tab);
    wave_lds_sync();
    grid_build(&tab, cell);
    wave_lds_sync();
    if (n > 0) {
        ((uint64_t *)grid)[lane] = ((const uint64_t *)cell)[lane];
        for (int c = lane; c < PYA_GRID_CELLS; c += 64) cells_out[c] = cell[c];
    } else {
        for (int c = lane; c < PYA_GRID_CELLS; c += 64) {   /* (an empty table has one cell) */
            grid[c] = 0;
            cells_out[c] = c == 0 ? cell[0] : 0u;
        }
    }
    if (lane == 0) cells_out[PYA_GRID_CELLS] = (uint32_t)tab.last_cell;
}

/* a wavefront per 64 queries at a time: out[4 q ..] = match_rank_lds, look4 (+ look_rest), match_rank_global, more();
 * the two look4 bytes are 255 where mz_error > 0.49 (look4 is not for those settings) */
__global__ __launch_bounds__(64) void pya_debug_lookup_kernel(const PeakEntry *table, uint32_t n, const DevConfig *cfg, const uint16_t *grid,
                                                              const float *query, uint32_t n_query, uint8_t *out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dbg_lds[];
    uint16_t *cell = (uint16_t *)dbg_lds;
    PeakEntry *e = (PeakEntry *)(dbg_lds + PYA_GRID_CELLS * sizeof(uint16_t));
    const int lane = lane_id();
    const BatchDev b = dbg_batch(table, grid, cfg);
    PeakTable tab, gtab;
    stage_peak_table_at(b, 0, (int)n, e, &tab);
    wave_lds_sync();
    grid_build(&tab, cell);
    wave_lds_sync();
    global_peak_table_at(b, 0, 0, (int)n, &gtab);
    for (uint32_t q0 = blockIdx.x * 64u; q0 < n_query; q0 += gridDim.x * 64u) {
        const uint32_t q = q0 + (uint32_t)lane;
        if (q >= n_query) continue;
        const float f = query[q];
        uint32_t r_look = 255u, more = 255u;
        if (!tab.half_check) {
            const Look k = look4(tab, f);
            more = k.more() ? 1u : 0u;
            r_look = (uint32_t)(k.more() ? look_rest(tab, k) : k.best);
        }
        const uint32_t r_lds = (uint32_t)match_rank_lds(tab, f);
        const uint32_t r_glb = (uint32_t)match_rank(gtab, f);   /* (gtab.e == NULL: match_rank_global) */
        ((uint32_t *)out)[q] = (r_lds & 255u) | ((r_look & 255u) << 8) | ((r_glb & 255u) << 16) | (more << 24);
    }
}

/* d_table: n entries and at least PYA_TABLE_PAD more behind them (match_rank_global reads up to three entries past the
 * table and masks them); d_grid: PYA_GRID_CELLS cells; d_cells: PYA_GRID_CELLS + 1 words; d_out: 4 bytes per query */
extern "C" int pya_launch_debug_lookup(const void *d_table, uint32_t n, const DevConfig *d_cfg, uint16_t *d_grid, uint32_t *d_cells,
                                       const float *d_query, uint32_t n_query, uint8_t *d_out, hipStream_t stream) {
    const size_t lds = dbg_lookup_lds_bytes(n);
    hipError_t e = PYA_ENSURE_MAX_LDS(pya_debug_grid_kernel);
    if (e != hipSuccess) return (int)e;
    e = PYA_ENSURE_MAX_LDS(pya_debug_lookup_kernel);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(pya_debug_grid_kernel, dim3(1), dim3(64), lds, stream, (const PeakEntry *)d_table, n, d_cfg, d_grid, d_cells);
    if (n_query) {
        const uint32_t blocks = (n_query + 63u) / 64u;
        hipLaunchKernelGGL(pya_debug_lookup_kernel, dim3(blocks < 32u ? blocks : 32u), dim3(64), lds, stream, (const PeakEntry *)d_table, n,
                           d_cfg, (const uint16_t *)d_grid, d_query, n_query, d_out);
    }
    return (int)hipGetLastError();
}

/* ---- one value per lane ---- */
__global__ __launch_bounds__(256) void pya_debug_lane_ops_kernel(uint32_t op, const uint64_t *a, const uint64_t *b, uint64_t n, uint64_t *out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint64_t x = a[i], y = b[i];
    uint64_t r = 0;
    switch (op) {
        case PYA_DBG_FASTDIV: r = fastdiv((uint32_t)x, fastdiv_make((uint32_t)y)); break;
        case PYA_DBG_CHARGE_MZ: r = __float_as_uint(charge_mz(__longlong_as_double((long long)x), (int)y)); break;
        case PYA_DBG_NTH_SET_BIT: r = (uint64_t)(uint32_t)nth_set_bit(x, (int)y); break;
        case PYA_DBG_DEPOSIT_SITES: r = deposit_sites(x, y); break;
        case PYA_DBG_XCD_SLOT: r = xcd_slot((uint32_t)x, (uint32_t)y); break;
        case PYA_DBG_NL_BUMP: r = nl_bump((uint32_t)x, (uint32_t)y); break;
        case PYA_DBG_LUT_ROW: r = lut_row((uint32_t)x); break;
        case PYA_DBG_HIST: {
            /* x: up to 16 ranks of 4 bits; y: how many of them | what to return << 8 (0 .. 15: hist_get, 16 .. 18: a word) */
            Hist h = {0ull, 0ull, 0ull};
            const int cnt = (int)(y & 255u), sel = (int)((y >> 8) & 255u);
            for (int j = 0; j < cnt && j < 16; j++) hist_add(h, (int)((x >> (4 * j)) & 15u));
            r = sel == 16 ? h.a : (sel == 17 ? h.b : (sel == 18 ? h.c : (uint64_t)hist_get(h, sel)));
            break;
        }
        default: r = ~0ull;
    }
    out[i] = r;
}
extern "C" int pya_launch_debug_lane_ops(uint32_t op, const uint64_t *d_a, const uint64_t *d_b, uint64_t n, uint64_t *d_out, hipStream_t stream) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(pya_debug_lane_ops_kernel, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, stream, op, d_a, d_b, n, d_out);
    return (int)hipGetLastError();
}

/* ---- one full wavefront ---- */
/* in: PYA_DBG_WAVE_IN words, out: PYA_DBG_WAVE_OUT words (zeroed by the host); the layout per op is the header's */
__global__ __launch_bounds__(64) void pya_debug_wave64_kernel(uint32_t op, const uint64_t *in, uint64_t *out) {
    const int lane = lane_id();
    const uint64_t v = in[lane];
    switch (op) {
        case PYA_DBG_WAVE_SUM_U64: out[lane] = wave_sum_u64(v); break;
        case PYA_DBG_WAVE_MINMAX_F64: {
            const double d = __longlong_as_double((long long)v);
            out[lane] = (uint64_t)__double_as_longlong(wave_min_f64(d));
            out[64 + lane] = (uint64_t)__double_as_longlong(wave_max_f64(d));
            break;
        }
        case PYA_DBG_MARKER_LANE_F64: {
            const double d = __longlong_as_double((long long)v);
            for (int src = 0; src < 64; src++) out[src * 64 + lane] = (uint64_t)__double_as_longlong(marker_lane_f64(d, src));
            break;
        }
        case PYA_DBG_HIST_WAVE_SUM: {
            Hist h = {v, in[64 + lane], in[128 + lane]};
            h = hist_wave_sum(h);
            out[lane] = h.a;
            out[64 + lane] = h.b;
            out[128 + lane] = h.c;
            break;
        }
        case PYA_DBG_SAME_DIGIT: out[lane] = ts_same_digit((uint32_t)v, in[64 + lane] != 0ull); break;
        default: out[lane] = ~0ull;
    }
}
extern "C" int pya_launch_debug_wave64(uint32_t op, const uint64_t *d_in, uint64_t *d_out, hipStream_t stream) {
    hipLaunchKernelGGL(pya_debug_wave64_kernel, dim3(1), dim3(64), 0, stream, op, d_in, d_out);
    return (int)hipGetLastError();
}

/* ---- the tile scans, over policies of this file's own ---- */
struct DbgAdd {                                              /* a 32-bit sum (wraps) */
    typedef uint32_t T;
    static DEV T identity() { return 0u; }
    static DEV T op(T a, T b) { return a + b; }
};
/* A segmented sum that also keeps the tag of the last flagged entry: three words, associative, NOT commutative.  An entry is
 * (v, f, f ? tag : 0); a before b:  v = b.f ? b.v : a.v + b.v,  f = a.f | b.f,  last = b.f ? b.last : a.last. */
struct DbgSegT {
    uint32_t v, f, last;
};
struct DbgSeg {
    typedef DbgSegT T;
    static DEV T identity() {
        T x = {0u, 0u, 0u};
        return x;
    }
    static DEV T op(T a, T b) {
        T x;
        x.v = b.f ? b.v : a.v + b.v;
        x.f = a.f | b.f;
        x.last = b.f ? b.last : a.last;
        return x;
    }
};

/* ts_block_scan by one workgroup: out[0 .. 255] the exclusive scan, out[256] the total */
template <typename S>
__global__ void __launch_bounds__(TS_THREADS) pya_debug_block_scan_kernel(const typename S::T *in, typename S::T *out) {
    typedef typename S::T T;
    __shared__ T lds[TS_THREADS / 64];
    T total;
    out[threadIdx.x] = ts_block_scan<S>(in[threadIdx.x], lds, &total);
    if (threadIdx.x == TS_THREADS - 1) out[TS_THREADS] = total;
}
extern "C" int pya_launch_debug_block_scan(uint32_t policy, const uint32_t *d_in, uint32_t *d_out, hipStream_t stream) {
    if (policy == PYA_DBG_SCAN_ADD)
        hipLaunchKernelGGL(pya_debug_block_scan_kernel<DbgAdd>, dim3(1), dim3(TS_THREADS), 0, stream, d_in, d_out);
    else
        hipLaunchKernelGGL(pya_debug_block_scan_kernel<DbgSeg>, dim3(1), dim3(TS_THREADS), 0, stream, (const DbgSegT *)d_in, (DbgSegT *)d_out);
    return (int)hipGetLastError();
}

/* entries (of the policy's words) a scan over n entries needs behind each other: tile_sort.hip.h, ts_levels_total */
extern "C" uint64_t pya_ts_scan_entries(uint64_t n) { return ts_levels_total(n); }
/* ts_scan in place over d_data[n] (+ the levels above it) */
extern "C" int pya_launch_debug_ts_scan(uint32_t policy, uint32_t *d_data, uint64_t n, hipStream_t stream) {
    if (n == 0) return 0;
    if (policy == PYA_DBG_SCAN_ADD) return (int)ts_scan<DbgAdd>(d_data, n, stream);
    return (int)ts_scan<DbgSeg>((DbgSegT *)d_data, n, stream);
}
