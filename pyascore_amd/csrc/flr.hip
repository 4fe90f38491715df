/* flr.hip -- false-localisation rates over a roll-up table: a global sort of the slots by best_prob and scans over the
 * sorted order, on the table where rollup.hip left it.  The definition is in include/pyascore_hip.h (pya_site_flr); the
 * reference has no counterpart.  The first kernels of this tree that are neither "one PSM per wavefront" nor a scatter of
 * atomics: every launch is a grid over tiles of FL_TILE slots, and KERNEL BOUNDARIES ARE THE ONLY GRID-WIDE SYNCHRONISATION --
 * no kernel waits on another workgroup (no look-back, no flag, no cooperative launch), so nothing here can hang a card whose
 * workgroups are not co-resident.  Everything is launched on the caller's stream into the caller's workspace; nothing is
 * allocated and the host waits for nothing.
 *
 *   keys      one thread per slot: key = ~bits(best_prob) of a ranked slot, all-ones otherwise; payload = the slot index, bit
 *             31 set for an unranked slot (n_slots <= 2^31 - 1 leaves the bit free).  p = +0.0 of a ranked slot has the
 *             all-ones key as well, which is why the unranked tail is split off by a pass of its own on that bit and not by
 *             the key.  Counts the ranked slots and the class bytes that are none of 0 / 1 / 2.
 *   sort      a stable LSD radix sort of (key, payload): FL_PASSES = 9 passes, eight over the bytes of the key from the
 *             lowest, the last over payload bit 31.  No pass is skipped.  A pass is three steps:
 *               histogram  per tile, 256 digit counts in LDS -> hist[digit * n_tiles + tile];
 *               scan       the exclusive prefix sum of that array as it lies (digit-major: every smaller digit of every tile,
 *                          then the same digit of the earlier tiles) is the place of a tile's first key of a digit;
 *               scatter    a wave owns 256 consecutive keys of the tile, 64 at a time; the lanes that hold one digit find
 *                          each other with eight ballots, a lane's rank among them is v_mbcnt of that mask, and the wave's
 *                          running count per digit lives in LDS (one wave touches one row: no atomics).  Ranks are in index
 *                          order, so the pass is stable.
 *   records   over the sorted order: tile sums of (1, decoy, err) -> exclusive scan; then the values at the END of a tie group
 *             reach its members and the running minimum of the decoy ratio reaches every better site by ONE backward scan --
 *             rank strictly rises from one group end to the next, so "the nearest group end at or behind me" is the element
 *             with the smallest rank, a commutative min, and the ratio takes a plain min beside it.  Tile minima -> exclusive
 *             scan (stored back to front) -> the last kernel recomputes both in-tile scans and writes the record of every
 *             slot (zero bytes for an unranked one) and the order.
 * Every multi-workgroup scan is reduce-then-scan with one set of three kernels (fl_reduce / fl_scan_block / fl_apply, 256
 * entries per workgroup) over as many levels as the length needs: 256 * n_tiles histogram entries are two levels from the
 * second tile and three from the 257th.
 * Sums are integers (err is the 2^32-scaled error truncated to a uint64), so no result depends on the order of anything.
 * No write lies outside d_out[0 .. n), d_order[0 .. n), d_n_ranked[0 .. 2) and the workspace bytes fl_layout() counts: every
 * scatter and record store is guarded by its index, and a payload indexes d_out only below n. */
#include "device_common.hip.h"
#include "../../include/pyascore_hip.h"

#define FL_THREADS 256
#define FL_ITEMS 4
#define FL_TILE (FL_THREADS * FL_ITEMS)
#define FL_WAVE_SPAN (64 * FL_ITEMS)          /* consecutive keys of a tile one wave owns */
#define FL_BINS 256
#define FL_PASSES 9
#define FL_UNRANKED 0x80000000u
static_assert(FL_TILE == PYA_FLR_TILE, "the tile size the header exports");
static_assert(FL_BINS == FL_THREADS, "one digit per thread where a tile's counts are combined");

/* ---- what is scanned: a type, an identity, a commutative and associative operator ---- */
struct FlAddU32 {
    typedef uint32_t T;
    static DEV T identity() { return 0u; }
    static DEV T op(T a, T b) { return a + b; }
    static DEV T shfl_up(T v, int o) { return __shfl_up(v, o, 64); }
};
/* (1, decoy, err) of the ranked slots: n = count (low word) | decoys (high word), neither reaches 2^31 */
struct FlSum {
    uint64_t n, err;
};
struct FlAddSum {
    typedef FlSum T;
    static DEV T identity() { return FlSum{0ull, 0ull}; }
    static DEV T op(T a, T b) { return FlSum{a.n + b.n, a.err + b.err}; }
    static DEV T shfl_up(T v, int o) { return FlSum{__shfl_up(v.n, o, 64), __shfl_up(v.err, o, 64)}; }
};
/* a group end: key = rank << 32 | n_decoy of the cut, err its error sum, q its decoy ratio; anything else is the identity.
 * op keeps (key, err) of the smaller key -- the nearest end -- and the smaller q */
struct FlEnd {
    uint64_t key, err;
    double q;
};
struct FlNearestEnd {
    typedef FlEnd T;
    static DEV T identity() { return FlEnd{~0ull, ~0ull, __builtin_huge_val()}; }
    static DEV T op(T a, T b) {
        const bool first = a.key <= b.key;
        return FlEnd{first ? a.key : b.key, first ? a.err : b.err, b.q < a.q ? b.q : a.q};
    }
    static DEV T shfl_up(T v, int o) { return FlEnd{__shfl_up(v.key, o, 64), __shfl_up(v.err, o, 64), __shfl_up(v.q, o, 64)}; }
};

/* inclusive scan over the 256 threads of a workgroup, thread order; every thread takes part.  lds: 4 entries.  *total: the
 * workgroup's. */
template <typename S>
DEV typename S::T fl_block_scan(typename S::T v, typename S::T *lds, typename S::T *total) {
    typedef typename S::T T;
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T y = S::shfl_up(v, o);
        if (lane >= o) v = S::op(y, v);
    }
    __syncthreads();                                      /* (lds may still be read from the call before) */
    if (lane == 63) lds[wave] = v;
    __syncthreads();
    T before = S::identity(), all = S::identity();
#pragma unroll
    for (int w = 0; w < FL_THREADS / 64; w++) {
        const T x = lds[w];
        if (w < wave) before = S::op(before, x);
        all = S::op(all, x);
    }
    *total = all;
    return S::op(before, v);
}

/* sums[b] = the entries b * 256 .. of in[n] combined */
template <typename S>
__global__ void __launch_bounds__(FL_THREADS) pya_flr_reduce_kernel(const typename S::T *in, uint64_t n, typename S::T *sums) {
    typedef typename S::T T;
    __shared__ T lds[FL_THREADS / 64];
    const uint64_t i = (uint64_t)blockIdx.x * FL_THREADS + threadIdx.x;
    T total;
    fl_block_scan<S>(i < n ? in[i] : S::identity(), lds, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}
/* data[n], n <= 256, one workgroup: the exclusive scan in place */
template <typename S>
__global__ void __launch_bounds__(FL_THREADS) pya_flr_scan_block_kernel(typename S::T *data, uint32_t n) {
    typedef typename S::T T;
    __shared__ T lds[FL_THREADS / 64];
    const uint32_t i = threadIdx.x;
    const T v = i < n ? data[i] : S::identity();
    T total;
    const T incl = fl_block_scan<S>(v, lds, &total);
    /* exclusive = everything before me: the inclusive value of the thread before */
    const T prev = S::shfl_up(incl, 1);
    __syncthreads();
    if ((i & 63u) == 63u) lds[i >> 6] = incl;
    __syncthreads();
    T ex = (i & 63u) ? prev : (i ? lds[(i >> 6) - 1] : S::identity());
    if (i < n) data[i] = ex;
}
/* data[n] in place: the exclusive scan of every run of 256 entries, started from offs[block] (the scanned sums) */
template <typename S>
__global__ void __launch_bounds__(FL_THREADS) pya_flr_apply_kernel(typename S::T *data, uint64_t n, const typename S::T *offs) {
    typedef typename S::T T;
    __shared__ T lds[FL_THREADS / 64];
    const uint64_t i = (uint64_t)blockIdx.x * FL_THREADS + threadIdx.x;
    const T v = i < n ? data[i] : S::identity();
    T total;
    const T incl = fl_block_scan<S>(v, lds, &total);
    const T prev = S::shfl_up(incl, 1);
    __syncthreads();
    if ((threadIdx.x & 63u) == 63u) lds[threadIdx.x >> 6] = incl;
    __syncthreads();
    const T ex = (threadIdx.x & 63u) ? prev : (threadIdx.x ? lds[(threadIdx.x >> 6) - 1] : S::identity());
    if (i < n) data[i] = S::op(offs[blockIdx.x], ex);
}

/* the number of entries of level l + 1 over a level of n entries */
static inline uint64_t fl_up(uint64_t n) { return (n + FL_THREADS - 1) / FL_THREADS; }
/* entries of every level of a scan over n entries together: n + ceil(n / 256) + ... down to a level of at most 256 */
static uint64_t fl_levels_total(uint64_t n) {
    uint64_t total = n;
    while (n > FL_THREADS) {
        n = fl_up(n);
        total += n;
    }
    return total;
}
/* the exclusive scan of data[n] in place; the levels above it follow it in memory (fl_levels_total entries in all) */
template <typename S>
static hipError_t fl_scan(typename S::T *data, uint64_t n, hipStream_t st) {
    typedef typename S::T T;
    T *level[8];
    uint64_t len[8];
    int top = 0;
    level[0] = data;
    len[0] = n;
    while (len[top] > FL_THREADS) {
        level[top + 1] = level[top] + len[top];
        len[top + 1] = fl_up(len[top]);
        top++;                                            /* (2^39 entries would be five levels) */
    }
    for (int l = 0; l < top; l++)
        hipLaunchKernelGGL(pya_flr_reduce_kernel<S>, dim3((uint32_t)len[l + 1]), dim3(FL_THREADS), 0, st, (const T *)level[l], len[l], level[l + 1]);
    hipLaunchKernelGGL(pya_flr_scan_block_kernel<S>, dim3(1), dim3(FL_THREADS), 0, st, level[top], (uint32_t)len[top]);
    for (int l = top - 1; l >= 0; l--)
        hipLaunchKernelGGL(pya_flr_apply_kernel<S>, dim3((uint32_t)len[l + 1]), dim3(FL_THREADS), 0, st, level[l], len[l], (const T *)level[l + 1]);
    return hipGetLastError();
}

/* ---- keys ---- */
__global__ void __launch_bounds__(FL_THREADS) pya_flr_keys_kernel(const uint4 *table, const uint8_t *cls, uint32_t n, uint32_t reported_only,
                                                                  uint64_t *keys, uint32_t *pay, uint32_t *n_ranked) {
    const uint32_t s = blockIdx.x * FL_THREADS + threadIdx.x;
    const bool in = s < n;
    bool ranked = false, bad = false;
    uint64_t bits = 0;
    if (in) {
        const uint4 a = table[(size_t)s * 2];             /* best_prob | best_psm | n_psm */
        bits = (uint64_t)a.y << 32 | a.x;
        const uint32_t c = cls ? (uint32_t)cls[s] : 0u;
        bad = c > 2u;
        ranked = a.w != 0u && c < 2u;
        if (reported_only) ranked = ranked && table[(size_t)s * 2 + 1].y != 0u;      /* n_confident | n_in_best | ... */
        keys[s] = ranked ? ~bits : ~0ull;
        pay[s] = ranked ? s : s | FL_UNRANKED;
    }
    const uint64_t r = __ballot(ranked), b = __ballot(bad);
    if (lane_id() == 0) {
        if (r) atomicAdd(&n_ranked[0], (uint32_t)__popcll(r));
        if (b) atomicAdd(&n_ranked[1], (uint32_t)__popcll(b));
    }
}

/* ---- sort ---- */
DEV uint32_t fl_digit(uint64_t key, uint32_t pay, int pass) {
    return pass < 8 ? (uint32_t)(key >> (8 * pass)) & 0xffu : pay >> 31;
}
/* the lanes of the wave that are `in` and hold digit d (every lane calls this) */
DEV uint64_t fl_same_digit(uint32_t d, bool in) {
    uint64_t m = __ballot(in);
#pragma unroll
    for (int b = 0; b < 8; b++) {
        const bool bit = (d >> b) & 1u;
        const uint64_t v = __ballot(bit);
        m &= bit ? v : ~v;
    }
    return m;
}

__global__ void __launch_bounds__(FL_THREADS) pya_flr_hist_kernel(const uint64_t *keys, const uint32_t *pay, uint32_t n, uint32_t n_tiles, int pass,
                                                                  uint32_t *hist) {
    __shared__ uint32_t cnt[FL_BINS];
    cnt[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t base = blockIdx.x * FL_TILE + (threadIdx.x >> 6) * FL_WAVE_SPAN + (uint32_t)lane_id();
#pragma unroll
    for (int r = 0; r < FL_ITEMS; r++) {
        const uint32_t i = base + r * 64;
        const bool in = i < n;
        const uint32_t d = in ? fl_digit(keys[i], pass == 8 ? pay[i] : 0u, pass) : 0u;
        const uint64_t m = fl_same_digit(d, in);
        if (in && mask_rank(m) == 0) atomicAdd(&cnt[d], (uint32_t)__popcll(m));
    }
    __syncthreads();
    hist[(size_t)threadIdx.x * n_tiles + blockIdx.x] = cnt[threadIdx.x];
}

__global__ void __launch_bounds__(FL_THREADS) pya_flr_scatter_kernel(const uint64_t *keys, const uint32_t *pay, uint32_t n, uint32_t n_tiles, int pass,
                                                                     const uint32_t *offs, uint64_t *keys_out, uint32_t *pay_out) {
    __shared__ uint32_t cnt[FL_THREADS / 64][FL_BINS];    /* a wave's running count of every digit, then the waves' before it */
    __shared__ uint32_t first[FL_BINS];                   /* where the tile's first key of a digit goes */
    const int wave = (int)(threadIdx.x >> 6);
#pragma unroll
    for (int w = 0; w < FL_THREADS / 64; w++) cnt[w][threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t base = blockIdx.x * FL_TILE + (uint32_t)wave * FL_WAVE_SPAN + (uint32_t)lane_id();
    uint64_t k[FL_ITEMS];
    uint32_t p[FL_ITEMS], d[FL_ITEMS], rk[FL_ITEMS];
#pragma unroll
    for (int r = 0; r < FL_ITEMS; r++) {
        const uint32_t i = base + r * 64;
        const bool in = i < n;
        k[r] = in ? keys[i] : 0ull;
        p[r] = in ? pay[i] : 0u;
    }
#pragma unroll
    for (int r = 0; r < FL_ITEMS; r++) {
        const bool in = base + r * 64 < n;
        d[r] = in ? fl_digit(k[r], p[r], pass) : 0u;
        const uint64_t m = fl_same_digit(d[r], in);
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
        for (int w = 0; w < FL_THREADS / 64; w++) {
            const uint32_t c = cnt[w][threadIdx.x];
            cnt[w][threadIdx.x] = run;
            run += c;
        }
        first[threadIdx.x] = offs[(size_t)threadIdx.x * n_tiles + blockIdx.x];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < FL_ITEMS; r++) {
        if (base + r * 64 < n) {
            const uint32_t dst = first[d[r]] + cnt[wave][d[r]] + rk[r];
            if (dst < n) {
                keys_out[dst] = k[r];
                pay_out[dst] = p[r];
            }
        }
    }
}

/* ---- records ---- */
struct FlRecArgs {
    const uint64_t *keys;             /* sorted */
    const uint32_t *pay;
    const uint8_t *cls;               /* or NULL */
    uint32_t n, n_tiles;
    FlSum *sums;                      /* [n_tiles]: tile sums, then their exclusive scan */
    FlEnd *ends;                      /* [n_tiles], BACK TO FRONT (entry t is tile n_tiles - 1 - t): tile minima, then their scan */
    uint4 *out;                       /* pya_site_flr as 2 x 16 bytes */
    uint32_t *order;                  /* or NULL */
};
/* err(p) of the header: one double subtraction, an exact scaling, truncation */
DEV uint64_t fl_err(uint64_t bits) {
    const double d = 1.0 - __longlong_as_double((long long)bits);
    return (uint64_t)((d > 0.0 ? d : 0.0) * 4294967296.0);
}
/* the sorted position i as a contribution to the sums */
DEV FlSum fl_element(const FlRecArgs &a, uint32_t i, uint64_t *key, uint32_t *pay) {
    *key = ~0ull;
    *pay = FL_UNRANKED;
    if (i >= a.n) return FlSum{0ull, 0ull};
    *key = a.keys[i];
    *pay = a.pay[i];
    if (*pay & FL_UNRANKED) return FlSum{0ull, 0ull};
    const uint32_t slot = *pay;
    const uint64_t decoy = (a.cls && slot < a.n && a.cls[slot] == 1u) ? 1ull : 0ull;
    return FlSum{1ull | decoy << 32, fl_err(~*key)};
}

/* A thread holds FL_ITEMS CONSECUTIVE positions here (tile * FL_TILE + thread * FL_ITEMS + j): its own run is scanned in
 * registers, the threads' totals by fl_block_scan. */
__global__ void __launch_bounds__(FL_THREADS) pya_flr_tile_sums_kernel(const FlRecArgs a) {
    __shared__ FlSum lds[FL_THREADS / 64];
    const uint32_t i0 = blockIdx.x * FL_TILE + threadIdx.x * FL_ITEMS;
    FlSum mine = FlAddSum::identity();
#pragma unroll
    for (int j = 0; j < FL_ITEMS; j++) {
        uint64_t key;
        uint32_t pay;
        mine = FlAddSum::op(mine, fl_element(a, i0 + j, &key, &pay));
    }
    FlSum total;
    fl_block_scan<FlAddSum>(mine, lds, &total);
    if (threadIdx.x == 0) a.sums[blockIdx.x] = total;
}

/* the inclusive sums at the thread's FL_ITEMS positions and the group ends among them (identity elsewhere) */
DEV void fl_tile_ends(const FlRecArgs &a, FlSum *lds, uint32_t *pay, FlEnd *e) {
    const uint32_t i0 = blockIdx.x * FL_TILE + threadIdx.x * FL_ITEMS;
    uint64_t key[FL_ITEMS + 1];
    uint32_t next_pay;
    FlSum v[FL_ITEMS], mine = FlAddSum::identity();
#pragma unroll
    for (int j = 0; j < FL_ITEMS; j++) {
        v[j] = fl_element(a, i0 + j, &key[j], &pay[j]);
        mine = FlAddSum::op(mine, v[j]);
        v[j] = mine;
    }
    /* the position behind the thread's last: of another thread or another tile */
    key[FL_ITEMS] = ~0ull;
    next_pay = FL_UNRANKED;
    if (i0 + FL_ITEMS < a.n) {
        key[FL_ITEMS] = a.keys[i0 + FL_ITEMS];
        next_pay = a.pay[i0 + FL_ITEMS];
    }
    FlSum total;
    const FlSum incl = fl_block_scan<FlAddSum>(mine, lds, &total);
    const FlSum before = FlAddSum::op(a.sums[blockIdx.x], FlSum{incl.n - mine.n, incl.err - mine.err});
#pragma unroll
    for (int j = 0; j < FL_ITEMS; j++) {
        const bool ranked = !(pay[j] & FL_UNRANKED);
        const bool next_ranked = !((j + 1 < FL_ITEMS ? pay[j + 1] : next_pay) & FL_UNRANKED);
        e[j] = FlNearestEnd::identity();
        if (ranked && (!next_ranked || key[j + 1] != key[j])) {
            const FlSum c = FlAddSum::op(before, v[j]);
            const uint32_t rank = (uint32_t)c.n, n_decoy = (uint32_t)(c.n >> 32), targets = rank - n_decoy;
            e[j].key = (uint64_t)rank << 32 | n_decoy;
            e[j].err = c.err;
            e[j].q = (double)n_decoy / (double)(targets ? targets : 1u);
        }
    }
}

__global__ void __launch_bounds__(FL_THREADS) pya_flr_tile_ends_kernel(const FlRecArgs a) {
    __shared__ FlSum lds[FL_THREADS / 64];
    __shared__ FlEnd lds_e[FL_THREADS / 64];
    uint32_t pay[FL_ITEMS];
    FlEnd e[FL_ITEMS], mine = FlNearestEnd::identity();
    fl_tile_ends(a, lds, pay, e);
#pragma unroll
    for (int j = 0; j < FL_ITEMS; j++) mine = FlNearestEnd::op(mine, e[j]);
    FlEnd total;
    fl_block_scan<FlNearestEnd>(mine, lds_e, &total);
    if (threadIdx.x == 0) a.ends[a.n_tiles - 1u - blockIdx.x] = total;
}

__global__ void __launch_bounds__(FL_THREADS) pya_flr_records_kernel(const FlRecArgs a) {
    __shared__ FlSum lds[FL_THREADS / 64];
    __shared__ FlEnd lds_e[FL_THREADS / 64];
    __shared__ FlEnd rev[FL_THREADS];
    uint32_t pay[FL_ITEMS];
    FlEnd e[FL_ITEMS];
    fl_tile_ends(a, lds, pay, e);
    /* backward: the thread's own positions from its last to its first, the threads in reverse order */
    FlEnd mine = FlNearestEnd::identity();
#pragma unroll
    for (int j = FL_ITEMS - 1; j >= 0; j--) {
        mine = FlNearestEnd::op(mine, e[j]);
        e[j] = mine;                                       /* ends at positions j .. of this thread */
    }
    rev[FL_THREADS - 1u - threadIdx.x] = mine;
    __syncthreads();
    FlEnd total;
    const FlEnd incl = fl_block_scan<FlNearestEnd>(rev[threadIdx.x], lds_e, &total);
    __syncthreads();
    rev[threadIdx.x] = incl;                               /* rev[t]: the ends of the threads FL_THREADS - 1 - t .. of the tile */
    __syncthreads();
    FlEnd behind = a.ends[a.n_tiles - 1u - blockIdx.x];    /* the ends of every later tile */
    if (threadIdx.x + 1u < FL_THREADS) behind = FlNearestEnd::op(behind, rev[FL_THREADS - 2u - threadIdx.x]);
    const uint32_t i0 = blockIdx.x * FL_TILE + threadIdx.x * FL_ITEMS;
#pragma unroll
    for (int j = 0; j < FL_ITEMS; j++) {
        const uint32_t i = i0 + j;
        if (i >= a.n) continue;
        const uint32_t slot = pay[j] & ~FL_UNRANKED;
        if (a.order) a.order[i] = slot;
        if (slot >= a.n) continue;                         /* (a payload is a slot index: never) */
        uint4 lo = make_uint4(0u, 0u, 0u, 0u), hi = lo;
        if (!(pay[j] & FL_UNRANKED)) {
            const FlEnd g = FlNearestEnd::op(e[j], behind);
            const uint32_t rank = (uint32_t)(g.key >> 32);
            const double flr = (double)g.err / (double)((uint64_t)rank << 32);
            const uint64_t fb = (uint64_t)__double_as_longlong(flr), qb = (uint64_t)__double_as_longlong(g.q);
            lo = make_uint4(rank, (uint32_t)g.key, (uint32_t)g.err, (uint32_t)(g.err >> 32));
            hi = make_uint4((uint32_t)fb, (uint32_t)(fb >> 32), (uint32_t)qb, (uint32_t)(qb >> 32));
        }
        a.out[(size_t)slot * 2] = lo;
        a.out[(size_t)slot * 2 + 1] = hi;
    }
}

/* ---- the workspace ---- */
struct FlLayout {
    uint64_t keys[2], pay[2], hist, sums, ends, bytes;
    uint32_t n_tiles;
};
static uint64_t fl_round(uint64_t b) { return (b + 255u) & ~(uint64_t)255u; }
static FlLayout fl_layout(uint64_t n) {
    FlLayout L;
    L.n_tiles = (uint32_t)((n + FL_TILE - 1) / FL_TILE);
    uint64_t at = 0;
    for (int b = 0; b < 2; b++) {
        L.keys[b] = at;
        at += fl_round(n * sizeof(uint64_t));
    }
    for (int b = 0; b < 2; b++) {
        L.pay[b] = at;
        at += fl_round(n * sizeof(uint32_t));
    }
    L.hist = at;
    at += fl_round(fl_levels_total((uint64_t)FL_BINS * L.n_tiles) * sizeof(uint32_t));
    L.sums = at;
    at += fl_round(fl_levels_total(L.n_tiles) * sizeof(FlSum));
    L.ends = at;
    at += fl_round(fl_levels_total(L.n_tiles) * sizeof(FlEnd));
    L.bytes = n ? at : 0;
    return L;
}

extern "C" uint64_t pya_flr_layout_bytes(uint64_t n_slots) { return fl_layout(n_slots).bytes; }

/* The whole stage on `stream`: d_table[n] (32-byte records), d_cls[n] or NULL, d_work of fl_layout(n).bytes (256-byte aligned
 * as the layout's parts are), d_out[n], d_order[n] or NULL, d_n_ranked[2].  The caller has checked the sizes; 0 < n < 2^31.
 * phase[PYA_FLR_PHASES + 1] or NULL: events recorded before the keys, before every pass, before the records and at the end. */
extern "C" int pya_launch_flr(const void *d_table, uint64_t n_slots, const uint8_t *d_cls, uint32_t reported_only, void *d_work, void *d_out,
                              uint32_t *d_order, uint32_t *d_n_ranked, hipEvent_t *phase, hipStream_t st) {
    if (n_slots == 0 || n_slots > 0x7fffffffull) return (int)hipErrorInvalidValue;
    const uint32_t n = (uint32_t)n_slots;
    const FlLayout L = fl_layout(n_slots);
    unsigned char *w = (unsigned char *)d_work;
    uint64_t *keys[2] = {(uint64_t *)(w + L.keys[0]), (uint64_t *)(w + L.keys[1])};
    uint32_t *pay[2] = {(uint32_t *)(w + L.pay[0]), (uint32_t *)(w + L.pay[1])};
    uint32_t *hist = (uint32_t *)(w + L.hist);
    const uint32_t threads_blocks = (n + FL_THREADS - 1) / FL_THREADS;
    hipError_t e;
    int ph = 0;
#define FL_PHASE()                                                                \
    do {                                                                          \
        if (phase && (e = hipEventRecord(phase[ph++], st)) != hipSuccess) return (int)e; \
    } while (0)
    FL_PHASE();
    hipLaunchKernelGGL(pya_flr_keys_kernel, dim3(threads_blocks), dim3(FL_THREADS), 0, st, (const uint4 *)d_table, d_cls, n, reported_only, keys[0],
                       pay[0], d_n_ranked);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    int cur = 0;
    for (int pass = 0; pass < FL_PASSES; pass++) {
        FL_PHASE();
        hipLaunchKernelGGL(pya_flr_hist_kernel, dim3(L.n_tiles), dim3(FL_THREADS), 0, st, (const uint64_t *)keys[cur], (const uint32_t *)pay[cur], n,
                           L.n_tiles, pass, hist);
        if ((e = fl_scan<FlAddU32>(hist, (uint64_t)FL_BINS * L.n_tiles, st)) != hipSuccess) return (int)e;
        hipLaunchKernelGGL(pya_flr_scatter_kernel, dim3(L.n_tiles), dim3(FL_THREADS), 0, st, (const uint64_t *)keys[cur], (const uint32_t *)pay[cur], n,
                           L.n_tiles, pass, (const uint32_t *)hist, keys[cur ^ 1], pay[cur ^ 1]);
        if ((e = hipGetLastError()) != hipSuccess) return (int)e;
        cur ^= 1;
    }
    FL_PHASE();
    const FlRecArgs a = {keys[cur], pay[cur], d_cls, n, L.n_tiles, (FlSum *)(w + L.sums), (FlEnd *)(w + L.ends), (uint4 *)d_out, d_order};
    hipLaunchKernelGGL(pya_flr_tile_sums_kernel, dim3(L.n_tiles), dim3(FL_THREADS), 0, st, a);
    if ((e = fl_scan<FlAddSum>(a.sums, L.n_tiles, st)) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(pya_flr_tile_ends_kernel, dim3(L.n_tiles), dim3(FL_THREADS), 0, st, a);
    if ((e = fl_scan<FlNearestEnd>(a.ends, L.n_tiles, st)) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(pya_flr_records_kernel, dim3(L.n_tiles), dim3(FL_THREADS), 0, st, a);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    FL_PHASE();
#undef FL_PHASE
    return 0;
}
