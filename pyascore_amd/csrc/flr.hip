/* flr.hip -- false-localisation rates over a roll-up table: a global sort of the slots by best_prob and scans over the
 * sorted order, on the table where rollup.hip left it.  The definition is in include/pyascore_hip.h (pya_site_flr); the
 * reference has no counterpart.  The first kernels of this tree that are neither "one PSM per wavefront" nor a scatter of
 * atomics: every launch is a grid over tiles of TS_TILE slots, and KERNEL BOUNDARIES ARE THE ONLY GRID-WIDE SYNCHRONISATION --
 * no kernel waits on another workgroup (no look-back, no flag, no cooperative launch), so nothing here can hang a card whose
 * workgroups are not co-resident.  Everything is launched on the caller's stream into the caller's workspace; nothing is
 * allocated and the host waits for nothing.  The tile geometry, the block scan, the multi-level scan and the radix sort are
 * tile_sort.hip.h's, shared with peptidoforms.hip; what a pass and a scan level do is described there.
 *
 *   keys      one thread per slot: key = ~bits(best_prob) of a ranked slot, all-ones otherwise; payload = the slot index, bit
 *             31 set for an unranked slot (n_slots <= 2^31 - 1 leaves the bit free).  p = +0.0 of a ranked slot has the
 *             all-ones key as well, which is why the unranked tail is split off by a pass of its own on that bit and not by
 *             the key.  Counts the ranked slots and the class bytes that are none of 0 / 1 / 2.
 *   sort      ts_sort over FlKey: (key, payload) in two arrays, FlKey::passes = 9 passes, eight over the bytes of the key from
 *             the lowest, the last over payload bit 31.
 *   records   over the sorted order: tile sums of (1, decoy, err) -> exclusive scan; then the values at the END of a tie group
 *             reach its members and the running minimum of the decoy ratio reaches every better site by ONE backward scan --
 *             rank strictly rises from one group end to the next, so "the nearest group end at or behind me" is the element
 *             with the smallest rank, a commutative min, and the ratio takes a plain min beside it.  Tile minima -> exclusive
 *             scan (stored back to front) -> the last kernel recomputes both in-tile scans and writes the record of every
 *             slot (zero bytes for an unranked one) and the order.
 * Sums are integers (err is the 2^32-scaled error truncated to a uint64), so no result depends on the order of anything.
 * No write lies outside d_out[0 .. n), d_order[0 .. n), d_n_ranked[0 .. 2) and the workspace bytes fl_layout() counts: every
 * scatter and record store is guarded by its index, and a payload indexes d_out only below n. */
#include "tile_sort.hip.h"

#define FL_UNRANKED 0x80000000u

/* ---- what is scanned (both operators commute) ---- */
/* (1, decoy, err) of the ranked slots: n = count (low word) | decoys (high word), neither reaches 2^31 */
struct FlSum {
    uint64_t n, err;
};
struct FlAddSum {
    typedef FlSum T;
    static DEV T identity() { return FlSum{0ull, 0ull}; }
    static DEV T op(T a, T b) { return FlSum{a.n + b.n, a.err + b.err}; }
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
};

/* ---- keys ---- */
__global__ void __launch_bounds__(TS_THREADS) pya_flr_keys_kernel(const uint4 *table, const uint8_t *cls, uint32_t n, uint32_t reported_only,
                                                                  uint64_t *keys, uint32_t *pay, uint32_t *n_ranked) {
    const uint32_t s = blockIdx.x * TS_THREADS + threadIdx.x;
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

/* ---- sort: the key policy ---- */
struct FlKey {
    struct E {
        uint64_t key;
        uint32_t pay;
    };
    struct Buf {
        uint64_t *keys;
        uint32_t *pay;
    };
    static const int passes = 9;
    static DEV E none() { return E{0ull, 0u}; }
    static DEV uint32_t digit(const E &e, int pass) { return pass < 8 ? (uint32_t)(e.key >> (8 * pass)) & 0xffu : e.pay >> 31; }
    static DEV E load(const Buf &b, uint32_t i) { return E{b.keys[i], b.pay[i]}; }
    /* only the last pass reads the payload: the other eight histograms move 8 bytes per slot, not 12 */
    static DEV E load_digit(const Buf &b, uint32_t i, int pass) { return E{b.keys[i], pass == 8 ? b.pay[i] : 0u}; }
    static DEV void store(const Buf &b, uint32_t i, const E &e) {
        b.keys[i] = e.key;
        b.pay[i] = e.pay;
    }
};

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

/* A thread holds TS_ITEMS CONSECUTIVE positions here (tile * TS_TILE + thread * TS_ITEMS + j): its own run is scanned in
 * registers, the threads' totals by ts_block_scan. */
__global__ void __launch_bounds__(TS_THREADS) pya_flr_tile_sums_kernel(const FlRecArgs a) {
    __shared__ FlSum lds[TS_THREADS / 64];
    const uint32_t i0 = blockIdx.x * TS_TILE + threadIdx.x * TS_ITEMS;
    FlSum mine = FlAddSum::identity();
#pragma unroll
    for (int j = 0; j < TS_ITEMS; j++) {
        uint64_t key;
        uint32_t pay;
        mine = FlAddSum::op(mine, fl_element(a, i0 + j, &key, &pay));
    }
    FlSum total;
    ts_block_scan<FlAddSum>(mine, lds, &total);
    if (threadIdx.x == 0) a.sums[blockIdx.x] = total;
}

/* the inclusive sums at the thread's TS_ITEMS positions and the group ends among them (identity elsewhere) */
DEV void fl_tile_ends(const FlRecArgs &a, FlSum *lds, uint32_t *pay, FlEnd *e) {
    const uint32_t i0 = blockIdx.x * TS_TILE + threadIdx.x * TS_ITEMS;
    uint64_t key[TS_ITEMS + 1];
    uint32_t next_pay;
    FlSum v[TS_ITEMS], mine = FlAddSum::identity();
#pragma unroll
    for (int j = 0; j < TS_ITEMS; j++) {
        v[j] = fl_element(a, i0 + j, &key[j], &pay[j]);
        mine = FlAddSum::op(mine, v[j]);
        v[j] = mine;
    }
    /* the position behind the thread's last: of another thread or another tile */
    key[TS_ITEMS] = ~0ull;
    next_pay = FL_UNRANKED;
    if (i0 + TS_ITEMS < a.n) {
        key[TS_ITEMS] = a.keys[i0 + TS_ITEMS];
        next_pay = a.pay[i0 + TS_ITEMS];
    }
    FlSum total;
    const FlSum before = FlAddSum::op(a.sums[blockIdx.x], ts_block_scan<FlAddSum>(mine, lds, &total));
#pragma unroll
    for (int j = 0; j < TS_ITEMS; j++) {
        const bool ranked = !(pay[j] & FL_UNRANKED);
        const bool next_ranked = !((j + 1 < TS_ITEMS ? pay[j + 1] : next_pay) & FL_UNRANKED);
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

__global__ void __launch_bounds__(TS_THREADS) pya_flr_tile_ends_kernel(const FlRecArgs a) {
    __shared__ FlSum lds[TS_THREADS / 64];
    __shared__ FlEnd lds_e[TS_THREADS / 64];
    uint32_t pay[TS_ITEMS];
    FlEnd e[TS_ITEMS], mine = FlNearestEnd::identity();
    fl_tile_ends(a, lds, pay, e);
#pragma unroll
    for (int j = 0; j < TS_ITEMS; j++) mine = FlNearestEnd::op(mine, e[j]);
    FlEnd total;
    ts_block_scan<FlNearestEnd>(mine, lds_e, &total);
    if (threadIdx.x == 0) a.ends[a.n_tiles - 1u - blockIdx.x] = total;
}

__global__ void __launch_bounds__(TS_THREADS) pya_flr_records_kernel(const FlRecArgs a) {
    __shared__ FlSum lds[TS_THREADS / 64];
    __shared__ FlEnd lds_e[TS_THREADS / 64];
    __shared__ FlEnd rev[TS_THREADS];
    uint32_t pay[TS_ITEMS];
    FlEnd e[TS_ITEMS];
    fl_tile_ends(a, lds, pay, e);
    /* backward: the thread's own positions from its last to its first, the threads in reverse order */
    FlEnd mine = FlNearestEnd::identity();
#pragma unroll
    for (int j = TS_ITEMS - 1; j >= 0; j--) {
        mine = FlNearestEnd::op(mine, e[j]);
        e[j] = mine;                                       /* ends at positions j .. of this thread */
    }
    rev[TS_THREADS - 1u - threadIdx.x] = mine;
    __syncthreads();
    FlEnd total;
    /* the exclusive value of thread t is every end behind thread TS_THREADS - 1 - t in this tile: it goes back to that thread
     * through rev[t], which no other thread touches between the two barriers */
    rev[threadIdx.x] = ts_block_scan<FlNearestEnd>(rev[threadIdx.x], lds_e, &total);
    __syncthreads();
    /* the ends of every later tile, then of the later threads of this one */
    const FlEnd behind = FlNearestEnd::op(a.ends[a.n_tiles - 1u - blockIdx.x], rev[TS_THREADS - 1u - threadIdx.x]);
    const uint32_t i0 = blockIdx.x * TS_TILE + threadIdx.x * TS_ITEMS;
#pragma unroll
    for (int j = 0; j < TS_ITEMS; j++) {
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
static FlLayout fl_layout(uint64_t n) {
    FlLayout L;
    L.n_tiles = (uint32_t)((n + TS_TILE - 1) / TS_TILE);
    uint64_t at = 0;
    for (int b = 0; b < 2; b++) {
        L.keys[b] = at;
        at += ts_round(n * sizeof(uint64_t));
    }
    for (int b = 0; b < 2; b++) {
        L.pay[b] = at;
        at += ts_round(n * sizeof(uint32_t));
    }
    L.hist = at;
    at += ts_round(ts_levels_total((uint64_t)TS_BINS * L.n_tiles) * sizeof(uint32_t));
    L.sums = at;
    at += ts_round(ts_levels_total(L.n_tiles) * sizeof(FlSum));
    L.ends = at;
    at += ts_round(ts_levels_total(L.n_tiles) * sizeof(FlEnd));
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
    const FlKey::Buf buf[2] = {{(uint64_t *)(w + L.keys[0]), (uint32_t *)(w + L.pay[0])}, {(uint64_t *)(w + L.keys[1]), (uint32_t *)(w + L.pay[1])}};
    const uint32_t threads_blocks = (n + TS_THREADS - 1) / TS_THREADS;
    hipError_t e;
    int ph = 0;
    TS_PHASE();
    hipLaunchKernelGGL(pya_flr_keys_kernel, dim3(threads_blocks), dim3(TS_THREADS), 0, st, (const uint4 *)d_table, d_cls, n, reported_only, buf[0].keys,
                       buf[0].pay, d_n_ranked);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    int cur;
    if ((e = ts_sort<FlKey>(buf, n, (uint32_t *)(w + L.hist), phase ? phase + ph : nullptr, st, &cur)) != hipSuccess) return (int)e;
    ph += FlKey::passes;
    TS_PHASE();
    const FlRecArgs a = {buf[cur].keys, buf[cur].pay, d_cls, n, L.n_tiles, (FlSum *)(w + L.sums), (FlEnd *)(w + L.ends), (uint4 *)d_out, d_order};
    hipLaunchKernelGGL(pya_flr_tile_sums_kernel, dim3(L.n_tiles), dim3(TS_THREADS), 0, st, a);
    if ((e = ts_scan<FlAddSum>(a.sums, L.n_tiles, st)) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(pya_flr_tile_ends_kernel, dim3(L.n_tiles), dim3(TS_THREADS), 0, st, a);
    if ((e = ts_scan<FlNearestEnd>(a.ends, L.n_tiles, st)) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(pya_flr_records_kernel, dim3(L.n_tiles), dim3(TS_THREADS), 0, st, a);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    TS_PHASE();
    return 0;
}
