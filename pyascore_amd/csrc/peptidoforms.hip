/* peptidoforms.hip -- peptidoform roll-up: one record per distinct (group, best_sig) among the contributing PSMs of a plan
 * and the records of earlier lists.  The definition is in include/pyascore_hip.h (pya_peptidoform); the reference has no
 * counterpart.  The second reduction over PSMs of this tree, and unlike rollup.hip its keys are sparse and known only after
 * scoring, so it is sort-and-segment-reduce, not a scatter of atomics.  As in flr.hip every launch is a grid over tiles of
 * TS_TILE entries and KERNEL BOUNDARIES ARE THE ONLY GRID-WIDE SYNCHRONISATION: no kernel waits on another workgroup.
 * Everything is launched on the caller's stream into the caller's workspace; nothing is allocated and the host waits for
 * nothing.  The tile geometry, the block scan, the multi-level scan and the radix sort are tile_sort.hip.h's, shared with
 * flr.hip; what a pass and a scan level do is described there.
 *
 *   entries   one thread per PSM / per input record: a 48-byte entry (a pya_peptidoform with n_psm == 1 for a PSM) and a
 *             16-byte key (sig_bits low, sig_bits high, group, entry index; bit 31 of the index word set for an entry that
 *             contributes nothing -- n_entries <= 2^31 - 1 leaves the bit free).
 *   sort      ts_sort over PfKey: the keys in one array, PfKey::passes = 13 passes, twelve over the bytes of sig_bits and group
 *             from the lowest, the last over the "nothing" bit, which sends those entries behind every other whatever key they
 *             carry.
 *   reduce    over the sorted order, a SEGMENTED scan: an element is (value, heads, group heads, flag) with flag set on the
 *             first entry of a key; op(a, b) keeps b's value when b carries a flag and merges the two otherwise.  The value
 *             merge is counts that add, a max / min over bit patterns and a min over ids, so any tree gives the same bytes.
 *             Tile totals -> exclusive scan -> the last kernel recomputes the in-tile scan; the LAST entry of a key holds
 *             the key's record and its number (heads - 1) and stores it at that place of a staging list, with the ordinal
 *             of its group where n_isomers will go; the first entry of a group stores the number of its first record.
 *   finish    one thread per record below min(count, cap): n_isomers = first record of the next group - first of its own,
 *             three 16-byte stores into d_out.
 * No write lies outside d_out[0 .. cap), d_n[0 .. 2) and the workspace bytes pf_layout() counts: every scatter, staging and
 * record store is guarded by its index. */
#include "tile_sort.hip.h"

#define PF_NOTHING 0x80000000u
#define PF_SCORED 1u                          /* PYA_SITE_SCORED */

/* the order-preserving image of a float's bits under -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN, and back */
DEV uint32_t pf_akey(uint32_t b) { return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u); }
DEV uint32_t pf_abits(uint32_t k) { return k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu); }

/* ---- what is scanned ---- */
/* the fields of a record that are reduced: counts, max prob bits with the smallest id that has them, min z bits, max Ascore key */
struct PfVal {
    uint64_t prob, z;
    uint32_t n, nc, psm, ak;
};
DEV PfVal pf_merge(const PfVal &a, const PfVal &b) {
    PfVal r;
    r.n = a.n + b.n;
    r.nc = a.nc + b.nc;
    r.prob = b.prob > a.prob ? b.prob : a.prob;
    r.psm = b.prob > a.prob ? b.psm : (a.prob > b.prob ? a.psm : (b.psm < a.psm ? b.psm : a.psm));
    r.z = b.z < a.z ? b.z : a.z;
    r.ak = b.ak > a.ak ? b.ak : a.ak;
    return r;
}
struct PfState {
    PfVal v;
    uint32_t heads, gheads, flag, pad;
};
struct PfSegmented {
    typedef PfState T;
    static DEV T identity() { return PfState{PfVal{0ull, ~0ull, 0u, 0u, 0xffffffffu, 0u}, 0u, 0u, 0u, 0u}; }
    /* a lies before b */
    static DEV T op(const T &a, const T &b) {
        T r;
        r.v = b.flag ? b.v : pf_merge(a.v, b.v);
        r.heads = a.heads + b.heads;
        r.gheads = a.gheads + b.gheads;
        r.flag = a.flag | b.flag;
        r.pad = 0u;
        return r;
    }
};
static_assert(sizeof(PfState) == 48, "twelve words per scan element");

/* ---- entries ---- */
struct PfPsmArgs {
    const int64_t *site_off;          /* [n_psm + 1] */
    const uint2 *site_probs;          /* pya_site_prob as 4 x uint32: with_prob is the first 8 bytes of 16 */
    const uint4 *psm_probs;           /* pya_psm_prob: z | n_summed | kind in the low byte of word 3 */
    const int32_t *group;             /* [n_psm] */
    const uint32_t *psm_id;           /* [n_psm] or NULL: psm_base + psm */
    const uint64_t *best_sig;
    const uint32_t *ascores;          /* float bits, row stride max_k */
    uint4 *entries, *keys;            /* [n_psm] of 3 x 16 and of 16 bytes: the first entries of the call */
    uint32_t *d_n;                    /* [2]; [1]: PSMs whose best_sig does not fit the plan's residue records or max_k */
    double threshold;
    uint32_t n_psm, psm_base, max_k;
};

__global__ void __launch_bounds__(TS_THREADS) pya_pform_psm_entries_kernel(const PfPsmArgs a) {
    const uint32_t i = blockIdx.x * TS_THREADS + threadIdx.x;
    if (i >= a.n_psm) return;
    const uint4 pp = a.psm_probs[i];
    const int32_t g = a.group[i];
    bool ok = (pp.w & 0xffu) == PF_SCORED && g >= 0;
    const uint64_t sig = ok ? a.best_sig[i] : 0ull;
    const int64_t lo = a.site_off[i], n_res = a.site_off[i + 1] - lo;
    const uint32_t k = (uint32_t)__popcll(sig);
    if (ok && (k > a.max_k || (sig && (63 - __clzll((long long)sig)) >= n_res))) {
        atomicAdd(&a.d_n[1], 1u);                            /* (results or records that are not this plan's) */
        ok = false;
    }
    if (!ok) {
        a.keys[i] = make_uint4(0u, 0u, 0u, i | PF_NOTHING);
        return;
    }
    uint64_t prob = 0x3ff0000000000000ull;                   /* 1.0: best_sig == 0 */
    if (sig) {
        prob = ~0ull;
        for (uint64_t m = sig; m; m &= m - 1) {
            const uint2 w = a.site_probs[(size_t)(lo + __builtin_ctzll(m)) * 2];
            const uint64_t b = (uint64_t)w.y << 32 | w.x;
            prob = b < prob ? b : prob;
        }
    }
    uint32_t ak = pf_akey(0x7f800000u);                      /* +inf: no modified residue */
    if (k) {
        ak = 0xffffffffu;
        for (uint32_t c = 0; c < k; c++) {
            const uint32_t x = pf_akey(a.ascores[(size_t)i * a.max_k + c]);
            ak = x < ak ? x : ak;
        }
    }
    const uint32_t conf = __longlong_as_double((long long)prob) >= a.threshold ? 1u : 0u;
    const uint32_t id = a.psm_id ? a.psm_id[i] : a.psm_base + i;
    a.entries[(size_t)i * 3] = make_uint4((uint32_t)sig, (uint32_t)(sig >> 32), (uint32_t)g, 1u);
    a.entries[(size_t)i * 3 + 1] = make_uint4(conf, id, (uint32_t)prob, (uint32_t)(prob >> 32));
    a.entries[(size_t)i * 3 + 2] = make_uint4(pp.x, pp.y, pf_abits(ak), 0u);
    a.keys[i] = make_uint4((uint32_t)sig, (uint32_t)(sig >> 32), (uint32_t)g, i);
}

/* records src[n] as the entries base .. base + n of the call */
__global__ void __launch_bounds__(TS_THREADS) pya_pform_rec_entries_kernel(const uint4 *src, uint32_t n, uint32_t base, uint4 *entries, uint4 *keys) {
    const uint32_t i = blockIdx.x * TS_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint4 q0 = src[(size_t)i * 3], q1 = src[(size_t)i * 3 + 1], q2 = src[(size_t)i * 3 + 2];
    const uint32_t e = base + i;
    entries[(size_t)e * 3] = q0;
    entries[(size_t)e * 3 + 1] = q1;
    entries[(size_t)e * 3 + 2] = q2;
    keys[e] = q0.w ? make_uint4(q0.x, q0.y, q0.z, e) : make_uint4(0u, 0u, 0u, e | PF_NOTHING);
}

/* ---- sort: the key policy ---- */
struct PfKey {
    typedef uint4 E;
    typedef uint4 *Buf;
    static const int passes = 13;
    static DEV E none() { return make_uint4(0u, 0u, 0u, 0u); }
    static DEV uint32_t digit(const E &k, int pass) {
        const uint32_t w = pass < 4 ? k.x : (pass < 8 ? k.y : k.z);
        return pass < 12 ? (w >> (8 * (pass & 3))) & 0xffu : k.w >> 31;
    }
    static DEV E load(Buf b, uint32_t i) { return b[i]; }
    static DEV E load_digit(Buf b, uint32_t i, int) { return b[i]; }
    static DEV void store(Buf b, uint32_t i, const E &e) { b[i] = e; }
};

/* ---- reduce ---- */
struct PfRedArgs {
    const uint4 *keys;                /* sorted */
    const uint4 *entries;
    uint32_t n, n_tiles;
    PfState *tiles;                   /* [n_tiles]: tile totals, then their exclusive scan */
    uint4 *staged;                    /* [n] records in list order, the group's ordinal in place of n_isomers */
    uint32_t *grp_first;              /* [n + 1]: the number of a group's first record; one more behind the last group */
    uint32_t *d_n;
};

/* A thread holds TS_ITEMS CONSECUTIVE sorted positions (tile * TS_TILE + thread * TS_ITEMS + j).  key[0] is the position
 * before its first, key[TS_ITEMS + 1] the one behind its last (the "nothing" key outside 0 .. n); s[j]: the positions as scan
 * elements, combined from the thread's first; returns the thread's total. */
DEV PfState pf_thread_items(const PfRedArgs &a, uint4 *key, PfState *s) {
    const uint32_t i0 = blockIdx.x * TS_TILE + threadIdx.x * TS_ITEMS;
#pragma unroll
    for (int j = 0; j < TS_ITEMS + 2; j++) {
        const uint32_t i = i0 + (uint32_t)j - 1u;          /* (i0 == 0, j == 0 wraps to 0xffffffff >= n) */
        key[j] = make_uint4(0u, 0u, 0u, PF_NOTHING);
        if (i < a.n) key[j] = a.keys[i];
    }
    PfState run = PfSegmented::identity();
#pragma unroll
    for (int j = 0; j < TS_ITEMS; j++) {
        const uint4 k = key[j + 1], p = key[j];
        PfState e = PfSegmented::identity();
        const uint32_t idx = k.w;
        if (!(idx & PF_NOTHING) && idx < a.n) {
            const uint4 q0 = a.entries[(size_t)idx * 3], q1 = a.entries[(size_t)idx * 3 + 1], q2 = a.entries[(size_t)idx * 3 + 2];
            e.v.n = q0.w;
            e.v.nc = q1.x;
            e.v.psm = q1.y;
            e.v.prob = (uint64_t)q1.w << 32 | q1.z;
            e.v.z = (uint64_t)q2.y << 32 | q2.x;
            e.v.ak = pf_akey(q2.z);
            /* (the entries that are nothing lie behind all others: a position with an entry has one before it or is the first) */
            const bool ghead = (p.w & PF_NOTHING) || p.z != k.z;
            const bool head = ghead || p.x != k.x || p.y != k.y;
            e.heads = e.flag = head ? 1u : 0u;
            e.gheads = ghead ? 1u : 0u;
        }
        run = PfSegmented::op(run, e);
        s[j] = run;
    }
    return run;
}

__global__ void __launch_bounds__(TS_THREADS) pya_pform_tile_totals_kernel(const PfRedArgs a) {
    __shared__ PfState lds[TS_THREADS / 64];
    uint4 key[TS_ITEMS + 2];
    PfState s[TS_ITEMS], total;
    const PfState mine = pf_thread_items(a, key, s);
    ts_block_scan<PfSegmented>(mine, lds, &total);
    if (threadIdx.x == 0) a.tiles[blockIdx.x] = total;
}

__global__ void __launch_bounds__(TS_THREADS) pya_pform_stage_kernel(const PfRedArgs a) {
    __shared__ PfState lds[TS_THREADS / 64];
    uint4 key[TS_ITEMS + 2];
    PfState s[TS_ITEMS], total;
    const PfState mine = pf_thread_items(a, key, s);
    const PfState ex = ts_block_scan<PfSegmented>(mine, lds, &total);
    const PfState before = PfSegmented::op(a.tiles[blockIdx.x], ex);
#pragma unroll
    for (int j = 0; j < TS_ITEMS; j++) {
        const uint4 k = key[j + 1], p = key[j], nx = key[j + 2];
        if (k.w & PF_NOTHING) continue;
        const PfState c = PfSegmented::op(before, s[j]);
        const uint32_t rec = c.heads - 1u, grp = c.gheads - 1u;
        if (rec >= a.n || grp >= a.n) continue;              /* (every entry lies behind the head of its key: never) */
        if ((p.w & PF_NOTHING) || p.z != k.z) a.grp_first[grp] = rec;
        const bool last = (nx.w & PF_NOTHING) != 0u;
        if (last || nx.x != k.x || nx.y != k.y || nx.z != k.z) {
            a.staged[(size_t)rec * 3] = make_uint4(k.x, k.y, k.z, c.v.n);
            a.staged[(size_t)rec * 3 + 1] = make_uint4(c.v.nc, c.v.psm, (uint32_t)c.v.prob, (uint32_t)(c.v.prob >> 32));
            a.staged[(size_t)rec * 3 + 2] = make_uint4((uint32_t)c.v.z, (uint32_t)(c.v.z >> 32), pf_abits(c.v.ak), grp);
        }
        if (last) {
            a.grp_first[grp + 1u] = c.heads;
            a.d_n[0] = c.heads;
        }
    }
}

/* ---- finish ---- */
__global__ void __launch_bounds__(TS_THREADS) pya_pform_finish_kernel(const uint4 *staged, const uint32_t *grp_first, const uint32_t *d_n, uint32_t n,
                                                                      uint64_t cap, uint4 *out) {
    const uint32_t j = blockIdx.x * TS_THREADS + threadIdx.x;
    if (j >= n || j >= d_n[0] || (uint64_t)j >= cap) return;
    const uint4 q0 = staged[(size_t)j * 3], q1 = staged[(size_t)j * 3 + 1];
    uint4 q2 = staged[(size_t)j * 3 + 2];
    const uint32_t grp = q2.w < n ? q2.w : 0u;
    q2.w = grp_first[grp + 1u] - grp_first[grp];
    out[(size_t)j * 3] = q0;
    out[(size_t)j * 3 + 1] = q1;
    out[(size_t)j * 3 + 2] = q2;
}

/* ---- the workspace ---- */
struct PfLayout {
    uint64_t keys[2], entries, staged, grp_first, hist, tiles, bytes;
    uint32_t n_tiles;
};
static PfLayout pf_layout(uint64_t n) {
    PfLayout L;
    L.n_tiles = (uint32_t)((n + TS_TILE - 1) / TS_TILE);
    uint64_t at = 0;
    for (int b = 0; b < 2; b++) {
        L.keys[b] = at;
        at += ts_round(n * sizeof(uint4));
    }
    L.entries = at;
    at += ts_round(n * 3 * sizeof(uint4));
    L.staged = at;
    at += ts_round(n * 3 * sizeof(uint4));
    L.grp_first = at;
    at += ts_round((n + 1) * sizeof(uint32_t));
    L.hist = at;
    at += ts_round(ts_levels_total((uint64_t)TS_BINS * L.n_tiles) * sizeof(uint32_t));
    L.tiles = at;
    at += ts_round(ts_levels_total(L.n_tiles) * sizeof(PfState));
    L.bytes = n ? at : 0;
    return L;
}

extern "C" uint64_t pya_pform_layout_bytes(uint64_t n_entries) { return pf_layout(n_entries).bytes; }

/* The whole stage on `st`.  The entries are, in this order: the n_psm PSMs of a plan (0: none; d_site_off .. max_k as
 * pya_launch_rollup takes them, d_group[n_psm]), then the records d_src0[n0] and d_src1[n1].  d_work: pf_layout(total).bytes,
 * 256-byte aligned as the layout's parts are; d_out[cap]; d_n[2], zeroed by the caller on `st`.  The caller has checked the
 * sizes: 0 < total < 2^31.  phase[PYA_PFORM_PHASES + 1] or NULL: events recorded before the entries, the sort, the reduction,
 * the finish and at the end. */
extern "C" int pya_launch_pform(const int64_t *d_site_off, uint64_t n_psm, const void *d_site_probs, const void *d_psm_probs, const int32_t *d_group,
                                double threshold, const uint32_t *d_psm_id, uint32_t psm_base, const uint64_t *best_sig, const float *ascores,
                                uint32_t max_k, const void *d_src0, uint64_t n0, const void *d_src1, uint64_t n1, void *d_work, void *d_out,
                                uint64_t cap, uint32_t *d_n, hipEvent_t *phase, hipStream_t st) {
    const void *const d_src[2] = {d_src0, d_src1};
    const uint64_t n_src[2] = {n0, n1};
    const uint64_t total = n_psm + n0 + n1;
    if (total == 0 || total > 0x7fffffffull) return (int)hipErrorInvalidValue;
    const uint32_t n = (uint32_t)total;
    const PfLayout L = pf_layout(total);
    unsigned char *w = (unsigned char *)d_work;
    uint4 *const keys[2] = {(uint4 *)(w + L.keys[0]), (uint4 *)(w + L.keys[1])};
    uint4 *entries = (uint4 *)(w + L.entries);
    hipError_t e;
    int ph = 0;
    TS_PHASE();
    uint32_t base = 0;
    if (n_psm) {
        const PfPsmArgs p = {d_site_off, (const uint2 *)d_site_probs, (const uint4 *)d_psm_probs, d_group, d_psm_id, best_sig, (const uint32_t *)ascores,
                             entries, keys[0], d_n, threshold, (uint32_t)n_psm, psm_base, max_k};
        hipLaunchKernelGGL(pya_pform_psm_entries_kernel, dim3(((uint32_t)n_psm + TS_THREADS - 1) / TS_THREADS), dim3(TS_THREADS), 0, st, p);
        base = (uint32_t)n_psm;
    }
    for (int s = 0; s < 2; s++) {
        if (!n_src[s]) continue;
        hipLaunchKernelGGL(pya_pform_rec_entries_kernel, dim3((uint32_t)((n_src[s] + TS_THREADS - 1) / TS_THREADS)), dim3(TS_THREADS), 0, st,
                           (const uint4 *)d_src[s], (uint32_t)n_src[s], base, entries, keys[0]);
        base += (uint32_t)n_src[s];
    }
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    TS_PHASE();
    int cur;
    if ((e = ts_sort<PfKey>(keys, n, (uint32_t *)(w + L.hist), nullptr, st, &cur)) != hipSuccess) return (int)e;
    TS_PHASE();
    const PfRedArgs a = {keys[cur], entries, n, L.n_tiles, (PfState *)(w + L.tiles), (uint4 *)(w + L.staged), (uint32_t *)(w + L.grp_first), d_n};
    hipLaunchKernelGGL(pya_pform_tile_totals_kernel, dim3(L.n_tiles), dim3(TS_THREADS), 0, st, a);
    if ((e = ts_scan<PfSegmented>(a.tiles, L.n_tiles, st)) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(pya_pform_stage_kernel, dim3(L.n_tiles), dim3(TS_THREADS), 0, st, a);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    TS_PHASE();
    if (cap) {
        const uint64_t m = total < cap ? total : cap;
        hipLaunchKernelGGL(pya_pform_finish_kernel, dim3((uint32_t)((m + TS_THREADS - 1) / TS_THREADS)), dim3(TS_THREADS), 0, st,
                           (const uint4 *)a.staged, (const uint32_t *)a.grp_first, (const uint32_t *)d_n, n, cap, (uint4 *)d_out);
        if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    }
    TS_PHASE();
    return 0;
}
