/* pform_quant.hip -- peptidoform quantification: the channel intensities of the PSMs behind every record of a peptidoform
 * list, summed per record and channel into a table that is ROW-ALIGNED with the list, launched BEHIND pya_launch_pform on the
 * same stream.  The definition is in include/pyascore_hip.h (peptidoform quantification); the reference has no counterpart.
 * The list is peptidoforms.hip's, untouched; the table's arithmetic is site_quant.hip's: every field is an integer sum (the
 * quantum rule is quant_rule.hip.h's, shared with it), so whatever the grouping below and whatever order the atomics arrive
 * in, the bytes are the same.  No float atomics, no LDS, no workspace of its own.
 *
 * One launch, one lane per ENTRY: the PSMs of the plan, then the records of up to two earlier lists with their tables.
 *   1  locate.  A PSM lane re-derives what the list stage decided (kind, group, best_sig inside the plan's records; min_prob
 *      as the smallest with_prob bits over the residues of best_sig), applies the quant threshold and its row; a record lane
 *      takes its key as it stands (n_psm == 0: skipped).  Every contributing lane then finds its list position by a LOWER-BOUND
 *      SEARCH of (group as uint32, sig_bits as uint64) in the finished list d_out[0 .. min(d_n[0], cap)), at most 31 steps of
 *      one 16-byte load.  A key that is not found lies at or behind cap and issues nothing.
 *      The search, not a walk of the list stage's sorted keys: it reads only the list the caller gets anyway, so nothing of
 *      peptidoforms.hip's workspace layout, its ping-pong buffers or its scan is part of this file's contract, and the reduce
 *      over two lists is the same code.  The price: a wavefront aggregates only what lies in 64 CONSECUTIVE entries, so the
 *      PSMs of one peptidoform scattered over a batch reach memory as one atomic each instead of one per key; the walk
 *      would merge them first.  The upper search steps hit the same few list records from every lane and stay in cache.
 *   2 to 4  quant_wave.hip.h, with the list position as the key.  An entry is a reading or an earlier record's cell and head:
 *      a PSM's row is one coalesced load of values[row * n_channels + lane], quantised there; an earlier record's cell is one
 *      16-byte load, integers already, added as they are, and its head is added to the group's.
 * No write lies outside head[0 .. cap) and cell[0 .. cap * n_channels): a lane is active only with a position that pq_find
 * returned, and pq_find's own last lines return a position below m = min(d_n[0], cap) or -1 -- so the reduce does not test
 * the position against m again --; a channel lane is below n_channels.  values is read at rows below n_rows only, an earlier
 * table at records below its n only.  A PSM that would contribute but whose row is at or above n_rows is counted in over[0]
 * (the smallest such PSM kept in over[1] as 0xffffffff - psm) and nothing of it is written.  The launcher clears the table on
 * the stream first. */
#include "quant_wave.hip.h"
#include "../../include/pyascore_hip.h"

#define PQ_SCORED 1u                  /* PYA_SITE_SCORED */
#define PQ_THREADS 256

struct PqArgs {
    const int64_t *site_off;          /* [n_psm + 1] */
    const uint2 *site_probs;          /* pya_site_prob as 4 x uint32: with_prob is the first 8 bytes of 16 */
    const uint4 *psm_probs;           /* pya_psm_prob: kind is the low byte of word 3 */
    const int32_t *group;             /* [n_psm] */
    const uint64_t *best_sig;
    const int32_t *row;               /* [n_psm] or NULL: row_base + psm */
    const uint2 *values;              /* [n_rows * n_ch] doubles */
    const uint4 *src0, *src1;         /* earlier lists: pya_peptidoform as 3 x 16 bytes */
    const unsigned long long *src_head0, *src_head1;  /* their tables; NULL: all zero, the list's entries add nothing */
    const uint4 *src_cell0, *src_cell1;
    const uint4 *list;                /* the finished list */
    const uint32_t *d_n;              /* [0]: its true length */
    unsigned long long *head;         /* pya_site_quant_head as one uint64 */
    unsigned long long *cell;         /* pya_site_quant as 2 x uint64 */
    uint32_t *over;                   /* NULL without PSMs */
    uint64_t cap, n_rows;
    double threshold, scale;          /* scale = 2^scale_log2, exact */
    uint32_t n_psm, n0, n1, row_base, max_k, n_ch, complete_only;
};

/* PSM `i` as a contribution: false when it has none; the key is the list stage's, row is inside the matrix when true */
DEV bool pq_psm(const PqArgs &a, uint32_t i, uint32_t &g, uint64_t &sig, uint32_t &row) {
    const uint4 pp = a.psm_probs[i];
    const int32_t gi = a.group[i];
    if ((pp.w & 0xffu) != PQ_SCORED || gi < 0) return false;
    sig = a.best_sig[i];
    const int64_t lo = a.site_off[i], n_res = a.site_off[i + 1] - lo;
    if ((uint32_t)__popcll(sig) > a.max_k || (sig && (63 - __clzll((long long)sig)) >= n_res)) return false;   /* (not in the list) */
    uint64_t prob = 0x3ff0000000000000ull;                   /* 1.0: best_sig == 0 */
    if (sig) {
        prob = ~0ull;
        for (uint64_t m = sig; m; m &= m - 1) {
            const uint2 w = a.site_probs[(size_t)(lo + __builtin_ctzll(m)) * 2];
            const uint64_t b = (uint64_t)w.y << 32 | w.x;
            prob = b < prob ? b : prob;
        }
    }
    if (!(__longlong_as_double((long long)prob) >= a.threshold)) return false;
    const int64_t rw = a.row ? (int64_t)a.row[i] : (int64_t)a.row_base + (int64_t)i;
    if (rw < 0) return false;
    if ((uint64_t)rw >= a.n_rows) {
        if (a.over) report_over(a.over, i);
        return false;
    }
    g = (uint32_t)gi;
    row = (uint32_t)rw;
    return true;
}

/* the place of (g, sig) in list[0 .. m), or -1 */
DEV int32_t pq_find(const uint4 *list, uint32_t m, uint32_t g, uint64_t sig) {
    uint32_t lo = 0, hi = m;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const uint4 q = list[(size_t)mid * 3];
        const uint64_t s = (uint64_t)q.y << 32 | q.x;
        if (q.z < g || (q.z == g && s < sig)) lo = mid + 1; else hi = mid;
    }
    if (lo >= m) return -1;
    const uint4 q = list[(size_t)lo * 3];
    return (q.z == g && ((uint64_t)q.y << 32 | q.x) == sig) ? (int32_t)lo : -1;
}

/* this lane's part of one entry of a group: a PSM's reading of the lane's channel (kind 0: the double's bits in c.x, c.y), or an
 * earlier record's cell of that channel and its head (kind 1 / 2); kind is wave-uniform */
struct PqEntry {
    uint4 c;
    unsigned long long hd;
    uint32_t kind;
};

__global__ void __launch_bounds__(PQ_THREADS) pya_pform_quant_kernel(const PqArgs a) {
    const uint64_t e = (uint64_t)blockIdx.x * PQ_THREADS + threadIdx.x;
    const uint64_t len = a.d_n[0];
    const uint32_t m = (uint32_t)(len < a.cap ? len : a.cap);
    int32_t pos = -1;
    uint32_t kind = 0u, ref = 0u;                            /* kind 0: PSM, ref its row; 1 / 2: record ref of src0 / src1 */
    {
        uint32_t g = 0u;
        uint64_t sig = 0ull;
        bool have = false;
        if (e < a.n_psm) {
            have = pq_psm(a, (uint32_t)e, g, sig, ref);
        } else if (e < (uint64_t)a.n_psm + a.n0 + a.n1) {
            const uint64_t r = e - a.n_psm;
            kind = r < a.n0 ? 1u : 2u;
            ref = (uint32_t)(r < a.n0 ? r : r - a.n0);
            if (kind == 1u ? a.src_head0 != nullptr : a.src_head1 != nullptr) {
                const uint4 q0 = (kind == 1u ? a.src0 : a.src1)[(size_t)ref * 3];
                have = q0.w != 0u;
                g = q0.z;
                sig = (uint64_t)q0.y << 32 | q0.x;
            }
        }
        if (have && m) pos = pq_find(a.list, m, g, sig);
    }
    /* (from here on the control flow is wave-uniform: no lane has left) */
    qw_reduce(
        pos >= 0, (uint32_t)pos, a.n_ch, a.head, a.cell,
        [&](int j, bool have) {
            PqEntry e = {make_uint4(0u, 0u, 0u, 0u), 0ull, (uint32_t)__builtin_amdgcn_readlane((int)kind, j)};
            const uint32_t rj = (uint32_t)__builtin_amdgcn_readlane((int)ref, j);
            const bool mine = qw_channel(a.n_ch);
            const size_t at = (size_t)rj * a.n_ch + (uint32_t)lane_id();
            if (have && e.kind == 0u) {
                if (mine) {
                    const uint2 v = a.values[at];
                    e.c.x = v.x;
                    e.c.y = v.y;
                }
            } else if (have) {
                if (mine) e.c = (e.kind == 1u ? a.src_cell0 : a.src_cell1)[at];
                /* (a uniform address: the compiler takes the head into scalar registers at once, so an earlier record's two
                 * loads are waited for before the next entry's are issued.  Readings, the common entry, stay in flight together) */
                e.hd = (e.kind == 1u ? a.src_head0 : a.src_head1)[rj];
            }
            return e;
        },
        [&](QwAcc &c, const PqEntry &e) {
            if (e.kind == 0u) {
                qw_add_reading(c, __longlong_as_double((long long)((uint64_t)e.c.y << 32 | e.c.x)), a.n_ch, a.scale, a.complete_only);
            } else {
                c.sum += (uint64_t)e.c.y << 32 | e.c.x;
                c.n += e.c.z;
                c.n_saturated += e.c.w;
                c.n_records += (uint32_t)e.hd;
                c.n_complete += (uint32_t)(e.hd >> 32);
            }
        });
}

/* Behind pya_launch_pform on `st`: d_list[cap] / d_n as that call leaves them; the entries are the n_psm PSMs of the plan (0:
 * none; the arrays as pya_launch_pform takes them), then the records d_src0[n0] and d_src1[n1] with their tables (d_head* /
 * d_cell*; both NULL: an all-zero table).  d_values / d_row / row_base as pya_launch_site_quant takes them; d_over: two words,
 * zeroed by the caller, or NULL with n_psm == 0.  Clears d_head[cap] and d_cell[cap * n_channels] first.  prm and the sizes
 * have been checked: n_psm + n0 + n1 < 2^31. */
extern "C" int pya_launch_pform_quant(const int64_t *d_site_off, uint64_t n_psm, const void *d_site_probs, const void *d_psm_probs,
                                      const int32_t *d_group, const uint64_t *best_sig, uint32_t max_k, const void *d_src0, const void *d_head0,
                                      const void *d_cell0, uint64_t n0, const void *d_src1, const void *d_head1, const void *d_cell1, uint64_t n1,
                                      const double *d_values, uint64_t n_rows, const int32_t *d_row, uint32_t row_base,
                                      const pya_site_quant_params *prm, double scale, const void *d_list, const uint32_t *d_n, void *d_head,
                                      void *d_cell, uint64_t cap, uint32_t *d_over, hipStream_t st) {
    hipError_t e;
    if (cap) {
        if ((e = hipMemsetAsync(d_head, 0, (size_t)cap * sizeof(pya_site_quant_head), st)) != hipSuccess) return (int)e;
        if ((e = hipMemsetAsync(d_cell, 0, (size_t)cap * prm->n_channels * sizeof(pya_site_quant), st)) != hipSuccess) return (int)e;
    }
    const uint64_t total = n_psm + n0 + n1;
    if (total == 0 || cap == 0) return 0;
    if (total > 0x7fffffffull) return (int)hipErrorInvalidValue;
    const PqArgs a = {d_site_off, (const uint2 *)d_site_probs, (const uint4 *)d_psm_probs, d_group, best_sig, d_row, (const uint2 *)d_values,
                      (const uint4 *)d_src0, (const uint4 *)d_src1, (const unsigned long long *)d_head0, (const unsigned long long *)d_head1,
                      (const uint4 *)d_cell0, (const uint4 *)d_cell1, (const uint4 *)d_list, d_n, (unsigned long long *)d_head,
                      (unsigned long long *)d_cell, d_over, cap, n_rows, prm->threshold, scale, (uint32_t)n_psm, (uint32_t)n0, (uint32_t)n1,
                      row_base, max_k, prm->n_channels, (prm->flags & PYA_QUANT_COMPLETE_ONLY) ? 1u : 0u};
    hipLaunchKernelGGL(pya_pform_quant_kernel, dim3((uint32_t)((total + PQ_THREADS - 1) / PQ_THREADS)), dim3(PQ_THREADS), 0, st, a);
    return (int)hipGetLastError();
}
