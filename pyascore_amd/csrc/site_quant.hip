/* site_quant.hip -- site quantification: the channel intensities (isobaric reporters, or any matrix of the caller's) of the
 * PSMs that place a modification on a roll-up slot confidently, summed per slot and channel, launched BEHIND a run, behind
 * probs.hip and beside rollup.hip.  The definition is in include/pyascore_hip.h (pya_site_quant); the reference has no
 * counterpart.
 *
 * Every field of the table is an integer sum -- a reading is scaled by a power of two and truncated to a uint64 before it
 * is added --, so the table is a function of the multiset of contributing records: whatever the grouping below and whatever
 * order the atomics arrive in, the bytes are the same.  No float atomics.
 *
 * The work is records x channels additions into a table whose slots are hot (many PSMs of one peptide share a slot), so a
 * wavefront aggregates before it reaches memory:
 *   1  lane = record.  A wavefront takes 64 consecutive residue records.  Each lane finds its PSM by the roll-up's binary search
 *      of the site offsets and decides whether the record contributes, its slot and its row.
 *   2 to 4  quant_wave.hip.h, with the slot as the key: the lanes of one slot find each other, the lanes as channels walk the
 *      group's rows -- an entry is a reading, one coalesced load of values[row * n_channels + lane] -- and one atomic per
 *      (group, channel) and one for the head reach memory.
 * With n_channels below 64 the lanes at and above it idle in step 3: for 3 channels that is most of the wavefront, and the
 * walk is then bound by the latency of a row's load, not by the lanes.  It is kept: step 3 costs a load per contributing record
 * however the lanes are used, and the atomics -- the part that serialises on hot slots -- are already one per (group, channel).
 * The table is never LOADED here, so the question rollup.hip's header answers about plain loads beside atomics does not
 * arise.  values, the records and the slots are only read, and nothing of this launch writes them.
 * No write lies outside head[0 .. n_slots) and cell[0 .. n_slots * n_channels): a record that would contribute but whose slot
 * is at or above n_slots or whose row is at or above n_rows is counted in over[0] (and the smallest such PSM kept in over[1]
 * as 0xffffffff - psm) and nothing of it is written; a row below n_rows is the only index values is read at.
 *
 * pya_marker_values_kernel, the second kernel: marker records to a channel matrix, one thread per element. */
#include "quant_wave.hip.h"
#include "../../include/pyascore_hip.h"

#define SQ_THREADS 256

struct SqArgs {
    const int64_t *site_off;          /* [n_psm + 1] */
    const uint2 *site_probs;          /* pya_site_prob as 4 x uint32: with_prob is the first 8 bytes of 16 */
    const uint32_t *psm_probs;        /* pya_psm_prob as 4 x uint32: kind is the low byte of word 3 */
    const int32_t *slot;              /* [n_rec] */
    const int32_t *row;               /* [n_psm] or NULL: row_base + psm */
    const uint64_t *best_sig;
    const double *values;             /* [n_rows * n_ch] */
    unsigned long long *head;         /* pya_site_quant_head as one uint64: n_records (low), n_complete (high) */
    unsigned long long *cell;         /* pya_site_quant as 2 x uint64: sum; n (low), n_saturated (high) */
    uint32_t *over;
    uint64_t n_rec, n_slots, n_rows;
    double threshold, scale;          /* scale = 2^scale_log2, exact */
    uint32_t n_psm, row_base, n_ch, complete_only;
};

/* the record `rec` as a contribution: false when it has none; slot and row are inside the table and the matrix when true */
DEV bool sq_record(const SqArgs &a, uint64_t rec, int32_t &slot, int32_t &row) {
    const int32_t s = a.slot[rec];
    if (s < 0) return false;
    uint32_t psm;
    uint64_t r;
    if (!record_psm(a.site_off, a.n_psm, a.psm_probs, rec, psm, r)) return false;
    if (!((a.best_sig[psm] >> r) & 1ull)) return false;
    const uint2 pb = a.site_probs[rec * 2];
    if (!(__longlong_as_double((long long)((uint64_t)pb.y << 32 | pb.x)) >= a.threshold)) return false;
    const int64_t rw = a.row ? (int64_t)a.row[psm] : (int64_t)a.row_base + (int64_t)psm;
    if (rw < 0) return false;
    if ((uint64_t)s >= a.n_slots || (uint64_t)rw >= a.n_rows) {
        report_over(a.over, psm);
        return false;
    }
    slot = s;
    row = (int32_t)rw;
    return true;
}

__global__ void __launch_bounds__(SQ_THREADS) pya_site_quant_kernel(const SqArgs a) {
    const uint64_t rec = (uint64_t)blockIdx.x * SQ_THREADS + threadIdx.x;
    int32_t slot = -1, row = -1;
    bool active = false;
    if (rec < a.n_rec) active = sq_record(a, rec, slot, row);
    /* (from here on the control flow is wave-uniform: no lane has left) */
    qw_reduce(
        active, (uint32_t)slot, a.n_ch, a.head, a.cell,
        [&](int j, bool have) {                              /* the reading of record j's row */
            const uint32_t rj = (uint32_t)__builtin_amdgcn_readlane(row, j);
            return have && qw_channel(a.n_ch) ? a.values[(size_t)rj * a.n_ch + (uint32_t)lane_id()] : 0.0;
        },
        [&](QwAcc &c, double v) { qw_add_reading(c, v, a.n_ch, a.scale, a.complete_only); });
}

/* element i of the matrix: spectrum i / n_ch, the (i % n_ch)-th set bit of the mask as its target */
__global__ void __launch_bounds__(SQ_THREADS) pya_marker_values_kernel(const pya_marker *markers, uint64_t n_out, uint32_t n_targets,
                                                                       uint32_t n_ch, uint64_t mask, double *values) {
    const uint64_t i = (uint64_t)blockIdx.x * SQ_THREADS + threadIdx.x;
    if (i >= n_out) return;
    const uint64_t s = i / n_ch;
    uint64_t m = mask;
    for (uint32_t k = (uint32_t)(i - s * n_ch); k; k--) m &= m - 1ull;
    const pya_marker r = markers[s * n_targets + (uint32_t)__builtin_ctzll(m)];
    values[i] = (r.flags & PYA_MARKER_PICKED) ? r.intensity : __longlong_as_double(0x7ff8000000000000ll);
}

/* d_site_off: [n_psm + 1] offsets of the site stage, n_rec = site_off[n_psm] of them as the host knows it; d_site_probs /
 * d_psm_probs: the probability stage's records; d_slot: [n_rec]; d_row: [n_psm] or NULL (row_base + PSM); d_values: n_rows x
 * n_channels doubles; d_head / d_cell: the table; d_over: two words, zeroed by the caller.  prm has been checked. */
extern "C" int pya_launch_site_quant(const int64_t *d_site_off, uint64_t n_psm, uint64_t n_rec, const void *d_site_probs, const void *d_psm_probs,
                                     const int32_t *d_slot, uint64_t n_slots, const double *d_values, uint64_t n_rows, const int32_t *d_row,
                                     uint32_t row_base, const pya_site_quant_params *prm, double scale, const uint64_t *best_sig, void *d_head,
                                     void *d_cell, uint32_t *d_over, hipStream_t stream) {
    if (n_rec == 0 || n_psm == 0) return 0;
    const uint64_t blocks = (n_rec + SQ_THREADS - 1) / SQ_THREADS;
    if (blocks > 0x7fffffffull || n_psm > 0x7fffffffull) return (int)hipErrorInvalidValue;
    const SqArgs a = {d_site_off, (const uint2 *)d_site_probs, (const uint32_t *)d_psm_probs, d_slot, d_row, best_sig, d_values,
                      (unsigned long long *)d_head, (unsigned long long *)d_cell, d_over, n_rec, n_slots, n_rows, prm->threshold, scale,
                      (uint32_t)n_psm, row_base, prm->n_channels, (prm->flags & PYA_QUANT_COMPLETE_ONLY) ? 1u : 0u};
    hipLaunchKernelGGL(pya_site_quant_kernel, dim3((uint32_t)blocks), dim3(SQ_THREADS), 0, stream, a);
    return (int)hipGetLastError();
}

extern "C" int pya_launch_marker_values(const pya_marker *d_markers, uint64_t n_spectra, uint32_t n_targets, uint64_t mask, double *d_values,
                                        hipStream_t stream) {
    const uint32_t n_ch = (uint32_t)__builtin_popcountll(mask);
    const uint64_t n_out = n_spectra * n_ch;
    if (n_out == 0) return 0;
    const uint64_t blocks = (n_out + SQ_THREADS - 1) / SQ_THREADS;
    if (blocks > 0x7fffffffull) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(pya_marker_values_kernel, dim3((uint32_t)blocks), dim3(SQ_THREADS), 0, stream, d_markers, n_out, n_targets, n_ch, mask,
                       d_values);
    return (int)hipGetLastError();
}
