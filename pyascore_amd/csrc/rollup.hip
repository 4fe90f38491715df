/* rollup.hip -- site roll-up: the probability stage's residue records of many PSMs collapsed onto a dense table of
 * caller-keyed slots ("one site" of a peptide or protein), launched BEHIND a run and behind probs.hip.  The definition is in
 * include/pyascore_hip.h (pya_site_rollup); the reference has no counterpart.  The first reduction over PSMs in this tree.
 *
 * One thread per residue record, two kernels per call, every field an integer count, a max over bit patterns or a min over
 * ids: the table is a function of the multiset of contributing records, whatever order the atomics arrive in and however the
 * records were spread over calls.  The table the caller holds between calls is the public record; nothing is decoded or
 * encoded around a call.
 *   kernel 1  best_prob    atomicMax on the uint64 bits of with_prob (non-negative doubles order like their bits).  A record
 *                          that raised the max stores "no PSM" into best_psm: whatever claimed the slot before belongs to a
 *                          smaller probability.  Every such writer stores the same word.
 *             counts       n_psm one atomicAdd; n_confident and n_in_best share an aligned 8 bytes and take one 64-bit add.
 *                          Its return value names the ONE record of the call that found n_in_best at 0 -- the slot had no
 *                          Ascore yet --, and that record stores RU_NO_ASCORE into best_ascore: nobody else touches the word
 *                          in this kernel.
 *   kernel 2  best_psm     a record whose bits equal the slot's max: atomicMin of its psm_id.  A slot whose max did not rise
 *                          keeps the earlier claim, which competes as one more id.
 *             best_ascore  a float max without a compare-and-swap loop: a value with the sign bit clear takes a SIGNED
 *                          atomicMax (it beats every negative pattern, RU_NO_ASCORE among them, and orders like its bits
 *                          among the others), a value with the sign bit set an UNSIGNED atomicMin (it loses to every
 *                          non-negative pattern and, among the negative ones, the smallest pattern is the largest float;
 *                          RU_NO_ASCORE is the largest pattern there is).  The result is the max under the total order
 *                          -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN, whatever the order of arrival.
 * Both kernels skip an atomic that a plain load of the slot shows to be lost already: a word only moves one way inside a
 * kernel, so a stale value errs towards issuing the atomic.  Hot slots then cost a load, not a serialised atomic.
 * Plain accesses beside device-scope atomics on one 32-byte record, on a chip with eight L2s: the atomics are performed at
 * device scope whichever XCD issues them; a plain LOAD may see an older value from its CU's L1 or its XCD's L2, which is the
 * case above; a plain STORE only ever goes to a word that no atomic of the SAME kernel touches (best_psm and best_ascore in
 * kernel 1, nothing in kernel 2), every writer of a word stores the same value, the stores are byte-masked 4-byte writes that
 * do not disturb their neighbours, and the end of kernel 1 writes them back and the start of kernel 2 invalidates the caches
 * before kernel 2's atomics and loads see the word.  So nothing here depends on where a workgroup runs.
 * An Ascore with the bits of RU_NO_ASCORE (a NaN) cannot be told from the seed; it is the minimum of the order anyway.
 * A record finds its PSM by a binary search of the site offsets (device_common.hip.h: record_psm).
 * No write lies outside table[0 .. n_slots): a slot at or above n_slots is counted in over[0] (and the smallest such PSM kept
 * in over[1] as 0xffffffff - psm) and nothing of it is written. */
#include "device_common.hip.h"

#define RU_NO_PSM 0xffffffffu
#define RU_NO_ASCORE 0xffffffffu
#define RU_THREADS 256

/* a pya_site_rollup as the kernels address it: 4 x 8 bytes, 8 x 4 bytes */
#define RU_W_PROB 0                   /* uint64 [0]: best_prob                                   */
#define RU_D_PSM 2                    /* uint32 [2]: best_psm                                    */
#define RU_D_NPSM 3                   /* uint32 [3]: n_psm                                       */
#define RU_W_COUNTS 2                 /* uint64 [2]: n_confident (low), n_in_best (high)         */
#define RU_D_ASCORE 6                 /* uint32 [6]: best_ascore; [7] reserved                   */

struct RuArgs {
    const int64_t *site_off;          /* [n_psm + 1] */
    const uint2 *site_probs;          /* pya_site_prob as 4 x uint32: with_prob is the first 8 bytes of 16 */
    const uint32_t *psm_probs;        /* pya_psm_prob as 4 x uint32: kind is the low byte of word 3 */
    const int32_t *slot;              /* [n_rec] */
    const uint32_t *psm_id;           /* [n_psm] or NULL: psm_base + psm */
    const uint64_t *best_sig;
    const float *ascores;             /* row stride max_k */
    uint64_t *table;
    uint32_t *over;
    uint64_t n_rec, n_slots;
    double threshold;
    uint32_t n_psm, psm_base, max_k;
};

struct RuRec {
    uint64_t *w;                      /* the slot's record */
    uint64_t bits;                    /* with_prob */
    uint32_t id, ascore;
    bool in_best, confident;
};

/* the record `rec` as a contribution: false when it has none (negative slot, PSM not SCORED, slot outside the table) */
template <bool REPORT>
DEV bool ru_record(const RuArgs &a, uint64_t rec, RuRec &o) {
    const int32_t s = a.slot[rec];
    if (s < 0) return false;
    uint32_t psm;
    uint64_t r;
    if (!record_psm(a.site_off, a.n_psm, a.psm_probs, rec, psm, r)) return false;
    if ((uint64_t)s >= a.n_slots) {
        if (REPORT) report_over(a.over, psm);
        return false;
    }
    o.w = a.table + (size_t)s * 4;
    const uint2 pb = a.site_probs[rec * 2];
    o.bits = (uint64_t)pb.y << 32 | pb.x;
    o.confident = __longlong_as_double((long long)o.bits) >= a.threshold;
    o.id = a.psm_id ? a.psm_id[psm] : a.psm_base + psm;
    const uint64_t sig = a.best_sig[psm];
    const uint32_t col = (uint32_t)__popcll(sig & ((1ull << r) - 1ull));
    o.in_best = ((sig >> r) & 1ull) != 0 && col < a.max_k;
    o.ascore = o.in_best ? __float_as_uint(a.ascores[(size_t)psm * a.max_k + col]) : 0u;
    return true;
}

__global__ void __launch_bounds__(RU_THREADS) pya_rollup_accumulate_kernel(const RuArgs a) {
    const uint64_t rec = (uint64_t)blockIdx.x * RU_THREADS + threadIdx.x;
    if (rec >= a.n_rec) return;
    RuRec c;
    if (!ru_record<true>(a, rec, c)) return;
    uint32_t *d = (uint32_t *)c.w;
    if (c.w[RU_W_PROB] < c.bits) {
        const uint64_t old = atomicMax((unsigned long long *)&c.w[RU_W_PROB], (unsigned long long)c.bits);
        if (old < c.bits) d[RU_D_PSM] = RU_NO_PSM;
    }
    atomicAdd(&d[RU_D_NPSM], 1u);
    const uint64_t add = (c.confident ? 1ull : 0ull) | (c.in_best ? 1ull << 32 : 0ull);
    if (add) {
        const uint64_t old = atomicAdd((unsigned long long *)&c.w[RU_W_COUNTS], (unsigned long long)add);
        if (c.in_best && (old >> 32) == 0u) d[RU_D_ASCORE] = RU_NO_ASCORE;
    }
}

/* the order-preserving image of a float's bits: key(a) < key(b) exactly when a comes before b in the total order above */
DEV uint32_t ru_key(uint32_t b) { return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u); }

__global__ void __launch_bounds__(RU_THREADS) pya_rollup_claim_kernel(const RuArgs a) {
    const uint64_t rec = (uint64_t)blockIdx.x * RU_THREADS + threadIdx.x;
    if (rec >= a.n_rec) return;
    RuRec c;
    if (!ru_record<false>(a, rec, c)) return;
    uint32_t *d = (uint32_t *)c.w;
    if (c.w[RU_W_PROB] == c.bits && d[RU_D_PSM] > c.id) atomicMin(&d[RU_D_PSM], c.id);
    if (c.in_best) {
        const uint32_t cur = d[RU_D_ASCORE];
        if (cur == RU_NO_ASCORE || ru_key(cur) < ru_key(c.ascore)) {
            if (c.ascore >> 31) atomicMin(&d[RU_D_ASCORE], c.ascore);
            else atomicMax((int *)&d[RU_D_ASCORE], (int)c.ascore);
        }
    }
}

/* the empty table: best_psm is "no PSM", everything else 0 -- two 16-byte stores per slot */
__global__ void __launch_bounds__(RU_THREADS) pya_rollup_clear_kernel(uint4 *table, uint64_t n_slots) {
    const uint64_t s = (uint64_t)blockIdx.x * RU_THREADS + threadIdx.x;
    if (s >= n_slots) return;
    table[s * 2] = make_uint4(0u, 0u, RU_NO_PSM, 0u);
    table[s * 2 + 1] = make_uint4(0u, 0u, 0u, 0u);
}

extern "C" int pya_launch_rollup_clear(void *d_table, uint64_t n_slots, hipStream_t stream) {
    if (n_slots == 0) return 0;
    const uint64_t blocks = (n_slots + RU_THREADS - 1) / RU_THREADS;
    if (blocks > 0x7fffffffull) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(pya_rollup_clear_kernel, dim3((uint32_t)blocks), dim3(RU_THREADS), 0, stream, (uint4 *)d_table, n_slots);
    return (int)hipGetLastError();
}

/* d_site_off: [n_psm + 1] offsets of the site stage, n_rec = site_off[n_psm] of them as the host knows it; d_site_probs /
 * d_psm_probs: the probability stage's records; d_slot: [n_rec]; d_psm_id: [n_psm] or NULL (psm_base + PSM); best_sig, ascores
 * (row stride max_k): the run's results; d_table: n_slots records of 32 bytes; d_over: two words, zeroed by the caller.
 * grid[0] / grid[1]: the blocks of the two launches (0: none), when not NULL */
extern "C" int pya_launch_rollup(const int64_t *d_site_off, uint64_t n_psm, uint64_t n_rec, const void *d_site_probs, const void *d_psm_probs,
                                 const int32_t *d_slot, uint64_t n_slots, double threshold, const uint32_t *d_psm_id, uint32_t psm_base,
                                 const uint64_t *best_sig, const float *ascores, uint32_t max_k, void *d_table, uint32_t *d_over,
                                 uint32_t grid[2], hipStream_t stream) {
    if (grid) grid[0] = grid[1] = 0u;
    if (n_rec == 0 || n_psm == 0) return 0;
    const uint64_t blocks = (n_rec + RU_THREADS - 1) / RU_THREADS;
    if (blocks > 0x7fffffffull || n_psm > 0x7fffffffull) return (int)hipErrorInvalidValue;
    const RuArgs a = {d_site_off, (const uint2 *)d_site_probs, (const uint32_t *)d_psm_probs, d_slot, d_psm_id, best_sig, ascores,
                      (uint64_t *)d_table, d_over, n_rec, n_slots, threshold, (uint32_t)n_psm, psm_base, max_k};
    hipLaunchKernelGGL(pya_rollup_accumulate_kernel, dim3((uint32_t)blocks), dim3(RU_THREADS), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(pya_rollup_claim_kernel, dim3((uint32_t)blocks), dim3(RU_THREADS), 0, stream, a);
    if (grid) grid[0] = grid[1] = (uint32_t)blocks;
    return (int)hipGetLastError();
}
