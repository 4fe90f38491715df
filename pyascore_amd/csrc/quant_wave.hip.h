/* quant_wave.hip.h -- the wave-level aggregation of the quantification tables (include/pyascore_hip.h: pya_site_quant,
 * pya_site_quant_head), once.  site_quant.hip and pform_quant.hip include it; each brings its own step 1 -- lane = entry: does
 * the entry contribute (`active`), and to which position of the table (`key`) -- and says at compile time what an entry is.
 *
 * The table's slots are hot (many PSMs share a slot or a peptidoform), so a wavefront aggregates before it reaches memory:
 *   2  the contributing lanes that share a key find each other in a wave-uniform loop: the key of the first lane still to do
 *      by v_readlane, a ballot of equality.  At most 64 turns, one per distinct key of the wavefront.
 *   3  lane = channel.  For each group the lanes walk the group's entries -- entry j from the group's mask, uniform; what the
 *      caller's lane j holds of it comes by v_readlane inside `load` --, QW_UNROLL entries' loads in flight together, and
 *      accumulate a QwAcc in registers.  An entry that is a reading (a row of the caller's matrix, one coalesced load of
 *      values[row * n_channels + lane]) goes through qw_add_reading: a ballot of "usable" says whether the row is complete.
 *   4  one 64-bit atomic add per (group, channel) to sum, one of n | n_saturated << 32 to the aligned pair behind it, and one of
 *      n_records | n_complete << 32 to the head from lane 0; a part that is zero adds nothing (an add of 0 would leave the
 *      bytes as they are).
 * From `active` on the control flow is wave-uniform: no lane may have left before qw_reduce, `load` and `add` are called by all
 * 64 lanes, and the loop conditions are ballots or values taken by v_readfirstlane / v_readlane.  Everything that reaches
 * memory is a device-scope atomic add of a vector lane (the eight L2s do not matter to it: an atomic is performed at device
 * scope whichever XCD issues it); the table is never LOADED here.  No LDS, no workspace, no float atomics: every field is an
 * integer sum, so the bytes are the same whatever the grouping and whatever order the atomics arrive in.
 * The writes go to head[key] and cell[key * n_channels + lane], lane below n_channels, of an active lane's key and of nothing
 * else: that the key lies inside the table is the caller's to establish BEFORE it sets `active`. */
#pragma once
#include "quant_rule.hip.h"

#define QW_UNROLL 4                   /* entries in flight per lane in step 3 */

/* what one lane sums for one (group, channel); n_records and n_complete are wave-uniform, lane 0's go to the head */
struct QwAcc {
    uint64_t sum;
    uint32_t n, n_saturated, n_records, n_complete;
};

/* this lane is a channel */
DEV bool qw_channel(uint32_t n_ch) { return (uint32_t)lane_id() < n_ch; }

/* one record's reading `v` of this lane's channel (anything in a lane that is no channel).  Wave-uniform: all 64 lanes call it. */
DEV void qw_add_reading(QwAcc &c, double v, uint32_t n_ch, double scale, uint32_t complete_only) {
    const bool usable = qw_channel(n_ch) && qr_usable(v);
    const bool complete = (uint32_t)__popcll(__ballot(usable)) == n_ch;
    c.n_records++;
    c.n_complete += complete ? 1u : 0u;
    if (usable && (complete || !complete_only)) {
        bool sat;
        c.sum += qr_quantum(v, scale, &sat);
        c.n_saturated += sat ? 1u : 0u;
        c.n++;
    }
}

/* step 4 for the group at `key` */
DEV void qw_flush(const QwAcc &c, uint32_t key, uint32_t n_ch, unsigned long long *head, unsigned long long *cell) {
    const int lane = lane_id();
    if (qw_channel(n_ch)) {
        unsigned long long *p = cell + ((size_t)key * n_ch + (uint32_t)lane) * 2;
        if (c.sum) atomicAdd(p, (unsigned long long)c.sum);
        if (c.n | c.n_saturated) atomicAdd(p + 1, (unsigned long long)c.n | (unsigned long long)c.n_saturated << 32);
    }
    if (lane == 0 && (c.n_records | c.n_complete))
        atomicAdd(head + key, (unsigned long long)c.n_records | (unsigned long long)c.n_complete << 32);
}

/* Steps 2 to 4.  load(j, have) -> E: this lane's part of the entry that the caller's lane j (uniform) stands for, loads
 * issued and not yet used; `have` false (uniform): no entry, nothing may be read.  add(acc, e): the entry into the
 * accumulator.  Both are called wave-uniformly, `add` only for entries that are there. */
template <typename Load, typename Add>
DEV void qw_reduce(bool active, uint32_t key, uint32_t n_ch, unsigned long long *head, unsigned long long *cell, const Load &load,
                   const Add &add) {
    uint64_t todo = __ballot(active);
    while (todo) {
        const int lead = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(todo));
        const uint32_t gk = (uint32_t)__builtin_amdgcn_readlane((int)key, lead);
        uint64_t grp = __ballot(active && key == gk);
        todo &= ~grp;
        QwAcc acc = {0ull, 0u, 0u, 0u, 0u};
        while (grp) {
            decltype(load(0, false)) e[QW_UNROLL];
            bool have[QW_UNROLL];
#pragma unroll
            for (int u = 0; u < QW_UNROLL; u++) {
                have[u] = grp != 0ull;
                const int j = __builtin_amdgcn_readfirstlane(have[u] ? (int)__builtin_ctzll(grp) : 0);
                grp &= grp - 1ull;                           /* (0 stays 0) */
                e[u] = load(j, have[u]);
            }
#pragma unroll
            for (int u = 0; u < QW_UNROLL; u++) {
                if (!have[u]) break;
                add(acc, e[u]);
            }
            /* vmcnt(0).  Every load of this turn has been used, so it waits for nothing; it tells the compiler so.  Without it
             * the compiler takes a load of an entry that was not there for pending on the way out of the loop, and when it next
             * touches that register -- in the flush, at the next group -- it waits for the atomics issued since: every group
             * then costs three trips to memory one after the other in place of one. */
            __builtin_amdgcn_s_waitcnt(0x0f70);
        }
        qw_flush(acc, gk, n_ch, head, cell);
    }
}
