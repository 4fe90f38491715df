/* decharge.hip -- charge deconvolution of spectra in front of a run (include/pyascore_hip.h: pya_decharge_params has THE RULE):
 * deisotoping, and every kept peak whose satellites testify to a charge of 2 or more moved to the m/z of the same fragment at
 * 1+.  Not part of a run, for deisotope.hip's reason: the peak counts change and a plan reads them on the host.  The reference
 * has no counterpart.
 *
 * Three stream-ordered passes, no float atomics, no LDS, the launch shape of deisotope.hip (one wavefront per spectrum striding
 * over its peaks 64 at a time, four wavefronts per workgroup, a capped grid that strides over the spectra):
 * MARK   each lane decides its own peak: deiso_removed (deiso_rule.hip.h) walks down to see whether it is removed; a kept peak
 *        then walks UP through x[j] - x[i] - spacing[0] <= tol, the one window that holds the children of every charge, and
 *        takes the largest charge a witnessed child testifies to.  Two ballots per stride: the keep word and the moved word.
 *        Lane 0 writes both and the number of kept-unmoved peaks before the stride; every moved lane writes (stored value, raw
 *        index, charge) into the spectrum's list at (moved peaks before the stride) + mbcnt of the moved word, so the list is in
 *        raw order.  At the end: the kept count to new_off[s], the moved count to n_moved[s].  A spectrum that is not ascending
 *        gets its words written again: every peak kept, none moved.
 * SCAN   the ion stage's exclusive scan (ions.hip, pya_launch_ions_scan) over new_off, in place.
 * PLACE  each kept peak computes its position in the output, which is the kept peaks sorted by (stored value, raw index), and
 *        writes itself there.  The kept-unmoved peaks are ascending as they stand and so is nothing else: the position of a
 *        peak is its rank among the kept-unmoved peaks plus its rank among the moved ones.
 *          unmoved peak k: (kept-unmoved before the stride, a running sum) + mbcnt of the stride's unmoved word, plus the
 *            moved entries with a smaller (value, index) key;
 *          moved peak i with value v: a lower-bound binary search of v in the raw m/z gives the first raw index whose m/z is
 *            not below v; the kept-unmoved peaks before that index are the stride's prefix plus a popcount of the unmoved word
 *            below it (a kept-unmoved peak of m/z equal to v has a higher raw index than i, v being above x[i], so it comes
 *            after); plus the moved entries with a smaller key.
 *        The count over the moved list is THE PLAIN FORM: one wave-uniform loop over the list per stride (the entry is a uniform
 *        load, each lane compares it with its own key), O(kept x moved / 64) wave steps per spectrum.  The list is not sorted
 *        in LDS: profiles/decharge/probe.txt says whether PLACE dominates on dense spectra.
 * The words of spectrum s (keep, moved, before) start at word (p0 >> 6) + s of their region: ceil(n / 64) words never reach the
 * next spectrum's first word.  Its list starts at entry p0 of the list region (two words an entry) and has at most n entries.
 * Both kernels clip the offsets of a spectrum to [0, total] as deisotope.hip does, total being peak_off[n_spectra] or the peaks
 * the lent workspace has room for, whichever is smaller; PLACE writes no element at or beyond total. */
#include "deiso_rule.hip.h"

/* the charge of kept peak i (m/z xi, intensity yi) of the spectrum that ends at p1: the largest z in 2 .. max_charge for which a
 * peak j has R(i, j, z) -- deiso_removed's test with i as the parent, operation for operation -- and y[j] >= y[i] witness; 1
 * without one.  e0 rises with j and the e of a higher charge is no smaller, so nothing beyond the first j that fails
 * e0 <= tol can match at any charge (an e0 that is a NaN -- infinite m/z on both sides -- ends the walk too: it matches nothing,
 * nor does anything behind it). */
template <typename TM, typename TI>
DEV uint32_t dechg_charge(const TM *mz, const TI *in, int64_t p1, int64_t i, double xi, double yi, const pya_decharge_params &prm) {
    const double least = yi * prm.witness;
    uint32_t c = 1;
    for (int64_t j = i + 1; j < p1; j++) {
        const double d = deiso_widen(mz[j]) - xi;
        const double e0 = d - prm.iso.spacing[0];
        if (!(e0 <= prm.iso.tol)) break;
        for (uint32_t z = 2; z <= prm.iso.max_charge; z++) {
            const double e = d - prm.iso.spacing[z - 1];
            if (__builtin_fabs(e) <= prm.iso.tol) {
                const double m = xi * (double)z;
                const double b = prm.iso.ratio0 + prm.iso.ratio_per_mz * m;
                const double yj = deiso_widen(in[j]);
                if (yj <= yi * b && yj >= least && z > c) c = z;
            }
        }
    }
    return c;
}

DEV void dechg_copy_bits(float *to, const float *from) { *(uint32_t *)to = *(const uint32_t *)from; }
DEV void dechg_copy_bits(double *to, const double *from) { *(uint64_t *)to = *(const uint64_t *)from; }
DEV uint64_t dechg_low_bits(int n) { return n >= 64 ? ~0ull : (1ull << n) - 1ull; }   /* n in 0 .. 64 */

template <typename TM, typename TI>
__global__ __launch_bounds__(64 * DEISO_WAVES) void pya_dechg_mark_kernel(const TM *mz, const TI *in, const int64_t *peak_off, uint64_t n_spectra,
                                                                          pya_decharge_params prm, int64_t cap_peaks, uint64_t *keep,
                                                                          uint64_t *moved, uint64_t *before, uint64_t *n_moved, uint64_t *list,
                                                                          int64_t *new_off, uint32_t *over) {
    const int lane = lane_id();
    const uint64_t wave = (uint64_t)blockIdx.x * DEISO_WAVES + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t n_waves = (uint64_t)gridDim.x * DEISO_WAVES;
    const int64_t total = deiso_total(peak_off, n_spectra, cap_peaks);
    for (uint64_t s = wave; s < n_spectra; s += n_waves) {
        int64_t p0, p1;
        bool clipped;
        deiso_range(peak_off, s, total, &p0, &p1, &clipped);
        const uint64_t w0 = ((uint64_t)p0 >> 6) + s;
        uint64_t *entries = list + 2ull * (uint64_t)p0;
        uint64_t kept = 0, n_mv = 0;
        bool bad = false;
        for (int64_t k0 = p0; k0 < p1; k0 += 64) {                     /* (wave-uniform trip count) */
            const int64_t i = k0 + lane;
            bool stay = false, unordered = false, moves = false;
            uint32_t c = 1;
            double stored = 0.;
            if (i < p1) {
                const double xi = deiso_widen(mz[i]), yi = deiso_widen(in[i]);
                if (i > p0 && !(deiso_widen(mz[i - 1]) <= xi)) unordered = true;
                stay = !deiso_removed(mz, in, p0, i, xi, yi, prm.iso);
                if (stay && prm.iso.max_charge >= 2) c = dechg_charge(mz, in, p1, i, xi, yi, prm);
                if (c >= 2) {
                    const double t = xi * (double)c;
                    const double u = (double)(c - 1) * prm.carrier;
                    const double v = t - u;
                    stored = deiso_widen((TM)v);                       /* (rounded once to the element type) */
                    moves = stored - stored == 0. && stored > xi;      /* (finite, and above where it was) */
                }
            }
            const uint64_t mask = __ballot(stay), mv = __ballot(moves);
            if (__ballot(unordered) != 0ull) bad = true;
            const uint64_t word = (uint64_t)(k0 - p0) >> 6;
            if (lane == 0) {
                keep[w0 + word] = mask;
                moved[w0 + word] = mv;
                before[w0 + word] = kept - n_mv;
            }
            if (moves) {
                const uint64_t at = n_mv + (uint64_t)mask_rank(mv);    /* (below p1 - p0: the list is the spectrum's own) */
                entries[2 * at] = (uint64_t)__double_as_longlong(stored);
                entries[2 * at + 1] = ((uint64_t)c << 56) | (uint64_t)(i - p0);
            }
            kept += (uint64_t)__builtin_popcountll(mask);
            n_mv += (uint64_t)__builtin_popcountll(mv);
        }
        if (bad) {                                                     /* not ascending: every peak stays where it is */
            for (int64_t k0 = p0; k0 < p1; k0 += 64) {
                const uint64_t word = (uint64_t)(k0 - p0) >> 6;
                if (lane == 0) {
                    keep[w0 + word] = dechg_low_bits((int)(p1 - k0 >= 64 ? 64 : p1 - k0));
                    moved[w0 + word] = 0ull;
                    before[w0 + word] = (uint64_t)(k0 - p0);
                }
            }
            kept = (uint64_t)(p1 - p0);
            n_mv = 0;
        }
        if (lane == 0) {
            new_off[s] = (int64_t)kept;
            n_moved[s] = n_mv;
            if (bad || clipped) report_over(over, (uint32_t)s);
        }
    }
}

/* TM: the m/z element type (its values are compared); TI: an unsigned integer of the width of the intensity elements */
template <typename TM, typename TI>
__global__ __launch_bounds__(64 * DEISO_WAVES) void pya_dechg_place_kernel(const TM *__restrict__ mz, const TI *__restrict__ in,
                                                                           const int64_t *__restrict__ peak_off, uint64_t n_spectra, int64_t cap_peaks,
                                                                           const uint64_t *__restrict__ keep, const uint64_t *__restrict__ moved,
                                                                           const uint64_t *__restrict__ before, const uint64_t *__restrict__ n_moved,
                                                                           const uint64_t *__restrict__ list, const int64_t *__restrict__ new_off,
                                                                           TM *__restrict__ out_mz, TI *__restrict__ out_in, uint8_t *__restrict__ out_charge) {
    const int lane = lane_id();
    const uint64_t wave = (uint64_t)blockIdx.x * DEISO_WAVES + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t n_waves = (uint64_t)gridDim.x * DEISO_WAVES;
    const int64_t total = deiso_total(peak_off, n_spectra, cap_peaks);
    for (uint64_t s = wave; s < n_spectra; s += n_waves) {
        int64_t p0, p1;
        bool clipped;
        deiso_range(peak_off, s, total, &p0, &p1, &clipped);
        const uint64_t w0 = ((uint64_t)p0 >> 6) + s;
        const uint64_t *entries = list + 2ull * (uint64_t)p0;
        const uint64_t n_mv = n_moved[s];
        const int64_t dst = new_off[s];
        uint64_t run_un = 0, run_mv = 0;
        for (int64_t k0 = p0; k0 < p1; k0 += 64) {
            const uint64_t word = (uint64_t)(k0 - p0) >> 6;
            const uint64_t mask = keep[w0 + word], mv = moved[w0 + word], un = mask & ~mv;
            const int64_t i = k0 + lane;
            const bool kept = ((mask >> lane) & 1ull) != 0ull && i < p1, moves = ((mv >> lane) & 1ull) != 0ull && kept;
            /* the lane's key, its charge, and its rank among the kept-unmoved peaks */
            double key = 0.;
            uint64_t key_idx = (uint64_t)(i - p0), rank = 0;
            uint32_t c = 1;
            if (moves) {
                uint64_t e = run_mv + (uint64_t)mask_rank(mv);         /* (below n_mv; held there should offsets overlap) */
                if (e >= (uint64_t)(p1 - p0)) e = (uint64_t)(p1 - p0) - 1ull;
                key = __longlong_as_double((long long)entries[2 * e]);
                c = (uint32_t)(entries[2 * e + 1] >> 56);
                int64_t lo = i + 1, hi = p1;                           /* (the value is above x[i]) */
                while (lo < hi) {
                    const int64_t mid = lo + ((hi - lo) >> 1);
                    if (deiso_widen(mz[mid]) < key) lo = mid + 1; else hi = mid;
                }
                const uint64_t last = (uint64_t)(lo - p0) - 1ull;      /* (lo > p0: the unmoved among raw 0 .. last) */
                rank = before[w0 + (last >> 6)] + (uint64_t)__builtin_popcountll((keep[w0 + (last >> 6)] & ~moved[w0 + (last >> 6)]) &
                                                                                 dechg_low_bits((int)(last & 63ull) + 1));
            } else if (kept) {
                key = deiso_widen(mz[i]);
                rank = run_un + (uint64_t)mask_rank(un);
            }
            /* its rank among the moved peaks: entries with a smaller (value, index); the entry is wave-uniform */
            uint64_t below = 0;
            for (uint64_t m = 0; m < n_mv; m++) {
                const double val = __longlong_as_double((long long)entries[2 * m]);
                const uint64_t idx = entries[2 * m + 1] & 0x00ffffffffffffffull;
                below += (val < key || (val == key && idx < key_idx)) ? 1ull : 0ull;
            }
            if (kept) {
                const int64_t at = dst + (int64_t)(rank + below);
                if (at >= 0 && at < total) {                           /* (offsets that overlap cannot push a write past the array) */
                    if (moves) out_mz[at] = (TM)key; else dechg_copy_bits(out_mz + at, mz + i);
                    out_in[at] = in[i];
                    if (out_charge) out_charge[at] = (uint8_t)c;
                }
            }
            run_un += (uint64_t)__builtin_popcountll(un);
            run_mv += (uint64_t)__builtin_popcountll(mv);
        }
    }
}

extern "C" int pya_launch_ions_scan(int64_t *d_off, uint32_t n, uint64_t *d_tiles, hipStream_t stream);

template <typename TM, typename TI>
static void dechg_mark(uint32_t blocks, hipStream_t stream, const void *mz, const void *in, const int64_t *peak_off, uint64_t n_spectra,
                       const pya_decharge_params *prm, int64_t cap_peaks, uint64_t *keep, uint64_t *moved, uint64_t *before, uint64_t *n_moved,
                       uint64_t *list, int64_t *new_off, uint32_t *over) {
    hipLaunchKernelGGL((pya_dechg_mark_kernel<TM, TI>), dim3(blocks), dim3(64 * DEISO_WAVES), 0, stream, (const TM *)mz, (const TI *)in, peak_off,
                       n_spectra, *prm, cap_peaks, keep, moved, before, n_moved, list, new_off, over);
}

template <typename TM, typename TI>
static void dechg_place(uint32_t blocks, hipStream_t stream, const void *mz, const void *in, const int64_t *peak_off, uint64_t n_spectra,
                        int64_t cap_peaks, const uint64_t *keep, const uint64_t *moved, const uint64_t *before, const uint64_t *n_moved,
                        const uint64_t *list, const int64_t *new_off, void *out_mz, void *out_in, uint8_t *out_charge) {
    hipLaunchKernelGGL((pya_dechg_place_kernel<TM, TI>), dim3(blocks), dim3(64 * DEISO_WAVES), 0, stream, (const TM *)mz, (const TI *)in, peak_off,
                       n_spectra, cap_peaks, keep, moved, before, n_moved, list, new_off, (TM *)out_mz, (TI *)out_in, out_charge);
}

/* d_tiles: room for pya_ions_scan_tiles(n_spectra) words; d_regions: the three word regions of region_words words each (keep,
 * moved, before), n_spectra words of moved counts and 2 cap_peaks words of list behind them; cap_peaks: the peaks they have room
 * for.  The types are checked by the caller: (F64, F64), (F64, F32) or (F32, F32).  n_spectra in 1 .. 2^32 - 2.  passes: bit 0
 * MARK, bit 1 SCAN, bit 2 PLACE (a probe times them apart; everything else passes 7). */
extern "C" int pya_launch_decharge(const void *d_mz, const void *d_in, uint32_t mz_type, uint32_t in_type, const int64_t *d_peak_off,
                                   uint64_t n_spectra, const pya_decharge_params *prm, int64_t cap_peaks, uint64_t *d_tiles, uint64_t *d_regions,
                                   uint64_t region_words, void *d_out_mz, void *d_out_in, int64_t *d_new_off, uint8_t *d_charge, uint32_t *d_over,
                                   uint32_t passes, hipStream_t stream) {
    if (n_spectra == 0) return 0;
    const uint64_t want = (n_spectra + DEISO_WAVES - 1) / DEISO_WAVES;
    const uint32_t blocks = (uint32_t)(want < DEISO_MAX_BLOCKS ? want : DEISO_MAX_BLOCKS);
    uint64_t *keep = d_regions, *moved = keep + region_words, *before = moved + region_words, *n_moved = before + region_words;
    uint64_t *list = n_moved + n_spectra;
    int e = 0;
    if (passes & 1u) {
        if (mz_type == PYA_F32)
            dechg_mark<float, float>(blocks, stream, d_mz, d_in, d_peak_off, n_spectra, prm, cap_peaks, keep, moved, before, n_moved, list, d_new_off, d_over);
        else if (in_type == PYA_F32)
            dechg_mark<double, float>(blocks, stream, d_mz, d_in, d_peak_off, n_spectra, prm, cap_peaks, keep, moved, before, n_moved, list, d_new_off, d_over);
        else
            dechg_mark<double, double>(blocks, stream, d_mz, d_in, d_peak_off, n_spectra, prm, cap_peaks, keep, moved, before, n_moved, list, d_new_off, d_over);
        e = (int)hipGetLastError();
        if (e) return e;
    }
    if (passes & 2u) {
        e = pya_launch_ions_scan(d_new_off, (uint32_t)n_spectra, d_tiles, stream);
        if (e) return e;
    }
    if (passes & 4u) {
        if (mz_type == PYA_F32)
            dechg_place<float, uint32_t>(blocks, stream, d_mz, d_in, d_peak_off, n_spectra, cap_peaks, keep, moved, before, n_moved, list, d_new_off,
                                         d_out_mz, d_out_in, d_charge);
        else if (in_type == PYA_F32)
            dechg_place<double, uint32_t>(blocks, stream, d_mz, d_in, d_peak_off, n_spectra, cap_peaks, keep, moved, before, n_moved, list, d_new_off,
                                          d_out_mz, d_out_in, d_charge);
        else
            dechg_place<double, uint64_t>(blocks, stream, d_mz, d_in, d_peak_off, n_spectra, cap_peaks, keep, moved, before, n_moved, list, d_new_off,
                                          d_out_mz, d_out_in, d_charge);
        e = (int)hipGetLastError();
    }
    return e;
}
