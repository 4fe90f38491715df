/* pyascore_debug.h -- TEST-ONLY part of libpyascore_hip.so's C ABI.
 *
 * The kernels behind pyascore.PyAscore.score are several routes that must all give the reference's results
 * (fused / lean / general localisation, shared-node or per-walker scoring, the sort emulation, the hand-over lists
 * between kernels ...).  The parity suite drives every one of them on the same inputs; which route a PSM takes in
 * production is decided by its shape alone.  The switches that force a route, make a kernel decline what it would
 * take, or resize a table so that a hand-over happens, are set PER HANDLE through this call and through nothing else:
 * no environment variable selects a route (the library reads four variables, none of them a route: pyascore_hip.h,
 * pya_reload_env).  No reference counterpart: the reference has one route.
 */
#ifndef PYASCORE_DEBUG_H
#define PYASCORE_DEBUG_H
#include "pyascore_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Sets one debug switch of the handle.  `key` is the switch's name, `value` its value as text; value == NULL puts the
 * switch back to its production default.  pya_reload_env resets all of them.  Unknown names: PYA_ERR_ARG.
 *   flags (any non-NULL value = on): PYA_NO_PLAIN PYA_NO_FUSED PYA_NO_BIG PYA_NO_TINY PYA_NO_PREFIX PYA_NO_CHUNKS
 *     PYA_NO_UPLOAD_THREAD PYA_ONE_PEAK_CLASS PYA_PEAK_CLASSES PYA_ONE_LDS_CLASS PYA_SORT_ROOM PYA_NO_BIG_INLINE
 *     PYA_NO_LOC_HASH PYA_NO_NODES PYA_NO_CNT PYA_NO_PROB_CNT (the probability stage scores every PSM with its
 *     general front end, csrc/probs.hip) PYA_HOST_TIMING PYA_STAMPS PYA_SLOW_NULL_STREAM PYA_NO_FORK (r06: the
 *     fused family behind the scoring kernels on the caller's stream instead of beside them on the plan's side stream)
 *   numbers: PYA_DEBUG (bit set, common.h; 0x08000000 = no split walk: the fused score-localize body walks every PSM
 *     on its walker lanes alone, for A/B runs and tests/test_gpu_split_walk.py; 0x04000000 = no span count: it pairs the
 *     span ions of every PSM by their m/z lists, for A/B runs and tests/test_gpu_span_count.py) PYA_PLAIN_MIN PYA_BIG_MIN_N PYA_TINY_MAX PYA_SORT_ROOM_MAX PYA_SB PYA_GTP
 *     PYA_HASH_PP PYA_NODE_CAP PYA_CHUNK_MB PYA_WORKSPACE_MB
 *     PYA_BIN_SELECT_MIN (r06: peak classes above this many peaks are binned by selection, csrc/bin_select.hip.h; default 640,
 *     0 = every class, a huge value = none) PYA_BIN_SELECT_SCAP (survivor slots per spectrum there; default 768) */
int pya_set_debug(pya_handle *h, const char *key, const char *value);

/* The wavefront primitives every kernel leans on (csrc/device_common.hip.h: prefix sums and reductions by DPP, the rank of
 * a lane in a ballot), run by one full wavefront on 64 values (as every call site does):
 *   out[0..63]    exclusive prefix sum of in[]
 *   out[64..127]  inclusive prefix sums within each half of 32 lanes
 *   out[128..191] inclusive prefix sum over the 64 lanes
 *   out[192..255] rank of the lane among the lanes whose value is odd
 *   out[256..262] total, sum, max and min (as unsigned), max and min of the values read as floats, min rank of an odd value's lane
 * No reference counterpart. */
int pya_debug_wave_ops(pya_handle *h, const int32_t in[64], int32_t out[263]);

/* ---- the device building blocks, one at a time (csrc/debug_ops.hip; tests/test_gpu_device_ops.py) ----
 * Test-only kernels around the functions of csrc/device_common.hip.h, lane_f64.hip.h, tile_sort.hip.h and the ion stage's
 * scan, with the production headers included as they are.  Each call allocates what it needs, runs on the null stream and
 * returns when the results are on the host.  No reference counterpart. */

/* The peak lookup.  mz[n], rank[n]: a retained table as the binning leaves one -- n <= PYA_DEBUG_LOOKUP_MAX_N entries, every
 * m/z finite and not below the one before, every rank below PYA_NO_MATCH = 15; mz_error in (0, 50) as pya_create takes it; query[n_query] any
 * float32 bit patterns.  Anything else (a NULL array with a count above 0 too) is PYA_ERR_ARG and NOTHING IS LAUNCHED: the
 * lookup's loops end at the +inf entries behind a table and must not see one production could not build.
 * A wavefront stages the table in LDS (copy_peak_table, grid_build; LDS above 64 KB allowed as the production launches allow
 * it) and leaves the grid in global memory; the queries are then looked up by wavefronts that stage it the same way, through
 * the LDS table and through global_peak_table_at on the table and grid in global memory (behind whose last entry lie four
 * entries at the last m/z with rank 0, which the global lookup reads and must mask).
 *   out[4 q + 0]  match_rank_lds(query[q])
 *   out[4 q + 1]  look4, finished by look_rest where more(); 255 where mz_error > 0.49 (look4 is not for those settings)
 *   out[4 q + 2]  match_rank_global
 *   out[4 q + 3]  more() of that look4 (0 / 1; 255 as above)
 *   cells[0 .. 255] the grid, cells[256] last_cell (cells above last_cell are never read and hold anything) */
#define PYA_DEBUG_LOOKUP_MAX_N 8192
int pya_debug_lookup(pya_handle *h, const float *mz, const uint32_t *rank, uint32_t n, float mz_error, const float *query, uint32_t n_query,
                     uint8_t *out, uint32_t cells[257]);

/* One value per lane: out[i] = op(a[i], b[i]) for i < n, all arrays 64-bit words (a function's 32-bit arguments are the low
 * halves, its 32-bit result is zero-extended).
 *   PYA_DBG_FASTDIV        fastdiv(a, fastdiv_make(b))
 *   PYA_DBG_CHARGE_MZ      the bits of charge_mz(a read as a double, z = b); b = 1 .. 255, else PYA_ERR_ARG
 *   PYA_DBG_NTH_SET_BIT    nth_set_bit(mask a, n = b)
 *   PYA_DBG_DEPOSIT_SITES  deposit_sites(bits a, site_mask b)
 *   PYA_DBG_XCD_SLOT       xcd_slot(block a, blocks b)
 *   PYA_DBG_NL_BUMP        nl_bump(state a, class b); b = 1 .. 16, else PYA_ERR_ARG
 *   PYA_DBG_LUT_ROW        lut_row(a)
 *   PYA_DBG_HIST           hist_add of the (b & 255) <= 16 ranks of 4 bits in a, lowest first, into an empty histogram; then
 *                          with s = (b >> 8) & 255:  s < 16 hist_get(s),  16 / 17 / 18 the word a / b / c */
enum { PYA_DBG_FASTDIV = 0, PYA_DBG_CHARGE_MZ, PYA_DBG_NTH_SET_BIT, PYA_DBG_DEPOSIT_SITES, PYA_DBG_XCD_SLOT, PYA_DBG_NL_BUMP,
       PYA_DBG_LUT_ROW, PYA_DBG_HIST, PYA_DBG_LANE_OPS };
int pya_debug_lane_ops(pya_handle *h, uint32_t op, const uint64_t *a, const uint64_t *b, uint64_t n, uint64_t *out);

/* One full wavefront: in[PYA_DBG_WAVE_IN], out[PYA_DBG_WAVE_OUT] 64-bit words, lane l's value at in[l] (words no op reads or
 * writes: ignored / 0).
 *   PYA_DBG_WAVE_SUM_U64      out[l] = wave_sum_u64 as lane l has it
 *   PYA_DBG_WAVE_MINMAX_F64   out[l], out[64 + l] = wave_min_f64, wave_max_f64 of the values read as doubles
 *   PYA_DBG_MARKER_LANE_F64   out[64 s + l] = marker_lane_f64(value, s) as lane l has it, for every source lane s
 *   PYA_DBG_ION_SCAN_U64      out[l] = ion_wave_excl_scan_u64 (csrc/ions.hip; values below 2^50), out[64 + l] its total
 *   PYA_DBG_HIST_WAVE_SUM     the three words of lane l's histogram at in[l], in[64 + l], in[128 + l]; the sums likewise
 *   PYA_DBG_SAME_DIGIT        out[l] = ts_same_digit(digit in[l], in = (in[64 + l] != 0)) */
enum { PYA_DBG_WAVE_SUM_U64 = 0, PYA_DBG_WAVE_MINMAX_F64, PYA_DBG_MARKER_LANE_F64, PYA_DBG_ION_SCAN_U64, PYA_DBG_HIST_WAVE_SUM,
       PYA_DBG_SAME_DIGIT, PYA_DBG_WAVE_OPS };
#define PYA_DBG_WAVE_IN 192
#define PYA_DBG_WAVE_OUT 4096
int pya_debug_wave64(pya_handle *h, uint32_t op, const uint64_t *in, uint64_t *out);

/* The scans of csrc/tile_sort.hip.h over two policies of the test kernels' own, entries as 32-bit words:
 *   PYA_DBG_SCAN_ADD  one word, a + b (wraps);
 *   PYA_DBG_SCAN_SEG  three words (v, f, last), associative and NOT commutative -- a before b:
 *                     v = b.f ? b.v : a.v + b.v,  f = a.f | b.f,  last = b.f ? b.last : a.last;  identity (0, 0, 0).
 * pya_debug_block_scan: ts_block_scan by one workgroup over in[256] entries; out: 257 entries, [0 .. 255] the exclusive
 * scan, [256] the total.  pya_debug_ts_scan: ts_scan as the stages launch it, the exclusive scan of data[n] in place
 * (n <= 2^24; three levels from 65 537 entries). */
enum { PYA_DBG_SCAN_ADD = 0, PYA_DBG_SCAN_SEG = 1 };
int pya_debug_block_scan(pya_handle *h, uint32_t policy, const uint32_t *in, uint32_t *out);
int pya_debug_ts_scan(pya_handle *h, uint32_t policy, uint32_t *data, uint64_t n);

/* pya_launch_ions_scan as the ion stage and the spectrum transforms launch it: off[0 .. n) counts in, offsets out, off[n]
 * their sum (n <= 2^24; the carry loop takes a second trip from 65 537 entries). */
int pya_debug_ions_scan(pya_handle *h, int64_t *off, uint32_t n);

/* The handle's device tables as they are now: out[0] entries of the signature order table that are on the device, out[1] rows
 * of the score table that are, out[2] uploads of the DevConfig so far, out[3] the device address of the score table as an
 * integer (a table that grows is uploaded into a new allocation).  The tests of live plans read from it that a table grew and
 * moved between two runs of one plan, and that a refused call uploaded nothing.  No reference counterpart. */
int pya_debug_table_sizes(const pya_handle *h, uint64_t out[4]);

/* Whether the fused score-localize kernel counts the site-determining ions of this PSM's spans instead of pairing them by
 * their m/z lists (csrc/span_guard.h), restated on the host in the kernel's float32 / float64 operations from the handle's
 * mod_group, mod_mass and mz_error, the peptide (len <= 64 letters) and its fixed modifications (aux_pos, aux_mass as in a
 * pya_batch: position 0 = the N-terminus, else residue aux_pos - 1).  Returns 1 (counted), 0 (paired) or PYA_ERR_ARG.  It is
 * the decision per PSM: a launch with fragment charges above 1 and PYA_DEBUG bits 2048 / 0x04000000 pair every PSM.  out (may be
 * NULL): [0] E = mz_error + the PSM's rounding margin, [1], [2] the interval every modifiable residue's mass delta must lie in.
 * The tests place inputs on a chosen side of the guard with it; the results are the same on both.  No reference counterpart. */
int pya_debug_span_guard(const pya_handle *h, const char *peptide, uint64_t len, const uint32_t *aux_pos, const float *aux_mass,
                         uint64_t n_aux, double out[3]);

/* The composite keys the common-case binning kernels rank the peaks of a spectrum by (csrc/bin_key.h: a float32 with the window
 * in its exponent and 23 bits of intensity in its mantissa), computed on the host with that header's own operations:
 * keys[i] for intensity[i] in window[i] (< 64), the key base taken from the largest intensity of the array as a spectrum's most
 * intense peak gives it (*key_base, may be NULL).  PYA_ERR_ARG: n == 0, a NULL array, a window of 64 or more, an intensity that
 * is negative, infinite or NaN (no spectrum with such a peak takes the fast path).  Needs no handle and no device.  The tests
 * place intensities a chosen number of key steps apart with it.  No reference counterpart. */
int pya_debug_bin_keys(const double *intensity, const uint32_t *window, uint64_t n, uint32_t *keys, uint32_t *key_base);

/* Plans the last pya_score_batch / pya_score_batch_shared / pya_score_batch_typed call on the handle was cut into (1: one
 * plan, not pipelined; 0: no call yet).  The tests read from it that a budget cuts a float32 batch into no more chunks than
 * the same batch widened.  No reference counterpart. */
uint64_t pya_debug_last_chunks(const pya_handle *h);

/* What the last pya_plan_probs call on a plan of this handle launched (a batch call with PYA_FLAG_PROBS makes one per chunk),
 * for its two launches -- [0] the PSMs inside the fast kernels' limits, [1] the plan's general list: front_ends = 1 the
 * count-node tables alone (every scored PSM of the launch went through them), 2 the general front end alone, 3 both carved
 * (the kernel chooses per PSM), 0 no launch; lds_bytes = the dynamic LDS of the launch.  No reference counterpart. */
int pya_debug_last_probs_launch(const pya_handle *h, uint32_t front_ends[2], uint64_t lds_bytes[2]);

/* The same for the last pya_plan_ranked call (a batch call with PYA_FLAG_RANKED makes one per chunk): the front ends and
 * the LDS bytes of its two launches, with the meanings above.  PYA_NO_PROB_CNT holds for this stage as well.  No reference
 * counterpart. */
int pya_debug_last_ranked_launch(const pya_handle *h, uint32_t front_ends[2], uint64_t lds_bytes[2]);

/* The last pya_plan_rollup call (a batch call with PYA_FLAG_ROLLUP makes one per chunk): the blocks of its two launches,
 * 0 when the plan had no residue records; *n_records = the records it walked.  No reference counterpart. */
int pya_debug_last_rollup_launch(const pya_handle *h, uint32_t grid[2], uint64_t *n_records);

/* pya_rollup_flr with HIP events between its phases: ms[0] the key build, ms[1 .. 9] the nine sort passes (histogram, scan,
 * scatter each), ms[10] the scans over the sorted order and the records, ms[11] the whole stage.  Synchronises hip_stream
 * before it returns.  For scripts/flr_probe.py.  No reference counterpart. */
#define PYA_FLR_PHASES 11
int pya_debug_rollup_flr_timed(pya_handle *h, const pya_site_rollup *d_table, uint64_t n_slots, const uint8_t *d_cls, uint32_t flags,
                               void *hip_stream, void *d_work, uint64_t work_bytes, pya_site_flr *d_out, uint32_t *d_order,
                               uint32_t *d_n_ranked, float ms[PYA_FLR_PHASES + 1]);

/* HIP events between the phases of the peptidoform stage (pya_plan_peptidoforms, pya_peptidoform_reduce and the batch calls
 * of this handle) while `on`: pya_debug_last_peptidoform_ms waits for the last such call and gives ms[0] the entries, ms[1]
 * the thirteen sort passes, ms[2] the segmented reduction, ms[3] the finish, ms[4] the whole stage.  PYA_ERR_STATE when no
 * call with entries was timed.  For scripts/peptidoforms_probe.py.  No reference counterpart. */
#define PYA_PFORM_PHASES 4
int pya_debug_peptidoform_timing(pya_handle *h, int on);
int pya_debug_last_peptidoform_ms(pya_handle *h, float ms[PYA_PFORM_PHASES + 1]);

/* The signature list of PSM `psm` of the handle's retained batch (the last PYA_FLAG_KEEP call): the sig bits of its site
 * assignments in the order every kernel scores them in and the probability stage sums them in (pya_get_pep_scores* returns
 * the reference's sorted order instead).  *n = their number; sig_bits may be NULL with cap 0 to ask.  No reference
 * counterpart. */
int pya_debug_signature_list(pya_handle *h, uint64_t psm, uint64_t *sig_bits, uint64_t cap, uint64_t *n);

/* The retained-peak table the binning kernels left in a plan's workspace for entry `index`, copied to the host: mz[i], rank[i]
 * = (float m/z, rank in its window) of table entry i, in table order (m/z ascending).  index = the PSM number, or the SPECTRUM
 * number for a plan with shared spectra (every spectrum has one table).  *n = the entry count the kernel stored (the +inf
 * entry padded behind an odd count is not part of it); *status = the status word beside it as the run left it, a PYA_ST_* code
 * of csrc/common.h (0 ok, 1 no windows, 2 too many windows -- the values of PYA_PSM_NO_WINDOWS / PYA_PSM_TOO_MANY_WINDOWS;
 * a shared plan's word is the spectrum's, written by the binning alone, a private PSM's may carry a later stage's code
 * instead).  Nothing of a plan's arena overlays the table after the binning (host_plan.cpp: layout_and_upload gives every
 * buffer its own range; the retained records and pya_calculate_ambiguity read the table later), so it is what the scoring
 * kernels read.  Waits for the stream of the plan's last run before it copies.
 * PYA_ERR_ARG: no plan or a plan that has not run, index out of range, an entry that was never binned (a PSM the pre-pass of
 * PYA_FLAG_SKIP_INVALID set aside: *status has its code; a shared spectrum without a scored PSM), n > cap (then *n says how
 * many; mz and rank may be NULL with cap 0 to ask).  TEST-ONLY; no reference counterpart (BinnedSpectra keeps its windows
 * private too: oracle/oracle_abi.h orc_binned is the checker's read-back). */
int pya_debug_plan_retained_table(pya_plan *p, uint64_t index, float *mz, uint32_t *rank, uint64_t cap, uint64_t *n, int32_t *status);
/* ... of the handle's retained plan (the last PYA_FLAG_KEEP batch, or the view pya_rescore_last_keep made of the last
 * pya_score_one PSM); a handle that retains nothing: the workspace of the last pya_score_one call, index 0 (the one-PSM kernel
 * stores its table whether the call retains or not, and also when the call failed with a binning status). */
int pya_debug_retained_table(pya_handle *h, uint64_t index, float *mz, uint32_t *rank, uint64_t cap, uint64_t *n, int32_t *status);

#ifdef __cplusplus
}
#endif
#endif
