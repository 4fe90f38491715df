/* host_internal.h -- host side of libpyascore_hip.so: the C ABI of include/pyascore_hip.h.
 *
 * Host work is limited to what is not data-parallel arithmetic over spectra:
 *   - validating PSMs and counting modifiable residues (one pass over the peptide letters),
 *   - per-shape signature order tables (the iteration order of the reference's
 *     std::unordered_map<long,...>, cpp/Ascore.cpp:54,114-120 -- reproduced with the same
 *     libstdc++ container, it depends only on (n_sites, n_mods, direction)),
 *   - the binomial score table (score_table.cpp),
 *   - workspace sizing, bucketing PSMs by C(n,k) so each launch gets the LDS it needs,
 *   - kernel launches and copies.
 * There is no CPU scoring path here: without a HIP device every entry point fails.
 *
 * This header holds what the host files share (handle, plan, buckets, device buffers, the kernels' launchers);
 * the code is in host_abi.cpp (handles, settings, strings, retained records), host_tables.cpp (DevConfig, score table,
 * order tables, environment switches), host_plan.cpp (creating a plan: the pre-pass in phases, the arena), host_run.cpp
 * (running it: the launch families, the timing ring), host_batch.cpp (pya_score_batch: chunking and pipelining) and
 * host_one.cpp (pya_score_one).
 */
#ifndef PYA_HOST_INTERNAL_H
#define PYA_HOST_INTERNAL_H
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <condition_variable>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/pyascore_hip.h"
#include "common.h"

void pya_score_table_extend(float mz_error, uint32_t n_top, uint32_t n_to, std::vector<float> &lut,
                            std::vector<uint32_t> &off);
extern "C" {
size_t pya_bin_lds_bytes(uint32_t cap);
size_t pya_score_lds_bytes(uint32_t cap, uint32_t prefix, uint32_t with_nl, uint32_t compact);
size_t pya_localize_lds_bytes(uint32_t push_cap, uint32_t n_cap, uint32_t pos_cap, uint32_t pool_cap, uint32_t sb);
/* (the binning launchers: `types` = PYA_SPEC_*, the element types of b->mz and b->inten) */
int pya_launch_bin(const BatchDev *b, const uint32_t *d_ids, uint32_t n_ids, uint32_t cap, uint32_t types, hipStream_t stream);
int pya_launch_bin_select(const BatchDev *b, const uint32_t *d_ids, uint32_t n_ids, uint32_t scap, uint32_t types, hipStream_t stream);
size_t pya_bin_select_lds_bytes(uint32_t scap);
int pya_launch_bin_exact(const BatchDev *b, uint32_t n_total, uint32_t cap, uint32_t types, hipStream_t stream);
int pya_launch_fan_out(const uint32_t *d_spec_of, const uint32_t *d_spec_ret_n, const int32_t *d_spec_status, uint32_t *d_ret_n,
                       int32_t *d_status, uint32_t n_psm, hipStream_t stream);
int pya_launch_score(const BatchDev *b, const uint32_t *d_ids, uint32_t n_ids, uint32_t cap, uint32_t prefix,
                     uint32_t with_nl, uint32_t compact, uint32_t node_cap, uint32_t node_cols, uint32_t node_words,
                     uint32_t res_cap, uint32_t nl_cap, hipStream_t stream);
size_t pya_score_node_lds_bytes(uint32_t cap, uint32_t with_nl, uint32_t node_cap, uint32_t node_cols, uint32_t node_words,
                                uint32_t res_cap, uint32_t nl_cap);
int pya_launch_localize(const BatchDev *b, const uint32_t *d_ids, uint32_t n_ids, uint32_t push_cap,
                        uint32_t n_cap, uint32_t pos_cap, uint32_t pool_cap, uint32_t sb, uint32_t gtp,
                        uint32_t plain, uint32_t sort_room, hipStream_t stream);
size_t pya_tiny_lds_bytes(uint32_t cap, uint32_t prefix, uint32_t with_nl, uint32_t compact, uint32_t push_cap,
                          uint32_t n_cap, uint32_t pos_cap, uint32_t pool_cap, uint32_t sb);
int pya_launch_tiny(const BatchDev *b, uint32_t n_psm, uint32_t cap, uint32_t prefix, uint32_t with_nl,
                    uint32_t compact, uint32_t push_cap, uint32_t n_cap, uint32_t pos_cap, uint32_t pool_cap,
                    uint32_t sb, uint32_t gtp, hipStream_t stream);
size_t pya_one_lds_bytes(uint32_t cap, uint32_t prefix, uint32_t with_nl, uint32_t compact, uint32_t push_cap, uint32_t n_cap,
                         uint32_t pos_cap, uint32_t pool_cap, uint32_t sb, uint32_t use_fused, uint32_t f_n_cap, uint32_t f_stride,
                         uint32_t f_ent_cap, uint32_t f_push_cap, uint32_t multi_z);
int pya_launch_one(const BatchDev *b, const OneMeta *m, uint32_t cap, uint32_t prefix, uint32_t with_nl, uint32_t compact,
                   uint32_t push_cap, uint32_t n_cap, uint32_t pos_cap, uint32_t pool_cap, uint32_t sb, uint32_t gtp,
                   uint32_t use_fused, uint32_t f_n_cap, uint32_t f_stride, uint32_t f_ent_cap, uint32_t f_push_cap,
                   uint32_t multi_z, int32_t *host_status, uint32_t *host_flag, hipStream_t stream);
int pya_launch_ambiguity(const BatchDev *b, uint32_t psm, uint32_t peak_cap, uint32_t list_cap,
                         uint64_t ref_bits, uint64_t oth_bits, const float *d_scores, float ref_ws,
                         float oth_ws, float *d_out, hipStream_t stream);
int pya_launch_debug_sort(const float *d_keys, uint32_t n, uint32_t *d_perm, hipStream_t stream);
int pya_launch_pack_records(const float *best_score, const int32_t *n_sig, const uint64_t *best_sig, const float *ascores,
                            const uint64_t *alt_mask, uint32_t k, uint32_t res_k, uint64_t n_psm, int32_t *out, hipStream_t stream);
int pya_launch_debug_wave_ops(const int32_t *d_in, int32_t *d_out, hipStream_t stream);
/* (debug_ops.hip: the test-only kernels behind include/pyascore_debug.h's pya_debug_lookup .. pya_debug_ts_scan) */
int pya_launch_debug_lookup(const void *d_table, uint32_t n, const DevConfig *d_cfg, uint16_t *d_grid, uint32_t *d_cells, const float *d_query,
                            uint32_t n_query, uint8_t *d_out, hipStream_t stream);
int pya_launch_debug_lane_ops(uint32_t op, const uint64_t *d_a, const uint64_t *d_b, uint64_t n, uint64_t *d_out, hipStream_t stream);
int pya_launch_debug_wave64(uint32_t op, const uint64_t *d_in, uint64_t *d_out, hipStream_t stream);
int pya_launch_debug_block_scan(uint32_t policy, const uint32_t *d_in, uint32_t *d_out, hipStream_t stream);
uint64_t pya_ts_scan_entries(uint64_t n);
int pya_launch_debug_ts_scan(uint32_t policy, uint32_t *d_data, uint64_t n, hipStream_t stream);
int pya_launch_debug_ion_wave_scan(const uint64_t *d_in, uint64_t *d_out, hipStream_t stream);   /* (ions.hip) */
size_t pya_score_big_lds_bytes(uint32_t cap, uint32_t pos_cap, uint32_t kc);
int pya_launch_score_big(const BatchDev *b, const uint32_t *d_ids, uint32_t n_ids, uint32_t cap, uint32_t pos_cap, uint32_t kc,
                         uint32_t inline_on, hipStream_t stream);
size_t pya_localize_recount_lds_bytes(uint32_t cap, uint32_t push_cap, uint32_t pos_cap, uint32_t pool_cap, uint32_t sb);
size_t pya_localize_hash_lds_bytes(uint32_t push_cap, uint32_t n_cap, uint32_t pos_cap, uint32_t sb, uint32_t vc, uint32_t hs,
                                   uint32_t pp, uint32_t max_k, uint32_t n_nl);
int pya_launch_localize_hash(const BatchDev *b, const uint32_t *d_ids, uint32_t n_ids, uint32_t push_cap, uint32_t n_cap,
                             uint32_t pos_cap, uint32_t pool_cap, uint32_t sb, uint32_t gtp, uint32_t vc, uint32_t hs, uint32_t pp,
                             uint32_t n_nl, hipStream_t stream);
int pya_launch_localize_recount(const BatchDev *b, const uint32_t *d_ids, uint32_t n_ids, uint32_t cap, uint32_t push_cap,
                                uint32_t pos_cap, uint32_t pool_cap, uint32_t sb, uint32_t gtp, uint32_t *d_redo_count, uint32_t *d_redo_ids, hipStream_t stream);
int pya_launch_score_big_list(const BatchDev *b, const uint32_t *d_count, const uint32_t *d_ids, uint32_t n_max, uint32_t cap,
                              uint32_t pos_cap, uint32_t kc, hipStream_t stream);
uint32_t pya_big_inline_max(void);
size_t pya_fused_lds_bytes(uint32_t cap, uint32_t n_cap, uint32_t stride, uint32_t pos_cap, uint32_t ent_cap, uint32_t push_cap,
                           uint32_t both, uint32_t multi_z);
int pya_launch_fused(const BatchDev *b, const uint32_t *d_ids, uint32_t n_ids, uint32_t cap, uint32_t n_cap,
                     uint32_t stride, uint32_t pos_cap, uint32_t ent_cap, uint32_t push_cap, uint32_t both,
                     uint32_t multi_z, uint32_t *d_redo_count, uint32_t *d_redo_ids, hipStream_t stream);
size_t pya_score_cnt_lds_bytes(uint32_t cap, uint32_t pos_cap, uint32_t kc, uint32_t k_cap, uint32_t n_cap);
int pya_launch_score_cnt(const BatchDev *b, const uint32_t *d_ids, uint32_t n_ids, uint32_t cap, uint32_t pos_cap, uint32_t kc, uint32_t k_cap,
                         uint32_t n_cap, hipStream_t stream);
size_t pya_score_cntg_lds_bytes(uint32_t cap, uint32_t pos_cap, uint32_t k_cap, uint32_t n_cap, uint32_t nl_cap);
int pya_launch_score_cntg(const BatchDev *b, const uint32_t *d_ids, uint32_t n_ids, uint32_t cap, uint32_t pos_cap, uint32_t k_cap, uint32_t n_cap,
                          uint32_t nl_cap, hipStream_t stream);
size_t pya_bin_global_scratch_bytes(uint32_t cap);
int pya_launch_bin_global(const BatchDev *b, const uint32_t *d_ids, uint32_t n_ids, unsigned char *d_scratch, uint64_t stride,
                          uint32_t cap, uint32_t types, hipStream_t stream);
size_t pya_general_lds_bytes(uint32_t l_cap, uint32_t list_cap);
size_t pya_general_scratch_bytes(uint32_t n_cap, uint32_t push_cap);
int pya_launch_general(const BatchDev *b, const uint32_t *d_ids, uint32_t n_ids, unsigned char *d_scratch, const uint64_t *d_scratch_off,
                       uint32_t l_cap, uint32_t list_cap, hipStream_t stream);
int pya_launch_general_ambiguity(const BatchDev *b, uint32_t psm, uint32_t l_cap, uint32_t list_cap, uint64_t ref_bits,
                                 uint64_t oth_bits, const float *d_scores, uint32_t n_scores, float ref_ws, float oth_ws,
                                 float *d_out, hipStream_t stream);
size_t pya_evidence_lds_bytes(uint32_t l_cap, uint32_t list_cap);
int pya_launch_evidence(const BatchDev *b, const uint32_t *d_ids, uint32_t n_ids, void *d_out, uint32_t l_cap, uint32_t list_cap,
                        hipStream_t stream);
size_t pya_ions_lds_bytes(uint32_t l_cap, uint32_t list_cap);
uint32_t pya_ions_scan_tiles(uint32_t n);
int pya_launch_ions(const BatchDev *b, const uint32_t *d_ids, uint32_t n_ids, const void *d_evid, int64_t *d_off, void *d_out, uint64_t cap,
                    uint32_t *d_over, uint32_t l_cap, uint32_t list_cap, hipStream_t stream);
int pya_launch_ions_scan(int64_t *d_off, uint32_t n, uint64_t *d_tiles, hipStream_t stream);
size_t pya_named_lds_bytes(uint32_t l_cap, uint32_t list_cap);
int pya_launch_named(const BatchDev *b, const uint32_t *d_ids, uint32_t n_ids, const int64_t *d_q_off, const uint64_t *d_q_bits,
                     uint64_t n_q, void *d_out, int32_t *d_counts, float *d_scores, uint32_t *d_over, uint32_t l_cap,
                     uint32_t list_cap, hipStream_t stream);
size_t pya_sites_lds_bytes(uint32_t l_cap, uint32_t list_cap);
int pya_launch_sites(const BatchDev *b, const uint32_t *d_ids, uint32_t n_ids, const int64_t *d_site_off, uint64_t n_out,
                     uint32_t sig_cap, void *d_out, uint32_t l_cap, hipStream_t stream);
size_t pya_probs_lds_bytes(uint32_t l_cap, const PcCaps *caps, uint32_t sw);
size_t pya_probs_cnt_bytes(const PcCaps *caps);
int pya_launch_probs(const BatchDev *b, const uint32_t *d_ids, uint32_t n_ids, const int64_t *d_site_off, uint64_t n_out,
                     uint32_t sig_cap, void *d_out, void *d_psms, uint32_t l_cap, const PcCaps *caps, uint32_t sw, hipStream_t stream);
size_t pya_ranked_lds_bytes(uint32_t l_cap, const PcCaps *caps, uint32_t sw);
int pya_launch_ranked(const BatchDev *b, const uint32_t *d_ids, uint32_t n_ids, const int64_t *d_site_off, uint32_t top_k,
                      uint32_t sig_cap, void *d_out, uint32_t l_cap, const PcCaps *caps, uint32_t sw, hipStream_t stream);
int pya_launch_rollup_clear(void *d_table, uint64_t n_slots, hipStream_t stream);
int pya_launch_rollup(const int64_t *d_site_off, uint64_t n_psm, uint64_t n_rec, const void *d_site_probs, const void *d_psm_probs,
                      const int32_t *d_slot, uint64_t n_slots, double threshold, const uint32_t *d_psm_id, uint32_t psm_base,
                      const uint64_t *best_sig, const float *ascores, uint32_t max_k, void *d_table, uint32_t *d_over, uint32_t grid[2],
                      hipStream_t stream);
int pya_launch_site_quant(const int64_t *d_site_off, uint64_t n_psm, uint64_t n_rec, const void *d_site_probs, const void *d_psm_probs,
                          const int32_t *d_slot, uint64_t n_slots, const double *d_values, uint64_t n_rows, const int32_t *d_row, uint32_t row_base,
                          const pya_site_quant_params *prm, double scale, const uint64_t *best_sig, void *d_head, void *d_cell, uint32_t *d_over,
                          hipStream_t stream);
int pya_launch_marker_values(const pya_marker *d_markers, uint64_t n_spectra, uint32_t n_targets, uint64_t mask, double *d_values,
                             hipStream_t stream);
size_t pya_mz_profile_lds_bytes(uint32_t l_cap);
int pya_launch_mz_profile(const BatchDev *b, const uint32_t *d_ids, uint32_t n_ids, const int32_t *d_run, uint64_t n_slots,
                          const pya_mz_profile_params *prm, void *d_table, uint32_t *d_over, uint32_t l_cap, hipStream_t stream);
size_t pya_coverage_lds_bytes(uint32_t l_cap, uint32_t peak_cap);
int pya_launch_coverage(const BatchDev *b, const uint32_t *d_ids, uint32_t n_ids, const uint32_t *d_spec_of, uint32_t types, void *d_out,
                        uint32_t l_cap, uint32_t peak_cap, hipStream_t stream);
int pya_launch_mz_fit(const void *d_table, uint64_t n_slots, double inv_ppm, uint32_t min_ions, void *d_cal, hipStream_t stream);
int pya_launch_mz_apply(const void *d_mz, uint32_t mz_type, const int64_t *d_peak_off, uint64_t n_spectra, const int32_t *d_run,
                        const void *d_cal, uint64_t n_slots, double inv_band, void *d_out, uint32_t *d_over, hipStream_t stream);
uint64_t pya_flr_layout_bytes(uint64_t n_slots);
int pya_launch_flr(const void *d_table, uint64_t n_slots, const uint8_t *d_cls, uint32_t reported_only, void *d_work, void *d_out,
                   uint32_t *d_order, uint32_t *d_n_ranked, hipEvent_t *phase, hipStream_t stream);
uint64_t pya_pform_layout_bytes(uint64_t n_entries);
int pya_launch_pform(const int64_t *d_site_off, uint64_t n_psm, const void *d_site_probs, const void *d_psm_probs, const int32_t *d_group,
                     double threshold, const uint32_t *d_psm_id, uint32_t psm_base, const uint64_t *best_sig, const float *ascores, uint32_t max_k,
                     const void *d_src0, uint64_t n0, const void *d_src1, uint64_t n1, void *d_work, void *d_out, uint64_t cap, uint32_t *d_n,
                     hipEvent_t *phase, hipStream_t stream);
int pya_launch_pform_quant(const int64_t *d_site_off, uint64_t n_psm, const void *d_site_probs, const void *d_psm_probs, const int32_t *d_group,
                           const uint64_t *best_sig, uint32_t max_k, const void *d_src0, const void *d_head0, const void *d_cell0, uint64_t n0,
                           const void *d_src1, const void *d_head1, const void *d_cell1, uint64_t n1, const double *d_values, uint64_t n_rows,
                           const int32_t *d_row, uint32_t row_base, const pya_site_quant_params *prm, double scale, const void *d_list,
                           const uint32_t *d_n, void *d_head, void *d_cell, uint64_t cap, uint32_t *d_over, hipStream_t stream);
int pya_launch_localize_redo(const BatchDev *b, const uint32_t *d_count, const uint32_t *d_ids, uint32_t n_max,
                             uint32_t push_cap, uint32_t n_cap, uint32_t pos_cap, uint32_t pool_cap, uint32_t sb,
                             uint32_t gtp, hipStream_t stream);
}


/* (shared by the host_*.cpp files; internal linkage where it is data, inline where it is code) */

const size_t kMaxLds = 160 * 1024;
const uint32_t kBucketLimits[] = {64, 512, 4096, PYA_FAST_SIGNATURES};
const int kNumBuckets = 4;
const size_t kRedoHead = 64;            /* words in front of the ids of a hand-over list (d_redo .. d_redo5): its counts */
const size_t kStageLimit = 1u << 20;   /* batches whose transfers are smaller than this go through one staged copy */

template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    bool owned = true;
    DevBuf() {}
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p && owned) (void)hipFree(p);
        p = nullptr;
        n = 0;
        owned = true;
    }
    /* points into somebody else's allocation (the plan's arena) */
    void adopt(void *ptr, size_t count) {
        release();
        p = (T *)ptr;
        n = count;
        owned = false;
    }
    hipError_t fill(const T *src, hipStream_t s = nullptr) {
        if (n == 0 || !src) return hipSuccess;
        return hipMemcpyAsync(p, src, n * sizeof(T), hipMemcpyHostToDevice, s);
    }
    hipError_t alloc(size_t count) {
        release();
        n = count;
        if (count == 0) count = 1;
        return hipMalloc((void **)&p, count * sizeof(T));
    }
    hipError_t upload(const T *src, size_t count, hipStream_t s = nullptr) {
        hipError_t e = alloc(count);
        if (e != hipSuccess || count == 0) return e;
        return hipMemcpyAsync(p, src, count * sizeof(T), hipMemcpyHostToDevice, s);
    }
    size_t bytes() const { return n * sizeof(T); }
    /* moves the allocation of `other` here if it is big enough; returns whether it did */
    bool take_if_fits(DevBuf &other, size_t count) {
        if (!other.p || !other.owned || other.n < count) return false;
        release();
        p = other.p;
        n = other.n;
        other.p = nullptr;
        other.n = 0;
        return true;
    }
    void give_to(DevBuf &other) {
        if (!p || !owned) return;
        if (other.p && other.n >= n) return;          /* keep the larger one */
        other.release();
        other.p = p;
        other.n = n;
        p = nullptr;
        n = 0;
    }
};

inline uint64_t binom(uint32_t n, uint32_t k) {
    if (k > n) return 0;
    if (k > n - k) k = n - k;
    unsigned __int128 r = 1;
    for (uint32_t i = 1; i <= k; i++) {
        r = r * (n - k + i) / i;
        if (r > (unsigned __int128)1 << 62) return ~0ull;
    }
    return (uint64_t)r;
}

uint32_t next_pow2(uint32_t v);              /* (host_tables.cpp) */

inline bool is_forward(char t) { return t == 'b' || t == 'c'; }
inline bool is_backward(char t) { return t == 'y' || t == 'z' || t == 'Z'; }

inline float std_residue_mass(char c) {                       /* Types.h:7-30 */
    switch (c) {
        case 'G': return 57.02146f;   case 'A': return 71.03711f;   case 'S': return 87.03203f;
        case 'P': return 97.05276f;   case 'V': return 99.06841f;   case 'T': return 101.04768f;
        case 'C': return 103.00919f;  case 'L': return 113.08406f;  case 'I': return 113.08406f;
        case 'N': return 114.04293f;  case 'D': return 115.02694f;  case 'Q': return 128.05858f;
        case 'K': return 128.09496f;  case 'E': return 129.04259f;  case 'M': return 131.04049f;
        case 'H': return 137.05891f;  case 'F': return 147.06841f;  case 'U': return 150.95364f;
        case 'R': return 156.10111f;  case 'Y': return 163.06333f;  case 'W': return 186.07931f;
        case 'O': return 237.14773f;
    }
    return 0.f;
}


/* Debug switches (route selection for the tests, diagnostics, A/B experiments): per handle, set through
 * pya_set_debug (include/pyascore_debug.h) -- NOT from the environment, which reaches the library through four
 * variables only (host_tables.cpp:read_env: PYA_WORKSPACE_MB, PYA_CHUNK_MB, PYA_HOST_TIMING, PYA_STAMPS; read in
 * pya_create, re-read by pya_reload_env).  Defaults are the production behaviour. */
struct Knobs {
    bool no_plain = false, no_fused = false, no_big = false, no_tiny = false, no_prefix = false, no_chunks = false;
    bool no_upload_thread = false, one_peak_class = false, peak_classes = false, one_lds_class = false;
    bool host_timing = false, stamps = false, sort_room = false, no_big_inline = false;
    bool no_loc_hash = false, no_nodes = false, no_cnt = false, no_prob_cnt = false;
    bool no_fork = false;                       /* r06: the fused family on the plan's stream behind the scoring kernels instead of beside them */
    bool slow_null_stream = false;              /* host_one.cpp: widens the window of a (fixed) workspace race for its regression test */
    uint32_t debug = 0;
    int64_t plain_min = 512, big_min_n = 1024, tiny_max = 64;
    int64_t bin_select_min = 640;               /* peak classes above this many peaks are binned by selection (bin_select.hip.h); tests: 0 = all, huge = none */
    int64_t bin_select_scap = 768;              /* survivor slots per spectrum there */
    uint32_t sort_room_max = 1024;
    int sb = -1, gtp = -1, hash_pp = -1;        /* < 0: the built-in rule */
    int node_cap = -1;                          /* >= 0: room for that many shared nodes per direction (tests: small values force the walkers) */
    double chunk_mb = 0.;                       /* 0: the default chunk size */
    int64_t workspace_mb = 0;                   /* 0: the default budget */
};

void read_knobs(Knobs &k);
bool set_knob(Knobs &k, const char *key, const char *value);

struct pya_handle {
    Knobs kn;
    int device = 0;
    hipStream_t side_stream = nullptr;        /* r06: where the plans' forked fused families run (pya_plan::fork) */
    float bin_size = 100.f, mod_mass = 0.f, mz_error = 0.5f;
    uint32_t n_top = PYA_NTOP;                /* 10: the fast kernels; 11..16: every PSM through the general kernel */
    uint32_t rec_words() const { return (n_top + 1u) / 2u + 1u; }   /* count record: n_top 16-bit counts + the fragment total */
    std::string mod_group, fragment_types;
    std::map<char, float> nl;                 /* letter -> neutral loss (ModifiedPeptide.h:19) */
    DevConfig cfg;
    bool cfg_dirty = true;
    DevBuf<DevConfig> d_cfg;
    /* The settings generation: bumped by everything that changes what a plan was sized under.  A plan records the value it was
     * made under (pya_plan::settings_gen) and every entry point that launches over a plan refuses with PYA_ERR_STATE when the
     * two differ (plan_settings_stale, below).
     *   bumps:       pya_add_neutral_loss -- a plan's routes (plain_types -> fused / count-node / lean lists), its caps (per_type,
     *                pair_cap, list_cap = f(n_uniq)), hash_ok(max_k, n_nl) and its score-table need were fixed under the old
     *                DevConfig, while the launch sizing of a run reads h->cfg as it is then.  Every call bumps, a repeated
     *                identical one too: the setter does not compare.
     *   does not:    pya_set_debug / pya_reload_env.  The switches a plan is BUILT under are copied into it or spent when it
     *                is made (PYA_SB, PYA_GTP, PYA_HASH_PP: Bucket::take_knobs; PYA_NO_FORK: pya_plan::fork; PYA_STAMPS,
     *                PYA_DEBUG's kernel bits: BatchDev; PYA_NO_PLAIN, PYA_NO_FUSED, PYA_NO_BIG, PYA_NO_BIG_INLINE, PYA_PLAIN_MIN,
     *                PYA_BIG_MIN_N, PYA_ONE_PEAK_CLASS, PYA_PEAK_CLASSES, PYA_ONE_LDS_CLASS: the id lists).  The ones a RUN
     *                reads (PYA_NO_CNT, PYA_DEBUG bit 0x8000, PYA_NO_NODES, PYA_NODE_CAP, PYA_NO_PREFIX, PYA_NO_TINY,
     *                PYA_TINY_MAX, PYA_BIN_SELECT_MIN, PYA_BIN_SELECT_SCAP, PYA_SORT_ROOM, PYA_SORT_ROOM_MAX, PYA_NO_LOC_HASH,
     *                PYA_NO_PROB_CNT) each choose between kernels that the same call sizes, LDS included, from the plan's bucket
     *                caps, which no switch enters; nothing of the arena depends on them.  PYA_HOST_TIMING prints.
     *                PYA_SLOW_NULL_STREAM, PYA_NO_UPLOAD_THREAD, PYA_NO_CHUNKS, PYA_CHUNK_MB, PYA_WORKSPACE_MB and
     *                pya_set_workspace_budget, pya_set_ranked_k, pya_set_site_sig_cap are read by pya_score_one / the batch
     *                calls, which make their own plans per call. */
    uint64_t settings_gen = 0;
    uint64_t cfg_uploads = 0;                 /* uploads of d_cfg so far (pya_debug_table_sizes) */

    std::vector<float> lut;
    std::vector<uint32_t> lut_off;
    uint32_t lut_uploaded_n = 0;              /* rows [0, lut_uploaded_n) are on the device */
    DevBuf<float> d_lut;
    DevBuf<uint32_t> d_lut_off;

    std::map<uint32_t, uint32_t> shape_off;   /* (n << 8 | k) -> offset into order_tab */
    std::map<uint32_t, uint32_t> shape_cols;  /* ... -> histogram columns its shared-node route needs (shapes of <= 64 signatures) */
    std::vector<uint64_t> order_tab;
    std::vector<uint32_t> inv_tab;            /* same offsets: combination rank -> index in order_tab */
    size_t order_uploaded = 0;
    DevBuf<uint64_t> d_order;
    DevBuf<uint32_t> d_inv, d_binom;

    /* device allocations recycled between pya_score_batch calls (hipMalloc/hipFree of a few
     * hundred MB cost milliseconds) */
    DevBuf<unsigned char> spare_arena, spare_arena2;   /* two: chunked calls keep two plans alive */
    void *pinned_stage[2] = {nullptr, nullptr};        /* chunked calls: results of chunk c land in slot c % 2 */
    size_t pinned_bytes[2] = {0, 0};
    /* what the last pya_plan_probs of a plan of this handle launched, per launch (the PSMs inside the fast limits, the general
     * list): the front ends carved (probs.hip: PB_CNT 1 | PB_GEN 2; 0: no launch) and the LDS bytes (pya_debug_last_probs_launch) */
    uint32_t last_probs_sw[2] = {0u, 0u};
    uint64_t last_probs_lds[2] = {0u, 0u};
    uint32_t last_ranked_sw[2] = {0u, 0u};     /* the same for the last pya_plan_ranked (pya_debug_last_ranked_launch) */
    uint64_t last_ranked_lds[2] = {0u, 0u};
    uint32_t last_rollup_grid[2] = {0u, 0u};   /* the blocks of the last pya_plan_rollup's launches, and the records it walked */
    uint64_t last_rollup_records = 0;          /* (pya_debug_last_rollup_launch) */
    uint64_t last_chunks = 0;                  /* plans the last pya_score_batch call was cut into (pya_debug_last_chunks) */
    DevBuf<unsigned char> io_buf;              /* spectra of big pya_score_batch calls (uploaded by a helper thread) */
    DevBuf<unsigned char> io_ring[2];          /* chunked calls: spectra of chunk c in slot c % 2 */
    hipStream_t copy_stream = nullptr, run_stream = nullptr;   /* chunked calls: uploads / kernels + results */
    size_t ws_budget = 0;                      /* device bytes one pya_score_batch call may hold (0 = default) */
    std::vector<unsigned char> stage;          /* host staging of small batches: one copy each way */

    /* pya_score_one: persistent pinned (device-mapped, coherent) host block + one PSM's device workspace */
    struct One {
        unsigned char *host = nullptr, *host_dev = nullptr;    /* the same block as the host / the device sees it */
        DevBuf<unsigned char> ws, probe;          /* (probe: the PYA_SLOW_NULL_STREAM test switch's 256 MB) */
        uint32_t sig_cap = 0;                      /* signatures the workspace has room for */
        uint32_t seq = 0;
        hipStream_t stream = nullptr;
        BatchDev dev;
        OneMeta meta;                              /* of the last call (pya_rescore_last_keep replays it) */
        bool have_last = false, last_keep = false;
        uint32_t last_max_k = 1;
        pya_plan *view = nullptr;                  /* what pya_get_pep_scores / pya_calculate_ambiguity read */
        double t_sum[5] = {0, 0, 0, 0, 0};         /* seconds in checks + tables, copy in, launch, wait, copy out (pya_one_times) */
        double t_dev[4] = {0, 0, 0, 0};            /* seconds inside the kernel: scalars, binning, scoring, rest */
        double t_cycles = 0;                       /* its shader clock cycles */
        uint64_t t_calls = 0;
    } one;

    std::string err;
    int64_t err_index = -1;
    std::vector<int32_t> last_status;         /* per-PSM codes of the last pya_score_batch */
    /* PYA_FLAG_EVIDENCE: the records of the last pya_score_batch, pinned so that a chunk's rows come back asynchronously
     * behind its results (pya_last_batch_evidence copies them out) */
    pya_evidence *evid_host = nullptr;
    size_t evid_cap = 0;                      /* records the block has room for */
    uint64_t evid_n = 0;                      /* PSMs of the batch they belong to */
    uint32_t evid_k = 0;                      /* its row stride */
    bool evid_valid = false;                  /* the last batch was scored with the flag */
    /* PYA_FLAG_IONS: the ion records of the last pya_score_batch in PSM order (pinned: a chunk's records come back
     * asynchronously behind its offsets) and the offsets of every PSM into them (pya_last_batch_ions copies them out) */
    pya_ion *ions_host = nullptr;
    size_t ions_cap = 0;                      /* records the block has room for */
    std::vector<int64_t> ions_off;            /* [n_psm + 1] of the batch they belong to */
    bool ions_valid = false;                  /* the last batch was scored with the flag */
    /* pya_score_batch_named: the records of the call's queries, pinned so that a chunk's slice comes back asynchronously
     * behind its results: [n_q] pya_named, then [n_q * n_top] counts and [n_q * n_top] scores where asked for */
    unsigned char *named_host = nullptr;
    size_t named_cap = 0;                     /* bytes of the block */
    /* PYA_FLAG_SITES: the site records of the last pya_score_batch in PSM order (pinned, sized before the first chunk from
     * the peptides' letters: a chunk's records come back asynchronously behind its results) and the offsets of every PSM
     * into them (pya_last_batch_sites copies them out); the cap on site assignments per PSM the stage is launched with */
    pya_site *sites_host = nullptr;
    size_t sites_cap = 0;                     /* records the block has room for */
    std::vector<int64_t> sites_off;           /* [n_psm + 1] of the batch they belong to */
    bool sites_valid = false;                 /* the last batch was scored with the flag */
    uint32_t site_sig_cap = PYA_FAST_SIGNATURES;
    /* PYA_FLAG_PROBS: the same for the probability records -- one pinned block, [probs_cap] pya_site_prob at the offsets of
     * the site table, then [probs_psm_cap] pya_psm_prob (zeroed: a PSM no plan reaches is PYA_SITE_NONE) */
    unsigned char *probs_host = nullptr;
    size_t probs_cap = 0, probs_psm_cap = 0;
    std::vector<int64_t> probs_off;
    bool probs_valid = false;
    pya_site_prob *probs_sites() const { return (pya_site_prob *)probs_host; }
    pya_psm_prob *probs_psms() const { return (pya_psm_prob *)(probs_host + probs_cap * sizeof(pya_site_prob)); }
    /* PYA_FLAG_RANKED: the ranked localisations of the last pya_score_batch, [ranked_n * ranked_batch_k] pya_ranked in PSM
     * order (pinned, zeroed: a PSM no plan reaches is PYA_RANK_NONE); ranked_k: the list length of the next batch call
     * (pya_set_ranked_k) */
    pya_ranked *ranked_host = nullptr;
    size_t ranked_cap = 0;                    /* records */
    uint64_t ranked_n = 0;
    uint32_t ranked_k = 5, ranked_batch_k = 0;
    bool ranked_valid = false;
    /* PYA_FLAG_ROLLUP: what pya_set_rollup lent for the next batch call (the caller's host arrays; the loan ends with that
     * call), the device table that lives for the call, the residue records the chunks so far had, whether the table has been
     * cleared, and the table of the last such call on the host */
    struct RollupLoan {
        const int32_t *slot = nullptr;
        const uint32_t *psm_id = nullptr;
        uint64_t n_records = 0, n_slots = 0;
        double threshold = 0.;
        bool set = false;
    } rollup_loan;
    DevBuf<pya_site_rollup> d_rollup;
    uint64_t rollup_seen = 0;
    bool rollup_cleared = false;
    std::vector<pya_site_rollup> rollup_host;
    bool rollup_valid = false;
    /* PYA_FLAG_PEPTIDOFORMS: what pya_set_peptidoforms lent for the next batch call, the two device lists of the call (a
     * chunk reads the one the chunk before wrote), the workspace and the two words of the stage, the length of the current
     * list as the host knows it, and the list of the last such call on the host */
    struct PformLoan {
        const int32_t *group = nullptr;
        const uint32_t *psm_id = nullptr;
        uint64_t n_psm = 0;
        double threshold = 0.;
        bool set = false;
    } pform_loan;
    DevBuf<pya_peptidoform> d_pform[2];
    DevBuf<unsigned char> d_pform_work;
    DevBuf<uint32_t> d_pform_n;
    uint32_t pform_n_host[2] = {0u, 0u};
    uint64_t pform_len = 0;
    int pform_cur = 0;
    std::vector<pya_peptidoform> pform_host;
    bool pform_valid = false;
    /* pya_debug_peptidoform_timing: events between the phases of the stage's next calls (include/pyascore_debug.h) */
    bool pform_timed = false, pform_ev_recorded = false;
    hipEvent_t pform_ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    /* PYA_FLAG_MZ_PROFILE: what pya_set_mz_profile lent for the next batch call, the device table that lives for the call
     * (zeroed when the call begins) and the table of the last such call on the host */
    struct MzpLoan {
        const int32_t *run = nullptr;
        uint64_t n_psm = 0, n_slots = 0;
        pya_mz_profile_params params = {};
        bool set = false;
    } mzp_loan;
    DevBuf<pya_mz_profile> d_mzp;
    std::vector<pya_mz_profile> mzp_host;
    bool mzp_valid = false;
    /* PYA_FLAG_QUANT: what pya_set_site_quant lent for the next batch call, the device copy of the matrix and the device
     * table that live for the call (the table zeroed when the call begins) and the table of the last such call on the host */
    struct QuantLoan {
        const double *values = nullptr;
        const int32_t *row = nullptr;
        uint64_t n_rows = 0, n_psm = 0;
        pya_site_quant_params params = {};
        bool set = false;
    } quant_loan;
    DevBuf<double> d_quant_values;
    DevBuf<pya_site_quant_head> d_quant_head;
    DevBuf<pya_site_quant> d_quant_cell;
    std::vector<pya_site_quant_head> quant_head_host;
    std::vector<pya_site_quant> quant_cell_host;
    uint32_t quant_channels = 0;
    bool quant_valid = false;
    /* PYA_FLAG_PFORM_QUANT: what pya_set_peptidoform_quant lent for the next batch call and, while such a call runs, the loan
     * as the call's own (pfq_active); the device copy of the matrix, the two device tables that travel with the two lists of
     * PYA_FLAG_PEPTIDOFORMS (d_pfq_head[i] / d_pfq_cell[i] is row-aligned with d_pform[i]) and the table of the last such
     * call on the host, row-aligned with pform_host */
    QuantLoan pfq_loan, pfq_call;
    bool pfq_active = false;
    DevBuf<double> d_pfq_values;
    DevBuf<pya_site_quant_head> d_pfq_head[2];
    DevBuf<pya_site_quant> d_pfq_cell[2];
    std::vector<pya_site_quant_head> pfq_head_host;
    std::vector<pya_site_quant> pfq_cell_host;
    uint32_t pfq_channels = 0;
    bool pfq_valid = false;
    /* PYA_FLAG_COVERAGE: the records of the last batch call, pinned like the evidence rows so that a chunk's records come
     * back asynchronously behind its results (pya_last_batch_coverage copies them out) */
    pya_coverage *cov_host = nullptr;
    size_t cov_cap = 0;                       /* records the block has room for */
    uint64_t cov_n = 0;                       /* PSMs of the batch they belong to */
    bool cov_valid = false;                   /* the last batch was scored with the flag */
    /* PYA_FLAG_RECALIBRATE: what pya_set_recalibration lent for the next batch call (the records are copied); the call's
     * device copy of the records and, per spectrum of the whole batch, the slot it is corrected with (-1: left alone) */
    struct RecalLoan {
        const int32_t *run = nullptr;
        uint64_t n_psm = 0, n_slots = 0;
        double inv_band = 0.;
        std::vector<pya_mz_calibration> cal;
        std::vector<int32_t> spec_slot;
        bool set = false;
    } recal_loan;
    DevBuf<pya_mz_calibration> d_recal;
    pya_plan *kept = nullptr;                 /* plan of the last PYA_FLAG_KEEP batch */
    /* settings only the general kernel takes: every PSM of the scorer goes there (cfg is rebuilt by every setter) */
    bool all_general() const { return n_top != PYA_NTOP || cfg.n_nl > PYA_FAST_NL; }

    int fail(int code, int64_t index, const char *fmt, ...) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        err = buf;
        err_index = index;
        return code;
    }
    int hip_fail(hipError_t e, const char *what) {
        return fail(PYA_ERR_HIP, -1, "HIP error in %s: %s", what, hipGetErrorString(e));
    }
    uint64_t binom_cache[64][64] = {{0}};     /* C(n,k), 0 = not computed yet (C >= 1 always) */
    uint32_t shape_cache[64][64];             /* offset of the shape's order table, ~0 = unknown */
    uint8_t in_group[256] = {0};              /* letter is in mod_group */
    uint8_t is_residue[256] = {0};            /* letter has a mass in Types.h */
    uint8_t letter_cls[256] = {0};            /* bit 0: residue of Types.h, bit 1: in mod_group */
    bool allow_n = false, allow_c = false;
    /* validity of the letters and the number of modifiable residues of one peptide (L >= 1) */
    bool scan_peptide(const uint8_t *s, int64_t L, uint32_t *n_sites) const {
        uint32_t all = 1, ns = 0;
        for (int64_t j = 0; j < L; j++) {
            const uint32_t c = letter_cls[s[j]];
            all &= c;
            ns += c >> 1;
        }
        if (allow_n && !(letter_cls[s[0]] >> 1)) ns++;
        if (allow_c && !(letter_cls[s[L - 1]] >> 1) && !(L == 1 && allow_n)) ns++;
        *n_sites = ns;
        return all & 1u;
    }
    void build_letter_tables() {
        std::memset(in_group, 0, sizeof in_group);
        std::memset(is_residue, 0, sizeof is_residue);
        for (unsigned char c : mod_group) in_group[c] = 1;
        for (int c = 'A'; c <= 'Z'; c++) is_residue[c] = std_residue_mass((char)c) != 0.f;
        for (int c = 0; c < 256; c++) letter_cls[c] = (uint8_t)((is_residue[c] ? 1 : 0) | (in_group[c] ? 2 : 0));
        allow_n = mod_group.find('n') != std::string::npos;
        allow_c = mod_group.find('c') != std::string::npos;
    }
    bool letter_modifiable(char c, size_t i, size_t L) const {
        return in_group[(unsigned char)c] || (i == 0 && allow_n) || (i + 1 == L && allow_c);
    }
};

#define HIPCHK(h, call)                                        \
    do {                                                       \
        hipError_t e_ = (call);                                \
        if (e_ != hipSuccess) return (h)->hip_fail(e_, #call); \
    } while (0)

/* The out-of-range report of a stage behind a run (device_common.hip.h: report_over): the two device words -- how many items
 * the last call wrote nothing of, and 0xffffffff - the smallest id among them --, the event behind that call's kernels, and
 * whether the last run has been asked at all.  Every call of the stage reports into the same two words, so a later call, on
 * whatever stream, waits for the earlier call's kernels before it clears them: the words are those of the LAST call. */
struct OverReport {
    DevBuf<uint32_t> d_over;
    hipEvent_t ev = nullptr;
    bool asked = false;
    ~OverReport() {
        if (ev) (void)hipEventDestroy(ev);
    }
    /* before the stage's launches on `st` */
    int begin(pya_handle *h, hipStream_t st) {
        if (!d_over.p) HIPCHK(h, d_over.alloc(2));
        if (!ev) HIPCHK(h, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        if (asked) HIPCHK(h, hipStreamWaitEvent(st, ev, 0));
        HIPCHK(h, hipMemsetAsync(d_over.p, 0, 2 * sizeof(uint32_t), st));
        return PYA_OK;
    }
    /* ... and behind them */
    int end(pya_handle *h, hipStream_t st) {
        HIPCHK(h, hipEventRecord(ev, st));
        asked = true;
        return PYA_OK;
    }
    /* waits for the last call's kernels; *count == 0: nothing was outside, or nothing was asked */
    int read(pya_handle *h, uint32_t *count, uint32_t *first_id) {
        uint32_t over[2] = {0u, 0u};
        if (asked) {
            HIPCHK(h, hipEventSynchronize(ev));
            HIPCHK(h, hipMemcpy(over, d_over.p, sizeof(over), hipMemcpyDeviceToHost));
        }
        *count = over[0];
        *first_id = 0xffffffffu - over[1];
        return PYA_OK;
    }
};
/* the stages of a plan that keep one (pya_plan::over), in the order pya_plan_check reports them */
enum { OVER_NAMED, OVER_ROLLUP, OVER_MZP, OVER_QUANT, OVER_PFQ, OVER_COUNT };

struct Bucket {
    std::vector<uint32_t> ids;          /* every PSM of the bucket (score_signatures launch), plain ones first */
    std::vector<uint32_t> general_ids;  /* filled while scanning; appended to ids afterwards */
    uint32_t n_plain = 0;               /* ids[0, n_plain): localised by the lean kernel instantiation */
    DevBuf<uint32_t> d_ids;
    uint32_t n_cap = 0, list_cap = 1, pos_cap = 1;
    /* Signatures localised together (winner included) -- LDS per wave decides the occupancy of
     * localize, the number of batches its instruction count. */
    /* the A/B overrides of the handle that owns the plan (PYA_SB, PYA_GTP, PYA_HASH_PP; < 0: the built-in rule), copied in by
     * take_knobs() when the plan is created: a second scorer in the process does not change them (r05 advisor) */
    int knob_sb = -1, knob_gtp = -1, knob_hash_pp = -1;
    void take_knobs(const Knobs &k) {
        knob_sb = k.sb;
        knob_gtp = k.gtp;
        knob_hash_pp = k.hash_pp;
    }
    uint32_t sb() const {
        if (knob_sb >= 0) return (uint32_t)knob_sb;                                /* A/B experiments (PYA_SB) */
        /* one batch holds the winner and one competitor per modified site.  (r01 gave long peptides -- large per-signature
         * tables -- two fewer to keep the LDS, hence the occupancy, up; r05 measured the opposite on cfg3, whose 40-mers then
         * needed two or three batches where one does: 0.465 -> 0.431 ms with the full batch.  These kernels are bound by the
         * instructions they issue, not by residency: DESIGN.md section 6.) */
        uint32_t v = k_max + 1;
        if (v < 2) v = 2;
        if (v > PYA_LOC_SB_MAX) v = PYA_LOC_SB_MAX;
        return v;
    }
    /* Ion types localised per pass (log2): as many as keep one signature's lists <= 256 floats,
     * so long multi-charge lists (cfg4: 228 per type) go one type at a time and the pool -- hence
     * the LDS per wave, hence the occupancy of localize -- stays small. */
    uint32_t gtp() const {
        if (knob_gtp >= 0) return (uint32_t)knob_gtp;                              /* A/B experiments (PYA_GTP) */
        uint32_t g = 0;
        while ((1u << g) < n_types) g++;
        while (g > 0 && (list_cap << g) > 256u) g--;
        return g;
    }
    /* fragment-list slots [signature][type slot][list_cap]: room for sb() signatures */
    uint32_t pool_cap() const {
        const uint32_t per_sig = list_cap << gtp();
        uint32_t want = sb() * per_sig;
        if (want > 2048u) want = 2048u;
        return 2u * per_sig > want ? 2u * per_sig : want;
    }
    uint32_t n_types = 1, k_max = 1;
    uint32_t ns_max = 1;                /* most modifiable residues of one PSM */
    uint32_t z_max = 1;                 /* largest fragment charge in the bucket */
    uint32_t list_max = 1;              /* longest fragment list of one (signature, ion type) */
    uint32_t pair_cap = 1;              /* largest (L - 1) * loss variants: (prefix, variant) pairs of one fragment list */
    uint32_t node_words = 0;            /* largest shared-node shape table (64-bit words) among the PSMs of <= 64 signatures */
    uint32_t node_cols = 0;             /* ... and the most histogram columns one of them needs */
    /* The hash route of the general localize launch (localize_hash.hip.h): ion table for the winner's list and at
     * least one competitor's in-span ions, a grid at most half full, room for the pair lists of a typical PSM
     * (a PSM that needs more is declined and goes to the list-based kernel). */
    uint32_t hash_vc() const { return (2u * list_max + 15u) & ~15u; }
    uint32_t hash_hs() const {
        uint32_t v = 64u;                              /* (a third full at most: 10.15 against 10.45 ms on cfg4 with half) */
        while (v < 3u * hash_vc()) v <<= 1;
        return v;
    }
    /* one direction's pair lists at a time: the winner's and, per competitor of a batch, its in-span pairs on both sides
     * -- room for the worst case, so the hash route never declines for lack of it (PYA_HASH_PP: another multiple of
     * pair_cap, for the tests of the hand-over; 6 instead of 7 measured 4 % slower on cfg4 at the same occupancy: where
     * the arrays behind the lists land in the LDS banks) */
    uint32_t hash_pp() const { return ((knob_hash_pp > 0 ? (uint32_t)knob_hash_pp : 1u + 2u * (sb() - 1u)) * pair_cap + 7u) & ~7u; }
    bool hash_ok(uint32_t max_k, uint32_t n_nl) const {
        return pos_cap <= 64u && hash_vc() <= 8192u &&
               pya_localize_hash_lds_bytes(push_cap(), n_cap, pos_cap, sb(), hash_vc(), hash_hs(), hash_pp(), max_k, n_nl) <= 64u * 1024u;
    }
    uint32_t push_max = 1;              /* largest k * (n_sites - k): single-move competitors of one PSM */
    uint32_t push_cap() const {
        uint32_t v = (push_max + 3u) & ~3u;
        return v > PYA_MAX_PUSHED ? PYA_MAX_PUSHED : v;
    }
    /* The caps grow in two ways only.  cover(): one more PSM -- N site assignments, L residues, charge z, k modifications
     * on ns modifiable residues, per_type fragments per ion type. */
    void cover(const pya_handle &h, uint32_t N, uint32_t L, uint32_t z, uint32_t k, uint32_t ns, uint32_t per_type) {
        const uint32_t n_uniq = (uint32_t)h.cfg.n_uniq;
        n_cap = std::max(n_cap, N);
        list_cap = std::max(list_cap, next_pow2(std::max(per_type, 1u)));
        pos_cap = std::max(pos_cap, std::max(L - 1u, 1u));
        n_types = (uint32_t)h.cfg.n_types;
        k_max = std::max(k_max, k);
        ns_max = std::max(ns_max, ns);
        push_max = std::max(push_max, k <= ns ? k * (ns - k) : 0u);
        z_max = std::max(z_max, z);
        pair_cap = std::max(pair_cap, (L - 1u) * n_uniq);
        list_max = std::max(list_max, per_type);
        if (N <= 64) {
            node_words = std::max(node_words, 2u * (ns + 1u) * (1u + (N + 7u) / 8u));
            auto sc = h.shape_cols.find(ns << 8 | k);
            if (sc != h.shape_cols.end()) node_cols = std::max(node_cols, sc->second);
        }
    }
    /* absorb(): the PSMs of another bucket join this one's launches -- EVERY cap, so that no launch of this bucket is
     * sized without them, whichever caps it reads. */
    void absorb(const Bucket &o) {
        for (uint32_t Bucket::*cap : {&Bucket::n_cap, &Bucket::list_cap, &Bucket::pos_cap, &Bucket::n_types, &Bucket::k_max, &Bucket::ns_max,
                                      &Bucket::z_max, &Bucket::push_max, &Bucket::list_max, &Bucket::pair_cap, &Bucket::node_words,
                                      &Bucket::node_cols})
            this->*cap = std::max(this->*cap, o.*cap);
    }
};

struct pya_plan {
    pya_handle *h = nullptr;
    uint64_t settings_gen = 0;           /* pya_handle::settings_gen when the plan was made */
    uint32_t flags = 0;
    uint64_t n_psm = 0;
    int64_t total_peaks = 0, total_sigs = 0;
    uint32_t peak_cap = 64;
    uint32_t max_k = 1;
    /* host copies needed later */
    std::vector<int64_t> peak_off, sig_off, pep_off, aux_off;
    std::vector<uint32_t> n_sig, order_off;
    std::vector<uint8_t> n_sites, pep;
    std::vector<int32_t> n_of_mod, max_charge;
    /* device metadata */
    DevBuf<int64_t> d_peak_off, d_pep_off, d_aux_off, d_sig_off;
    DevBuf<uint8_t> d_pep, d_n_sites;
    DevBuf<int32_t> d_n_of_mod, d_max_charge, d_status;
    DevBuf<uint32_t> d_aux_pos, d_n_sig, d_order_off, d_ret_n, d_rec, d_sorted;
    DevBuf<float> d_aux_mass, d_ws;
    DevBuf<PeakEntry> d_ret;             /* retained tables, 8-byte entries, every PSM's from an even offset */
    DevBuf<int64_t> d_ret_off;
    std::vector<int64_t> ret_off;        /* [n_psm + 1] */
    /* Shared spectra (pya_plan_create_shared): PSM i is scored against spectrum spec_of[i], the PSMs of a spectrum are
     * consecutive.  peak_off / d_peak_off then describe the n_spec spectra, every spectrum is binned ONCE into one retained
     * table (sret_off; a spectrum no PSM uses has none), and the binning kernels see a spectrum-side view of the plan:
     * ids, ret_off, ret_n and status by spectrum.  ret_off[i] and descriptor word 0 of PSM i carry its spectrum's offset;
     * after the binning pya_fan_out_kernel gives every PSM its spectrum's ret_n and status, so that nothing behind the
     * binning knows the difference.  Unshared plans: spec_of is empty, PSM i has spectrum i. */
    bool shared = false;
    uint64_t n_spec = 0;
    std::vector<uint32_t> spec_of;       /* [n_psm] */
    std::vector<int64_t> sret_off;       /* [n_spec + 1] */
    DevBuf<uint32_t> d_spec_of;          /* [n_psm] as the fan-out reads it: ~0u = set aside by the host pre-pass, keeps its status */
    DevBuf<int64_t> d_sret_off;
    DevBuf<uint32_t> d_sret_n;
    DevBuf<int32_t> d_sstatus;
    uint64_t spec(uint64_t i) const { return spec_of.empty() ? i : spec_of[i]; }
    int64_t n_peaks(uint64_t i) const {
        const uint64_t s = spec(i);
        return peak_off[s + 1] - peak_off[s];
    }
    DevBuf<uint16_t> d_grid;
    DevBuf<uint32_t> d_redo3;            /* the same for localize's lean instantiation */
    DevBuf<uint32_t> d_redo;             /* [1 + n_psm]: count, then the ids bin_spectra hands to its exact variant */
    Bucket buckets[kNumBuckets];
    /* bin_spectra and score_signatures size their LDS by the peak count, so they are launched per
     * peak class (caps = a few quantiles of the batch's peak counts): one 8 000-peak spectrum must
     * not set the occupancy of a batch of 300-peak spectra.  score lists are additionally split by
     * the C(n,k) class (prefix sharing on / off). */
    struct IdList {
        uint32_t off, n, cap, ncls;
    };
    static bool any_ids(const std::vector<IdList> &lists) {         /* (lists exist per class even when no PSM is in them) */
        bool any = false;
        for (const IdList &l : lists) any = any || l.n != 0;
        return any;
    }
    std::vector<uint32_t> bin_ids, score_ids, fused_ids, big_ids;
    std::vector<IdList> bin_lists, score_lists, big_lists;
    /* launches of the fused kernel: per peak class and charge class, and -- since the kernel's speed
     * follows its LDS footprint -- per LDS class: short peptides with a handful of signatures are not
     * launched with the footprint of the longest peptide with 32 */
    struct FusedLaunch {
        uint32_t off, n, cap, multi_z, n_cap, stride, pos_cap, ent_cap, push_cap;
    };
    std::vector<FusedLaunch> fused_launches;
    uint32_t n_fused_total = 0;
    /* PSMs beyond a limit of the fast kernels (peptide > 64 residues, > 15 000 site assignments, > 2 048 fragments per ion
     * type): binned like every other one, then scored and localised by the general kernel (general_psm.hip) */
    std::vector<uint8_t> gen;           /* [n_psm] */
    std::vector<uint32_t> gen_ids;
    DevBuf<uint32_t> d_gen_ids;
    DevBuf<unsigned char> d_gen_scratch;
    uint32_t gen_l_cap = 1, gen_list_cap = 1;
    std::vector<uint64_t> gen_off;      /* [gen_ids.size() + 1] every general PSM's own slice of the scratch */
    DevBuf<uint64_t> d_gen_off;
    /* ... of them the spectra of more than 8 192 peaks: binned by pya_bin_global_kernel (arrays in the workspace) */
    std::vector<uint32_t> bigbin_ids;
    DevBuf<uint32_t> d_bigbin_ids;
    DevBuf<unsigned char> d_bigbin_scratch;
    uint32_t bigbin_cap = 32;
    size_t bigbin_stride = 0;
    std::vector<uint8_t> big;           /* [n_psm] scored by score_big.hip (thousands of site assignments, plain settings) */
    DevBuf<uint32_t> d_big_ids;
    uint32_t big_pos_cap = 1, big_k_max = 1;
    uint32_t big_kc() const {            /* row length of score_big's count-node table: a power of two >= 8, > the most modifications */
        uint32_t v = 8u;
        while (v < big_k_max + 1u) v <<= 1;
        return v;
    }
    /* score_big's own localisation (summary mode, plain settings, C(n,k) <= pya_big_inline_max()): those PSMs are
     * in no localize list; `bigloc` carries the lean localize body's caps for them, d_redo5 the ones it declines */
    bool big_inline = false;
    uint32_t n_big_inline = 0;
    Bucket bigloc;
    DevBuf<uint32_t> d_redo5;
    /* PSMs scored AND localised by the fused kernel (score_localize.hip): few site assignments, plain
     * settings.  `fusedb` carries the caps the general localize instantiation needs for the ones the
     * fused kernel hands over. */
    Bucket fusedb;
    std::vector<uint8_t> fused;         /* [n_psm] */
    std::vector<uint64_t> desc;         /* [n_psm][PYA_DESC_WORDS] packed descriptors (common.h) */
    DevBuf<uint64_t> d_desc;
    uint32_t fused_both = 0, fused_n_cap = 0, fused_stride = 0, fused_ent_cap = 1;
    DevBuf<uint32_t> d_fused_ids, d_redo4, d_ws_top;
    std::vector<uint8_t> ncls;          /* [n_psm] C(n,k) class of the PSM */
    std::vector<int32_t> pre_status;    /* [n_psm] PSMs the host pre-pass set aside (PYA_FLAG_SKIP_INVALID) */
    uint64_t n_skipped = 0;
    DevBuf<uint32_t> d_bin_ids, d_score_ids;
    /* owned copies of inputs/outputs (pya_score_batch path) */
    DevBuf<unsigned char> d_mz, d_inten;  /* (bytes: float64 or float32 elements, IoReq::sp says which) */
    DevBuf<float> d_best_score, d_ascores;
    DevBuf<uint64_t> d_best_sig, d_alt;
    DevBuf<int32_t> d_n_sig_out;
    DevBuf<unsigned long long> d_stamps;
    DevBuf<unsigned char> arena;          /* one allocation behind every device buffer of the plan */
    /* arena layout: [uploaded metadata (+ spectra) | status (+ results) | workspace]; the middle
     * part comes back to the host in one copy on the pya_score_batch path */
    size_t o_status = 0, d2h_bytes = 0, o_best_score = 0, o_best_sig = 0, o_n_sig_out = 0, o_ascores = 0, o_alt = 0;
    uint32_t io_max_k = 0;
    BatchDev dev;
    /* PYA_FLAG_TIMING: five events per run, in a ring so that a caller can enqueue run after run and read the
     * timings of all of them afterwards (pya_plan_timings_sum) instead of waiting for every run */
    static constexpr uint32_t kEvRing = 128;
    static constexpr uint32_t kEvPerRun = 7;      /* boundaries 0 .. 4 of the caller's stream; 5, 6: begin and end of the fused family on the side stream */
    std::vector<hipEvent_t> evring;      /* [kEvRing][kEvPerRun] */
    std::vector<uint8_t> evalias;        /* [kEvRing][kEvPerRun] the event that marks boundary i of the run: a family that launched
                                          * nothing records no event of its own (a record costs microseconds of stream time);
                                          * entry 5 != 0: the run's fused family ran on the side stream, between events 5 and 6 */
    uint64_t ev_runs = 0, ev_read = 0;   /* runs recorded, runs already summed */
    hipEvent_t *ev_set(uint64_t run) { return evring.data() + kEvPerRun * (run % kEvRing); }
    uint8_t *ev_alias(uint64_t run) { return evalias.data() + kEvPerRun * (run % kEvRing); }
    /* r06 -- a batch of mixed shapes has two independent chains behind the binning: the fused score + localize kernels (few
     * site assignments) and the scoring + localize kernels of everything else.  They run BESIDE each other: the fused family
     * on a stream of the plan's own, forked after the binning and joined at the end of the run (two events); the latency-bound
     * localize kernels and the issue-bound fused kernels fill each other's idle slots, and no launch waits for another
     * family's tail. */
    bool fork = false;
    hipStream_t side = nullptr;          /* the handle's (pya_handle::side_stream: created once, plans share it) */
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipStream_t last_stream = nullptr;
    /* pya_plan_evidence: the launch caps of the PSMs inside the fast limits (their longest peptide and fragment list, for
     * the loss sums the handle had then) and, when the plan has general PSMs too, the list of the others; the records of a
     * pya_score_batch plan; the event a call on another stream than the run's waits for */
    bool evid_caps = false;
    uint32_t evid_uniq = 0, evid_l_cap = 1, evid_list_cap = 1, evid_n_fast = 0;
    DevBuf<uint32_t> d_evid_ids;
    DevBuf<pya_evidence> d_evid;
    hipEvent_t ev_evid = nullptr;
    /* pya_plan_ions_count / pya_plan_ions: the evidence rows the two passes read (competitor and depth of every counted
     * column), the tile sums of the scan, the overflow report of the last fill (count, 0xffffffff - smallest PSM), the
     * event the fill and pya_plan_check wait for, and how far the last run has come (0: no count yet, 1: counted, 2: filled);
     * offsets and records of a pya_score_batch plan */
    DevBuf<pya_evidence> d_ions_evid;
    DevBuf<uint64_t> d_ions_tiles;
    DevBuf<uint32_t> d_ions_over;
    DevBuf<int64_t> d_ion_off;
    DevBuf<pya_ion> d_ions;
    hipEvent_t ev_ions = nullptr;
    uint32_t ions_max_k = 0;
    int ions_state = 0;
    /* the out-of-range reports of the last calls behind this run: PSMs whose query range is not inside the output
     * (pya_plan_named), records whose slot is at or above n_slots (pya_plan_rollup), PSMs whose run slot is (pya_plan_mz_profile),
     * records whose slot or row is outside the call's table or matrix (pya_plan_site_quant), PSMs whose row is at or above
     * n_rows (pya_plan_peptidoform_quant) */
    OverReport over[OVER_COUNT];
    /* a pya_score_batch_named plan's slice of the queries (host offsets rebased to the chunk: they outlive the asynchronous
     * upload) and its records */
    std::vector<int64_t> named_q_off;
    DevBuf<int64_t> d_named_q_off;
    DevBuf<uint64_t> d_named_q_bits;
    DevBuf<unsigned char> d_named;
    /* pya_plan_sites: the record offsets of the PSMs (the pre-pass's modifiable residues, summed; a PSM set aside has none),
     * their copy on the device (uploaded by the first call, on its stream), the event a later call on another stream waits
     * for; the records of a pya_score_batch plan */
    std::vector<int64_t> site_off;
    DevBuf<int64_t> d_site_off;
    hipEvent_t ev_sites = nullptr;
    bool site_off_sent = false;
    DevBuf<pya_site> d_sites;
    /* pya_plan_probs: the count-node caps of its two launches (the PSMs inside the fast limits, the general list) -- the
     * largest L - 1, n_of_mod and n_sites among the PSMs of a list whose shape the count-node front end takes, the peaks a
     * staged table may then have inside the 64 KiB the tables are held to, the largest spectrum (rounded up to 32 peaks)
     * among the PSMs that qualify, how many those are and how many PSMs of the list will be scored at all (host_run.cpp:
     * prob_lists) --, the records of a pya_score_batch plan */
    struct ProbList {
        uint32_t pos_max = 1, k_max = 0, ns_max = 0, kc = 8, peak_room = 0, peak_max = 0, n_fit = 0, n_scored = 0;
    };
    ProbList prob_lists[2];
    bool prob_lists_made = false;
    DevBuf<pya_site_prob> d_prob_sites;
    DevBuf<pya_psm_prob> d_prob_psms;
    DevBuf<pya_ranked> d_ranked;         /* pya_plan_ranked: the records of a pya_score_batch plan */
    /* pya_plan_rollup: a pya_score_batch plan's slice of the caller's slots and ids */
    DevBuf<int32_t> d_rollup_slot;
    DevBuf<uint32_t> d_rollup_id;
    /* a pya_score_batch plan's slice of the caller's groups and ids (PYA_FLAG_PEPTIDOFORMS), and its residue records */
    DevBuf<int32_t> d_pform_group;
    DevBuf<uint32_t> d_pform_id;
    uint64_t pform_records = 0;
    /* pya_plan_mz_profile: a pya_score_batch plan's slice of the caller's run slots */
    DevBuf<int32_t> d_mzp_run;
    /* pya_plan_site_quant: a pya_score_batch plan's slice of the caller's rows */
    DevBuf<int32_t> d_quant_row;
    /* pya_plan_peptidoform_quant: a pya_score_batch plan's slice of the caller's rows */
    DevBuf<int32_t> d_pfq_row;
    /* pya_plan_coverage: the raw peak caps of its two launches (the largest spectrum of a PSM inside the fast limits, of a
     * general PSM; once per plan), the event behind the last call's kernels (a later call, on whatever stream, writes
     * behind them) and a pya_score_batch plan's records */
    bool cov_caps = false, cov_asked = false;
    uint32_t cov_peak_fast = 1, cov_peak_gen = 1;
    hipEvent_t ev_cov = nullptr;
    DevBuf<pya_coverage> d_cov;
    /* PYA_FLAG_RECALIBRATE: a pya_score_batch plan's slice of the spectra's slots and the report words of the apply kernel */
    DevBuf<int32_t> d_recal_slot;
    DevBuf<uint32_t> d_recal_over;
    uint64_t n_runs = 0;                 /* pya_plan_run calls so far (which set of hand-over counts is in use) */
    bool ran = false;
    bool quiesced = false;               /* the owner has waited for everything that used the buffers */

    ~pya_plan() {
        for (auto &e : evring)
            if (e) (void)hipEventDestroy(e);
        if (ev_fork) (void)hipEventDestroy(ev_fork);
        if (ev_join) (void)hipEventDestroy(ev_join);
        if (ev_evid) (void)hipEventDestroy(ev_evid);
        if (ev_ions) (void)hipEventDestroy(ev_ions);
        if (ev_sites) (void)hipEventDestroy(ev_sites);
        if (ev_cov) (void)hipEventDestroy(ev_cov);
    }
    uint64_t workspace_bytes() const { return arena.bytes(); }
};

/* Asked by every entry point that launches over a plan, before anything is enqueued: PYA_ERR_STATE when a setting the plan
 * was sized under has changed since (pya_handle::settings_gen).  Read-backs of what a run has produced do not ask. */
inline int plan_settings_stale(pya_plan *p, const char *who) {
    if (p->settings_gen == p->h->settings_gen) return PYA_OK;
    return p->h->fail(PYA_ERR_STATE, -1, "%s: settings changed since the plan was made (pya_add_neutral_loss): its routes and caps belong "
                                         "to the old settings; make a new plan", who);
}

/* ---- functions shared between the host files ---- */
/* host_tables.cpp: configuration -> DevConfig, score table, pre-sort order tables */
int build_dev_config(pya_handle *h);
int sync_config(pya_handle *h);
int ensure_lut(pya_handle *h, uint32_t n_max);
uint32_t shape_offset(pya_handle *h, uint32_t n, uint32_t k);
/* the signature order / inverse / binomial tables on the device (uploaded again when a new shape extended them) */
int upload_shared_tables(pya_handle *h);
/* ... and the handle's tables as the kernels see them: seven fields of every BatchDev */
void shared_tables(const pya_handle *h, BatchDev &d);

/* Which scoring kernel instantiation the settings allow (read at launch time: the handle's settings may change between
 * the runs of a plan). */
inline bool plain_types(const DevConfig &c) { return c.n_nl == 0 && c.n_fwd <= 1 && c.n_types - c.n_fwd <= 1; }
inline bool general_settings(const DevConfig &c) { return !plain_types(c); }     /* neutral losses, or several ion types per direction */
inline uint32_t with_nl(const DevConfig &c) { return c.n_nl != 0 ? 1u : 0u; }
/* loss states the scoring kernels' LDS table has room for: 2 bits per neutral-loss class */
inline uint32_t nl_cap(const DevConfig &c) {
    const uint32_t nnl = (uint32_t)c.n_nl;
    return nnl >= 4u ? 256u : (nnl == 0u ? 4u : 1u << (2u * nnl));
}
/* launches of more than 64 site assignments share the walk over the first sites between signatures ... */
inline uint32_t score_prefix(const pya_handle *h, uint32_t n_cap) { return (n_cap >= 128 && !h->kn.no_prefix) ? 1u : 0u; }
/* ... with compact prefix entries when every PSM is on the straight-line walker */
inline uint32_t score_compact(const DevConfig &c, uint32_t z_max) { return (plain_types(c) && z_max == 1) ? 1u : 0u; }

/* fn(lo, hi) over the PSMs [0, n): on up to eight threads when the batch is big enough to pay for them */
template <typename F>
void for_psm_ranges(uint64_t n, const F &fn) {
    const unsigned nt = n >= 20000 ? std::min(8u, std::max(1u, std::thread::hardware_concurrency())) : 1u;
    if (nt == 1) return fn(0, n);
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; t++) th.emplace_back(fn, n * t / nt, n * (t + 1) / nt);
    for (auto &x : th) x.join();
}

/* ---- one PSM's validity: the plan's pre-pass and pya_score_one ask the same questions, in the same order, and give the
 * same messages ("PSM <i>: ...", written to msg[kPsmMsg]); the return value is PYA_OK or the error code ---- */
const size_t kPsmMsg = 400;
/* the letters alone, without an explanation (the threaded scans): valid residues, *ns = the modifiable ones */
inline bool psm_letters_ok(const pya_handle *h, const uint8_t *pep, int64_t L, uint32_t *ns) {
    return L >= 1 && L <= PYA_MAX_PEPTIDE_LEN && h->scan_peptide(pep, L, ns);
}
/* ranges, letters, fixed-modification positions (n_aux < 0: the batch's aux_off runs backwards); *ns on success */
int check_psm_shape(const pya_handle *h, uint64_t i, int64_t P, int64_t L, int32_t k, int32_t z, const uint8_t *pep,
                    const uint32_t *aux_pos, int64_t n_aux, uint32_t *ns, char *msg);
/* the limits of a PSM whose shape is fine: *N = C(ns, k) (0 when k > ns), *per_type = its fragments per ion type */
inline int check_psm_limits(pya_handle *h, uint64_t i, int64_t L, int32_t k, int32_t z, uint32_t ns, uint64_t *N,
                            uint32_t *per_type, char *msg) {
    *N = 0;
    if ((uint32_t)k <= ns) {
        uint64_t &cached = h->binom_cache[ns][k];
        if (cached == 0) cached = binom(ns, (uint32_t)k);
        *N = cached;
    }
    *per_type = (uint32_t)(L - 1) * (uint32_t)z * (uint32_t)h->cfg.n_uniq;
    if (*N <= PYA_MAX_SIGNATURES && *per_type <= PYA_MAX_FRAGMENTS_PER_TYPE) return PYA_OK;
    if (*N > PYA_MAX_SIGNATURES)
        std::snprintf(msg, kPsmMsg, "PSM %llu: C(%u,%d) site assignments exceed the limit of %d", (unsigned long long)i, ns, k, PYA_MAX_SIGNATURES);
    else
        std::snprintf(msg, kPsmMsg, "PSM %llu: %u fragments per ion type exceed %d", (unsigned long long)i, *per_type, PYA_MAX_FRAGMENTS_PER_TYPE);
    return PYA_ERR_LIMIT;
}
/* descriptor words 4 and 5 (common.h: BatchDev.desc) */
inline void pack_desc_tail(uint64_t L, uint64_t n_aux, int32_t k, uint32_t ns, int32_t z, uint32_t N, uint32_t order_off,
                           uint64_t *w) {
    w[4] = L | n_aux << 16 | (uint64_t)((uint32_t)k & 0xffffu) << 32 | (uint64_t)ns << 48 | (uint64_t)((uint32_t)z & 0xffu) << 56;
    w[5] = (uint64_t)N | (uint64_t)order_off << 32;
}

/* host_plan.cpp: creating a plan (the host pre-pass in phases, the arena); host_run.cpp: running it */
/* Typed spectra (pya_typed_spectra): bytes of one element, 0 for a value that is no type */
inline size_t spec_elem_bytes(uint32_t type) { return type == PYA_F64 ? 8u : type == PYA_F32 ? 4u : 0u; }
/* the supported combinations as the binning launchers name them (common.h: PYA_SPEC_*); anything else: PYA_ERR_ARG with a
 * message that starts with `who` */
int spectra_types(pya_handle *h, const pya_typed_spectra *s, const char *who, uint32_t *types);
/* where the intensities start behind n m/z values of one allocation: at the arena's granule, which aligns every load the
 * kernels make of either type */
inline size_t spec_inten_offset(size_t n_peaks, uint32_t mz_type) { return (n_peaks * spec_elem_bytes(mz_type) + 255) & ~(size_t)255; }
inline size_t spec_pair_bytes(size_t n_peaks, const pya_typed_spectra &s) {
    return spec_inten_offset(n_peaks, s.mz_type) + n_peaks * spec_elem_bytes(s.intensity_type);
}
inline const unsigned char *spec_at(const void *arr, uint32_t type, int64_t peak) {
    return (const unsigned char *)arr + (size_t)peak * spec_elem_bytes(type);
}

struct IoReq {                       /* pya_score_batch: spectra and results live in the plan's arena too */
    pya_typed_spectra sp;            /* the caller's host arrays and their element types */
    uint32_t max_k;
    unsigned char *d_mz_ext, *d_inten_ext;  /* ... unless the caller uploads the spectra itself (big batches) */
    hipStream_t stream;              /* metadata upload: on this stream, waited for alone (nullptr: device-wide) */
    const uint8_t *pre_sites;        /* letter scan already done by the caller: sites per PSM, 255 = invalid letters */
};
/* which spectrum every PSM uses (pya_score_batch_shared / pya_plan_create_shared): spec_of[i] - base, one of the n_spectra
 * that b->peak_off describes -- checked by check_spec_of before it gets here */
struct SpecShare {
    const uint32_t *spec_of;
    uint64_t n_spectra;
    uint32_t base;                   /* (a chunk of a bigger call: its first spectrum) */
};
int check_spec_of(pya_handle *h, uint64_t n_psm, const uint32_t *spec_of, uint64_t n_spectra);
int plan_create_impl(pya_handle *h, const pya_batch *b, uint32_t flags, const IoReq *io, const SpecShare *sh, pya_plan **out);
int check_status(pya_handle *h, const int32_t *st, uint64_t n, bool skip_invalid = false);
/* host_run.cpp: what the last call of stage `which` (OVER_*) behind this run wrote nothing of, as that stage's PYA_ERR_LIMIT;
 * psm_lo: what the plan's first PSM is called in the message, a chunk's place in its batch */
int over_report(pya_plan *p, int which, uint64_t psm_lo);
/* host_peptidoforms.cpp: everything the peptidoform calls refuse, before anything is launched (*run: there are entries), and
 * the stage on `st` behind it: d_n zeroed, then the launches of csrc/peptidoforms.hip */
int pform_check(pya_handle *h, const char *who, uint64_t n_first, const void *d_second, uint64_t n_second, const void *d_work, uint64_t work_bytes,
                const void *d_out, uint64_t cap, const uint32_t *d_n, bool *run);
int pform_run(pya_handle *h, const int64_t *d_site_off, uint64_t n_psm, const void *d_site_probs, const void *d_psm_probs, const int32_t *d_group,
              double threshold, const uint32_t *d_psm_id, uint32_t psm_base, const uint64_t *best_sig, const float *ascores, uint32_t max_k,
              const void *d_src0, uint64_t n0, const void *d_src1, uint64_t n1, void *d_work, void *d_out, uint64_t cap, uint32_t *d_n, bool run,
              hipStream_t st);
/* host_mz_profile.cpp: everything the mass-error profile calls refuse, before anything is launched */
int mzp_check(pya_handle *h, const char *who, uint64_t n_slots, const pya_mz_profile_params *prm);
/* host_site_quant.cpp: everything the site quantification calls refuse, before anything is launched */
int quant_check(pya_handle *h, const char *who, uint64_t n_slots, uint64_t n_rows, const pya_site_quant_params *prm);
/* host_pform_quant.cpp: what the peptidoform quantification calls refuse beyond pform_check and quant_check (the tables of
 * the call and of the earlier lists), and the stage on `st`: the list by pform_run, then csrc/pform_quant.hip behind it */
int pfq_check(pya_handle *h, const char *who, const void *d_head0, const void *d_cell0, const void *d_head1, const void *d_cell1,
              const void *d_head, const void *d_cell, uint64_t cap);
int pfq_run(pya_handle *h, const int64_t *d_site_off, uint64_t n_psm, const void *d_site_probs, const void *d_psm_probs, const int32_t *d_group,
            double threshold, const uint32_t *d_psm_id, uint32_t psm_base, const uint64_t *best_sig, const float *ascores, uint32_t max_k,
            const void *d_src0, const void *d_head0, const void *d_cell0, uint64_t n0, const void *d_src1, const void *d_head1, const void *d_cell1,
            uint64_t n1, const double *d_values, uint64_t n_rows, const int32_t *d_row, uint32_t row_base, const pya_site_quant_params *prm,
            void *d_work, void *d_out, void *d_head, void *d_cell, uint64_t cap, uint32_t *d_n, uint32_t *d_over, bool run, hipStream_t st);
/* host_coverage.cpp: PYA_FLAG_COVERAGE of the batch calls -- the handle's pinned block for the records of a batch of n PSMs
 * (zeroed: a PSM no plan reaches has a PYA_COV_NONE record), and the stage behind a plan's kernels on `st` with its records
 * on their way into the block at PSM `lo` (asynchronous: whoever waits for the chunk's results waits for them too) */
int coverage_host_block(pya_handle *h, uint64_t n);
int coverage_behind_run(pya_handle *h, pya_plan *p, const pya_results *d_out, const pya_typed_spectra *d_sp, uint64_t lo, hipStream_t st);
/* host_deisotope.cpp: what is wrong with a set of deisotoping parameters (NULL: nothing); host_decharge.cpp asks it of the
 * rule inside its own */
const char *deiso_params_fault(const pya_deisotope_params *p);
/* host_transform.cpp, the frame of the spectrum transforms (host_deisotope.cpp, host_decharge.cpp, host_strip.cpp,
 * host_centroid.cpp).  xform_check: everything such a call refuses before anything is launched, in the order of the messages --
 * more than 2^32 - 2 spectra, `params_fault` (what the stage's *_params_fault found, NULL: nothing), the arrays.
 * xform_check_work: a workspace that is NULL, misaligned or smaller than `least_bytes`, what the function named `sizer` gives
 * for no peaks. */
int xform_check(pya_handle *h, const char *who, const char *params_fault, const pya_typed_spectra *in, const int64_t *peak_off,
                uint64_t n_spectra, const pya_typed_spectra *out, const int64_t *new_off, const uint32_t *over);
int xform_check_work(pya_handle *h, const char *who, const char *sizer, uint64_t n_spectra, const void *d_work, uint64_t work_bytes,
                     uint64_t least_bytes);
/* the words of a workspace in front of a stage's own: the tile sums of the scan over the spectra (0 beyond the cap, where the
 * call is refused anyway); and the peaks that keep words behind them -- (n_peaks >> 6) + n_spectra + 1 of them, a spectrum's
 * bits in words of its own (deisotope.hip) -- have bits for */
uint64_t xform_tile_words(uint64_t n_spectra);
int64_t xform_keep_cap(uint64_t n_spectra, uint64_t work_bytes);
/* the device form without spectra: new_off[0] = 0 on the stream */
int xform_no_spectra(pya_handle *h, int64_t *d_new_off, hipStream_t st);
/* a buffer a stage takes beside the spectra: read per spectrum (uploaded), written per spectrum (copied back with new_off) or
 * per output peak (the first new_off[n_spectra] elements copied back); `host` NULL: not passed, and `dev` stays NULL */
const size_t kXformMaxSides = 3;     /* (strip: two precursor arrays and the report) */
struct XformSide {
    enum Kind { SPECTRUM_IN, SPECTRUM_OUT, PEAK_OUT } kind;
    void *host;
    size_t elem_bytes;
    void *dev;                       /* (set by xform_host before it calls the device form) */
};
/* the arguments of a device form that xform_host makes: the device copies, the handle's run stream, the workspace */
struct XformDevice {
    const pya_typed_spectra *in, *out;
    const int64_t *peak_off;
    hipStream_t stream;
    void *work;
    uint64_t work_bytes;
    int64_t *new_off;
    uint32_t *over;
};
/* the host form of a stage whose own checks have passed: validates peak_off, uploads the spectra, the offsets and the
 * SPECTRUM_IN sides, allocates the out arrays, the other sides, a workspace of workspace_bytes(n_spectra, n_peaks), new_off and
 * a zeroed over, calls `device_form`, and copies back new_off, over and the SPECTRUM_OUT sides, then the kept peaks and that
 * many elements of the PEAK_OUT sides */
int xform_host(pya_handle *h, const char *who, const pya_typed_spectra *in, const int64_t *peak_off, uint64_t n_spectra,
               const pya_typed_spectra *out, int64_t *new_off, uint32_t *over, XformSide *side, size_t n_side,
               uint64_t (*workspace_bytes)(uint64_t, uint64_t), const std::function<int(const XformDevice &)> &device_form);
/* host_batch.cpp */
size_t workspace_budget(const pya_handle *h);
static_assert(sizeof(pya_evidence) == 16, "pya_evidence is one 16-byte store of evidence.hip");
static_assert(sizeof(pya_ion) == 16, "pya_ion is one 16-byte store of ions.hip");
static_assert(sizeof(pya_named) == 32 && offsetof(pya_named, pep_score) == 8 && offsetof(pya_named, ambiguity) == 12 &&
                  offsetof(pya_named, total_fragments) == 16 && offsetof(pya_named, kind) == 20 && offsetof(pya_named, depth) == 21 &&
                  offsetof(pya_named, n_moved) == 22 && offsetof(pya_named, reserved) == 23 && offsetof(pya_named, ref_matched) == 24 &&
                  offsetof(pya_named, ref_possible) == 26 && offsetof(pya_named, comp_matched) == 28 &&
                  offsetof(pya_named, comp_possible) == 30,
              "pya_named is two 16-byte stores of named.hip");
static_assert(sizeof(pya_site) == 32 && offsetof(pya_site, without_sig) == 8 && offsetof(pya_site, with_score) == 16 &&
                  offsetof(pya_site, without_score) == 20 && offsetof(pya_site, pos) == 24 && offsetof(pya_site, kind) == 26 &&
                  offsetof(pya_site, flags) == 27 && offsetof(pya_site, reserved) == 28,
              "pya_site is two 16-byte stores of sites.hip");
static_assert(sizeof(pya_site_prob) == 16 && offsetof(pya_site_prob, without_prob) == 8 && sizeof(pya_psm_prob) == 16 &&
                  offsetof(pya_psm_prob, n_summed) == 8 && offsetof(pya_psm_prob, kind) == 12,
              "pya_site_prob and pya_psm_prob are one 16-byte store of probs.hip each");
static_assert(sizeof(pya_ranked) == 16 && offsetof(pya_ranked, pep_score) == 8 && offsetof(pya_ranked, rank) == 12 &&
                  offsetof(pya_ranked, kind) == 14 && offsetof(pya_ranked, flags) == 15,
              "pya_ranked is one 16-byte store of ranked.hip");
static_assert(sizeof(pya_site_rollup) == 32 && offsetof(pya_site_rollup, best_psm) == 8 && offsetof(pya_site_rollup, n_psm) == 12 &&
                  offsetof(pya_site_rollup, n_confident) == 16 && offsetof(pya_site_rollup, n_in_best) == 20 &&
                  offsetof(pya_site_rollup, best_ascore) == 24 && offsetof(pya_site_rollup, reserved) == 28,
              "pya_site_rollup is the 4 x 8 bytes rollup.hip addresses");
static_assert(sizeof(pya_peptidoform) == 48 && offsetof(pya_peptidoform, group) == 8 && offsetof(pya_peptidoform, n_psm) == 12 &&
                  offsetof(pya_peptidoform, n_confident) == 16 && offsetof(pya_peptidoform, best_psm) == 20 &&
                  offsetof(pya_peptidoform, best_min_prob) == 24 && offsetof(pya_peptidoform, best_z) == 32 &&
                  offsetof(pya_peptidoform, best_min_ascore) == 40 && offsetof(pya_peptidoform, n_isomers) == 44,
              "pya_peptidoform is the three 16-byte stores of peptidoforms.hip");
static_assert(sizeof(pya_mz_profile) == 4128 && offsetof(pya_mz_profile, n_ions) == 4 && offsetof(pya_mz_profile, n_rank_skipped) == 8 &&
                  offsetof(pya_mz_profile, out_da) == 12 && offsetof(pya_mz_profile, out_ppm) == 20 && offsetof(pya_mz_profile, reserved) == 28 &&
                  offsetof(pya_mz_profile, da) == 32 && offsetof(pya_mz_profile, ppm) == 32 + 4 * PYA_MZP_BANDS * PYA_MZP_BINS &&
                  sizeof(pya_mz_profile_params) == 32 && offsetof(pya_mz_profile_params, max_rank) == 24,
              "pya_mz_profile is the 1 032 words mz_profile.hip flushes");
static_assert(sizeof(pya_mz_calibration) == 128 && offsetof(pya_mz_calibration, spread_ppm) == 64 && offsetof(pya_mz_calibration, n_signal) == 96,
              "pya_mz_calibration is the 128-byte record mz_calibrate.hip writes");
static_assert(sizeof(pya_site_quant_params) == 24 && offsetof(pya_site_quant_params, scale_log2) == 8 &&
                  offsetof(pya_site_quant_params, n_channels) == 12 && offsetof(pya_site_quant_params, flags) == 16 &&
                  sizeof(pya_site_quant_head) == 8 && offsetof(pya_site_quant_head, n_complete) == 4 && sizeof(pya_site_quant) == 16 &&
                  offsetof(pya_site_quant, n) == 8 && offsetof(pya_site_quant, n_saturated) == 12,
              "pya_site_quant_head is one and pya_site_quant two of the 64-bit words site_quant.hip adds to");
static_assert(sizeof(pya_site_flr) == 32 && offsetof(pya_site_flr, n_decoy) == 4 && offsetof(pya_site_flr, err_sum) == 8 &&
                  offsetof(pya_site_flr, flr) == 16 && offsetof(pya_site_flr, decoy_q) == 24,
              "pya_site_flr is two 16-byte stores of flr.hip");
/* pya_score_batch_named's queries and outputs (host arrays of the caller), nullptr for the other batch entry points */
struct NamedReq {
    const int64_t *q_off;
    const uint64_t *q_bits;
    pya_named *out;
    int32_t *counts;
    float *scores;
};

#endif
