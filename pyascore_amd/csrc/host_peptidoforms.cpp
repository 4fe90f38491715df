/* host_peptidoforms.cpp -- the C ABI of the peptidoform stage (include/pyascore_hip.h: pya_peptidoform; kernels:
 * peptidoforms.hip): the argument checks every form shares, the reduce over device arrays, the host form that uploads, lends
 * a workspace of its own and downloads, and the batch loan.  pya_plan_peptidoforms is host_run.cpp's (it needs the plan's
 * site offsets). */
#include "host_internal.h"
#include "../../include/pyascore_debug.h"

static bool misaligned(const void *p) { return ((uintptr_t)p & 15u) != 0; }

int pform_check(pya_handle *h, const char *who, uint64_t n_first, const void *d_second, uint64_t n_second, const void *d_work, uint64_t work_bytes,
                const void *d_out, uint64_t cap, const uint32_t *d_n, bool *run) {
    *run = false;
    const uint64_t total = n_first + n_second;
    if (n_first > 0x7fffffffull || n_second > 0x7fffffffull || total > 0x7fffffffull)
        return h->fail(PYA_ERR_ARG, -1, "%s: %llu entries are more than 2^31 - 1", who, (unsigned long long)total);
    if (!d_n) return h->fail(PYA_ERR_ARG, -1, "NULL d_n passed to %s", who);
    if (total == 0) return PYA_OK;
    if ((n_second && !d_second) || (cap && !d_out) || !d_work) return h->fail(PYA_ERR_ARG, -1, "NULL device pointer passed to %s", who);
    if (misaligned(d_second) || misaligned(d_out) || misaligned(d_work))
        return h->fail(PYA_ERR_ARG, -1, "%s: the record arrays and the workspace must be 16-byte aligned", who);
    const uint64_t need = pya_pform_layout_bytes(total);
    if (work_bytes < need)
        return h->fail(PYA_ERR_ARG, -1, "%s: a workspace of %llu bytes, %llu entries need %llu", who, (unsigned long long)work_bytes,
                       (unsigned long long)total, (unsigned long long)need);
    *run = true;
    return PYA_OK;
}

int pform_run(pya_handle *h, const int64_t *d_site_off, uint64_t n_psm, const void *d_site_probs, const void *d_psm_probs, const int32_t *d_group,
              double threshold, const uint32_t *d_psm_id, uint32_t psm_base, const uint64_t *best_sig, const float *ascores, uint32_t max_k,
              const void *d_src0, uint64_t n0, const void *d_src1, uint64_t n1, void *d_work, void *d_out, uint64_t cap, uint32_t *d_n, bool run,
              hipStream_t st) {
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemsetAsync(d_n, 0, 2 * sizeof(uint32_t), st));
    h->pform_ev_recorded = false;
    if (!run) return PYA_OK;
    if (h->pform_timed)
        for (hipEvent_t &ev : h->pform_ev)
            if (!ev) HIPCHK(h, hipEventCreate(&ev));
    const int e = pya_launch_pform(d_site_off, n_psm, d_site_probs, d_psm_probs, d_group, threshold, d_psm_id, psm_base, best_sig, ascores, max_k,
                                   d_src0, n0, d_src1, n1, d_work, d_out, cap, d_n, h->pform_timed ? h->pform_ev : nullptr, st);
    if (e) return h->hip_fail((hipError_t)e, "peptidoform launch");
    h->pform_ev_recorded = h->pform_timed;
    return PYA_OK;
}

extern "C" {

uint64_t pya_peptidoform_workspace_bytes(uint64_t n_entries) { return n_entries > 0x7fffffffull ? 0 : pya_pform_layout_bytes(n_entries); }

int pya_peptidoform_reduce(pya_handle *h, const pya_peptidoform *d_a, uint64_t n_a, const pya_peptidoform *d_b, uint64_t n_b, void *hip_stream,
                           void *d_work, uint64_t work_bytes, pya_peptidoform *d_out, uint64_t cap, uint32_t *d_n) {
    if (!h) return PYA_ERR_ARG;
    if (n_a <= 0x7fffffffull && n_a && (!d_a || misaligned(d_a)))
        return h->fail(PYA_ERR_ARG, -1, "pya_peptidoform_reduce: d_a is NULL or not 16-byte aligned");
    bool run;
    const int rc = pform_check(h, "pya_peptidoform_reduce", n_a, d_b, n_b, d_work, work_bytes, d_out, cap, d_n, &run);
    if (rc) return rc;
    return pform_run(h, nullptr, 0, nullptr, nullptr, nullptr, 0., nullptr, 0u, nullptr, nullptr, 0u, d_a, n_a, d_b, n_b, d_work, d_out, cap, d_n,
                     run, (hipStream_t)hip_stream);
}

int pya_peptidoform_reduce_host(pya_handle *h, const pya_peptidoform *a, uint64_t n_a, const pya_peptidoform *b, uint64_t n_b,
                                pya_peptidoform *out, uint64_t cap, uint64_t *n) {
    if (!h) return PYA_ERR_ARG;
    if (!n) return h->fail(PYA_ERR_ARG, -1, "NULL n passed to pya_peptidoform_reduce_host");
    *n = 0;
    const uint64_t total = n_a + n_b;
    if (n_a > 0x7fffffffull || n_b > 0x7fffffffull || total > 0x7fffffffull)
        return h->fail(PYA_ERR_ARG, -1, "pya_peptidoform_reduce_host: %llu entries are more than 2^31 - 1", (unsigned long long)total);
    if (total == 0) return PYA_OK;
    if ((n_a && !a) || (n_b && !b) || (cap && !out)) return h->fail(PYA_ERR_ARG, -1, "NULL array passed to pya_peptidoform_reduce_host");
    HIPCHK(h, hipSetDevice(h->device));
    if (!h->run_stream) HIPCHK(h, hipStreamCreateWithFlags(&h->run_stream, hipStreamNonBlocking));
    const hipStream_t st = h->run_stream;
    DevBuf<pya_peptidoform> d_a, d_b, d_out;
    DevBuf<unsigned char> d_work;
    DevBuf<uint32_t> d_n;
    const uint64_t work = pya_pform_layout_bytes(total), room = std::min(cap, total);
    HIPCHK(h, d_a.upload(a, (size_t)n_a, st));
    HIPCHK(h, d_b.upload(b, (size_t)n_b, st));
    HIPCHK(h, d_work.alloc((size_t)work));
    HIPCHK(h, d_out.alloc((size_t)room));
    HIPCHK(h, d_n.alloc(2));
    const int rc = pya_peptidoform_reduce(h, d_a.p, n_a, d_b.p, n_b, st, d_work.p, work, d_out.p, room, d_n.p);
    if (rc) {
        (void)hipStreamSynchronize(st);                      /* (the buffers are freed on return) */
        return rc;
    }
    uint32_t got[2] = {0u, 0u};
    HIPCHK(h, hipMemcpyAsync(got, d_n.p, sizeof got, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    const uint64_t m = std::min<uint64_t>(got[0], room);
    if (m) HIPCHK(h, hipMemcpy(out, d_out.p, (size_t)m * sizeof(pya_peptidoform), hipMemcpyDeviceToHost));
    *n = got[0];
    return PYA_OK;
}

int pya_set_peptidoforms(pya_handle *h, const int32_t *group, uint64_t n_psm, double threshold, const uint32_t *psm_id) {
    if (!h) return PYA_ERR_ARG;
    h->pform_loan = pya_handle::PformLoan{};
    if (n_psm && !group) return h->fail(PYA_ERR_ARG, -1, "pya_set_peptidoforms: NULL group array for %llu PSMs", (unsigned long long)n_psm);
    if (n_psm > 0x7fffffffull) return h->fail(PYA_ERR_ARG, -1, "pya_set_peptidoforms: %llu PSMs are more than 2^31 - 1", (unsigned long long)n_psm);
    h->pform_loan.group = group;
    h->pform_loan.psm_id = psm_id;
    h->pform_loan.n_psm = n_psm;
    h->pform_loan.threshold = threshold;
    h->pform_loan.set = true;
    return PYA_OK;
}

int pya_last_batch_peptidoforms(pya_handle *h, pya_peptidoform *out, uint64_t cap, uint64_t *n) {
    if (!h) return PYA_ERR_ARG;
    if (!h->pform_valid) return h->fail(PYA_ERR_STATE, -1, "the last batch was scored without PYA_FLAG_PEPTIDOFORMS");
    if (!n) return h->fail(PYA_ERR_ARG, -1, "NULL n passed to pya_last_batch_peptidoforms");
    *n = h->pform_host.size();
    const uint64_t m = std::min<uint64_t>(cap, h->pform_host.size());
    if (m && !out) return h->fail(PYA_ERR_ARG, -1, "NULL array passed to pya_last_batch_peptidoforms");
    if (m) std::memcpy(out, h->pform_host.data(), (size_t)m * sizeof(pya_peptidoform));
    return PYA_OK;
}

int pya_debug_peptidoform_timing(pya_handle *h, int on) {
    if (!h) return PYA_ERR_ARG;
    h->pform_timed = on != 0;
    h->pform_ev_recorded = false;
    return PYA_OK;
}

int pya_debug_last_peptidoform_ms(pya_handle *h, float ms[PYA_PFORM_PHASES + 1]) {
    if (!h || !ms) return PYA_ERR_ARG;
    if (!h->pform_ev_recorded) return h->fail(PYA_ERR_STATE, -1, "no peptidoform call was timed (pya_debug_peptidoform_timing)");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipEventSynchronize(h->pform_ev[PYA_PFORM_PHASES]));
    for (int i = 0; i < PYA_PFORM_PHASES; i++) HIPCHK(h, hipEventElapsedTime(&ms[i], h->pform_ev[i], h->pform_ev[i + 1]));
    HIPCHK(h, hipEventElapsedTime(&ms[PYA_PFORM_PHASES], h->pform_ev[0], h->pform_ev[PYA_PFORM_PHASES]));
    return PYA_OK;
}

}
