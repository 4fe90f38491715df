/* host_pform_quant.cpp -- the C ABI of the peptidoform quantification (include/pyascore_hip.h: peptidoform quantification;
 * kernel: pform_quant.hip): the argument checks every form shares, the stage (the list by host_peptidoforms.cpp's pform_run,
 * the table behind it), the reduce over device arrays, the host form that uploads, lends a workspace of its own and
 * downloads, the batch loan and the table of the last batch call.  pya_plan_peptidoform_quant is host_run.cpp's (it needs the
 * plan's site offsets and the wait for the run), the batch path host_batch.cpp's. */
#include "host_internal.h"

#include <cmath>

static bool misaligned(const void *p) { return ((uintptr_t)p & 15u) != 0; }

int pfq_check(pya_handle *h, const char *who, const void *d_head0, const void *d_cell0, const void *d_head1, const void *d_cell1,
              const void *d_head, const void *d_cell, uint64_t cap) {
    if ((d_head0 == nullptr) != (d_cell0 == nullptr) || (d_head1 == nullptr) != (d_cell1 == nullptr))
        return h->fail(PYA_ERR_ARG, -1, "%s: the head and the cells of an earlier table must both be given or both be NULL", who);
    if (cap && (!d_head || !d_cell)) return h->fail(PYA_ERR_ARG, -1, "NULL device pointer passed to %s", who);
    if (misaligned(d_cell0) || misaligned(d_cell1) || misaligned(d_cell) || ((uintptr_t)d_head0 & 7u) || ((uintptr_t)d_head1 & 7u) ||
        ((uintptr_t)d_head & 7u))
        return h->fail(PYA_ERR_ARG, -1, "%s: the cells must be 16-byte and the heads 8-byte aligned", who);
    return PYA_OK;
}

int pfq_run(pya_handle *h, const int64_t *d_site_off, uint64_t n_psm, const void *d_site_probs, const void *d_psm_probs, const int32_t *d_group,
            double threshold, const uint32_t *d_psm_id, uint32_t psm_base, const uint64_t *best_sig, const float *ascores, uint32_t max_k,
            const void *d_src0, const void *d_head0, const void *d_cell0, uint64_t n0, const void *d_src1, const void *d_head1, const void *d_cell1,
            uint64_t n1, const double *d_values, uint64_t n_rows, const int32_t *d_row, uint32_t row_base, const pya_site_quant_params *prm,
            void *d_work, void *d_out, void *d_head, void *d_cell, uint64_t cap, uint32_t *d_n, uint32_t *d_over, bool run, hipStream_t st) {
    const int rc = pform_run(h, d_site_off, n_psm, d_site_probs, d_psm_probs, d_group, threshold, d_psm_id, psm_base, best_sig, ascores, max_k,
                             d_src0, n0, d_src1, n1, d_work, d_out, cap, d_n, run, st);
    if (rc) return rc;
    /* (without entries the launcher clears the table and launches nothing) */
    const int e = pya_launch_pform_quant(d_site_off, run ? n_psm : 0, d_site_probs, d_psm_probs, d_group, best_sig, max_k, d_src0, d_head0, d_cell0,
                                         run ? n0 : 0, d_src1, d_head1, d_cell1, run ? n1 : 0, d_values, n_rows, d_row, row_base, prm,
                                         std::ldexp(1.0, prm->scale_log2), d_out, d_n, d_head, d_cell, cap, d_over, st);
    if (e) return h->hip_fail((hipError_t)e, "peptidoform quantification launch");
    return PYA_OK;
}

extern "C" {

uint64_t pya_peptidoform_quant_workspace_bytes(uint64_t n_entries, uint32_t n_channels) {
    (void)n_channels;                                        /* (the table stage keeps nothing in the workspace) */
    return pya_peptidoform_workspace_bytes(n_entries);
}

int pya_peptidoform_quant_reduce(pya_handle *h, const pya_peptidoform *d_a, const pya_site_quant_head *d_a_head, const pya_site_quant *d_a_cell,
                                 uint64_t n_a, const pya_peptidoform *d_b, const pya_site_quant_head *d_b_head, const pya_site_quant *d_b_cell,
                                 uint64_t n_b, uint32_t n_channels, void *hip_stream, void *d_work, uint64_t work_bytes, pya_peptidoform *d_out,
                                 pya_site_quant_head *d_head, pya_site_quant *d_cell, uint64_t cap, uint32_t *d_n) {
    if (!h) return PYA_ERR_ARG;
    const char *who = "pya_peptidoform_quant_reduce";
    if (n_channels < 1u || n_channels > (uint32_t)PYA_QUANT_MAX_CHANNELS)
        return h->fail(PYA_ERR_ARG, -1, "%s: n_channels %u is not in 1 .. %d", who, n_channels, PYA_QUANT_MAX_CHANNELS);
    if (n_a <= 0x7fffffffull && n_a && (!d_a || misaligned(d_a))) return h->fail(PYA_ERR_ARG, -1, "%s: d_a is NULL or not 16-byte aligned", who);
    bool run;
    int rc = pform_check(h, who, n_a, d_b, n_b, d_work, work_bytes, d_out, cap, d_n, &run);
    if (rc) return rc;
    if ((rc = pfq_check(h, who, d_a_head, d_a_cell, d_b_head, d_b_cell, d_head, d_cell, cap))) return rc;
    const pya_site_quant_params prm = {0., 0, n_channels, 0u, 0u};
    return pfq_run(h, nullptr, 0, nullptr, nullptr, nullptr, 0., nullptr, 0u, nullptr, nullptr, 0u, d_a, d_a_head, d_a_cell, n_a, d_b, d_b_head,
                   d_b_cell, n_b, nullptr, 0, nullptr, 0u, &prm, d_work, d_out, d_head, d_cell, cap, d_n, nullptr, run, (hipStream_t)hip_stream);
}

int pya_peptidoform_quant_reduce_host(pya_handle *h, const pya_peptidoform *a, const pya_site_quant_head *a_head, const pya_site_quant *a_cell,
                                      uint64_t n_a, const pya_peptidoform *b, const pya_site_quant_head *b_head, const pya_site_quant *b_cell,
                                      uint64_t n_b, uint32_t n_channels, pya_peptidoform *out, pya_site_quant_head *head, pya_site_quant *cell,
                                      uint64_t cap, uint64_t *n) {
    if (!h) return PYA_ERR_ARG;
    const char *who = "pya_peptidoform_quant_reduce_host";
    if (!n) return h->fail(PYA_ERR_ARG, -1, "NULL n passed to %s", who);
    *n = 0;
    if (n_channels < 1u || n_channels > (uint32_t)PYA_QUANT_MAX_CHANNELS)
        return h->fail(PYA_ERR_ARG, -1, "%s: n_channels %u is not in 1 .. %d", who, n_channels, PYA_QUANT_MAX_CHANNELS);
    const uint64_t total = n_a + n_b;
    if (n_a > 0x7fffffffull || n_b > 0x7fffffffull || total > 0x7fffffffull)
        return h->fail(PYA_ERR_ARG, -1, "%s: %llu entries are more than 2^31 - 1", who, (unsigned long long)total);
    if ((a_head == nullptr) != (a_cell == nullptr) || (b_head == nullptr) != (b_cell == nullptr))
        return h->fail(PYA_ERR_ARG, -1, "%s: the head and the cells of a table must both be given or both be NULL", who);
    if ((n_a && !a) || (n_b && !b) || (cap && (!out || !head || !cell))) return h->fail(PYA_ERR_ARG, -1, "NULL array passed to %s", who);
    const uint64_t room = std::min(cap, total);
    if (room) {
        std::memset(head, 0, (size_t)room * sizeof(pya_site_quant_head));
        std::memset(cell, 0, (size_t)room * n_channels * sizeof(pya_site_quant));
    }
    if (total == 0) return PYA_OK;
    HIPCHK(h, hipSetDevice(h->device));
    if (!h->run_stream) HIPCHK(h, hipStreamCreateWithFlags(&h->run_stream, hipStreamNonBlocking));
    const hipStream_t st = h->run_stream;
    DevBuf<pya_peptidoform> d_a, d_b, d_out;
    DevBuf<pya_site_quant_head> d_a_head, d_b_head, d_head;
    DevBuf<pya_site_quant> d_a_cell, d_b_cell, d_cell;
    DevBuf<unsigned char> d_work;
    DevBuf<uint32_t> d_n;
    const uint64_t work = pya_pform_layout_bytes(total);
    HIPCHK(h, d_a.upload(a, (size_t)n_a, st));
    HIPCHK(h, d_b.upload(b, (size_t)n_b, st));
    if (a_head && n_a) {
        HIPCHK(h, d_a_head.upload(a_head, (size_t)n_a, st));
        HIPCHK(h, d_a_cell.upload(a_cell, (size_t)n_a * n_channels, st));
    }
    if (b_head && n_b) {
        HIPCHK(h, d_b_head.upload(b_head, (size_t)n_b, st));
        HIPCHK(h, d_b_cell.upload(b_cell, (size_t)n_b * n_channels, st));
    }
    HIPCHK(h, d_work.alloc((size_t)work));
    HIPCHK(h, d_out.alloc((size_t)std::max<uint64_t>(room, 1)));
    HIPCHK(h, d_head.alloc((size_t)std::max<uint64_t>(room, 1)));
    HIPCHK(h, d_cell.alloc((size_t)std::max<uint64_t>(room, 1) * n_channels));
    HIPCHK(h, d_n.alloc(2));
    const int rc = pya_peptidoform_quant_reduce(h, d_a.p, d_a_head.p, d_a_cell.p, n_a, d_b.p, d_b_head.p, d_b_cell.p, n_b, n_channels, st, d_work.p,
                                                work, d_out.p, d_head.p, d_cell.p, room, d_n.p);
    if (rc) {
        (void)hipStreamSynchronize(st);                      /* (the buffers are freed on return) */
        return rc;
    }
    uint32_t got[2] = {0u, 0u};
    HIPCHK(h, hipMemcpyAsync(got, d_n.p, sizeof got, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    const uint64_t m = std::min<uint64_t>(got[0], room);
    if (m) {
        HIPCHK(h, hipMemcpy(out, d_out.p, (size_t)m * sizeof(pya_peptidoform), hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(head, d_head.p, (size_t)m * sizeof(pya_site_quant_head), hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(cell, d_cell.p, (size_t)m * n_channels * sizeof(pya_site_quant), hipMemcpyDeviceToHost));
    }
    *n = got[0];
    return PYA_OK;
}

int pya_set_peptidoform_quant(pya_handle *h, const double *values, uint64_t n_rows, const int32_t *row, uint64_t n_psm,
                              const pya_site_quant_params *params) {
    if (!h) return PYA_ERR_ARG;
    h->pfq_loan = pya_handle::QuantLoan{};
    if (n_psm > 0x7fffffffull) return h->fail(PYA_ERR_ARG, -1, "pya_set_peptidoform_quant: %llu PSMs are more than 2^31 - 1", (unsigned long long)n_psm);
    const int rc = quant_check(h, "pya_set_peptidoform_quant", 0, n_rows, params);
    if (rc) return rc;
    if (n_rows && !values) return h->fail(PYA_ERR_ARG, -1, "NULL values passed to pya_set_peptidoform_quant");
    h->pfq_loan.values = values;
    h->pfq_loan.row = row;
    h->pfq_loan.n_rows = n_rows;
    h->pfq_loan.n_psm = n_psm;
    h->pfq_loan.params = *params;
    h->pfq_loan.set = true;
    return PYA_OK;
}

int pya_last_batch_peptidoform_quant(pya_handle *h, pya_site_quant_head *head, pya_site_quant *cell, uint64_t n, uint32_t n_channels) {
    if (!h) return PYA_ERR_ARG;
    if (!h->pfq_valid) return h->fail(PYA_ERR_STATE, -1, "the last batch was scored without PYA_FLAG_PFORM_QUANT");
    if (n != h->pfq_head_host.size() || n_channels != h->pfq_channels)
        return h->fail(PYA_ERR_ARG, -1, "the peptidoform quantification of the last batch has %llu rows of %u channels, not %llu of %u",
                       (unsigned long long)h->pfq_head_host.size(), h->pfq_channels, (unsigned long long)n, n_channels);
    if (n == 0) return PYA_OK;
    if (!head || !cell) return h->fail(PYA_ERR_ARG, -1, "NULL array passed to pya_last_batch_peptidoform_quant");
    std::memcpy(head, h->pfq_head_host.data(), (size_t)n * sizeof(pya_site_quant_head));
    std::memcpy(cell, h->pfq_cell_host.data(), (size_t)n * n_channels * sizeof(pya_site_quant));
    return PYA_OK;
}

}
