/* host_site_quant.cpp -- the C ABI of the site quantification (include/pyascore_hip.h: pya_site_quant; kernels: site_quant.hip):
 * the argument checks every form shares, the batch loan, the table of the last batch call and pya_marker_values.
 * pya_plan_site_quant is host_run.cpp's (it needs the plan's site offsets and the wait for the run), the batch path
 * host_batch.cpp's. */
#include "host_internal.h"

#include <cmath>

int quant_check(pya_handle *h, const char *who, uint64_t n_slots, uint64_t n_rows, const pya_site_quant_params *prm) {
    if (!prm) return h->fail(PYA_ERR_ARG, -1, "NULL params passed to %s", who);
    if (n_slots > 0x7fffffffull) return h->fail(PYA_ERR_ARG, -1, "%s: %llu slots are more than an int32 slot can name", who, (unsigned long long)n_slots);
    if (n_rows > 0x7fffffffull) return h->fail(PYA_ERR_ARG, -1, "%s: %llu rows are more than an int32 row can name", who, (unsigned long long)n_rows);
    if (std::isnan(prm->threshold)) return h->fail(PYA_ERR_ARG, -1, "%s: threshold is not a number", who);
    if (prm->scale_log2 < -64 || prm->scale_log2 > 64) return h->fail(PYA_ERR_ARG, -1, "%s: scale_log2 %d is not in -64 .. 64", who, prm->scale_log2);
    if (prm->n_channels < 1u || prm->n_channels > (uint32_t)PYA_QUANT_MAX_CHANNELS)
        return h->fail(PYA_ERR_ARG, -1, "%s: n_channels %u is not in 1 .. %d", who, prm->n_channels, PYA_QUANT_MAX_CHANNELS);
    if (prm->flags & ~PYA_QUANT_COMPLETE_ONLY) return h->fail(PYA_ERR_ARG, -1, "%s: unknown flag bits 0x%x", who, prm->flags & ~PYA_QUANT_COMPLETE_ONLY);
    if (prm->reserved != 0u) return h->fail(PYA_ERR_ARG, -1, "%s: reserved is not 0", who);
    return PYA_OK;
}

extern "C" {

int pya_set_site_quant(pya_handle *h, const double *values, uint64_t n_rows, const int32_t *row, uint64_t n_psm,
                       const pya_site_quant_params *params) {
    if (!h) return PYA_ERR_ARG;
    h->quant_loan = pya_handle::QuantLoan{};
    if (n_psm > 0x7fffffffull) return h->fail(PYA_ERR_ARG, -1, "pya_set_site_quant: %llu PSMs are more than 2^31 - 1", (unsigned long long)n_psm);
    const int rc = quant_check(h, "pya_set_site_quant", 0, n_rows, params);
    if (rc) return rc;
    if (n_rows && !values) return h->fail(PYA_ERR_ARG, -1, "NULL values passed to pya_set_site_quant");
    h->quant_loan.values = values;
    h->quant_loan.row = row;
    h->quant_loan.n_rows = n_rows;
    h->quant_loan.n_psm = n_psm;
    h->quant_loan.params = *params;
    h->quant_loan.set = true;
    return PYA_OK;
}

int pya_last_batch_site_quant(pya_handle *h, pya_site_quant_head *head, pya_site_quant *cell, uint64_t n_slots, uint32_t n_channels) {
    if (!h) return PYA_ERR_ARG;
    if (!h->quant_valid) return h->fail(PYA_ERR_STATE, -1, "the last batch was scored without PYA_FLAG_QUANT");
    if (n_slots != h->quant_head_host.size() || n_channels != h->quant_channels)
        return h->fail(PYA_ERR_ARG, -1, "the quantification of the last batch has %llu slots of %u channels, not %llu of %u",
                       (unsigned long long)h->quant_head_host.size(), h->quant_channels, (unsigned long long)n_slots, n_channels);
    if (n_slots == 0) return PYA_OK;
    if (!head || !cell) return h->fail(PYA_ERR_ARG, -1, "NULL array passed to pya_last_batch_site_quant");
    std::memcpy(head, h->quant_head_host.data(), (size_t)n_slots * sizeof(pya_site_quant_head));
    std::memcpy(cell, h->quant_cell_host.data(), (size_t)n_slots * n_channels * sizeof(pya_site_quant));
    return PYA_OK;
}

int pya_marker_values(pya_handle *h, const pya_marker *d_markers, uint64_t n_spectra, uint32_t n_targets, uint64_t channel_mask,
                      void *hip_stream, double *d_values) {
    if (!h) return PYA_ERR_ARG;
    const char *who = "pya_marker_values";
    if (n_targets < 1u || n_targets > (uint32_t)PYA_MARKER_MAX_TARGETS)
        return h->fail(PYA_ERR_ARG, -1, "%s: n_targets %u is not in 1 .. %d", who, n_targets, PYA_MARKER_MAX_TARGETS);
    if (channel_mask == 0ull) return h->fail(PYA_ERR_ARG, -1, "%s: channel_mask names no target", who);
    if (n_targets < 64u && (channel_mask >> n_targets) != 0ull) return h->fail(PYA_ERR_ARG, -1, "%s: channel_mask has a bit at or above n_targets", who);
    if (n_spectra > 0xfffffffeull) return h->fail(PYA_ERR_ARG, -1, "%s: %llu spectra are more than 2^32 - 2", who, (unsigned long long)n_spectra);
    if (n_spectra == 0) return PYA_OK;
    if (!d_markers || !d_values) return h->fail(PYA_ERR_ARG, -1, "NULL array passed to %s", who);
    HIPCHK(h, hipSetDevice(h->device));
    const int e = pya_launch_marker_values(d_markers, n_spectra, n_targets, channel_mask, d_values, (hipStream_t)hip_stream);
    if (e) return h->hip_fail((hipError_t)e, "marker values launch");
    return PYA_OK;
}

}
