/* host_channel_correct.cpp -- the C ABI of the channel correction (include/pyascore_hip.h: channel correction; kernels:
 * channel_correct.hip): the argument checks of the three device forms and the host form, which chains them on the handle's
 * stream between one upload and one download. */
#include "host_internal.h"

#include <cmath>

extern "C" int pya_launch_channel_correct(const double *d_values, uint64_t n_rows, uint32_t n_ch, const double *d_matrix, const double *d_factor,
                                          double *d_out, hipStream_t stream);
extern "C" int pya_launch_channel_sums(const double *d_values, uint64_t n_rows, uint32_t n_ch, const uint8_t *d_select, double scale, void *d_cell,
                                       hipStream_t stream);
extern "C" int pya_launch_channel_factors(const void *d_cell, uint32_t n_ch, double *d_factor, hipStream_t stream);

static_assert(sizeof(pya_site_quant) == 16 && offsetof(pya_site_quant, n) == 8 && offsetof(pya_site_quant, n_saturated) == 12,
              "pya_site_quant is two 64-bit words: sum; n | n_saturated << 32");

static const uint64_t kChannelMaxRows = 0xfffffffeull;

static bool misaligned(const void *p) { return ((uintptr_t)p & 7u) != 0; }

/* what every form refuses about the shape of the matrix */
static int channel_shape_check(pya_handle *h, const char *who, uint64_t n_rows, uint32_t n_channels) {
    if (n_channels < 1u || n_channels > (uint32_t)PYA_QUANT_MAX_CHANNELS)
        return h->fail(PYA_ERR_ARG, -1, "%s: n_channels %u is not in 1 .. %d", who, n_channels, PYA_QUANT_MAX_CHANNELS);
    if (n_rows > kChannelMaxRows) return h->fail(PYA_ERR_ARG, -1, "%s: %llu rows are more than 2^32 - 2", who, (unsigned long long)n_rows);
    return PYA_OK;
}

static int channel_scale_check(pya_handle *h, const char *who, int32_t scale_log2) {
    if (scale_log2 < -64 || scale_log2 > 64) return h->fail(PYA_ERR_ARG, -1, "%s: scale_log2 %d is not in -64 .. 64", who, scale_log2);
    return PYA_OK;
}

extern "C" {

int pya_channel_correct(pya_handle *h, const double *d_values, uint64_t n_rows, uint32_t n_channels, const double *d_matrix,
                        const double *d_factor, void *hip_stream, double *d_out) {
    if (!h) return PYA_ERR_ARG;
    const char *who = "pya_channel_correct";
    if (const int rc = channel_shape_check(h, who, n_rows, n_channels)) return rc;
    if (!d_matrix && !d_factor) return h->fail(PYA_ERR_ARG, -1, "%s: neither a matrix nor a factor", who);
    if (misaligned(d_values) || misaligned(d_out) || misaligned(d_matrix) || misaligned(d_factor))
        return h->fail(PYA_ERR_ARG, -1, "%s: the arrays are not 8-byte aligned", who);
    if (n_rows == 0) return PYA_OK;
    if (!d_values || !d_out) return h->fail(PYA_ERR_ARG, -1, "NULL array passed to %s", who);
    HIPCHK(h, hipSetDevice(h->device));
    const int e = pya_launch_channel_correct(d_values, n_rows, n_channels, d_matrix, d_factor, d_out, (hipStream_t)hip_stream);
    if (e) return h->hip_fail((hipError_t)e, "channel correct launch");
    return PYA_OK;
}

int pya_channel_sums(pya_handle *h, const double *d_values, uint64_t n_rows, uint32_t n_channels, const uint8_t *d_select, int32_t scale_log2,
                     void *hip_stream, pya_site_quant *d_cell) {
    if (!h) return PYA_ERR_ARG;
    const char *who = "pya_channel_sums";
    if (const int rc = channel_shape_check(h, who, n_rows, n_channels)) return rc;
    if (const int rc = channel_scale_check(h, who, scale_log2)) return rc;
    if (misaligned(d_values) || misaligned(d_cell)) return h->fail(PYA_ERR_ARG, -1, "%s: the arrays are not 8-byte aligned", who);
    if (n_rows == 0) return PYA_OK;
    if (!d_values || !d_cell) return h->fail(PYA_ERR_ARG, -1, "NULL array passed to %s", who);
    HIPCHK(h, hipSetDevice(h->device));
    const int e = pya_launch_channel_sums(d_values, n_rows, n_channels, d_select, std::ldexp(1.0, scale_log2), d_cell, (hipStream_t)hip_stream);
    if (e) return h->hip_fail((hipError_t)e, "channel sums launch");
    return PYA_OK;
}

int pya_channel_factors(pya_handle *h, const pya_site_quant *d_cell, uint32_t n_channels, void *hip_stream, double *d_factor) {
    if (!h) return PYA_ERR_ARG;
    const char *who = "pya_channel_factors";
    if (const int rc = channel_shape_check(h, who, 0, n_channels)) return rc;
    if (!d_cell || !d_factor) return h->fail(PYA_ERR_ARG, -1, "NULL array passed to %s", who);
    if (misaligned(d_cell) || misaligned(d_factor)) return h->fail(PYA_ERR_ARG, -1, "%s: the arrays are not 8-byte aligned", who);
    HIPCHK(h, hipSetDevice(h->device));
    const int e = pya_launch_channel_factors(d_cell, n_channels, d_factor, (hipStream_t)hip_stream);
    if (e) return h->hip_fail((hipError_t)e, "channel factors launch");
    return PYA_OK;
}

int pya_channel_correct_host(pya_handle *h, const double *values, uint64_t n_rows, uint32_t n_channels, const double *matrix,
                             const uint8_t *select, int32_t scale_log2, uint32_t flags, double *out, pya_site_quant *cell, double *factor) {
    if (!h) return PYA_ERR_ARG;
    const char *who = "pya_channel_correct_host";
    if (const int rc = channel_shape_check(h, who, n_rows, n_channels)) return rc;
    if (const int rc = channel_scale_check(h, who, scale_log2)) return rc;
    if (flags & ~PYA_CHANNEL_NORMALIZE) return h->fail(PYA_ERR_ARG, -1, "%s: unknown flag bits 0x%x", who, flags & ~PYA_CHANNEL_NORMALIZE);
    const bool normalize = (flags & PYA_CHANNEL_NORMALIZE) != 0u;
    if (!matrix && !normalize) return h->fail(PYA_ERR_ARG, -1, "%s: neither a matrix nor PYA_CHANNEL_NORMALIZE", who);
    if (normalize && (!cell || !factor)) return h->fail(PYA_ERR_ARG, -1, "NULL array passed to %s", who);
    if (n_rows && (!values || !out)) return h->fail(PYA_ERR_ARG, -1, "NULL array passed to %s", who);
    if (misaligned(values) || misaligned(out) || misaligned(matrix) || misaligned(cell) || misaligned(factor))
        return h->fail(PYA_ERR_ARG, -1, "%s: the arrays are not 8-byte aligned", who);
    const size_t n = (size_t)n_rows * n_channels;
    HIPCHK(h, hipSetDevice(h->device));
    if (!h->run_stream) HIPCHK(h, hipStreamCreateWithFlags(&h->run_stream, hipStreamNonBlocking));
    const hipStream_t st = h->run_stream;
    DevBuf<double> d_values, d_matrix, d_factor;
    DevBuf<uint8_t> d_select;
    DevBuf<pya_site_quant> d_cell;
    HIPCHK(h, d_values.upload(values, n, st));
    if (matrix) HIPCHK(h, d_matrix.upload(matrix, (size_t)n_channels * n_channels, st));
    if (select && cell) HIPCHK(h, d_select.upload(select, (size_t)n_rows, st));
    int rc = PYA_OK;
    if (matrix) rc = pya_channel_correct(h, d_values.p, n_rows, n_channels, d_matrix.p, nullptr, st, d_values.p);
    if (!rc && cell) {
        HIPCHK(h, d_cell.alloc(n_channels));
        HIPCHK(h, hipMemsetAsync(d_cell.p, 0, (size_t)n_channels * sizeof(pya_site_quant), st));
        rc = pya_channel_sums(h, d_values.p, n_rows, n_channels, select ? d_select.p : nullptr, scale_log2, st, d_cell.p);
    }
    if (!rc && normalize) {
        HIPCHK(h, d_factor.alloc(n_channels));
        rc = pya_channel_factors(h, d_cell.p, n_channels, st, d_factor.p);
        if (!rc) rc = pya_channel_correct(h, d_values.p, n_rows, n_channels, nullptr, d_factor.p, st, d_values.p);
    }
    if (rc) {
        (void)hipStreamSynchronize(st);                      /* (the buffers are freed on return) */
        return rc;
    }
    if (n) HIPCHK(h, hipMemcpyAsync(out, d_values.p, n * sizeof(double), hipMemcpyDeviceToHost, st));
    if (cell) HIPCHK(h, hipMemcpyAsync(cell, d_cell.p, (size_t)n_channels * sizeof(pya_site_quant), hipMemcpyDeviceToHost, st));
    if (normalize) HIPCHK(h, hipMemcpyAsync(factor, d_factor.p, (size_t)n_channels * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    return PYA_OK;
}

}
