/* host_purity.cpp -- the C ABI of the precursor-purity stage (include/pyascore_hip.h: pya_purity_params; kernels: purity.hip):
 * the argument checks, the host form and the gate.  As the marker stage it reads spectra and writes records -- no out arrays,
 * no new offsets, no workspace --, so it shares the wording and the order of host_markers.cpp's refusals, and its host form is
 * the small one: upload the survey spectra and the queries once, copy only the records back. */
#include "host_internal.h"

#include <cmath>

extern "C" int pya_launch_purity(const void *d_mz, const void *d_in, uint32_t mz_type, uint32_t in_type, const int64_t *d_peak_off,
                                 uint64_t n_survey, int64_t cap_peaks, const int64_t *d_survey, const double *d_prec_mz, const int32_t *d_prec_z,
                                 const double *d_win_lo, const double *d_win_hi, uint64_t n_query, const pya_purity_params *prm,
                                 pya_purity *d_purity, uint32_t *d_over, hipStream_t stream);
extern "C" int pya_launch_purity_gate(const pya_purity *d_purity, uint64_t n_rows, double threshold, uint32_t keep_unknown, const double *d_values,
                                      uint32_t n_ch, double *d_out, uint8_t *d_select, hipStream_t stream);

static_assert(sizeof(pya_purity_params) == 40 && offsetof(pya_purity_params, tol_ppm) == 8 && offsetof(pya_purity_params, step) == 16 &&
                  offsetof(pya_purity_params, below) == 24 && offsetof(pya_purity_params, isotopes) == 28 &&
                  offsetof(pya_purity_params, reserved) == 32,
              "pya_purity_params is a 40-byte record");
static_assert(sizeof(pya_purity) == 48 && offsetof(pya_purity, precursor) == 8 && offsetof(pya_purity, other_mz) == 16 &&
                  offsetof(pya_purity, other_intensity) == 24 && offsetof(pya_purity, n_window) == 32 && offsetof(pya_purity, n_precursor) == 36 &&
                  offsetof(pya_purity, iso_hit) == 40 && offsetof(pya_purity, flags) == 44,
              "pya_purity is a 48-byte record");
static_assert(PYA_PURITY_MAX_CENTRES == 16 && PYA_PURITY_MAX_BELOW == 4, "one centre per lane, one bit of iso_hit each");

static const uint64_t kPurityMaxRows = 0xfffffffeull;

static const char *purity_params_fault(const pya_purity_params *p) {
    if (!p) return "params is NULL";
    if (!std::isfinite(p->tol) || !(p->tol >= 0.)) return "tol is not a finite number >= 0";
    if (!std::isfinite(p->tol_ppm) || !(p->tol_ppm >= 0.)) return "tol_ppm is not a finite number >= 0";
    if (!std::isfinite(p->step) || !(p->step > 0.)) return "step is not finite and positive";
    if (p->below > PYA_PURITY_MAX_BELOW) return "below is not in 0 .. PYA_PURITY_MAX_BELOW";
    if (p->isotopes > PYA_PURITY_MAX_CENTRES || p->below + 1u + p->isotopes > PYA_PURITY_MAX_CENTRES)
        return "below + 1 + isotopes is not in 1 .. PYA_PURITY_MAX_CENTRES";
    if (p->reserved[0] != 0 || p->reserved[1] != 0) return "reserved is not 0";
    return nullptr;
}

/* everything either form refuses before anything is launched, in the order of the marker stage's messages */
static int purity_check(pya_handle *h, const char *who, const pya_typed_spectra *in, const int64_t *peak_off, uint64_t n_survey,
                        const int64_t *survey, const double *prec_mz, const int32_t *prec_z, const double *win_lo, const double *win_hi,
                        uint64_t n_query, const pya_purity_params *params, const pya_purity *purity, const uint32_t *over) {
    if (n_query > kPurityMaxRows) return h->fail(PYA_ERR_ARG, -1, "%s: %llu queries are more than 2^32 - 2", who, (unsigned long long)n_query);
    if (n_survey > kPurityMaxRows)
        return h->fail(PYA_ERR_ARG, -1, "%s: %llu survey spectra are more than 2^32 - 2", who, (unsigned long long)n_survey);
    if (const char *fault = purity_params_fault(params)) return h->fail(PYA_ERR_ARG, -1, "%s: %s", who, fault);
    if (!in) return h->fail(PYA_ERR_ARG, -1, "NULL pointer passed to %s", who);
    if ((in->mz_type != PYA_F64 && in->mz_type != PYA_F32) || (in->intensity_type != PYA_F64 && in->intensity_type != PYA_F32))
        return h->fail(PYA_ERR_ARG, -1, "%s: element types %u / %u are neither PYA_F64 nor PYA_F32", who, in->mz_type, in->intensity_type);
    if (in->mz_type == PYA_F32 && in->intensity_type == PYA_F64)
        return h->fail(PYA_ERR_ARG, -1, "%s: float32 m/z beside float64 intensities is not supported", who);
    if (n_query == 0) return PYA_OK;
    if ((n_survey && (!in->mz || !in->intensity)) || !peak_off || !survey || !prec_mz || !prec_z || !win_lo || !win_hi || !purity || !over)
        return h->fail(PYA_ERR_ARG, -1, "NULL array passed to %s", who);
    if ((uintptr_t)purity & 7u) return h->fail(PYA_ERR_ARG, -1, "%s: the records are not 8-byte aligned", who);
    return PYA_OK;
}

extern "C" {

int pya_purity_spectra(pya_handle *h, const pya_typed_spectra *d_in, const int64_t *d_peak_off, uint64_t n_survey, uint64_t n_peaks,
                       const int64_t *d_survey, const double *d_prec_mz, const int32_t *d_prec_z, const double *d_win_lo, const double *d_win_hi,
                       uint64_t n_query, const pya_purity_params *params, void *hip_stream, pya_purity *d_purity, uint32_t *d_over) {
    if (!h) return PYA_ERR_ARG;
    const char *who = "pya_purity_spectra";
    if (const int rc = purity_check(h, who, d_in, d_peak_off, n_survey, d_survey, d_prec_mz, d_prec_z, d_win_lo, d_win_hi, n_query, params,
                                    d_purity, d_over))
        return rc;
    if (n_query == 0) return PYA_OK;
    HIPCHK(h, hipSetDevice(h->device));
    const int64_t cap = n_peaks > (uint64_t)INT64_MAX ? INT64_MAX : (int64_t)n_peaks;
    const int e = pya_launch_purity(d_in->mz, d_in->intensity, d_in->mz_type, d_in->intensity_type, d_peak_off, n_survey, cap, d_survey, d_prec_mz,
                                    d_prec_z, d_win_lo, d_win_hi, n_query, params, d_purity, d_over, (hipStream_t)hip_stream);
    if (e) return h->hip_fail((hipError_t)e, "purity launch");
    return PYA_OK;
}

int pya_purity_spectra_host(pya_handle *h, const pya_typed_spectra *in, const int64_t *peak_off, uint64_t n_survey, const int64_t *survey,
                            const double *prec_mz, const int32_t *prec_z, const double *win_lo, const double *win_hi, uint64_t n_query,
                            const pya_purity_params *params, pya_purity *purity, uint32_t *over) {
    if (!h) return PYA_ERR_ARG;
    const char *who = "pya_purity_spectra_host";
    if (const int rc = purity_check(h, who, in, peak_off, n_survey, survey, prec_mz, prec_z, win_lo, win_hi, n_query, params, purity, over))
        return rc;
    if (n_query == 0) return PYA_OK;
    if (peak_off[0] < 0) return h->fail(PYA_ERR_ARG, 0, "%s: peak_off[0] is negative", who);
    for (uint64_t s = 0; s < n_survey; s++)
        if (peak_off[s + 1] < peak_off[s]) return h->fail(PYA_ERR_ARG, (int64_t)s, "%s: peak_off descends at spectrum %llu", who, (unsigned long long)s);
    const size_t n_peaks = (size_t)peak_off[n_survey];
    const size_t mz_size = in->mz_type == PYA_F32 ? 4 : 8, in_size = in->intensity_type == PYA_F32 ? 4 : 8;
    HIPCHK(h, hipSetDevice(h->device));
    if (!h->run_stream) HIPCHK(h, hipStreamCreateWithFlags(&h->run_stream, hipStreamNonBlocking));
    const hipStream_t st = h->run_stream;
    DevBuf<unsigned char> d_mz, d_in;
    DevBuf<int64_t> d_off, d_survey;
    DevBuf<double> d_pm, d_lo, d_hi;
    DevBuf<int32_t> d_pz;
    DevBuf<pya_purity> d_purity;
    DevBuf<uint32_t> d_over;
    HIPCHK(h, d_mz.upload((const unsigned char *)in->mz, n_peaks * mz_size, st));
    HIPCHK(h, d_in.upload((const unsigned char *)in->intensity, n_peaks * in_size, st));
    HIPCHK(h, d_off.upload(peak_off, (size_t)n_survey + 1, st));
    HIPCHK(h, d_survey.upload(survey, (size_t)n_query, st));
    HIPCHK(h, d_pm.upload(prec_mz, (size_t)n_query, st));
    HIPCHK(h, d_pz.upload(prec_z, (size_t)n_query, st));
    HIPCHK(h, d_lo.upload(win_lo, (size_t)n_query, st));
    HIPCHK(h, d_hi.upload(win_hi, (size_t)n_query, st));
    HIPCHK(h, d_purity.alloc((size_t)n_query));
    HIPCHK(h, d_over.alloc(2));
    HIPCHK(h, hipMemsetAsync(d_over.p, 0, 2 * sizeof(uint32_t), st));
    const pya_typed_spectra t_in = {d_mz.p, d_in.p, in->mz_type, in->intensity_type};
    const int rc = pya_purity_spectra(h, &t_in, d_off.p, n_survey, n_peaks, d_survey.p, d_pm.p, d_pz.p, d_lo.p, d_hi.p, n_query, params, st,
                                      d_purity.p, d_over.p);
    if (rc) {
        (void)hipStreamSynchronize(st);                      /* (the buffers are freed on return) */
        return rc;
    }
    HIPCHK(h, hipMemcpyAsync(purity, d_purity.p, (size_t)n_query * sizeof(pya_purity), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipMemcpyAsync(over, d_over.p, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    return PYA_OK;
}

int pya_purity_gate(pya_handle *h, const pya_purity *d_purity, uint64_t n_rows, double threshold, uint32_t keep_unknown, const double *d_values,
                    uint32_t n_channels, double *d_out, uint8_t *d_select, void *hip_stream) {
    if (!h) return PYA_ERR_ARG;
    const char *who = "pya_purity_gate";
    if (n_channels > (uint32_t)PYA_QUANT_MAX_CHANNELS)
        return h->fail(PYA_ERR_ARG, -1, "%s: n_channels %u is not in 0 .. %d", who, n_channels, PYA_QUANT_MAX_CHANNELS);
    if (n_rows > kPurityMaxRows) return h->fail(PYA_ERR_ARG, -1, "%s: %llu rows are more than 2^32 - 2", who, (unsigned long long)n_rows);
    if (!(threshold >= 0. && threshold <= 1.)) return h->fail(PYA_ERR_ARG, -1, "%s: threshold %g is not in 0 .. 1", who, threshold);
    if (keep_unknown > 1u) return h->fail(PYA_ERR_ARG, -1, "%s: keep_unknown %u is neither 0 nor 1", who, keep_unknown);
    if (n_channels == 0 && !d_select) return h->fail(PYA_ERR_ARG, -1, "%s: neither a matrix nor select", who);
    if (((uintptr_t)d_purity & 7u) || (n_channels && (((uintptr_t)d_values & 7u) || ((uintptr_t)d_out & 7u))))
        return h->fail(PYA_ERR_ARG, -1, "%s: the records and the matrices are not 8-byte aligned", who);
    if (n_rows == 0) return PYA_OK;
    if (!d_purity || (n_channels && (!d_values || !d_out))) return h->fail(PYA_ERR_ARG, -1, "NULL array passed to %s", who);
    HIPCHK(h, hipSetDevice(h->device));
    const int e = pya_launch_purity_gate(d_purity, n_rows, threshold, keep_unknown, d_values, n_channels, d_out, d_select, (hipStream_t)hip_stream);
    if (e) return h->hip_fail((hipError_t)e, "purity gate launch");
    return PYA_OK;
}

}
