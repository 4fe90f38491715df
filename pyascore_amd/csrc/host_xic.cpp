/* host_xic.cpp -- the C ABI of the precursor-XIC stage (include/pyascore_hip.h: pya_xic_params; kernels: xic.hip): the argument
 * checks, the survey check, the host form and the values column.  As the purity stage it reads survey spectra and writes
 * records -- no out arrays, no new offsets, no workspace --, so it shares the wording and the order of host_purity.cpp's
 * refusals, and its host form is the small one: upload the survey spectra and the queries once, copy only the records back. */
#include "host_internal.h"

#include <cmath>

extern "C" int pya_launch_xic_check(const void *d_mz, uint32_t mz_type, const int64_t *d_peak_off, uint64_t n_survey, int64_t cap_peaks,
                                    uint8_t *d_scan_ok, hipStream_t stream);
extern "C" int pya_launch_xic(const void *d_mz, const void *d_in, uint32_t mz_type, uint32_t in_type, const int64_t *d_peak_off, uint64_t n_survey,
                              int64_t cap_peaks, const double *d_rt, const uint8_t *d_scan_ok, const int64_t *d_seed, const int64_t *d_scan_lo,
                              const int64_t *d_scan_hi, const double *d_prec_mz, const int32_t *d_prec_z, uint64_t n_query,
                              const pya_xic_params *prm, pya_xic *d_xic, uint32_t *d_over, hipStream_t stream);
extern "C" int pya_launch_xic_values(const pya_xic *d_xic, uint64_t n, uint32_t which, double *d_out, hipStream_t stream);

static_assert(sizeof(pya_xic_params) == 40 && offsetof(pya_xic_params, tol_ppm) == 8 && offsetof(pya_xic_params, step) == 16 &&
                  offsetof(pya_xic_params, rise) == 24 && offsetof(pya_xic_params, isotopes) == 32 && offsetof(pya_xic_params, max_gap) == 36,
              "pya_xic_params is a 40-byte record");
static_assert(sizeof(pya_xic) == 64 && offsetof(pya_xic, apex_intensity) == 8 && offsetof(pya_xic, seed_intensity) == 16 &&
                  offsetof(pya_xic, sum_intensity) == 24 && offsetof(pya_xic, apex_scan) == 32 && offsetof(pya_xic, left_scan) == 36 &&
                  offsetof(pya_xic, right_scan) == 40 && offsetof(pya_xic, start_scan) == 44 && offsetof(pya_xic, n_points) == 48 &&
                  offsetof(pya_xic, n_present) == 52 && offsetof(pya_xic, iso_hit) == 56 && offsetof(pya_xic, flags) == 60,
              "pya_xic is a 64-byte record");
static_assert(PYA_XIC_MAX_SCANS == 64 && PYA_XIC_MAX_ISOTOPES == 3 && PYA_XIC_MAX_GAP == 8, "one scan per lane, one bit of iso_hit per isotope");

static const uint64_t kXicMaxRows = 0xfffffffeull;

static const char *xic_params_fault(const pya_xic_params *p) {
    if (!p) return "params is NULL";
    if (!std::isfinite(p->tol) || !(p->tol >= 0.)) return "tol is not a finite number >= 0";
    if (!std::isfinite(p->tol_ppm) || !(p->tol_ppm >= 0.)) return "tol_ppm is not a finite number >= 0";
    if (!std::isfinite(p->step) || !(p->step > 0.)) return "step is not finite and positive";
    if (!std::isfinite(p->rise) || !(p->rise >= 1.)) return "rise is not a finite number >= 1";
    if (p->isotopes > PYA_XIC_MAX_ISOTOPES) return "isotopes is not in 0 .. PYA_XIC_MAX_ISOTOPES";
    if (p->max_gap > PYA_XIC_MAX_GAP) return "max_gap is not in 0 .. PYA_XIC_MAX_GAP";
    return nullptr;
}

/* what every entry point that reads spectra refuses about them, in the order of the purity stage's messages */
static int xic_spectra_check(pya_handle *h, const char *who, const pya_typed_spectra *in, uint64_t n_survey) {
    if (n_survey > kXicMaxRows) return h->fail(PYA_ERR_ARG, -1, "%s: %llu survey spectra are more than 2^32 - 2", who, (unsigned long long)n_survey);
    if (!in) return h->fail(PYA_ERR_ARG, -1, "NULL pointer passed to %s", who);
    if ((in->mz_type != PYA_F64 && in->mz_type != PYA_F32) || (in->intensity_type != PYA_F64 && in->intensity_type != PYA_F32))
        return h->fail(PYA_ERR_ARG, -1, "%s: element types %u / %u are neither PYA_F64 nor PYA_F32", who, in->mz_type, in->intensity_type);
    if (in->mz_type == PYA_F32 && in->intensity_type == PYA_F64)
        return h->fail(PYA_ERR_ARG, -1, "%s: float32 m/z beside float64 intensities is not supported", who);
    return PYA_OK;
}

/* everything either form of the trace refuses before anything is launched; scan_ok may be NULL where need_ok is false */
static int xic_check(pya_handle *h, const char *who, const pya_typed_spectra *in, const int64_t *peak_off, uint64_t n_survey, const double *rt,
                     const uint8_t *scan_ok, bool need_ok, const int64_t *seed, const int64_t *scan_lo, const int64_t *scan_hi,
                     const double *prec_mz, const int32_t *prec_z, uint64_t n_query, const pya_xic_params *params, const pya_xic *xic,
                     const uint32_t *over) {
    if (n_query > kXicMaxRows) return h->fail(PYA_ERR_ARG, -1, "%s: %llu queries are more than 2^32 - 2", who, (unsigned long long)n_query);
    if (n_survey > kXicMaxRows) return h->fail(PYA_ERR_ARG, -1, "%s: %llu survey spectra are more than 2^32 - 2", who, (unsigned long long)n_survey);
    if (const char *fault = xic_params_fault(params)) return h->fail(PYA_ERR_ARG, -1, "%s: %s", who, fault);
    if (const int rc = xic_spectra_check(h, who, in, n_survey)) return rc;
    if (n_query == 0) return PYA_OK;
    if ((n_survey && (!in->mz || !in->intensity || !rt || (need_ok && !scan_ok))) || !peak_off || !seed || !scan_lo || !scan_hi || !prec_mz ||
        !prec_z || !xic || !over)
        return h->fail(PYA_ERR_ARG, -1, "NULL array passed to %s", who);
    if ((uintptr_t)xic & 7u) return h->fail(PYA_ERR_ARG, -1, "%s: the records are not 8-byte aligned", who);
    return PYA_OK;
}

static int64_t xic_cap(uint64_t n_peaks) { return n_peaks > (uint64_t)INT64_MAX ? INT64_MAX : (int64_t)n_peaks; }

extern "C" {

int pya_xic_survey_check(pya_handle *h, const pya_typed_spectra *d_in, const int64_t *d_peak_off, uint64_t n_survey, uint64_t n_peaks,
                         void *hip_stream, uint8_t *d_scan_ok) {
    if (!h) return PYA_ERR_ARG;
    const char *who = "pya_xic_survey_check";
    if (const int rc = xic_spectra_check(h, who, d_in, n_survey)) return rc;
    if (n_survey == 0) return PYA_OK;
    if (!d_in->mz || !d_peak_off || !d_scan_ok) return h->fail(PYA_ERR_ARG, -1, "NULL array passed to %s", who);
    HIPCHK(h, hipSetDevice(h->device));
    const int e = pya_launch_xic_check(d_in->mz, d_in->mz_type, d_peak_off, n_survey, xic_cap(n_peaks), d_scan_ok, (hipStream_t)hip_stream);
    if (e) return h->hip_fail((hipError_t)e, "xic survey check launch");
    return PYA_OK;
}

int pya_xic_spectra(pya_handle *h, const pya_typed_spectra *d_in, const int64_t *d_peak_off, uint64_t n_survey, uint64_t n_peaks,
                    const double *d_rt, const uint8_t *d_scan_ok, const int64_t *d_seed, const int64_t *d_scan_lo, const int64_t *d_scan_hi,
                    const double *d_prec_mz, const int32_t *d_prec_z, uint64_t n_query, const pya_xic_params *params, void *hip_stream,
                    pya_xic *d_xic, uint32_t *d_over) {
    if (!h) return PYA_ERR_ARG;
    const char *who = "pya_xic_spectra";
    if (const int rc = xic_check(h, who, d_in, d_peak_off, n_survey, d_rt, d_scan_ok, true, d_seed, d_scan_lo, d_scan_hi, d_prec_mz, d_prec_z,
                                 n_query, params, d_xic, d_over))
        return rc;
    if (n_query == 0) return PYA_OK;
    HIPCHK(h, hipSetDevice(h->device));
    const int e = pya_launch_xic(d_in->mz, d_in->intensity, d_in->mz_type, d_in->intensity_type, d_peak_off, n_survey, xic_cap(n_peaks), d_rt,
                                 d_scan_ok, d_seed, d_scan_lo, d_scan_hi, d_prec_mz, d_prec_z, n_query, params, d_xic, d_over,
                                 (hipStream_t)hip_stream);
    if (e) return h->hip_fail((hipError_t)e, "xic launch");
    return PYA_OK;
}

int pya_xic_spectra_host(pya_handle *h, const pya_typed_spectra *in, const int64_t *peak_off, uint64_t n_survey, const double *rt,
                         const uint8_t *scan_ok, const int64_t *seed, const int64_t *scan_lo, const int64_t *scan_hi, const double *prec_mz,
                         const int32_t *prec_z, uint64_t n_query, const pya_xic_params *params, pya_xic *xic, uint32_t *over) {
    if (!h) return PYA_ERR_ARG;
    const char *who = "pya_xic_spectra_host";
    if (const int rc = xic_check(h, who, in, peak_off, n_survey, rt, scan_ok, false, seed, scan_lo, scan_hi, prec_mz, prec_z, n_query, params, xic,
                                 over))
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
    DevBuf<unsigned char> d_mz, d_in, d_ok;
    DevBuf<int64_t> d_off, d_seed, d_lo, d_hi;
    DevBuf<double> d_rt, d_pm;
    DevBuf<int32_t> d_pz;
    DevBuf<pya_xic> d_xic;
    DevBuf<uint32_t> d_over;
    HIPCHK(h, d_mz.upload((const unsigned char *)in->mz, n_peaks * mz_size, st));
    HIPCHK(h, d_in.upload((const unsigned char *)in->intensity, n_peaks * in_size, st));
    HIPCHK(h, d_off.upload(peak_off, (size_t)n_survey + 1, st));
    HIPCHK(h, d_rt.upload(rt, (size_t)n_survey, st));
    HIPCHK(h, d_seed.upload(seed, (size_t)n_query, st));
    HIPCHK(h, d_lo.upload(scan_lo, (size_t)n_query, st));
    HIPCHK(h, d_hi.upload(scan_hi, (size_t)n_query, st));
    HIPCHK(h, d_pm.upload(prec_mz, (size_t)n_query, st));
    HIPCHK(h, d_pz.upload(prec_z, (size_t)n_query, st));
    HIPCHK(h, d_xic.alloc((size_t)n_query));
    HIPCHK(h, d_over.alloc(2));
    HIPCHK(h, hipMemsetAsync(d_over.p, 0, 2 * sizeof(uint32_t), st));
    const pya_typed_spectra t_in = {d_mz.p, d_in.p, in->mz_type, in->intensity_type};
    int rc = PYA_OK;
    if (scan_ok) {
        HIPCHK(h, d_ok.upload(scan_ok, (size_t)n_survey, st));
    } else {
        HIPCHK(h, d_ok.alloc((size_t)n_survey));
        rc = pya_xic_survey_check(h, &t_in, d_off.p, n_survey, n_peaks, st, d_ok.p);
    }
    if (!rc)
        rc = pya_xic_spectra(h, &t_in, d_off.p, n_survey, n_peaks, d_rt.p, d_ok.p, d_seed.p, d_lo.p, d_hi.p, d_pm.p, d_pz.p, n_query, params, st,
                             d_xic.p, d_over.p);
    if (rc) {
        (void)hipStreamSynchronize(st);                      /* (the buffers are freed on return) */
        return rc;
    }
    HIPCHK(h, hipMemcpyAsync(xic, d_xic.p, (size_t)n_query * sizeof(pya_xic), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipMemcpyAsync(over, d_over.p, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    return PYA_OK;
}

int pya_xic_values(pya_handle *h, const pya_xic *d_xic, uint64_t n, uint32_t which, void *hip_stream, double *d_out) {
    if (!h) return PYA_ERR_ARG;
    const char *who = "pya_xic_values";
    if (which > PYA_XIC_SUM) return h->fail(PYA_ERR_ARG, -1, "%s: which = %u is not in 0 .. 3", who, which);
    if (n > kXicMaxRows) return h->fail(PYA_ERR_ARG, -1, "%s: %llu records are more than 2^32 - 2", who, (unsigned long long)n);
    if (((uintptr_t)d_xic & 7u) || ((uintptr_t)d_out & 7u)) return h->fail(PYA_ERR_ARG, -1, "%s: the records and the column are not 8-byte aligned", who);
    if (n == 0) return PYA_OK;
    if (!d_xic || !d_out) return h->fail(PYA_ERR_ARG, -1, "NULL array passed to %s", who);
    HIPCHK(h, hipSetDevice(h->device));
    const int e = pya_launch_xic_values(d_xic, n, which, d_out, (hipStream_t)hip_stream);
    if (e) return h->hip_fail((hipError_t)e, "xic values launch");
    return PYA_OK;
}

}
