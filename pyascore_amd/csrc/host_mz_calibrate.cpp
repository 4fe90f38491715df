/* host_mz_calibrate.cpp -- the C ABI of the fragment m/z recalibration (include/pyascore_hip.h: pya_mz_calibration; kernels:
 * mz_calibrate.hip): the argument checks of the fit and of the apply, the host form of the fit and the batch loan.  The
 * batch path itself is host_batch.cpp's. */
#include "host_internal.h"

#include <cmath>

static int fit_check(pya_handle *h, const char *who, const void *table, uint64_t n_slots, const pya_mz_profile_params *prm, uint32_t min_ions,
                     const void *cal) {
    const int rc = mzp_check(h, who, n_slots, prm);
    if (rc) return rc;
    if (min_ions == 0) return h->fail(PYA_ERR_ARG, -1, "%s: min_ions must be at least 1", who);
    if (n_slots && (!table || !cal)) return h->fail(PYA_ERR_ARG, -1, "NULL array passed to %s", who);
    return PYA_OK;
}

static bool knots_ok(const pya_mz_calibration &c) {
    for (int b = 0; b < PYA_MZP_BANDS; b++)
        if (!(std::fabs(c.ppm[b]) <= (double)PYA_MZC_MAX_PPM)) return false;      /* (NaN and inf fail the comparison) */
    return true;
}

extern "C" {

int pya_mz_profile_fit(pya_handle *h, const pya_mz_profile *d_table, uint64_t n_slots, const pya_mz_profile_params *params, uint32_t min_ions,
                       void *hip_stream, pya_mz_calibration *d_cal) {
    if (!h) return PYA_ERR_ARG;
    const int rc = fit_check(h, "pya_mz_profile_fit", d_table, n_slots, params, min_ions, d_cal);
    if (rc) return rc;
    if (n_slots == 0) return PYA_OK;
    HIPCHK(h, hipSetDevice(h->device));
    const int e = pya_launch_mz_fit(d_table, n_slots, params->inv_ppm, min_ions, d_cal, (hipStream_t)hip_stream);
    if (e) return h->hip_fail((hipError_t)e, "m/z calibration fit launch");
    return PYA_OK;
}

int pya_mz_profile_fit_host(pya_handle *h, const pya_mz_profile *table, uint64_t n_slots, const pya_mz_profile_params *params,
                            uint32_t min_ions, pya_mz_calibration *out) {
    if (!h) return PYA_ERR_ARG;
    const int rc_arg = fit_check(h, "pya_mz_profile_fit_host", table, n_slots, params, min_ions, out);
    if (rc_arg) return rc_arg;
    if (n_slots == 0) return PYA_OK;
    HIPCHK(h, hipSetDevice(h->device));
    if (!h->run_stream) HIPCHK(h, hipStreamCreateWithFlags(&h->run_stream, hipStreamNonBlocking));
    const hipStream_t st = h->run_stream;
    DevBuf<pya_mz_profile> d_table;
    DevBuf<pya_mz_calibration> d_cal;
    HIPCHK(h, d_table.upload(table, (size_t)n_slots, st));
    HIPCHK(h, d_cal.alloc((size_t)n_slots));
    const int rc = pya_mz_profile_fit(h, d_table.p, n_slots, params, min_ions, st, d_cal.p);
    if (rc) {
        (void)hipStreamSynchronize(st);                      /* (the buffers are freed on return) */
        return rc;
    }
    HIPCHK(h, hipMemcpyAsync(out, d_cal.p, (size_t)n_slots * sizeof(pya_mz_calibration), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    return PYA_OK;
}

int pya_recalibrate_spectra(pya_handle *h, const pya_typed_spectra *d_spectra, const int64_t *d_peak_off, uint64_t n_spectra,
                            const int32_t *d_run, const pya_mz_calibration *d_cal, uint64_t n_slots, double inv_band, void *hip_stream,
                            void *d_mz_out, uint32_t *d_over) {
    if (!h) return PYA_ERR_ARG;
    if (n_spectra > 0xfffffffeull)
        return h->fail(PYA_ERR_ARG, -1, "pya_recalibrate_spectra: %llu spectra are more than 2^32 - 2", (unsigned long long)n_spectra);
    if (n_slots > 0x7fffffffull)
        return h->fail(PYA_ERR_ARG, -1, "pya_recalibrate_spectra: %llu slots are more than an int32 slot can name", (unsigned long long)n_slots);
    if (!std::isfinite(inv_band) || !(inv_band > 0.)) return h->fail(PYA_ERR_ARG, -1, "pya_recalibrate_spectra: inv_band is not a finite positive number");
    if (d_spectra && d_spectra->mz_type != PYA_F64 && d_spectra->mz_type != PYA_F32)
        return h->fail(PYA_ERR_ARG, -1, "pya_recalibrate_spectra: mz_type %u is neither PYA_F64 nor PYA_F32", d_spectra->mz_type);
    if (n_spectra == 0) return PYA_OK;
    if (!d_spectra || !d_spectra->mz || !d_peak_off || !d_mz_out || !d_over || (n_slots && !d_cal))
        return h->fail(PYA_ERR_ARG, -1, "NULL device pointer passed to pya_recalibrate_spectra");
    HIPCHK(h, hipSetDevice(h->device));
    const int e = pya_launch_mz_apply(d_spectra->mz, d_spectra->mz_type, d_peak_off, n_spectra, d_run, d_cal, n_slots, inv_band, d_mz_out, d_over,
                                      (hipStream_t)hip_stream);
    if (e) return h->hip_fail((hipError_t)e, "m/z recalibration launch");
    return PYA_OK;
}

int pya_set_recalibration(pya_handle *h, const int32_t *run, uint64_t n_psm, const pya_mz_calibration *cal, uint64_t n_slots, double inv_band) {
    if (!h) return PYA_ERR_ARG;
    h->recal_loan = pya_handle::RecalLoan{};
    if (n_psm > 0x7fffffffull) return h->fail(PYA_ERR_ARG, -1, "pya_set_recalibration: %llu PSMs are more than 2^31 - 1", (unsigned long long)n_psm);
    if (n_slots > 0x7fffffffull)
        return h->fail(PYA_ERR_ARG, -1, "pya_set_recalibration: %llu slots are more than an int32 slot can name", (unsigned long long)n_slots);
    if (!std::isfinite(inv_band) || !(inv_band > 0.)) return h->fail(PYA_ERR_ARG, -1, "pya_set_recalibration: inv_band is not a finite positive number");
    if (n_slots && !cal) return h->fail(PYA_ERR_ARG, -1, "NULL calibration passed to pya_set_recalibration");
    for (uint64_t s = 0; s < n_slots; s++)
        if (!knots_ok(cal[s]))
            return h->fail(PYA_ERR_ARG, (int64_t)s, "pya_set_recalibration: slot %llu has a knot that is not finite or beyond %d ppm",
                           (unsigned long long)s, PYA_MZC_MAX_PPM);
    h->recal_loan.run = run;
    h->recal_loan.n_psm = n_psm;
    h->recal_loan.n_slots = n_slots;
    h->recal_loan.inv_band = inv_band;
    if (n_slots) h->recal_loan.cal.assign(cal, cal + n_slots);
    h->recal_loan.set = true;
    return PYA_OK;
}

}
