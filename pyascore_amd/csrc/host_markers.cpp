/* host_markers.cpp -- the C ABI of the marker-ion stage (include/pyascore_hip.h: pya_marker_params; kernel: markers.hip): the
 * argument checks and the host form.  The stage reads spectra and writes records: it has no out arrays, no new offsets and no
 * workspace, so it shares the wording of the transforms' refusals (host_transform.cpp) but not their frame, and its host form
 * is the small one below -- upload the spectra once, copy only the records back. */
#include "host_internal.h"

#include <cmath>

extern "C" int pya_launch_markers(const void *d_mz, const void *d_in, uint32_t mz_type, uint32_t in_type, const int64_t *d_peak_off,
                                  uint64_t n_spectra, int64_t cap_peaks, const double *d_prec_mz, const int32_t *d_prec_z,
                                  const pya_marker_params *prm, pya_marker *d_markers, pya_marker_spectrum *d_spectra, uint32_t *d_over,
                                  hipStream_t stream);

static_assert(sizeof(pya_marker_params) == 544 && offsetof(pya_marker_params, tol_ppm) == 8 && offsetof(pya_marker_params, value) == 16 &&
                  offsetof(pya_marker_params, loss_mask) == 528 && offsetof(pya_marker_params, n_targets) == 536 &&
                  offsetof(pya_marker_params, reserved) == 540,
              "pya_marker_params is a 544-byte record");
static_assert(sizeof(pya_marker) == 24 && offsetof(pya_marker, intensity) == 8 && offsetof(pya_marker, n_peaks) == 16 &&
                  offsetof(pya_marker, flags) == 20,
              "pya_marker is a 24-byte record");
static_assert(sizeof(pya_marker_spectrum) == 32 && offsetof(pya_marker_spectrum, base_peak) == 8 && offsetof(pya_marker_spectrum, hit) == 16 &&
                  offsetof(pya_marker_spectrum, n_peaks) == 24 && offsetof(pya_marker_spectrum, n_active) == 28,
              "pya_marker_spectrum is a 32-byte record");
static_assert(PYA_MARKER_MAX_TARGETS == 64, "one target per lane of a wavefront, one bit of hit and of loss_mask each");

static const uint64_t kMarkerMaxSpectra = 0xfffffffeull;

static const char *marker_params_fault(const pya_marker_params *p) {
    if (!p) return "params is NULL";
    if (!std::isfinite(p->tol) || !(p->tol >= 0.)) return "tol is not a finite number >= 0";
    if (!std::isfinite(p->tol_ppm) || !(p->tol_ppm >= 0.)) return "tol_ppm is not a finite number >= 0";
    if (p->n_targets < 1u || p->n_targets > PYA_MARKER_MAX_TARGETS) return "n_targets is not in 1 .. PYA_MARKER_MAX_TARGETS";
    if (p->n_targets < 64u && (p->loss_mask >> p->n_targets) != 0ull) return "loss_mask has a bit at or above n_targets";
    for (uint32_t t = 0; t < p->n_targets; t++) {
        const double v = p->value[t];
        if ((p->loss_mask >> t) & 1ull) {
            if (!std::isfinite(v) || !(v >= 0.)) return "the value of a loss target is not a finite number >= 0";
        } else if (!std::isfinite(v) || !(v > 0.))
            return "the value of a fixed target is not finite and positive";
    }
    if (p->reserved != 0) return "reserved is not 0";
    return nullptr;
}

/* everything either form refuses before anything is launched, in the order of the transforms' messages */
static int marker_check(pya_handle *h, const char *who, const pya_typed_spectra *in, const int64_t *peak_off, uint64_t n_spectra,
                        const double *prec_mz, const int32_t *prec_z, const pya_marker_params *params, const pya_marker *markers,
                        const pya_marker_spectrum *spectra, const uint32_t *over) {
    if (n_spectra > kMarkerMaxSpectra) return h->fail(PYA_ERR_ARG, -1, "%s: %llu spectra are more than 2^32 - 2", who, (unsigned long long)n_spectra);
    if (const char *fault = marker_params_fault(params)) return h->fail(PYA_ERR_ARG, -1, "%s: %s", who, fault);
    if (!in) return h->fail(PYA_ERR_ARG, -1, "NULL pointer passed to %s", who);
    if ((in->mz_type != PYA_F64 && in->mz_type != PYA_F32) || (in->intensity_type != PYA_F64 && in->intensity_type != PYA_F32))
        return h->fail(PYA_ERR_ARG, -1, "%s: element types %u / %u are neither PYA_F64 nor PYA_F32", who, in->mz_type, in->intensity_type);
    if (in->mz_type == PYA_F32 && in->intensity_type == PYA_F64)
        return h->fail(PYA_ERR_ARG, -1, "%s: float32 m/z beside float64 intensities is not supported", who);
    if (n_spectra == 0) return PYA_OK;
    if (!in->mz || !in->intensity || !peak_off || !markers || !over) return h->fail(PYA_ERR_ARG, -1, "NULL array passed to %s", who);
    if (params->loss_mask != 0ull && (!prec_mz || !prec_z))
        return h->fail(PYA_ERR_ARG, -1, "NULL precursor array passed to %s beside loss targets", who);
    if (((uintptr_t)markers & 7u) || ((uintptr_t)spectra & 7u)) return h->fail(PYA_ERR_ARG, -1, "%s: the records are not 8-byte aligned", who);
    return PYA_OK;
}

extern "C" {

int pya_marker_spectra(pya_handle *h, const pya_typed_spectra *d_in, const int64_t *d_peak_off, uint64_t n_spectra, uint64_t n_peaks,
                       const double *d_prec_mz, const int32_t *d_prec_z, const pya_marker_params *params, void *hip_stream,
                       pya_marker *d_markers, pya_marker_spectrum *d_spectra, uint32_t *d_over) {
    if (!h) return PYA_ERR_ARG;
    const char *who = "pya_marker_spectra";
    if (const int rc = marker_check(h, who, d_in, d_peak_off, n_spectra, d_prec_mz, d_prec_z, params, d_markers, d_spectra, d_over)) return rc;
    if (n_spectra == 0) return PYA_OK;
    HIPCHK(h, hipSetDevice(h->device));
    const int64_t cap = n_peaks > (uint64_t)INT64_MAX ? INT64_MAX : (int64_t)n_peaks;
    const int e = pya_launch_markers(d_in->mz, d_in->intensity, d_in->mz_type, d_in->intensity_type, d_peak_off, n_spectra, cap, d_prec_mz,
                                     d_prec_z, params, d_markers, d_spectra, d_over, (hipStream_t)hip_stream);
    if (e) return h->hip_fail((hipError_t)e, "markers launch");
    return PYA_OK;
}

int pya_marker_spectra_host(pya_handle *h, const pya_typed_spectra *in, const int64_t *peak_off, uint64_t n_spectra, const double *prec_mz,
                            const int32_t *prec_z, const pya_marker_params *params, pya_marker *markers, pya_marker_spectrum *spectra,
                            uint32_t *over) {
    if (!h) return PYA_ERR_ARG;
    const char *who = "pya_marker_spectra_host";
    if (const int rc = marker_check(h, who, in, peak_off, n_spectra, prec_mz, prec_z, params, markers, spectra, over)) return rc;
    if (n_spectra == 0) return PYA_OK;
    if (peak_off[0] < 0) return h->fail(PYA_ERR_ARG, 0, "%s: peak_off[0] is negative", who);
    for (uint64_t s = 0; s < n_spectra; s++)
        if (peak_off[s + 1] < peak_off[s]) return h->fail(PYA_ERR_ARG, (int64_t)s, "%s: peak_off descends at spectrum %llu", who, (unsigned long long)s);
    const size_t n_peaks = (size_t)peak_off[n_spectra];
    const size_t mz_size = in->mz_type == PYA_F32 ? 4 : 8, in_size = in->intensity_type == PYA_F32 ? 4 : 8;
    const size_t n_rec = (size_t)n_spectra * params->n_targets;
    const bool with_prec = params->loss_mask != 0ull;
    HIPCHK(h, hipSetDevice(h->device));
    if (!h->run_stream) HIPCHK(h, hipStreamCreateWithFlags(&h->run_stream, hipStreamNonBlocking));
    const hipStream_t st = h->run_stream;
    DevBuf<unsigned char> d_mz, d_in;
    DevBuf<int64_t> d_off;
    DevBuf<double> d_pm;
    DevBuf<int32_t> d_pz;
    DevBuf<pya_marker> d_markers;
    DevBuf<pya_marker_spectrum> d_spectra;
    DevBuf<uint32_t> d_over;
    HIPCHK(h, d_mz.upload((const unsigned char *)in->mz, n_peaks * mz_size, st));
    HIPCHK(h, d_in.upload((const unsigned char *)in->intensity, n_peaks * in_size, st));
    HIPCHK(h, d_off.upload(peak_off, (size_t)n_spectra + 1, st));
    if (with_prec) {
        HIPCHK(h, d_pm.upload(prec_mz, (size_t)n_spectra, st));
        HIPCHK(h, d_pz.upload(prec_z, (size_t)n_spectra, st));
    }
    HIPCHK(h, d_markers.alloc(n_rec));
    if (spectra) HIPCHK(h, d_spectra.alloc((size_t)n_spectra));
    HIPCHK(h, d_over.alloc(2));
    HIPCHK(h, hipMemsetAsync(d_over.p, 0, 2 * sizeof(uint32_t), st));
    const pya_typed_spectra t_in = {d_mz.p, d_in.p, in->mz_type, in->intensity_type};
    const int rc = pya_marker_spectra(h, &t_in, d_off.p, n_spectra, n_peaks, d_pm.p, d_pz.p, params, st, d_markers.p, d_spectra.p, d_over.p);
    if (rc) {
        (void)hipStreamSynchronize(st);                      /* (the buffers are freed on return) */
        return rc;
    }
    HIPCHK(h, hipMemcpyAsync(markers, d_markers.p, n_rec * sizeof(pya_marker), hipMemcpyDeviceToHost, st));
    if (spectra) HIPCHK(h, hipMemcpyAsync(spectra, d_spectra.p, (size_t)n_spectra * sizeof(pya_marker_spectrum), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipMemcpyAsync(over, d_over.p, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    return PYA_OK;
}

}
