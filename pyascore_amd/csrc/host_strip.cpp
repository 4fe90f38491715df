/* host_strip.cpp -- the C ABI of precursor stripping (include/pyascore_hip.h: pya_strip_params; kernels: strip.hip and
 * deisotope.hip's fill): the argument checks, the workspace layout and the host form.  The checks of the arrays and the host
 * form itself are host_transform.cpp's. */
#include "host_internal.h"

#include <cmath>

extern "C" int pya_launch_strip(const void *d_mz, const void *d_in, uint32_t mz_type, uint32_t in_type, const int64_t *d_peak_off,
                                uint64_t n_spectra, const double *d_prec_mz, const int32_t *d_prec_z, const pya_strip_params *prm,
                                int64_t cap_peaks, uint64_t *d_tiles, uint64_t *d_keep, void *d_out_mz, void *d_out_in, int64_t *d_new_off,
                                pya_strip_report *d_report, uint32_t *d_over, hipStream_t stream);

static_assert(sizeof(pya_strip_params) == 112 && offsetof(pya_strip_params, loss) == 32 && offsetof(pya_strip_params, n_loss) == 96,
              "pya_strip_params is a 112-byte record");
static_assert(sizeof(pya_strip_report) == 16, "pya_strip_report is a 16-byte record");
static_assert(PYA_STRIP_MAX_CHARGE * (PYA_STRIP_MAX_LOSS + 1) == 64, "one window per lane of a wavefront, one bit of hit each");

static const char *strip_params_fault(const pya_strip_params *p) {
    if (!p) return "params is NULL";
    if (!std::isfinite(p->tol) || !(p->tol >= 0.)) return "tol is not a finite number >= 0";
    if (!std::isfinite(p->step) || !(p->step > 0.)) return "step is not finite and positive";
    if (std::isnan(p->mz_lo) || std::isnan(p->mz_hi) || !(p->mz_lo <= p->mz_hi)) return "mz_lo and mz_hi are not numbers with mz_lo <= mz_hi";
    if (p->n_loss > PYA_STRIP_MAX_LOSS) return "n_loss is above PYA_STRIP_MAX_LOSS";
    if (p->loss[0] != 0.) return "loss[0] is not 0";
    for (uint32_t l = 1; l <= p->n_loss; l++)
        if (!std::isfinite(p->loss[l]) || !(p->loss[l] >= 0.)) return "a loss is not a finite number >= 0";
    if (p->reduced > 1u) return "reduced is neither 0 nor 1";
    if (p->isotopes > PYA_STRIP_MAX_ISOTOPES) return "isotopes is above PYA_STRIP_MAX_ISOTOPES";
    if (p->reserved != 0) return "reserved is not 0";
    return nullptr;
}

static int strip_check(pya_handle *h, const char *who, const pya_typed_spectra *in, const int64_t *peak_off, uint64_t n_spectra,
                       const double *prec_mz, const int32_t *prec_z, const pya_strip_params *params, const pya_typed_spectra *out,
                       const int64_t *new_off, const pya_strip_report *report, const uint32_t *over) {
    const int rc = xform_check(h, who, strip_params_fault(params), in, peak_off, n_spectra, out, new_off, over);
    if (rc) return rc;
    if (n_spectra && (!prec_mz || !prec_z)) return h->fail(PYA_ERR_ARG, -1, "NULL precursor array passed to %s", who);
    if (n_spectra && ((uintptr_t)report & 7u)) return h->fail(PYA_ERR_ARG, -1, "%s: the report is not 8-byte aligned", who);
    return PYA_OK;
}

extern "C" {

/* the workspace in 8-byte words, laid out as deisotoping's (the fill kernel is its): the tile sums of the scan, then the keep
 * words -- (n_peaks >> 6) + n_spectra of them, one more so that no spectra is still a workspace */
uint64_t pya_strip_workspace_bytes(uint64_t n_spectra, uint64_t n_peaks) {
    return 8ull * (xform_tile_words(n_spectra) + (n_peaks >> 6) + n_spectra + 1ull);
}

int pya_strip_spectra(pya_handle *h, const pya_typed_spectra *d_in, const int64_t *d_peak_off, uint64_t n_spectra,
                      const double *d_prec_mz, const int32_t *d_prec_z, const pya_strip_params *params, void *hip_stream,
                      void *d_work, uint64_t work_bytes, const pya_typed_spectra *d_out, int64_t *d_new_off,
                      pya_strip_report *d_report, uint32_t *d_over) {
    if (!h) return PYA_ERR_ARG;
    const char *who = "pya_strip_spectra";
    if (const int rc = strip_check(h, who, d_in, d_peak_off, n_spectra, d_prec_mz, d_prec_z, params, d_out, d_new_off, d_report, d_over)) return rc;
    if (const int rc = xform_check_work(h, who, "pya_strip_workspace_bytes", n_spectra, d_work, work_bytes, pya_strip_workspace_bytes(n_spectra, 0)))
        return rc;
    HIPCHK(h, hipSetDevice(h->device));
    const hipStream_t st = (hipStream_t)hip_stream;
    if (n_spectra == 0) return xform_no_spectra(h, d_new_off, st);
    uint64_t *d_tiles = (uint64_t *)d_work;
    const int e = pya_launch_strip(d_in->mz, d_in->intensity, d_in->mz_type, d_in->intensity_type, d_peak_off, n_spectra, d_prec_mz, d_prec_z,
                                   params, xform_keep_cap(n_spectra, work_bytes), d_tiles, d_tiles + xform_tile_words(n_spectra),
                                   (void *)d_out->mz, (void *)d_out->intensity, d_new_off, d_report, d_over, st);
    if (e) return h->hip_fail((hipError_t)e, "strip launch");
    return PYA_OK;
}

int pya_strip_spectra_host(pya_handle *h, const pya_typed_spectra *in, const int64_t *peak_off, uint64_t n_spectra,
                           const double *prec_mz, const int32_t *prec_z, const pya_strip_params *params,
                           const pya_typed_spectra *out, int64_t *new_off, pya_strip_report *report, uint32_t *over) {
    if (!h) return PYA_ERR_ARG;
    const char *who = "pya_strip_spectra_host";
    if (const int rc = strip_check(h, who, in, peak_off, n_spectra, prec_mz, prec_z, params, out, new_off, report, over)) return rc;
    XformSide side[] = {{XformSide::SPECTRUM_IN, (void *)prec_mz, sizeof(double), nullptr},
                        {XformSide::SPECTRUM_IN, (void *)prec_z, sizeof(int32_t), nullptr},
                        {XformSide::SPECTRUM_OUT, report, sizeof(pya_strip_report), nullptr}};
    return xform_host(h, who, in, peak_off, n_spectra, out, new_off, over, side, 3, pya_strip_workspace_bytes, [&](const XformDevice &d) {
        return pya_strip_spectra(h, d.in, d.peak_off, n_spectra, (const double *)side[0].dev, (const int32_t *)side[1].dev, params, d.stream,
                                 d.work, d.work_bytes, d.out, d.new_off, (pya_strip_report *)side[2].dev, d.over);
    });
}

}
