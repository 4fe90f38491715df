/* host_centroid.cpp -- the C ABI of centroiding (include/pyascore_hip.h: pya_centroid_params; kernels: centroid.hip): the
 * argument checks, the workspace layout and the host form.  The checks of the arrays and the host form itself are
 * host_transform.cpp's. */
#include "host_internal.h"

#include <cmath>

extern "C" int pya_launch_centroid(const void *d_mz, const void *d_in, uint32_t mz_type, uint32_t in_type, const int64_t *d_peak_off,
                                   uint64_t n_spectra, const uint8_t *d_select, const pya_centroid_params *prm, int64_t cap_peaks,
                                   uint64_t *d_tiles, uint64_t *d_keep, void *d_out_mz, void *d_out_in, int64_t *d_new_off, uint32_t *d_over,
                                   uint32_t passes, hipStream_t stream);

static_assert(sizeof(pya_centroid_params) == 40 && offsetof(pya_centroid_params, half_width) == 24 && offsetof(pya_centroid_params, reserved) == 32,
              "pya_centroid_params is a 40-byte record");

static uint32_t g_centroid_passes = 7u;                    /* (pya_debug_centroid_passes: a probe times MARK and PLACE apart) */

static const char *centroid_params_fault(const pya_centroid_params *p) {
    if (!p) return "params is NULL";
    if (!std::isfinite(p->gap0) || !(p->gap0 >= 0.) || !std::isfinite(p->gap_per_mz) || !(p->gap_per_mz >= 0.))
        return "gap0 or gap_per_mz is not a finite number >= 0";
    if (p->gap0 == 0. && p->gap_per_mz == 0.) return "gap0 and gap_per_mz are both 0";
    if (!std::isfinite(p->min_height) || !(p->min_height >= 0.)) return "min_height is not a finite number >= 0";
    if (p->half_width < 1 || p->half_width > PYA_CENTROID_MAX_HALF_WIDTH) return "half_width is not in 1 .. PYA_CENTROID_MAX_HALF_WIDTH";
    if (p->area > 1u) return "area is neither 0 nor 1";
    if (p->reserved != 0) return "reserved is not 0";
    return nullptr;
}

extern "C" {

void pya_debug_centroid_passes(uint32_t passes) { g_centroid_passes = passes & 7u; }

/* deisotoping's figure: the tile sums of the scan, then one keep bit per point in words that no two spectra share */
uint64_t pya_centroid_workspace_bytes(uint64_t n_spectra, uint64_t n_peaks) { return pya_deisotope_workspace_bytes(n_spectra, n_peaks); }

int pya_centroid_spectra(pya_handle *h, const pya_typed_spectra *d_in, const int64_t *d_peak_off, uint64_t n_spectra,
                         const uint8_t *d_select, const pya_centroid_params *params, void *hip_stream, void *d_work,
                         uint64_t work_bytes, const pya_typed_spectra *d_out, int64_t *d_new_off, uint32_t *d_over) {
    if (!h) return PYA_ERR_ARG;
    const char *who = "pya_centroid_spectra";
    if (const int rc = xform_check(h, who, centroid_params_fault(params), d_in, d_peak_off, n_spectra, d_out, d_new_off, d_over)) return rc;
    if (const int rc = xform_check_work(h, who, "pya_centroid_workspace_bytes", n_spectra, d_work, work_bytes,
                                        pya_centroid_workspace_bytes(n_spectra, 0)))
        return rc;
    HIPCHK(h, hipSetDevice(h->device));
    const hipStream_t st = (hipStream_t)hip_stream;
    if (n_spectra == 0) return xform_no_spectra(h, d_new_off, st);
    uint64_t *d_tiles = (uint64_t *)d_work;
    const int e = pya_launch_centroid(d_in->mz, d_in->intensity, d_in->mz_type, d_in->intensity_type, d_peak_off, n_spectra, d_select, params,
                                      xform_keep_cap(n_spectra, work_bytes), d_tiles, d_tiles + xform_tile_words(n_spectra), (void *)d_out->mz,
                                      (void *)d_out->intensity, d_new_off, d_over, g_centroid_passes, st);
    if (e) return h->hip_fail((hipError_t)e, "centroid launch");
    return PYA_OK;
}

int pya_centroid_spectra_host(pya_handle *h, const pya_typed_spectra *in, const int64_t *peak_off, uint64_t n_spectra,
                              const uint8_t *select, const pya_centroid_params *params, const pya_typed_spectra *out,
                              int64_t *new_off, uint32_t *over) {
    if (!h) return PYA_ERR_ARG;
    const char *who = "pya_centroid_spectra_host";
    if (const int rc = xform_check(h, who, centroid_params_fault(params), in, peak_off, n_spectra, out, new_off, over)) return rc;
    XformSide side[] = {{XformSide::SPECTRUM_IN, (void *)select, 1, nullptr}};
    return xform_host(h, who, in, peak_off, n_spectra, out, new_off, over, side, 1, pya_centroid_workspace_bytes, [&](const XformDevice &d) {
        return pya_centroid_spectra(h, d.in, d.peak_off, n_spectra, (const uint8_t *)side[0].dev, params, d.stream, d.work, d.work_bytes, d.out,
                                    d.new_off, d.over);
    });
}

}
