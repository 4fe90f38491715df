/* host_deisotope.cpp -- the C ABI of deisotoping (include/pyascore_hip.h: pya_deisotope_params; kernels: deisotope.hip): the
 * argument checks, the workspace layout and the host form.  The checks of the arrays and the host form itself are
 * host_transform.cpp's. */
#include "host_internal.h"

#include <cmath>

extern "C" int pya_launch_deisotope(const void *d_mz, const void *d_in, uint32_t mz_type, uint32_t in_type, const int64_t *d_peak_off,
                                    uint64_t n_spectra, const pya_deisotope_params *prm, int64_t cap_peaks, uint64_t *d_tiles, uint64_t *d_keep,
                                    void *d_out_mz, void *d_out_in, int64_t *d_new_off, uint32_t *d_over, hipStream_t stream);

const char *deiso_params_fault(const pya_deisotope_params *p) {
    if (!p) return "params is NULL";
    if (!std::isfinite(p->tol) || !(p->tol >= 0.)) return "tol is not a finite number >= 0";
    if (!std::isfinite(p->ratio0) || !std::isfinite(p->ratio_per_mz)) return "ratio0 or ratio_per_mz is not finite";
    if (p->max_charge < 1 || p->max_charge > PYA_DEISO_MAX_CHARGE) return "max_charge is not in 1 .. PYA_DEISO_MAX_CHARGE";
    if (p->reserved != 0) return "reserved is not 0";
    for (uint32_t z = 0; z < p->max_charge; z++) {
        if (!std::isfinite(p->spacing[z]) || !(p->spacing[z] > 0.)) return "a spacing is not finite and positive";
        if (z && !(p->spacing[z] < p->spacing[z - 1])) return "spacing is not strictly decreasing";
    }
    if (!(p->spacing[p->max_charge - 1] > 2. * p->tol)) return "the smallest spacing is not above 2 tol";
    return nullptr;
}

extern "C" {

/* the workspace in 8-byte words: the tile sums of the scan, then the keep words -- (n_peaks >> 6) + n_spectra of them hold every
 * spectrum's bits in words of its own (deisotope.hip), one more so that no spectra is still a workspace */
uint64_t pya_deisotope_workspace_bytes(uint64_t n_spectra, uint64_t n_peaks) {
    return 8ull * (xform_tile_words(n_spectra) + (n_peaks >> 6) + n_spectra + 1ull);
}

int pya_deisotope_spectra(pya_handle *h, const pya_typed_spectra *d_in, const int64_t *d_peak_off, uint64_t n_spectra,
                          const pya_deisotope_params *params, void *hip_stream, void *d_work, uint64_t work_bytes,
                          const pya_typed_spectra *d_out, int64_t *d_new_off, uint32_t *d_over) {
    if (!h) return PYA_ERR_ARG;
    const char *who = "pya_deisotope_spectra";
    if (const int rc = xform_check(h, who, deiso_params_fault(params), d_in, d_peak_off, n_spectra, d_out, d_new_off, d_over)) return rc;
    if (const int rc = xform_check_work(h, who, "pya_deisotope_workspace_bytes", n_spectra, d_work, work_bytes,
                                        pya_deisotope_workspace_bytes(n_spectra, 0)))
        return rc;
    HIPCHK(h, hipSetDevice(h->device));
    const hipStream_t st = (hipStream_t)hip_stream;
    if (n_spectra == 0) return xform_no_spectra(h, d_new_off, st);
    uint64_t *d_tiles = (uint64_t *)d_work;
    const int e = pya_launch_deisotope(d_in->mz, d_in->intensity, d_in->mz_type, d_in->intensity_type, d_peak_off, n_spectra, params,
                                       xform_keep_cap(n_spectra, work_bytes), d_tiles, d_tiles + xform_tile_words(n_spectra), (void *)d_out->mz,
                                       (void *)d_out->intensity, d_new_off, d_over, st);
    if (e) return h->hip_fail((hipError_t)e, "deisotope launch");
    return PYA_OK;
}

int pya_deisotope_spectra_host(pya_handle *h, const pya_typed_spectra *in, const int64_t *peak_off, uint64_t n_spectra,
                               const pya_deisotope_params *params, const pya_typed_spectra *out, int64_t *new_off, uint32_t *over) {
    if (!h) return PYA_ERR_ARG;
    const char *who = "pya_deisotope_spectra_host";
    if (const int rc = xform_check(h, who, deiso_params_fault(params), in, peak_off, n_spectra, out, new_off, over)) return rc;
    return xform_host(h, who, in, peak_off, n_spectra, out, new_off, over, nullptr, 0, pya_deisotope_workspace_bytes, [&](const XformDevice &d) {
        return pya_deisotope_spectra(h, d.in, d.peak_off, n_spectra, params, d.stream, d.work, d.work_bytes, d.out, d.new_off, d.over);
    });
}

}
