/* host_decharge.cpp -- the C ABI of charge deconvolution (include/pyascore_hip.h: pya_decharge_params; kernels: decharge.hip):
 * the argument checks, the workspace layout and the host form.  The checks of the arrays and the host form itself are
 * host_transform.cpp's, the check of the deisotoping rule inside the parameters is host_deisotope.cpp's. */
#include "host_internal.h"

#include <cmath>

extern "C" int pya_launch_decharge(const void *d_mz, const void *d_in, uint32_t mz_type, uint32_t in_type, const int64_t *d_peak_off,
                                   uint64_t n_spectra, const pya_decharge_params *prm, int64_t cap_peaks, uint64_t *d_tiles, uint64_t *d_regions,
                                   uint64_t region_words, void *d_out_mz, void *d_out_in, int64_t *d_new_off, uint8_t *d_charge, uint32_t *d_over,
                                   uint32_t passes, hipStream_t stream);

static_assert(sizeof(pya_decharge_params) == 112 && offsetof(pya_decharge_params, carrier) == 96, "pya_decharge_params is a 112-byte record");

static uint32_t g_dechg_passes = 7u;                       /* (pya_debug_decharge_passes: a probe times MARK and PLACE apart) */

/* The workspace in 8-byte words.  Peaks are lent in groups of 64: a group costs three words (one each of the keep, moved and
 * before regions of decharge.hip) and 128 words of list (two an entry), 131 together.  Beside the groups: the tile sums of the
 * scan, per spectrum one word in each of the three regions and one moved count, and one word more in each region so that word
 * (cap >> 6) + n_spectra - 1 + 1 exists.  G groups hold cap = 64 G peaks; n_peaks peaks need (n_peaks >> 6) + 1 groups. */
static uint64_t dechg_fixed_words(uint64_t n_spectra) { return xform_tile_words(n_spectra) + 4ull * n_spectra + 3ull; }

static int dechg_check(pya_handle *h, const char *who, const pya_typed_spectra *in, const int64_t *peak_off, uint64_t n_spectra,
                       const pya_decharge_params *params, const pya_typed_spectra *out, const int64_t *new_off, const uint32_t *over) {
    if (!params) return h->fail(PYA_ERR_ARG, -1, "%s: params is NULL", who);
    const int rc = xform_check(h, who, deiso_params_fault(&params->iso), in, peak_off, n_spectra, out, new_off, over);
    if (rc) return rc;
    if (!std::isfinite(params->carrier) || !(params->carrier > 0.)) return h->fail(PYA_ERR_ARG, -1, "%s: carrier is not finite and positive", who);
    if (!std::isfinite(params->witness) || !(params->witness >= 0.)) return h->fail(PYA_ERR_ARG, -1, "%s: witness is not a finite number >= 0", who);
    return PYA_OK;
}

extern "C" {

uint64_t pya_decharge_workspace_bytes(uint64_t n_spectra, uint64_t n_peaks) {
    return 8ull * (dechg_fixed_words(n_spectra) + 131ull * ((n_peaks >> 6) + 1ull));
}

void pya_debug_decharge_passes(uint32_t passes) { g_dechg_passes = passes & 7u; }

int pya_decharge_spectra(pya_handle *h, const pya_typed_spectra *d_in, const int64_t *d_peak_off, uint64_t n_spectra,
                         const pya_decharge_params *params, void *hip_stream, void *d_work, uint64_t work_bytes,
                         const pya_typed_spectra *d_out, int64_t *d_new_off, uint8_t *d_charge, uint32_t *d_over) {
    if (!h) return PYA_ERR_ARG;
    const char *who = "pya_decharge_spectra";
    if (const int rc = dechg_check(h, who, d_in, d_peak_off, n_spectra, params, d_out, d_new_off, d_over)) return rc;
    if (const int rc = xform_check_work(h, who, "pya_decharge_workspace_bytes", n_spectra, d_work, work_bytes,
                                        pya_decharge_workspace_bytes(n_spectra, 0)))
        return rc;
    if (n_spectra && d_charge && (d_charge == d_in->mz || d_charge == d_in->intensity || d_charge == d_out->mz || d_charge == d_out->intensity))
        return h->fail(PYA_ERR_ARG, -1, "%s: d_charge is one of the spectrum arrays", who);
    HIPCHK(h, hipSetDevice(h->device));
    const hipStream_t st = (hipStream_t)hip_stream;
    if (n_spectra == 0) return xform_no_spectra(h, d_new_off, st);
    /* the groups of 64 peaks the workspace lent has room for (>= 1: checked above; no more than 2^50, so that nothing overflows) */
    uint64_t groups = (work_bytes / 8ull - dechg_fixed_words(n_spectra)) / 131ull;
    if (groups > (1ull << 50)) groups = 1ull << 50;
    const int64_t cap_peaks = (int64_t)(groups << 6);
    const uint64_t region_words = groups + n_spectra + 1ull;
    uint64_t *d_tiles = (uint64_t *)d_work;
    const int e = pya_launch_decharge(d_in->mz, d_in->intensity, d_in->mz_type, d_in->intensity_type, d_peak_off, n_spectra, params, cap_peaks,
                                      d_tiles, d_tiles + xform_tile_words(n_spectra), region_words, (void *)d_out->mz, (void *)d_out->intensity,
                                      d_new_off, d_charge, d_over, g_dechg_passes, st);
    if (e) return h->hip_fail((hipError_t)e, "decharge launch");
    return PYA_OK;
}

int pya_decharge_spectra_host(pya_handle *h, const pya_typed_spectra *in, const int64_t *peak_off, uint64_t n_spectra,
                              const pya_decharge_params *params, const pya_typed_spectra *out, int64_t *new_off, uint8_t *charge,
                              uint32_t *over) {
    if (!h) return PYA_ERR_ARG;
    const char *who = "pya_decharge_spectra_host";
    if (const int rc = dechg_check(h, who, in, peak_off, n_spectra, params, out, new_off, over)) return rc;
    XformSide side[] = {{XformSide::PEAK_OUT, charge, 1, nullptr}};
    return xform_host(h, who, in, peak_off, n_spectra, out, new_off, over, side, 1, pya_decharge_workspace_bytes, [&](const XformDevice &d) {
        return pya_decharge_spectra(h, d.in, d.peak_off, n_spectra, params, d.stream, d.work, d.work_bytes, d.out, d.new_off,
                                    (uint8_t *)side[0].dev, d.over);
    });
}

}
