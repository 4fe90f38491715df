/* host_centroid.cpp -- the C ABI of centroiding (include/pyascore_hip.h: pya_centroid_params; kernels: centroid.hip): the
 * argument checks, the workspace layout and the host form.  The checks of the arrays are host_deisotope.cpp's. */
#include "host_internal.h"

#include <cmath>

extern "C" int pya_launch_centroid(const void *d_mz, const void *d_in, uint32_t mz_type, uint32_t in_type, const int64_t *d_peak_off,
                                   uint64_t n_spectra, const uint8_t *d_select, const pya_centroid_params *prm, int64_t cap_peaks,
                                   uint64_t *d_tiles, uint64_t *d_keep, void *d_out_mz, void *d_out_in, int64_t *d_new_off, uint32_t *d_over,
                                   uint32_t passes, hipStream_t stream);

static_assert(sizeof(pya_centroid_params) == 40 && offsetof(pya_centroid_params, half_width) == 24 && offsetof(pya_centroid_params, reserved) == 32,
              "pya_centroid_params is a 40-byte record");

static const uint64_t kCentroidMaxSpectra = 0xfffffffeull;
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

static int centroid_check(pya_handle *h, const char *who, const pya_typed_spectra *in, const int64_t *peak_off, uint64_t n_spectra,
                          const pya_centroid_params *params, const pya_typed_spectra *out, const int64_t *new_off, const uint32_t *over) {
    if (n_spectra > kCentroidMaxSpectra) return h->fail(PYA_ERR_ARG, -1, "%s: %llu spectra are more than 2^32 - 2", who, (unsigned long long)n_spectra);
    if (const char *why = centroid_params_fault(params)) return h->fail(PYA_ERR_ARG, -1, "%s: %s", who, why);
    return deiso_check_arrays(h, who, in, peak_off, n_spectra, out, new_off, over);
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
    const int rc = centroid_check(h, who, d_in, d_peak_off, n_spectra, params, d_out, d_new_off, d_over);
    if (rc) return rc;
    if (n_spectra && (!d_work || ((uintptr_t)d_work & 7u))) return h->fail(PYA_ERR_ARG, -1, "%s: the workspace is NULL or not 8-byte aligned", who);
    if (n_spectra && work_bytes < pya_centroid_workspace_bytes(n_spectra, 0))
        return h->fail(PYA_ERR_ARG, -1, "%s: a workspace of %llu bytes is smaller than pya_centroid_workspace_bytes (%llu for no peaks)", who,
                       (unsigned long long)work_bytes, (unsigned long long)pya_centroid_workspace_bytes(n_spectra, 0));
    HIPCHK(h, hipSetDevice(h->device));
    const hipStream_t st = (hipStream_t)hip_stream;
    if (n_spectra == 0) {
        HIPCHK(h, hipMemsetAsync(d_new_off, 0, sizeof(int64_t), st));
        return PYA_OK;
    }
    /* the points the keep words lent have bits for: (cap >> 6) + n_spectra <= words */
    const uint64_t tiles = pya_ions_scan_tiles((uint32_t)n_spectra);
    const uint64_t spare = work_bytes / 8ull - tiles - n_spectra;       /* (>= 1: checked above) */
    const int64_t cap_peaks = spare >= (1ull << 56) ? INT64_MAX : (int64_t)((spare << 6) - 1ull);
    uint64_t *d_tiles = (uint64_t *)d_work;
    const int e = pya_launch_centroid(d_in->mz, d_in->intensity, d_in->mz_type, d_in->intensity_type, d_peak_off, n_spectra, d_select, params,
                                      cap_peaks, d_tiles, d_tiles + tiles, (void *)d_out->mz, (void *)d_out->intensity, d_new_off, d_over,
                                      g_centroid_passes, st);
    if (e) return h->hip_fail((hipError_t)e, "centroid launch");
    return PYA_OK;
}

int pya_centroid_spectra_host(pya_handle *h, const pya_typed_spectra *in, const int64_t *peak_off, uint64_t n_spectra,
                              const uint8_t *select, const pya_centroid_params *params, const pya_typed_spectra *out,
                              int64_t *new_off, uint32_t *over) {
    if (!h) return PYA_ERR_ARG;
    const char *who = "pya_centroid_spectra_host";
    const int rc_arg = centroid_check(h, who, in, peak_off, n_spectra, params, out, new_off, over);
    if (rc_arg) return rc_arg;
    if (n_spectra == 0) {
        new_off[0] = 0;
        return PYA_OK;
    }
    if (peak_off[0] < 0) return h->fail(PYA_ERR_ARG, 0, "%s: peak_off[0] is negative", who);
    for (uint64_t s = 0; s < n_spectra; s++)
        if (peak_off[s + 1] < peak_off[s]) return h->fail(PYA_ERR_ARG, (int64_t)s, "%s: peak_off descends at spectrum %llu", who, (unsigned long long)s);
    const size_t n_peaks = (size_t)peak_off[n_spectra];
    const size_t mz_size = in->mz_type == PYA_F32 ? 4 : 8, in_size = in->intensity_type == PYA_F32 ? 4 : 8;
    HIPCHK(h, hipSetDevice(h->device));
    if (!h->run_stream) HIPCHK(h, hipStreamCreateWithFlags(&h->run_stream, hipStreamNonBlocking));
    const hipStream_t st = h->run_stream;
    DevBuf<unsigned char> d_mz, d_in, d_omz, d_oin, d_work, d_sel;
    DevBuf<int64_t> d_off, d_new;
    DevBuf<uint32_t> d_over;
    const uint64_t work_bytes = pya_centroid_workspace_bytes(n_spectra, n_peaks);
    HIPCHK(h, d_mz.upload((const unsigned char *)in->mz, n_peaks * mz_size, st));
    HIPCHK(h, d_in.upload((const unsigned char *)in->intensity, n_peaks * in_size, st));
    HIPCHK(h, d_off.upload(peak_off, (size_t)n_spectra + 1, st));
    if (select) HIPCHK(h, d_sel.upload(select, (size_t)n_spectra, st));
    HIPCHK(h, d_omz.alloc(n_peaks * mz_size));
    HIPCHK(h, d_oin.alloc(n_peaks * in_size));
    HIPCHK(h, d_work.alloc((size_t)work_bytes));
    HIPCHK(h, d_new.alloc((size_t)n_spectra + 1));
    HIPCHK(h, d_over.alloc(2));
    HIPCHK(h, hipMemsetAsync(d_over.p, 0, 2 * sizeof(uint32_t), st));
    const pya_typed_spectra t_in = {d_mz.p, d_in.p, in->mz_type, in->intensity_type};
    const pya_typed_spectra t_out = {d_omz.p, d_oin.p, in->mz_type, in->intensity_type};
    int rc = pya_centroid_spectra(h, &t_in, d_off.p, n_spectra, select ? d_sel.p : nullptr, params, st, d_work.p, work_bytes, &t_out, d_new.p,
                                  d_over.p);
    if (rc) {
        (void)hipStreamSynchronize(st);                      /* (the buffers are freed on return) */
        return rc;
    }
    HIPCHK(h, hipMemcpyAsync(new_off, d_new.p, ((size_t)n_spectra + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipMemcpyAsync(over, d_over.p, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    const int64_t kept = new_off[n_spectra];
    if (kept < 0 || (uint64_t)kept > n_peaks) return h->fail(PYA_ERR_HIP, -1, "%s: the device kept %lld peaks of %llu", who, (long long)kept, (unsigned long long)n_peaks);
    if (kept) {
        HIPCHK(h, hipMemcpyAsync((void *)out->mz, d_omz.p, (size_t)kept * mz_size, hipMemcpyDeviceToHost, st));
        HIPCHK(h, hipMemcpyAsync((void *)out->intensity, d_oin.p, (size_t)kept * in_size, hipMemcpyDeviceToHost, st));
        HIPCHK(h, hipStreamSynchronize(st));
    }
    return PYA_OK;
}

}
