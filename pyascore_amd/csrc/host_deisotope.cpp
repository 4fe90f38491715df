/* host_deisotope.cpp -- the C ABI of deisotoping (include/pyascore_hip.h: pya_deisotope_params; kernels: deisotope.hip): the
 * argument checks, the workspace layout and the host form. */
#include "host_internal.h"

#include <cmath>

extern "C" int pya_launch_deisotope(const void *d_mz, const void *d_in, uint32_t mz_type, uint32_t in_type, const int64_t *d_peak_off,
                                    uint64_t n_spectra, const pya_deisotope_params *prm, int64_t cap_peaks, uint64_t *d_tiles, uint64_t *d_keep,
                                    void *d_out_mz, void *d_out_in, int64_t *d_new_off, uint32_t *d_over, hipStream_t stream);

static const uint64_t kDeisoMaxSpectra = 0xfffffffeull;

/* the workspace in 8-byte words: the tile sums of the scan, then the keep words -- (n_peaks >> 6) + n_spectra of them hold every
 * spectrum's bits in words of its own (deisotope.hip), one more so that no spectra is still a workspace */
static uint64_t deiso_tile_words(uint64_t n_spectra) { return n_spectra > kDeisoMaxSpectra ? 0 : pya_ions_scan_tiles((uint32_t)n_spectra); }

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

int deiso_check(pya_handle *h, const char *who, const pya_typed_spectra *in, const int64_t *peak_off, uint64_t n_spectra,
                const pya_deisotope_params *params, const pya_typed_spectra *out, const int64_t *new_off, const uint32_t *over) {
    if (n_spectra > kDeisoMaxSpectra) return h->fail(PYA_ERR_ARG, -1, "%s: %llu spectra are more than 2^32 - 2", who, (unsigned long long)n_spectra);
    if (const char *why = deiso_params_fault(params)) return h->fail(PYA_ERR_ARG, -1, "%s: %s", who, why);
    return deiso_check_arrays(h, who, in, peak_off, n_spectra, out, new_off, over);
}

int deiso_check_arrays(pya_handle *h, const char *who, const pya_typed_spectra *in, const int64_t *peak_off, uint64_t n_spectra,
                       const pya_typed_spectra *out, const int64_t *new_off, const uint32_t *over) {
    if (n_spectra > kDeisoMaxSpectra) return h->fail(PYA_ERR_ARG, -1, "%s: %llu spectra are more than 2^32 - 2", who, (unsigned long long)n_spectra);
    if (!in || !out || !new_off) return h->fail(PYA_ERR_ARG, -1, "NULL pointer passed to %s", who);
    if ((in->mz_type != PYA_F64 && in->mz_type != PYA_F32) || (in->intensity_type != PYA_F64 && in->intensity_type != PYA_F32))
        return h->fail(PYA_ERR_ARG, -1, "%s: element types %u / %u are neither PYA_F64 nor PYA_F32", who, in->mz_type, in->intensity_type);
    if (in->mz_type == PYA_F32 && in->intensity_type == PYA_F64)
        return h->fail(PYA_ERR_ARG, -1, "%s: float32 m/z beside float64 intensities is not supported", who);
    if (out->mz_type != in->mz_type || out->intensity_type != in->intensity_type)
        return h->fail(PYA_ERR_ARG, -1, "%s: the out arrays are of types %u / %u, the in arrays of %u / %u", who, out->mz_type, out->intensity_type,
                       in->mz_type, in->intensity_type);
    if (n_spectra == 0) return PYA_OK;
    if (!in->mz || !in->intensity || !out->mz || !out->intensity || !peak_off || !over) return h->fail(PYA_ERR_ARG, -1, "NULL array passed to %s", who);
    if (out->mz == in->mz || out->mz == in->intensity || out->intensity == in->mz || out->intensity == in->intensity || out->mz == out->intensity)
        return h->fail(PYA_ERR_ARG, -1, "%s: an out array is an in array (the filter does not work in place)", who);
    return PYA_OK;
}

extern "C" {

uint64_t pya_deisotope_workspace_bytes(uint64_t n_spectra, uint64_t n_peaks) {
    return 8ull * (deiso_tile_words(n_spectra) + (n_peaks >> 6) + n_spectra + 1ull);
}

int pya_deisotope_spectra(pya_handle *h, const pya_typed_spectra *d_in, const int64_t *d_peak_off, uint64_t n_spectra,
                          const pya_deisotope_params *params, void *hip_stream, void *d_work, uint64_t work_bytes,
                          const pya_typed_spectra *d_out, int64_t *d_new_off, uint32_t *d_over) {
    if (!h) return PYA_ERR_ARG;
    const char *who = "pya_deisotope_spectra";
    const int rc = deiso_check(h, who, d_in, d_peak_off, n_spectra, params, d_out, d_new_off, d_over);
    if (rc) return rc;
    if (n_spectra && (!d_work || ((uintptr_t)d_work & 7u))) return h->fail(PYA_ERR_ARG, -1, "%s: the workspace is NULL or not 8-byte aligned", who);
    if (n_spectra && work_bytes < pya_deisotope_workspace_bytes(n_spectra, 0))
        return h->fail(PYA_ERR_ARG, -1, "%s: a workspace of %llu bytes is smaller than pya_deisotope_workspace_bytes (%llu for no peaks)", who,
                       (unsigned long long)work_bytes, (unsigned long long)pya_deisotope_workspace_bytes(n_spectra, 0));
    HIPCHK(h, hipSetDevice(h->device));
    const hipStream_t st = (hipStream_t)hip_stream;
    if (n_spectra == 0) {
        HIPCHK(h, hipMemsetAsync(d_new_off, 0, sizeof(int64_t), st));
        return PYA_OK;
    }
    /* the peaks the keep words lent have bits for: (cap >> 6) + n_spectra <= words */
    const uint64_t tiles = deiso_tile_words(n_spectra);
    const uint64_t spare = work_bytes / 8ull - tiles - n_spectra;       /* (>= 1: checked above) */
    const int64_t cap_peaks = spare >= (1ull << 56) ? INT64_MAX : (int64_t)((spare << 6) - 1ull);
    uint64_t *d_tiles = (uint64_t *)d_work;
    const int e = pya_launch_deisotope(d_in->mz, d_in->intensity, d_in->mz_type, d_in->intensity_type, d_peak_off, n_spectra, params, cap_peaks,
                                       d_tiles, d_tiles + tiles, (void *)d_out->mz, (void *)d_out->intensity, d_new_off, d_over, st);
    if (e) return h->hip_fail((hipError_t)e, "deisotope launch");
    return PYA_OK;
}

int pya_deisotope_spectra_host(pya_handle *h, const pya_typed_spectra *in, const int64_t *peak_off, uint64_t n_spectra,
                               const pya_deisotope_params *params, const pya_typed_spectra *out, int64_t *new_off, uint32_t *over) {
    if (!h) return PYA_ERR_ARG;
    const char *who = "pya_deisotope_spectra_host";
    const int rc_arg = deiso_check(h, who, in, peak_off, n_spectra, params, out, new_off, over);
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
    DevBuf<unsigned char> d_mz, d_in, d_omz, d_oin, d_work;
    DevBuf<int64_t> d_off, d_new;
    DevBuf<uint32_t> d_over;
    const uint64_t work_bytes = pya_deisotope_workspace_bytes(n_spectra, n_peaks);
    HIPCHK(h, d_mz.upload((const unsigned char *)in->mz, n_peaks * mz_size, st));
    HIPCHK(h, d_in.upload((const unsigned char *)in->intensity, n_peaks * in_size, st));
    HIPCHK(h, d_off.upload(peak_off, (size_t)n_spectra + 1, st));
    HIPCHK(h, d_omz.alloc(n_peaks * mz_size));
    HIPCHK(h, d_oin.alloc(n_peaks * in_size));
    HIPCHK(h, d_work.alloc((size_t)work_bytes));
    HIPCHK(h, d_new.alloc((size_t)n_spectra + 1));
    HIPCHK(h, d_over.alloc(2));
    HIPCHK(h, hipMemsetAsync(d_over.p, 0, 2 * sizeof(uint32_t), st));
    const pya_typed_spectra t_in = {d_mz.p, d_in.p, in->mz_type, in->intensity_type};
    const pya_typed_spectra t_out = {d_omz.p, d_oin.p, in->mz_type, in->intensity_type};
    int rc = pya_deisotope_spectra(h, &t_in, d_off.p, n_spectra, params, st, d_work.p, work_bytes, &t_out, d_new.p, d_over.p);
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
