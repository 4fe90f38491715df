/* host_transform.cpp -- the frame of the spectrum transforms in front of a plan (deisotope, decharge, strip, centroid;
 * host_deisotope.cpp, host_decharge.cpp, host_strip.cpp, host_centroid.cpp): what they refuse about their arrays and their
 * workspace, the keep words of a workspace, the call without spectra and the host form.  A stage brings its parameters and
 * their fault, its workspace formula, its launcher and the buffers it takes beside the spectra. */
#include "host_internal.h"

static const uint64_t kXformMaxSpectra = 0xfffffffeull;

int xform_check(pya_handle *h, const char *who, const char *params_fault, const pya_typed_spectra *in, const int64_t *peak_off,
                uint64_t n_spectra, const pya_typed_spectra *out, const int64_t *new_off, const uint32_t *over) {
    if (n_spectra > kXformMaxSpectra) return h->fail(PYA_ERR_ARG, -1, "%s: %llu spectra are more than 2^32 - 2", who, (unsigned long long)n_spectra);
    if (params_fault) return h->fail(PYA_ERR_ARG, -1, "%s: %s", who, params_fault);
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

int xform_check_work(pya_handle *h, const char *who, const char *sizer, uint64_t n_spectra, const void *d_work, uint64_t work_bytes,
                     uint64_t least_bytes) {
    if (n_spectra == 0) return PYA_OK;
    if (!d_work || ((uintptr_t)d_work & 7u)) return h->fail(PYA_ERR_ARG, -1, "%s: the workspace is NULL or not 8-byte aligned", who);
    if (work_bytes < least_bytes)
        return h->fail(PYA_ERR_ARG, -1, "%s: a workspace of %llu bytes is smaller than %s (%llu for no peaks)", who, (unsigned long long)work_bytes,
                       sizer, (unsigned long long)least_bytes);
    return PYA_OK;
}

uint64_t xform_tile_words(uint64_t n_spectra) { return n_spectra > kXformMaxSpectra ? 0 : pya_ions_scan_tiles((uint32_t)n_spectra); }

/* (cap >> 6) + n_spectra <= the words behind the tile sums */
int64_t xform_keep_cap(uint64_t n_spectra, uint64_t work_bytes) {
    const uint64_t spare = work_bytes / 8ull - xform_tile_words(n_spectra) - n_spectra;       /* (>= 1: xform_check_work) */
    return spare >= (1ull << 56) ? INT64_MAX : (int64_t)((spare << 6) - 1ull);
}

int xform_no_spectra(pya_handle *h, int64_t *d_new_off, hipStream_t st) {
    HIPCHK(h, hipMemsetAsync(d_new_off, 0, sizeof(int64_t), st));
    return PYA_OK;
}

int xform_host(pya_handle *h, const char *who, const pya_typed_spectra *in, const int64_t *peak_off, uint64_t n_spectra,
               const pya_typed_spectra *out, int64_t *new_off, uint32_t *over, XformSide *side, size_t n_side,
               uint64_t (*workspace_bytes)(uint64_t, uint64_t), const std::function<int(const XformDevice &)> &device_form) {
    if (n_side > kXformMaxSides) return h->fail(PYA_ERR_STATE, -1, "%s: more side buffers than the host form carries", who);
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
    DevBuf<unsigned char> d_side[kXformMaxSides];
    DevBuf<int64_t> d_off, d_new;
    DevBuf<uint32_t> d_over;
    const uint64_t work_bytes = workspace_bytes(n_spectra, n_peaks);
    HIPCHK(h, d_mz.upload((const unsigned char *)in->mz, n_peaks * mz_size, st));
    HIPCHK(h, d_in.upload((const unsigned char *)in->intensity, n_peaks * in_size, st));
    HIPCHK(h, d_off.upload(peak_off, (size_t)n_spectra + 1, st));
    for (size_t i = 0; i < n_side; i++)
        if (side[i].host && side[i].kind == XformSide::SPECTRUM_IN)
            HIPCHK(h, d_side[i].upload((const unsigned char *)side[i].host, (size_t)n_spectra * side[i].elem_bytes, st));
    HIPCHK(h, d_omz.alloc(n_peaks * mz_size));
    HIPCHK(h, d_oin.alloc(n_peaks * in_size));
    for (size_t i = 0; i < n_side; i++)
        if (side[i].host && side[i].kind != XformSide::SPECTRUM_IN)
            HIPCHK(h, d_side[i].alloc((side[i].kind == XformSide::PEAK_OUT ? n_peaks : (size_t)n_spectra) * side[i].elem_bytes));
    HIPCHK(h, d_work.alloc((size_t)work_bytes));
    HIPCHK(h, d_new.alloc((size_t)n_spectra + 1));
    HIPCHK(h, d_over.alloc(2));
    HIPCHK(h, hipMemsetAsync(d_over.p, 0, 2 * sizeof(uint32_t), st));
    for (size_t i = 0; i < n_side; i++) side[i].dev = d_side[i].p;                    /* (NULL where the caller passed none) */
    const pya_typed_spectra t_in = {d_mz.p, d_in.p, in->mz_type, in->intensity_type};
    const pya_typed_spectra t_out = {d_omz.p, d_oin.p, in->mz_type, in->intensity_type};
    const int rc = device_form(XformDevice{&t_in, &t_out, d_off.p, st, d_work.p, work_bytes, d_new.p, d_over.p});
    if (rc) {
        (void)hipStreamSynchronize(st);                      /* (the buffers are freed on return) */
        return rc;
    }
    HIPCHK(h, hipMemcpyAsync(new_off, d_new.p, ((size_t)n_spectra + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipMemcpyAsync(over, d_over.p, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    for (size_t i = 0; i < n_side; i++)
        if (side[i].host && side[i].kind == XformSide::SPECTRUM_OUT)
            HIPCHK(h, hipMemcpyAsync(side[i].host, d_side[i].p, (size_t)n_spectra * side[i].elem_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    const int64_t kept = new_off[n_spectra];
    if (kept < 0 || (uint64_t)kept > n_peaks) return h->fail(PYA_ERR_HIP, -1, "%s: the device kept %lld peaks of %llu", who, (long long)kept, (unsigned long long)n_peaks);
    if (kept) {
        HIPCHK(h, hipMemcpyAsync((void *)out->mz, d_omz.p, (size_t)kept * mz_size, hipMemcpyDeviceToHost, st));
        HIPCHK(h, hipMemcpyAsync((void *)out->intensity, d_oin.p, (size_t)kept * in_size, hipMemcpyDeviceToHost, st));
        for (size_t i = 0; i < n_side; i++)
            if (side[i].host && side[i].kind == XformSide::PEAK_OUT)
                HIPCHK(h, hipMemcpyAsync(side[i].host, d_side[i].p, (size_t)kept * side[i].elem_bytes, hipMemcpyDeviceToHost, st));
        HIPCHK(h, hipStreamSynchronize(st));
    }
    return PYA_OK;
}
