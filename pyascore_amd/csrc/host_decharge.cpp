/* host_decharge.cpp -- the C ABI of charge deconvolution (include/pyascore_hip.h: pya_decharge_params; kernels: decharge.hip):
 * the argument checks, the workspace layout and the host form.  The checks of the arrays and of the deisotoping rule inside the
 * parameters are host_deisotope.cpp's. */
#include "host_internal.h"

#include <cmath>

extern "C" int pya_launch_decharge(const void *d_mz, const void *d_in, uint32_t mz_type, uint32_t in_type, const int64_t *d_peak_off,
                                   uint64_t n_spectra, const pya_decharge_params *prm, int64_t cap_peaks, uint64_t *d_tiles, uint64_t *d_regions,
                                   uint64_t region_words, void *d_out_mz, void *d_out_in, int64_t *d_new_off, uint8_t *d_charge, uint32_t *d_over,
                                   uint32_t passes, hipStream_t stream);

static_assert(sizeof(pya_decharge_params) == 112 && offsetof(pya_decharge_params, carrier) == 96, "pya_decharge_params is a 112-byte record");

static const uint64_t kDechgMaxSpectra = 0xfffffffeull;
static uint32_t g_dechg_passes = 7u;                       /* (pya_debug_decharge_passes: a probe times MARK and PLACE apart) */

/* The workspace in 8-byte words.  Peaks are lent in groups of 64: a group costs three words (one each of the keep, moved and
 * before regions of decharge.hip) and 128 words of list (two an entry), 131 together.  Beside the groups: the tile sums of the
 * scan, per spectrum one word in each of the three regions and one moved count, and one word more in each region so that word
 * (cap >> 6) + n_spectra - 1 + 1 exists.  G groups hold cap = 64 G peaks; n_peaks peaks need (n_peaks >> 6) + 1 groups. */
static uint64_t dechg_tile_words(uint64_t n_spectra) { return n_spectra > kDechgMaxSpectra ? 0 : pya_ions_scan_tiles((uint32_t)n_spectra); }
static uint64_t dechg_fixed_words(uint64_t n_spectra) { return dechg_tile_words(n_spectra) + 4ull * n_spectra + 3ull; }

static int dechg_check(pya_handle *h, const char *who, const pya_typed_spectra *in, const int64_t *peak_off, uint64_t n_spectra,
                       const pya_decharge_params *params, const pya_typed_spectra *out, const int64_t *new_off, const uint32_t *over) {
    if (!params) return h->fail(PYA_ERR_ARG, -1, "%s: params is NULL", who);
    const int rc = deiso_check(h, who, in, peak_off, n_spectra, &params->iso, out, new_off, over);
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
    const int rc = dechg_check(h, who, d_in, d_peak_off, n_spectra, params, d_out, d_new_off, d_over);
    if (rc) return rc;
    if (n_spectra && (!d_work || ((uintptr_t)d_work & 7u))) return h->fail(PYA_ERR_ARG, -1, "%s: the workspace is NULL or not 8-byte aligned", who);
    if (n_spectra && work_bytes < pya_decharge_workspace_bytes(n_spectra, 0))
        return h->fail(PYA_ERR_ARG, -1, "%s: a workspace of %llu bytes is smaller than pya_decharge_workspace_bytes (%llu for no peaks)", who,
                       (unsigned long long)work_bytes, (unsigned long long)pya_decharge_workspace_bytes(n_spectra, 0));
    if (n_spectra && d_charge && (d_charge == d_in->mz || d_charge == d_in->intensity || d_charge == d_out->mz || d_charge == d_out->intensity))
        return h->fail(PYA_ERR_ARG, -1, "%s: d_charge is one of the spectrum arrays", who);
    HIPCHK(h, hipSetDevice(h->device));
    const hipStream_t st = (hipStream_t)hip_stream;
    if (n_spectra == 0) {
        HIPCHK(h, hipMemsetAsync(d_new_off, 0, sizeof(int64_t), st));
        return PYA_OK;
    }
    /* the groups of 64 peaks the workspace lent has room for (>= 1: checked above; no more than 2^50, so that nothing overflows) */
    uint64_t groups = (work_bytes / 8ull - dechg_fixed_words(n_spectra)) / 131ull;
    if (groups > (1ull << 50)) groups = 1ull << 50;
    const int64_t cap_peaks = (int64_t)(groups << 6);
    const uint64_t region_words = groups + n_spectra + 1ull;
    uint64_t *d_tiles = (uint64_t *)d_work;
    const int e = pya_launch_decharge(d_in->mz, d_in->intensity, d_in->mz_type, d_in->intensity_type, d_peak_off, n_spectra, params, cap_peaks,
                                      d_tiles, d_tiles + dechg_tile_words(n_spectra), region_words, (void *)d_out->mz, (void *)d_out->intensity,
                                      d_new_off, d_charge, d_over, g_dechg_passes, st);
    if (e) return h->hip_fail((hipError_t)e, "decharge launch");
    return PYA_OK;
}

int pya_decharge_spectra_host(pya_handle *h, const pya_typed_spectra *in, const int64_t *peak_off, uint64_t n_spectra,
                              const pya_decharge_params *params, const pya_typed_spectra *out, int64_t *new_off, uint8_t *charge,
                              uint32_t *over) {
    if (!h) return PYA_ERR_ARG;
    const char *who = "pya_decharge_spectra_host";
    const int rc_arg = dechg_check(h, who, in, peak_off, n_spectra, params, out, new_off, over);
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
    DevBuf<unsigned char> d_mz, d_in, d_omz, d_oin, d_work, d_chg;
    DevBuf<int64_t> d_off, d_new;
    DevBuf<uint32_t> d_over;
    const uint64_t work_bytes = pya_decharge_workspace_bytes(n_spectra, n_peaks);
    HIPCHK(h, d_mz.upload((const unsigned char *)in->mz, n_peaks * mz_size, st));
    HIPCHK(h, d_in.upload((const unsigned char *)in->intensity, n_peaks * in_size, st));
    HIPCHK(h, d_off.upload(peak_off, (size_t)n_spectra + 1, st));
    HIPCHK(h, d_omz.alloc(n_peaks * mz_size));
    HIPCHK(h, d_oin.alloc(n_peaks * in_size));
    if (charge) HIPCHK(h, d_chg.alloc(n_peaks));
    HIPCHK(h, d_work.alloc((size_t)work_bytes));
    HIPCHK(h, d_new.alloc((size_t)n_spectra + 1));
    HIPCHK(h, d_over.alloc(2));
    HIPCHK(h, hipMemsetAsync(d_over.p, 0, 2 * sizeof(uint32_t), st));
    const pya_typed_spectra t_in = {d_mz.p, d_in.p, in->mz_type, in->intensity_type};
    const pya_typed_spectra t_out = {d_omz.p, d_oin.p, in->mz_type, in->intensity_type};
    int rc = pya_decharge_spectra(h, &t_in, d_off.p, n_spectra, params, st, d_work.p, work_bytes, &t_out, d_new.p, charge ? d_chg.p : nullptr,
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
        if (charge) HIPCHK(h, hipMemcpyAsync(charge, d_chg.p, (size_t)kept, hipMemcpyDeviceToHost, st));
        HIPCHK(h, hipStreamSynchronize(st));
    }
    return PYA_OK;
}

}
