/* host_strip.cpp -- the C ABI of precursor stripping (include/pyascore_hip.h: pya_strip_params; kernels: strip.hip and
 * deisotope.hip's fill): the argument checks, the workspace layout and the host form.  The checks of the arrays are
 * host_deisotope.cpp's. */
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

static const uint64_t kStripMaxSpectra = 0xfffffffeull;

/* the workspace in 8-byte words, laid out as deisotoping's (the fill kernel is its): the tile sums of the scan, then the keep
 * words -- (n_peaks >> 6) + n_spectra of them, one more so that no spectra is still a workspace */
static uint64_t strip_tile_words(uint64_t n_spectra) { return n_spectra > kStripMaxSpectra ? 0 : pya_ions_scan_tiles((uint32_t)n_spectra); }

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
    if (n_spectra > kStripMaxSpectra) return h->fail(PYA_ERR_ARG, -1, "%s: %llu spectra are more than 2^32 - 2", who, (unsigned long long)n_spectra);
    if (const char *why = strip_params_fault(params)) return h->fail(PYA_ERR_ARG, -1, "%s: %s", who, why);
    const int rc = deiso_check_arrays(h, who, in, peak_off, n_spectra, out, new_off, over);
    if (rc) return rc;
    if (n_spectra && (!prec_mz || !prec_z)) return h->fail(PYA_ERR_ARG, -1, "NULL precursor array passed to %s", who);
    if (n_spectra && ((uintptr_t)report & 7u)) return h->fail(PYA_ERR_ARG, -1, "%s: the report is not 8-byte aligned", who);
    return PYA_OK;
}

extern "C" {

uint64_t pya_strip_workspace_bytes(uint64_t n_spectra, uint64_t n_peaks) {
    return 8ull * (strip_tile_words(n_spectra) + (n_peaks >> 6) + n_spectra + 1ull);
}

int pya_strip_spectra(pya_handle *h, const pya_typed_spectra *d_in, const int64_t *d_peak_off, uint64_t n_spectra,
                      const double *d_prec_mz, const int32_t *d_prec_z, const pya_strip_params *params, void *hip_stream,
                      void *d_work, uint64_t work_bytes, const pya_typed_spectra *d_out, int64_t *d_new_off,
                      pya_strip_report *d_report, uint32_t *d_over) {
    if (!h) return PYA_ERR_ARG;
    const char *who = "pya_strip_spectra";
    const int rc = strip_check(h, who, d_in, d_peak_off, n_spectra, d_prec_mz, d_prec_z, params, d_out, d_new_off, d_report, d_over);
    if (rc) return rc;
    if (n_spectra && (!d_work || ((uintptr_t)d_work & 7u))) return h->fail(PYA_ERR_ARG, -1, "%s: the workspace is NULL or not 8-byte aligned", who);
    if (n_spectra && work_bytes < pya_strip_workspace_bytes(n_spectra, 0))
        return h->fail(PYA_ERR_ARG, -1, "%s: a workspace of %llu bytes is smaller than pya_strip_workspace_bytes (%llu for no peaks)", who,
                       (unsigned long long)work_bytes, (unsigned long long)pya_strip_workspace_bytes(n_spectra, 0));
    HIPCHK(h, hipSetDevice(h->device));
    const hipStream_t st = (hipStream_t)hip_stream;
    if (n_spectra == 0) {
        HIPCHK(h, hipMemsetAsync(d_new_off, 0, sizeof(int64_t), st));
        return PYA_OK;
    }
    /* the peaks the keep words lent have bits for: (cap >> 6) + n_spectra <= words */
    const uint64_t tiles = strip_tile_words(n_spectra);
    const uint64_t spare = work_bytes / 8ull - tiles - n_spectra;       /* (>= 1: checked above) */
    const int64_t cap_peaks = spare >= (1ull << 56) ? INT64_MAX : (int64_t)((spare << 6) - 1ull);
    uint64_t *d_tiles = (uint64_t *)d_work;
    const int e = pya_launch_strip(d_in->mz, d_in->intensity, d_in->mz_type, d_in->intensity_type, d_peak_off, n_spectra, d_prec_mz, d_prec_z,
                                   params, cap_peaks, d_tiles, d_tiles + tiles, (void *)d_out->mz, (void *)d_out->intensity, d_new_off, d_report,
                                   d_over, st);
    if (e) return h->hip_fail((hipError_t)e, "strip launch");
    return PYA_OK;
}

int pya_strip_spectra_host(pya_handle *h, const pya_typed_spectra *in, const int64_t *peak_off, uint64_t n_spectra,
                           const double *prec_mz, const int32_t *prec_z, const pya_strip_params *params,
                           const pya_typed_spectra *out, int64_t *new_off, pya_strip_report *report, uint32_t *over) {
    if (!h) return PYA_ERR_ARG;
    const char *who = "pya_strip_spectra_host";
    const int rc_arg = strip_check(h, who, in, peak_off, n_spectra, prec_mz, prec_z, params, out, new_off, report, over);
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
    DevBuf<double> d_pm;
    DevBuf<int32_t> d_pz;
    DevBuf<pya_strip_report> d_rep;
    DevBuf<uint32_t> d_over;
    const uint64_t work_bytes = pya_strip_workspace_bytes(n_spectra, n_peaks);
    HIPCHK(h, d_mz.upload((const unsigned char *)in->mz, n_peaks * mz_size, st));
    HIPCHK(h, d_in.upload((const unsigned char *)in->intensity, n_peaks * in_size, st));
    HIPCHK(h, d_off.upload(peak_off, (size_t)n_spectra + 1, st));
    HIPCHK(h, d_pm.upload(prec_mz, (size_t)n_spectra, st));
    HIPCHK(h, d_pz.upload(prec_z, (size_t)n_spectra, st));
    HIPCHK(h, d_omz.alloc(n_peaks * mz_size));
    HIPCHK(h, d_oin.alloc(n_peaks * in_size));
    if (report) HIPCHK(h, d_rep.alloc((size_t)n_spectra));
    HIPCHK(h, d_work.alloc((size_t)work_bytes));
    HIPCHK(h, d_new.alloc((size_t)n_spectra + 1));
    HIPCHK(h, d_over.alloc(2));
    HIPCHK(h, hipMemsetAsync(d_over.p, 0, 2 * sizeof(uint32_t), st));
    const pya_typed_spectra t_in = {d_mz.p, d_in.p, in->mz_type, in->intensity_type};
    const pya_typed_spectra t_out = {d_omz.p, d_oin.p, in->mz_type, in->intensity_type};
    int rc = pya_strip_spectra(h, &t_in, d_off.p, n_spectra, d_pm.p, d_pz.p, params, st, d_work.p, work_bytes, &t_out, d_new.p,
                               report ? d_rep.p : nullptr, d_over.p);
    if (rc) {
        (void)hipStreamSynchronize(st);                      /* (the buffers are freed on return) */
        return rc;
    }
    HIPCHK(h, hipMemcpyAsync(new_off, d_new.p, ((size_t)n_spectra + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipMemcpyAsync(over, d_over.p, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (report) HIPCHK(h, hipMemcpyAsync(report, d_rep.p, (size_t)n_spectra * sizeof(pya_strip_report), hipMemcpyDeviceToHost, st));
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
