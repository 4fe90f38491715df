/* host_coverage.cpp -- the batch side of the coverage records (include/pyascore_hip.h: pya_coverage; kernel: coverage.hip):
 * the handle's pinned block, the stage behind a plan of pya_score_batch* and the records of the last batch call.
 * pya_plan_coverage is host_run.cpp's (it needs the plan's lists and the wait for the run). */
#include "host_internal.h"

int coverage_host_block(pya_handle *h, uint64_t n) {
    HIPCHK(h, hipSetDevice(h->device));
    if (h->cov_cap < n) {
        if (h->cov_host) (void)hipHostFree(h->cov_host);
        h->cov_host = nullptr;
        h->cov_cap = 0;
        HIPCHK(h, hipHostMalloc((void **)&h->cov_host, std::max<size_t>((size_t)n, 1) * sizeof(pya_coverage), hipHostMallocDefault));
        h->cov_cap = std::max<size_t>((size_t)n, 1);
    }
    std::memset(h->cov_host, 0, (size_t)n * sizeof(pya_coverage));
    h->cov_n = n;
    return PYA_OK;
}

int coverage_behind_run(pya_handle *h, pya_plan *p, const pya_results *d_out, const pya_typed_spectra *d_sp, uint64_t lo, hipStream_t st) {
    const size_t n = (size_t)p->n_psm;
    if (n == 0) return PYA_OK;
    HIPCHK(h, p->d_cov.alloc(n));
    const int rc = pya_plan_coverage(p, d_out, d_sp, st, p->d_cov.p);
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(h->cov_host + lo, p->d_cov.p, n * sizeof(pya_coverage), hipMemcpyDeviceToHost, st));
    return PYA_OK;
}

extern "C" {

int pya_last_batch_coverage(pya_handle *h, pya_coverage *out, uint64_t n_psm) {
    if (!h) return PYA_ERR_ARG;
    if (!h->cov_valid) return h->fail(PYA_ERR_STATE, -1, "the last batch was scored without PYA_FLAG_COVERAGE");
    if (n_psm != h->cov_n)
        return h->fail(PYA_ERR_ARG, -1, "the coverage records of the last batch are of %llu PSMs, not %llu", (unsigned long long)h->cov_n,
                       (unsigned long long)n_psm);
    if (n_psm == 0) return PYA_OK;
    if (!out) return h->fail(PYA_ERR_ARG, -1, "NULL array passed to pya_last_batch_coverage");
    std::memcpy(out, h->cov_host, (size_t)n_psm * sizeof(pya_coverage));
    return PYA_OK;
}

}
