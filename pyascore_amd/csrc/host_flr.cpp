/* host_flr.cpp -- the C ABI of the site FLR stage (include/pyascore_hip.h: pya_site_flr; kernels: flr.hip): the argument
 * checks of the device form, and the host form that uploads a table, lends a workspace of its own and downloads. */
#include "host_internal.h"
#include "../../include/pyascore_debug.h"

static bool misaligned(const void *p) { return ((uintptr_t)p & 15u) != 0; }

/* everything pya_rollup_flr refuses, before anything is launched; *run: the table has slots */
static int flr_check(pya_handle *h, const void *d_table, uint64_t n_slots, uint32_t flags, const void *d_work, uint64_t work_bytes,
                     const void *d_out, const uint32_t *d_n_ranked, bool *run) {
    *run = false;
    if (n_slots > 0x7fffffffull) return h->fail(PYA_ERR_ARG, -1, "pya_rollup_flr: %llu slots are more than 2^31 - 1", (unsigned long long)n_slots);
    if (flags & ~PYA_FLR_REPORTED_ONLY) return h->fail(PYA_ERR_ARG, -1, "pya_rollup_flr: unknown flag bits 0x%x", flags & ~PYA_FLR_REPORTED_ONLY);
    if (!d_n_ranked) return h->fail(PYA_ERR_ARG, -1, "NULL d_n_ranked passed to pya_rollup_flr");
    if (n_slots == 0) return PYA_OK;
    if (!d_table || !d_out || !d_work) return h->fail(PYA_ERR_ARG, -1, "NULL device pointer passed to pya_rollup_flr");
    if (misaligned(d_table) || misaligned(d_out) || misaligned(d_work))
        return h->fail(PYA_ERR_ARG, -1, "pya_rollup_flr: the table, the records and the workspace must be 16-byte aligned");
    const uint64_t need = pya_flr_layout_bytes(n_slots);
    if (work_bytes < need)
        return h->fail(PYA_ERR_ARG, -1, "pya_rollup_flr: a workspace of %llu bytes, %llu slots need %llu", (unsigned long long)work_bytes,
                       (unsigned long long)n_slots, (unsigned long long)need);
    *run = true;
    return PYA_OK;
}

extern "C" {

uint64_t pya_flr_workspace_bytes(uint64_t n_slots) { return n_slots > 0x7fffffffull ? 0 : pya_flr_layout_bytes(n_slots); }

int pya_rollup_flr(pya_handle *h, const pya_site_rollup *d_table, uint64_t n_slots, const uint8_t *d_cls, uint32_t flags, void *hip_stream,
                   void *d_work, uint64_t work_bytes, pya_site_flr *d_out, uint32_t *d_order, uint32_t *d_n_ranked) {
    if (!h) return PYA_ERR_ARG;
    bool run;
    const int rc = flr_check(h, d_table, n_slots, flags, d_work, work_bytes, d_out, d_n_ranked, &run);
    if (rc) return rc;
    const hipStream_t st = (hipStream_t)hip_stream;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemsetAsync(d_n_ranked, 0, 2 * sizeof(uint32_t), st));
    if (!run) return PYA_OK;
    const int e = pya_launch_flr(d_table, n_slots, d_cls, flags & PYA_FLR_REPORTED_ONLY, d_work, d_out, d_order, d_n_ranked, nullptr, st);
    if (e) return h->hip_fail((hipError_t)e, "site FLR launch");
    return PYA_OK;
}

int pya_debug_rollup_flr_timed(pya_handle *h, const pya_site_rollup *d_table, uint64_t n_slots, const uint8_t *d_cls, uint32_t flags,
                               void *hip_stream, void *d_work, uint64_t work_bytes, pya_site_flr *d_out, uint32_t *d_order,
                               uint32_t *d_n_ranked, float ms[PYA_FLR_PHASES + 1]) {
    if (!h || !ms) return PYA_ERR_ARG;
    bool run;
    const int rc = flr_check(h, d_table, n_slots, flags, d_work, work_bytes, d_out, d_n_ranked, &run);
    if (rc) return rc;
    for (int i = 0; i <= PYA_FLR_PHASES; i++) ms[i] = 0.f;
    const hipStream_t st = (hipStream_t)hip_stream;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemsetAsync(d_n_ranked, 0, 2 * sizeof(uint32_t), st));
    if (!run) return PYA_OK;
    hipEvent_t ev[PYA_FLR_PHASES + 1] = {};
    int out = PYA_OK;
    for (int i = 0; i <= PYA_FLR_PHASES && out == PYA_OK; i++)
        if (hipEventCreate(&ev[i]) != hipSuccess) out = h->fail(PYA_ERR_HIP, -1, "hipEventCreate failed");
    if (out == PYA_OK) {
        const int e = pya_launch_flr(d_table, n_slots, d_cls, flags & PYA_FLR_REPORTED_ONLY, d_work, d_out, d_order, d_n_ranked, ev, st);
        if (e) out = h->hip_fail((hipError_t)e, "site FLR launch");
    }
    if (out == PYA_OK) {
        const hipError_t e = hipStreamSynchronize(st);
        if (e != hipSuccess) out = h->hip_fail(e, "site FLR");
    }
    for (int i = 0; i < PYA_FLR_PHASES && out == PYA_OK; i++)
        if (hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]) != hipSuccess) out = h->fail(PYA_ERR_HIP, -1, "hipEventElapsedTime failed");
    if (out == PYA_OK && hipEventElapsedTime(&ms[PYA_FLR_PHASES], ev[0], ev[PYA_FLR_PHASES]) != hipSuccess)
        out = h->fail(PYA_ERR_HIP, -1, "hipEventElapsedTime failed");
    for (int i = 0; i <= PYA_FLR_PHASES; i++)
        if (ev[i]) (void)hipEventDestroy(ev[i]);
    return out;
}

int pya_rollup_flr_host(pya_handle *h, const pya_site_rollup *table, uint64_t n_slots, const uint8_t *cls, uint32_t flags, pya_site_flr *out,
                        uint32_t *order, uint32_t *n_ranked) {
    if (!h) return PYA_ERR_ARG;
    if (n_slots > 0x7fffffffull) return h->fail(PYA_ERR_ARG, -1, "pya_rollup_flr_host: %llu slots are more than 2^31 - 1", (unsigned long long)n_slots);
    if (flags & ~PYA_FLR_REPORTED_ONLY) return h->fail(PYA_ERR_ARG, -1, "pya_rollup_flr_host: unknown flag bits 0x%x", flags & ~PYA_FLR_REPORTED_ONLY);
    if (!n_ranked) return h->fail(PYA_ERR_ARG, -1, "NULL n_ranked passed to pya_rollup_flr_host");
    *n_ranked = 0;
    if (n_slots == 0) return PYA_OK;
    if (!table || !out) return h->fail(PYA_ERR_ARG, -1, "NULL array passed to pya_rollup_flr_host");
    if (cls)
        for (uint64_t s = 0; s < n_slots; s++)
            if (cls[s] > PYA_FLR_LEFT_OUT)
                return h->fail(PYA_ERR_ARG, (int64_t)s, "pya_rollup_flr_host: class byte %u of slot %llu is none of 0, 1, 2", (unsigned)cls[s],
                               (unsigned long long)s);
    HIPCHK(h, hipSetDevice(h->device));
    if (!h->run_stream) HIPCHK(h, hipStreamCreateWithFlags(&h->run_stream, hipStreamNonBlocking));
    const hipStream_t st = h->run_stream;
    DevBuf<pya_site_rollup> d_table;
    DevBuf<uint8_t> d_cls, d_work;
    DevBuf<pya_site_flr> d_out;
    DevBuf<uint32_t> d_order, d_nr;
    const uint64_t work = pya_flr_layout_bytes(n_slots);
    HIPCHK(h, d_table.upload(table, (size_t)n_slots, st));
    if (cls) HIPCHK(h, d_cls.upload(cls, (size_t)n_slots, st));
    HIPCHK(h, d_work.alloc((size_t)work));
    HIPCHK(h, d_out.alloc((size_t)n_slots));
    if (order) HIPCHK(h, d_order.alloc((size_t)n_slots));
    HIPCHK(h, d_nr.alloc(2));
    const int rc = pya_rollup_flr(h, d_table.p, n_slots, cls ? d_cls.p : nullptr, flags, st, d_work.p, work, d_out.p, order ? d_order.p : nullptr,
                                  d_nr.p);
    if (rc) {
        (void)hipStreamSynchronize(st);                      /* (the buffers are freed on return) */
        return rc;
    }
    uint32_t nr[2] = {0u, 0u};
    HIPCHK(h, hipMemcpyAsync(out, d_out.p, (size_t)n_slots * sizeof(pya_site_flr), hipMemcpyDeviceToHost, st));
    if (order) HIPCHK(h, hipMemcpyAsync(order, d_order.p, (size_t)n_slots * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipMemcpyAsync(nr, d_nr.p, sizeof nr, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    if (nr[1]) return h->fail(PYA_ERR_ARG, -1, "pya_rollup_flr_host: %u class bytes are none of 0, 1, 2", nr[1]);
    *n_ranked = nr[0];
    return PYA_OK;
}

}
