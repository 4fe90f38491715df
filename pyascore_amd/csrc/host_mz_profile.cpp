/* host_mz_profile.cpp -- the C ABI of the fragment mass-error profile (include/pyascore_hip.h: pya_mz_profile; kernel:
 * mz_profile.hip): the argument checks every form shares, the batch loan and the table of the last batch call.
 * pya_plan_mz_profile is host_run.cpp's (it needs the plan's lists and the wait for the run), the batch path host_batch.cpp's. */
#include "host_internal.h"

#include <cmath>

int mzp_check(pya_handle *h, const char *who, uint64_t n_slots, const pya_mz_profile_params *prm) {
    if (!prm) return h->fail(PYA_ERR_ARG, -1, "NULL params passed to %s", who);
    if (n_slots > 0x7fffffffull) return h->fail(PYA_ERR_ARG, -1, "%s: %llu slots are more than an int32 slot can name", who, (unsigned long long)n_slots);
    if (prm->max_rank >= (uint32_t)PYA_NTOP_MAX) return h->fail(PYA_ERR_ARG, -1, "%s: max_rank %u is not in 0 .. %d", who, prm->max_rank, PYA_NTOP_MAX - 1);
    const double inv[3] = {prm->inv_da, prm->inv_ppm, prm->inv_band};
    const char *const name[3] = {"inv_da", "inv_ppm", "inv_band"};
    for (int i = 0; i < 3; i++)
        if (!std::isfinite(inv[i]) || !(inv[i] > 0.)) return h->fail(PYA_ERR_ARG, -1, "%s: %s is not a finite positive number", who, name[i]);
    return PYA_OK;
}

extern "C" {

int pya_set_mz_profile(pya_handle *h, const int32_t *run, uint64_t n_psm, uint64_t n_slots, const pya_mz_profile_params *params) {
    if (!h) return PYA_ERR_ARG;
    h->mzp_loan = pya_handle::MzpLoan{};
    if (n_psm > 0x7fffffffull) return h->fail(PYA_ERR_ARG, -1, "pya_set_mz_profile: %llu PSMs are more than 2^31 - 1", (unsigned long long)n_psm);
    const int rc = mzp_check(h, "pya_set_mz_profile", n_slots, params);
    if (rc) return rc;
    h->mzp_loan.run = run;
    h->mzp_loan.n_psm = n_psm;
    h->mzp_loan.n_slots = n_slots;
    h->mzp_loan.params = *params;
    h->mzp_loan.params.reserved = 0u;
    h->mzp_loan.set = true;
    return PYA_OK;
}

int pya_last_batch_mz_profile(pya_handle *h, pya_mz_profile *out, uint64_t n_slots) {
    if (!h) return PYA_ERR_ARG;
    if (!h->mzp_valid) return h->fail(PYA_ERR_STATE, -1, "the last batch was scored without PYA_FLAG_MZ_PROFILE");
    if (n_slots != h->mzp_host.size())
        return h->fail(PYA_ERR_ARG, -1, "the profile of the last batch has %llu slots, not %llu", (unsigned long long)h->mzp_host.size(),
                       (unsigned long long)n_slots);
    if (n_slots == 0) return PYA_OK;
    if (!out) return h->fail(PYA_ERR_ARG, -1, "NULL array passed to pya_last_batch_mz_profile");
    std::memcpy(out, h->mzp_host.data(), (size_t)n_slots * sizeof(pya_mz_profile));
    return PYA_OK;
}

}
