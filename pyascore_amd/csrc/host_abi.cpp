/* host_abi.cpp -- the C ABI of include/pyascore_hip.h that is not a plan, a batch call or the one-PSM path: handles, settings,
 * strings, retained records, ambiguity. */
#include "host_internal.h"
#include "../../include/pyascore_debug.h"
#include "span_guard.h"
#include "bin_key.h"

extern "C" {


int pya_create(const pya_config *cfg, pya_handle **out) {
    if (!cfg || !out) return PYA_ERR_ARG;
    *out = nullptr;
    std::unique_ptr<pya_handle> h(new pya_handle);
    *out = h.get();                                    /* so the caller can read the message */
    pya_handle *hp = h.release();
    if (!cfg->mod_group || !cfg->fragment_types) return hp->fail(PYA_ERR_ARG, -1, "NULL string in config");
    /* n_top peaks retained per window = depths scored.  Below 10 the reference's weighted sum reads past its scores
     * (cpp/Ascore.cpp:135-137: undefined); above 10 it retains, counts and scores n_top depths, weights the first ten
     * and searches all of them for the depth of an Ascore (:15-36, :123-139, :164-172) -- the general kernel does that,
     * for every PSM of such a scorer. */
    if (cfg->n_top < PYA_NTOP || cfg->n_top > PYA_NTOP_MAX)
        return hp->fail(PYA_ERR_ARG, -1, "n_top must be %d..%d (the PepScore weights are %d long, Ascore.cpp:16-18; "
                        "below that the reference reads past its scores); got %u", PYA_NTOP, PYA_NTOP_MAX, PYA_NTOP, cfg->n_top);
    hp->n_top = cfg->n_top;
    if (!(cfg->bin_size > 0.f)) return hp->fail(PYA_ERR_ARG, -1, "bin_size must be positive");
    if (!(cfg->mz_error > 0.f) || !(cfg->mz_error < 50.f))
        return hp->fail(PYA_ERR_ARG, -1, "mz_error must be in (0, 50)");
    std::string ft = cfg->fragment_types;
    if (ft.empty() || ft.size() > PYA_MAX_FRAGMENT_TYPES)
        return hp->fail(PYA_ERR_ARG, -1, "fragment_types must name 1..%d ion types", PYA_MAX_FRAGMENT_TYPES);
    for (char t : ft)
        if (!is_forward(t) && !is_backward(t))
            return hp->fail(PYA_ERR_ARG, -1, "unknown fragment type '%c' (b, c, y, z, Z are supported)", t);
    hp->device = cfg->device;
    hp->bin_size = cfg->bin_size;
    hp->mod_mass = cfg->mod_mass;
    hp->mz_error = cfg->mz_error;
    hp->mod_group = cfg->mod_group;
    hp->fragment_types = ft;
    hp->build_letter_tables();
    read_knobs(hp->kn);
    std::memset(hp->shape_cache, 0xff, sizeof hp->shape_cache);
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return hp->fail(PYA_ERR_HIP, -1, "no HIP device available (%s); this library has no CPU path",
                        e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    if (cfg->device < 0 || cfg->device >= ndev) return hp->fail(PYA_ERR_ARG, -1, "device %d out of range", cfg->device);
    HIPCHK(hp, hipSetDevice(cfg->device));
    int rc = build_dev_config(hp);
    if (rc) return rc;
    return PYA_OK;
}

void pya_destroy(pya_handle *h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->kept) pya_plan_destroy(h->kept);                 /* (unhooks the one-PSM view if that is what it is) */
    if (h->one.view) delete h->one.view;
    if (h->one.host) (void)hipHostFree(h->one.host);
    if (h->one.stream) (void)hipStreamDestroy(h->one.stream);
    for (void *ps : h->pinned_stage)
        if (ps) (void)hipHostFree(ps);
    if (h->evid_host) (void)hipHostFree(h->evid_host);
    if (h->ions_host) (void)hipHostFree(h->ions_host);
    if (h->named_host) (void)hipHostFree(h->named_host);
    if (h->sites_host) (void)hipHostFree(h->sites_host);
    if (h->probs_host) (void)hipHostFree(h->probs_host);
    if (h->ranked_host) (void)hipHostFree(h->ranked_host);
    if (h->cov_host) (void)hipHostFree(h->cov_host);
    for (hipEvent_t ev : h->pform_ev)
        if (ev) (void)hipEventDestroy(ev);
    if (h->copy_stream) (void)hipStreamDestroy(h->copy_stream);
    if (h->run_stream) (void)hipStreamDestroy(h->run_stream);
    if (h->side_stream) (void)hipStreamDestroy(h->side_stream);
    delete h;
}

int pya_reload_env(pya_handle *h) {
    if (!h) return PYA_ERR_ARG;
    read_knobs(h->kn);
    h->one.have_last = false;        /* (a replay of the last pya_score_one PSM would run under other switches) */
    return PYA_OK;
}

int pya_set_debug(pya_handle *h, const char *key, const char *value) {
    if (!h || !key) return PYA_ERR_ARG;
    if (!set_knob(h->kn, key, value)) return h->fail(PYA_ERR_ARG, -1, "pya_set_debug: \"%s\" is not a debug switch", key);
    h->one.have_last = false;        /* (a replay of the last pya_score_one PSM would run under other switches) */
    return PYA_OK;
}

const char *pya_last_error(const pya_handle *h) { return h ? h->err.c_str() : "NULL handle"; }
int64_t pya_error_index(const pya_handle *h) { return h ? h->err_index : -1; }

int pya_add_neutral_loss(pya_handle *h, const char *group, float mass) {
    if (!h || !group) return PYA_ERR_ARG;
    std::map<char, float> saved = h->nl;
    for (const char *c = group; *c; c++) h->nl[*c] = mass;     /* ModifiedPeptide.cpp:99-103 */
    h->cfg_dirty = true;
    h->one.have_last = false;        /* (a replay of the last pya_score_one PSM would score it under the new settings) */
    h->settings_gen++;               /* every call, an identical or a refused one too: plans made before it do not launch again */
    int rc = build_dev_config(h);
    if (rc) {
        h->nl = saved;
        build_dev_config(h);
    }
    return rc;
}

int pya_count_sites(const pya_handle *h, const uint8_t *pep, uint64_t L, int32_t *n_sites, uint16_t *site_pos) {
    if (!h || !pep || !n_sites) return PYA_ERR_ARG;
    int n = 0;
    for (uint64_t i = 0; i < L; i++)
        if (h->letter_modifiable((char)pep[i], i, L)) {
            if (site_pos && n < PYA_MAX_PEPTIDE_LEN) site_pos[n] = (uint16_t)i;
            n++;
        }
    *n_sites = n;
    return PYA_OK;
}

/* ModifiedPeptide::getPeptide, cpp/ModifiedPeptide.cpp:199-253 */
static void format_one(const pya_handle *h, const uint8_t *pep, uint64_t L, int32_t n_of_mod, const uint32_t *aux_pos,
                       const float *aux_mass, uint64_t n_aux, uint64_t sig_bits, int32_t sig_len, std::string &out) {
    size_t sites[PYA_MAX_PEPTIDE_LEN];
    size_t n = 0;
    for (uint64_t i = 0; i < L; i++)
        if (h->letter_modifiable((char)pep[i], i, L) && n < PYA_MAX_PEPTIDE_LEN) sites[n++] = i;
    std::vector<float> mm(L + 2, 0.f);
    if ((size_t)n_of_mod > n) {
        if (h->allow_n) mm.front() += h->mod_mass;
        else mm.back() += h->mod_mass;
    }
    if (sig_len < 0) sig_len = (int32_t)n;
    for (int32_t j = 0; j < sig_len && j < 64; j++) {
        if (!(sig_bits >> j & 1)) continue;
        size_t pos = (size_t)j < n ? sites[j] : L;
        unsigned char aa = pos < L ? pep[pos] : 0;
        if (aa && h->in_group[aa]) mm[pos + 1] += h->mod_mass;
        else if (pos == 0) mm.front() += h->mod_mass;
        else if (pos + 1 == L) mm.back() += h->mod_mass;
    }
    for (uint64_t a = 0; a < n_aux; a++)
        if (aux_pos[a] < mm.size()) mm[aux_pos[a]] += aux_mass[a];
    size_t s = 0, e = mm.size();
    if (mm.front() == 0.f) s++;
    if (mm.back() == 0.f) e--;
    out.clear();
    for (size_t i = s; i < e; i++) {
        out += i == 0 ? 'n' : (i == L + 1 ? 'c' : (char)pep[i - 1]);
        if (mm[i] > 0.f) {
            char t[16];
            std::snprintf(t, sizeof t, "[%d]", (int)std::round(mm[i]));
            out += t;
        }
    }
}

int pya_format_peptide(const pya_handle *h, const uint8_t *pep, uint64_t L, int32_t n_of_mod,
                       const uint32_t *aux_pos, const float *aux_mass, uint64_t n_aux, uint64_t sig_bits,
                       int32_t sig_len, char *buf, uint64_t cap) {
    if (!h || !pep || !buf || cap == 0) return PYA_ERR_ARG;
    if (L > PYA_MAX_PEPTIDE_LEN) return PYA_ERR_LIMIT;
    std::string out;
    format_one(h, pep, L, n_of_mod, aux_pos, aux_mass, n_aux, sig_bits, sig_len, out);
    size_t ncopy = std::min<size_t>(out.size(), cap - 1);
    std::memcpy(buf, out.data(), ncopy);
    buf[ncopy] = 0;
    return (int)out.size();
}

/* the same for many records in one call (threaded above 20 000 records) */
int pya_format_peptides(const pya_handle *h, const pya_batch *b, uint64_t n_rec, const int64_t *rec_psm,
                        const uint64_t *sig_bits, const int32_t *rec_valid, int64_t *str_off, char *buf,
                        uint64_t cap) {
    if (!h || !b || !sig_bits || !str_off) return PYA_ERR_ARG;
    if (b->n_psm && (!b->pep || !b->pep_off || !b->n_of_mod)) return PYA_ERR_ARG;
    const bool has_aux = b->aux_off && b->aux_pos && b->aux_mass;
    std::vector<std::string> strs(n_rec);
    int bad = 0;
    auto work = [&](uint64_t lo, uint64_t hi) {
        for (uint64_t r = lo; r < hi; r++) {
            if (rec_valid && rec_valid[r] <= 0) continue;           /* no localisation: empty string */
            const uint64_t i = rec_psm ? (uint64_t)rec_psm[r] : r;
            if (i >= b->n_psm) {
                bad = 1;
                continue;
            }
            const int64_t p0 = b->pep_off[i], L = b->pep_off[i + 1] - p0;
            if (L < 1 || L > PYA_MAX_PEPTIDE_LEN) continue;         /* set-aside PSM */
            const int64_t a0 = has_aux ? b->aux_off[i] : 0, a1 = has_aux ? b->aux_off[i + 1] : 0;
            format_one(h, b->pep + p0, (uint64_t)L, b->n_of_mod[i], has_aux ? b->aux_pos + a0 : nullptr,
                       has_aux ? b->aux_mass + a0 : nullptr, (uint64_t)(a1 - a0), sig_bits[r], -1, strs[r]);
        }
    };
    unsigned nt = n_rec >= 20000 ? std::min(8u, std::max(1u, std::thread::hardware_concurrency())) : 1u;
    if (nt == 1) {
        work(0, n_rec);
    } else {
        std::vector<std::thread> th;
        for (unsigned t = 0; t < nt; t++) th.emplace_back(work, n_rec * t / nt, n_rec * (t + 1) / nt);
        for (auto &x : th) x.join();
    }
    if (bad) return PYA_ERR_ARG;
    int64_t total = 0;
    for (uint64_t r = 0; r < n_rec; r++) {
        str_off[r] = total;
        total += (int64_t)strs[r].size();
    }
    str_off[n_rec] = total;
    if (cap == 0 || !buf) return PYA_OK;                            /* size query */
    if ((uint64_t)total > cap) return PYA_ERR_ARG;
    for (uint64_t r = 0; r < n_rec; r++) std::memcpy(buf + str_off[r], strs[r].data(), strs[r].size());
    return PYA_OK;
}

} /* extern "C" */

extern "C" {

uint64_t pya_get_workspace_budget(const pya_handle *h) { return h ? (uint64_t)workspace_budget(h) : 0; }

int pya_set_workspace_budget(pya_handle *h, uint64_t bytes) {
    if (!h) return PYA_ERR_ARG;
    if (bytes && bytes < ((uint64_t)16 << 20)) return h->fail(PYA_ERR_ARG, -1, "workspace budget below 16 MiB");
    h->ws_budget = (size_t)bytes;
    return PYA_OK;
}

int pya_last_batch_status(pya_handle *h, int32_t *status, uint64_t n) {
    if (!h || !status) return PYA_ERR_ARG;
    if (h->last_status.empty()) {                       /* nothing was set aside (or the flag was not given) */
        std::memset(status, 0, n * sizeof(int32_t));
        return PYA_OK;
    }
    if (n != h->last_status.size()) return h->fail(PYA_ERR_ARG, -1, "the last batch had %zu PSMs", h->last_status.size());
    std::memcpy(status, h->last_status.data(), n * sizeof(int32_t));
    return PYA_OK;
}

int pya_last_batch_evidence(pya_handle *h, pya_evidence *out, uint64_t n_psm, uint32_t max_k) {
    if (!h) return PYA_ERR_ARG;
    if (!h->evid_valid) return h->fail(PYA_ERR_STATE, -1, "the last batch was scored without PYA_FLAG_EVIDENCE");
    if (n_psm != h->evid_n || max_k != h->evid_k)
        return h->fail(PYA_ERR_ARG, -1, "the last batch had %llu PSMs and rows of %u", (unsigned long long)h->evid_n, h->evid_k);
    if (!out && n_psm * max_k != 0) return h->fail(PYA_ERR_ARG, -1, "NULL evidence array");
    if (n_psm * max_k != 0) std::memcpy(out, h->evid_host, (size_t)n_psm * max_k * sizeof(pya_evidence));
    return PYA_OK;
}

int pya_last_batch_ions(pya_handle *h, int64_t *ion_off, pya_ion *out, uint64_t cap) {
    if (!h || !ion_off) return PYA_ERR_ARG;
    if (!h->ions_valid) return h->fail(PYA_ERR_STATE, -1, "the last batch was scored without PYA_FLAG_IONS");
    std::memcpy(ion_off, h->ions_off.data(), h->ions_off.size() * sizeof(int64_t));
    const uint64_t total = (uint64_t)h->ions_off.back();
    if (total == 0 || cap == 0) return PYA_OK;
    if (cap < total)
        return h->fail(PYA_ERR_ARG, -1, "capacity %llu < %llu records", (unsigned long long)cap, (unsigned long long)total);
    if (!out) return h->fail(PYA_ERR_ARG, -1, "NULL ion array");
    std::memcpy(out, h->ions_host, (size_t)total * sizeof(pya_ion));
    return PYA_OK;
}

int pya_last_batch_sites(pya_handle *h, int64_t *site_off, pya_site *out, uint64_t cap) {
    if (!h || !site_off) return PYA_ERR_ARG;
    if (!h->sites_valid) return h->fail(PYA_ERR_STATE, -1, "the last batch was scored without PYA_FLAG_SITES");
    std::memcpy(site_off, h->sites_off.data(), h->sites_off.size() * sizeof(int64_t));
    const uint64_t total = (uint64_t)h->sites_off.back();
    if (total == 0 || cap == 0) return PYA_OK;
    if (cap < total)
        return h->fail(PYA_ERR_ARG, -1, "capacity %llu < %llu records", (unsigned long long)cap, (unsigned long long)total);
    if (!out) return h->fail(PYA_ERR_ARG, -1, "NULL site array");
    std::memcpy(out, h->sites_host, (size_t)total * sizeof(pya_site));
    return PYA_OK;
}

int pya_last_batch_probs(pya_handle *h, int64_t *site_off, pya_site_prob *sites, pya_psm_prob *psms, uint64_t cap) {
    if (!h || !site_off) return PYA_ERR_ARG;
    if (!h->probs_valid) return h->fail(PYA_ERR_STATE, -1, "the last batch was scored without PYA_FLAG_PROBS");
    std::memcpy(site_off, h->probs_off.data(), h->probs_off.size() * sizeof(int64_t));
    const uint64_t total = (uint64_t)h->probs_off.back(), n_psm = h->probs_off.size() - 1;
    if (cap == 0 || n_psm == 0) return PYA_OK;
    if (cap < total)
        return h->fail(PYA_ERR_ARG, -1, "capacity %llu < %llu records", (unsigned long long)cap, (unsigned long long)total);
    if (!psms || (total && !sites)) return h->fail(PYA_ERR_ARG, -1, "NULL probability array");
    if (total) std::memcpy(sites, h->probs_sites(), (size_t)total * sizeof(pya_site_prob));
    std::memcpy(psms, h->probs_psms(), (size_t)n_psm * sizeof(pya_psm_prob));
    return PYA_OK;
}

int pya_last_batch_ranked(pya_handle *h, pya_ranked *out, uint64_t n_psm, uint32_t top_k) {
    if (!h) return PYA_ERR_ARG;
    if (!h->ranked_valid) return h->fail(PYA_ERR_STATE, -1, "the last batch was scored without PYA_FLAG_RANKED");
    if (n_psm != h->ranked_n || top_k != h->ranked_batch_k)
        return h->fail(PYA_ERR_ARG, -1, "the last batch has %llu PSMs with %u rows each, not %llu with %u", (unsigned long long)h->ranked_n,
                       h->ranked_batch_k, (unsigned long long)n_psm, top_k);
    if (n_psm == 0) return PYA_OK;
    if (!out) return h->fail(PYA_ERR_ARG, -1, "NULL record array");
    std::memcpy(out, h->ranked_host, (size_t)n_psm * top_k * sizeof(pya_ranked));
    return PYA_OK;
}

int pya_set_rollup(pya_handle *h, const int32_t *slot, uint64_t n_records, uint64_t n_slots, double threshold, const uint32_t *psm_id) {
    if (!h) return PYA_ERR_ARG;
    h->rollup_loan = pya_handle::RollupLoan{};
    if (n_records && !slot) return h->fail(PYA_ERR_ARG, -1, "pya_set_rollup: NULL slot array for %llu records", (unsigned long long)n_records);
    if (n_slots > 0x7fffffffull) return h->fail(PYA_ERR_ARG, -1, "pya_set_rollup: %llu slots are more than an int32 slot can name", (unsigned long long)n_slots);
    h->rollup_loan.slot = slot;
    h->rollup_loan.psm_id = psm_id;
    h->rollup_loan.n_records = n_records;
    h->rollup_loan.n_slots = n_slots;
    h->rollup_loan.threshold = threshold;
    h->rollup_loan.set = true;
    return PYA_OK;
}

int pya_last_batch_rollup(pya_handle *h, pya_site_rollup *out, uint64_t n_slots) {
    if (!h) return PYA_ERR_ARG;
    if (!h->rollup_valid) return h->fail(PYA_ERR_STATE, -1, "the last batch was scored without PYA_FLAG_ROLLUP");
    if (n_slots != h->rollup_host.size())
        return h->fail(PYA_ERR_ARG, -1, "the table of the last batch has %llu slots, not %llu", (unsigned long long)h->rollup_host.size(),
                       (unsigned long long)n_slots);
    if (n_slots == 0) return PYA_OK;
    if (!out) return h->fail(PYA_ERR_ARG, -1, "NULL record array");
    std::memcpy(out, h->rollup_host.data(), (size_t)n_slots * sizeof(pya_site_rollup));
    return PYA_OK;
}

int pya_rollup_clear(pya_handle *h, pya_site_rollup *d_table, uint64_t n_slots, void *hip_stream) {
    if (!h) return PYA_ERR_ARG;
    if (n_slots == 0) return PYA_OK;
    if (!d_table) return h->fail(PYA_ERR_ARG, -1, "NULL device pointer passed to pya_rollup_clear");
    if (n_slots > 0x7fffffffull) return h->fail(PYA_ERR_ARG, -1, "pya_rollup_clear: %llu slots are more than an int32 slot can name", (unsigned long long)n_slots);
    HIPCHK(h, hipSetDevice(h->device));
    const int e = pya_launch_rollup_clear(d_table, n_slots, (hipStream_t)hip_stream);
    if (e) return h->hip_fail((hipError_t)e, "roll-up clear launch");
    return PYA_OK;
}

int pya_set_ranked_k(pya_handle *h, uint32_t top_k) {
    if (!h) return PYA_ERR_ARG;
    if (top_k < 1u || top_k > PYA_MAX_RANKED) return h->fail(PYA_ERR_ARG, -1, "ranked list length %u is not in 1 .. %d", top_k, PYA_MAX_RANKED);
    h->ranked_k = top_k;
    return PYA_OK;
}

uint32_t pya_get_ranked_k(const pya_handle *h) { return h ? h->ranked_k : 0u; }

int pya_set_site_sig_cap(pya_handle *h, uint32_t sig_cap) {
    if (!h) return PYA_ERR_ARG;
    h->site_sig_cap = sig_cap;
    return PYA_OK;
}

uint32_t pya_get_site_sig_cap(const pya_handle *h) { return h ? h->site_sig_cap : 0u; }

int pya_get_pep_scores_range(pya_handle *h, uint64_t psm_begin, uint64_t psm_end, uint64_t cap, int64_t *rec_off,
                             uint64_t *sig_bits, int32_t *counts, float *scores, float *ws_out,
                             int32_t *nfrag_out) {
    if (!h || !rec_off) return PYA_ERR_ARG;
    pya_plan *p = h->kept;
    if (!p) return h->fail(PYA_ERR_STATE, -1, "no batch retained: call pya_score_batch with PYA_FLAG_KEEP first");
    if (psm_begin > psm_end || psm_end > p->n_psm) return h->fail(PYA_ERR_ARG, -1, "PSM index out of range");
    const int64_t s_begin = p->sig_off[psm_begin], s_end = p->sig_off[psm_end];
    const uint64_t total = (uint64_t)(s_end - s_begin);
    for (uint64_t i = psm_begin; i <= psm_end; i++) rec_off[i - psm_begin] = p->sig_off[i] - s_begin;
    if (total == 0 || cap == 0) return PYA_OK;
    if (cap < total)
        return h->fail(PYA_ERR_ARG, -1, "capacity %llu < %llu records", (unsigned long long)cap,
                       (unsigned long long)total);
    if (!sig_bits || !counts || !scores || !ws_out || !nfrag_out) return h->fail(PYA_ERR_ARG, -1, "NULL output array");
    HIPCHK(h, hipSetDevice(h->device));
    /* one copy per workspace array for the whole range, then the permutation on the host */
    const uint32_t RW = h->rec_words(), NT = h->n_top;
    std::vector<uint32_t> rec((size_t)total * RW), sorted(total);
    std::vector<float> ws(total);
    HIPCHK(h, hipMemcpy(rec.data(), p->d_rec.p + s_begin * RW, rec.size() * 4, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(sorted.data(), p->d_sorted.p + s_begin, (size_t)total * 4, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(ws.data(), p->d_ws.p + s_begin, (size_t)total * 4, hipMemcpyDeviceToHost));
    for (uint64_t psm = psm_begin; psm < psm_end; psm++) {
        const uint32_t N = p->n_sig[psm];
        const size_t o = (size_t)(p->sig_off[psm] - s_begin);
        const uint64_t *order = h->order_tab.data() + p->order_off[psm];
        for (uint32_t r = 0; r < N; r++) {
            const uint32_t i = sorted[o + r];
            if (i >= N) return h->fail(PYA_ERR_HIP, (int64_t)psm, "corrupt sort permutation");
            const uint32_t *w = &rec[(o + i) * RW];
            const uint32_t nf = w[RW - 1];
            sig_bits[o + r] = order[i];
            ws_out[o + r] = ws[o + i];
            nfrag_out[o + r] = (int32_t)nf;
            for (uint32_t d = 0; d < NT; d++) {
                const uint32_t c = (w[d >> 1] >> ((d & 1) * 16)) & 0xffffu;
                counts[(o + r) * NT + d] = (int32_t)c;
                /* same table the kernels read (score_table.cpp) */
                scores[(o + r) * NT + d] =
                    nf < h->lut_off.size() ? h->lut[h->lut_off[nf] + (uint32_t)d * (nf + 1) + c] : 0.f;
            }
        }
    }
    return PYA_OK;
}

int pya_get_pep_scores(pya_handle *h, uint64_t psm, uint64_t cap, uint64_t *n_out, uint64_t *sig_bits,
                       int32_t *counts, float *scores, float *ws_out, int32_t *nfrag_out) {
    if (!h || !n_out) return PYA_ERR_ARG;
    int64_t off[2] = {0, 0};
    const int rc = pya_get_pep_scores_range(h, psm, psm + 1, 0, off, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (rc) return rc;
    *n_out = (uint64_t)off[1];
    if (off[1] == 0 || cap == 0) return PYA_OK;
    return pya_get_pep_scores_range(h, psm, psm + 1, cap, off, sig_bits, counts, scores, ws_out, nfrag_out);
}

int pya_calculate_ambiguity(pya_handle *h, uint64_t psm, uint64_t ref_bits, const float *ref_scores,
                            float ref_ws, uint64_t other_bits, const float *other_scores, float other_ws,
                            float *out) {
    if (!h || !ref_scores || !other_scores || !out) return PYA_ERR_ARG;
    pya_plan *p = h->kept;
    if (!p) return h->fail(PYA_ERR_STATE, -1, "no batch retained: call pya_score_batch with PYA_FLAG_KEEP first");
    if (const int rc_gen = plan_settings_stale(p, "pya_calculate_ambiguity")) return rc_gen;   /* (the retained batch is a plan) */
    if (psm >= p->n_psm) return h->fail(PYA_ERR_ARG, -1, "PSM index out of range");
    HIPCHK(h, hipSetDevice(h->device));
    const int64_t L = p->pep_off[psm + 1] - p->pep_off[psm];
    /* (the one-PSM kernel's retained view carries no peak offsets: its spectra are staged in LDS, never big) */
    const int64_t P = p->peak_off.size() > p->spec(psm) + 1 ? p->n_peaks(psm) : 0;
    const uint32_t NT = h->n_top;                                  /* depth scores per container (Ascore.pyx:196-201) */
    const uint32_t per_type = (uint32_t)std::max<int64_t>(L - 1, 1) * (uint32_t)p->max_charge[psm] * (uint32_t)h->cfg.n_uniq;
    std::vector<float> host_scores(2 * (size_t)NT);
    std::memcpy(host_scores.data(), ref_scores, NT * sizeof(float));
    std::memcpy(host_scores.data() + NT, other_scores, NT * sizeof(float));
    DevBuf<float> d_scores, d_out;
    shared_tables(h, p->dev);
    HIPCHK(h, d_scores.upload(host_scores.data(), host_scores.size()));
    HIPCHK(h, d_out.alloc(2));
    int e;
    /* The fast kernel stages the PSM's retained table in LDS sized by the plan's peak_cap, which covers the spectra of
     * up to PYA_FAST_PEAKS peaks only; it takes peptides of up to 64 residues and ten depths.  Everything else -- a long
     * peptide, n_top 11..16, a spectrum binned by the global kernel -- goes through the general kernel's own Ascore
     * code (general_psm.hip), which reads the retained table where it lies. */
    if (L > PYA_FAST_PEPTIDE_LEN || h->all_general() || P > PYA_FAST_PEAKS || per_type > PYA_FAST_FRAGMENTS_PER_TYPE) {
        if (pya_general_lds_bytes((uint32_t)L, per_type) > kMaxLds)
            return h->fail(PYA_ERR_LIMIT, (int64_t)psm, "calculate_ambiguity: %u fragments per ion type exceed the general kernel's room", per_type);
        e = pya_launch_general_ambiguity(&p->dev, (uint32_t)psm, (uint32_t)L, per_type, ref_bits, other_bits, d_scores.p, NT,
                                         ref_ws, other_ws, d_out.p, nullptr);
    } else {
        const uint32_t list_cap = next_pow2(std::max<uint32_t>(1, per_type));
        e = pya_launch_ambiguity(&p->dev, (uint32_t)psm, p->peak_cap, list_cap, ref_bits, other_bits, d_scores.p,
                                 ref_ws, other_ws, d_out.p, nullptr);
    }
    if (e) return h->hip_fail((hipError_t)e, "ambiguity launch");
    float res[2];
    HIPCHK(h, hipMemcpy(res, d_out.p, sizeof res, hipMemcpyDeviceToHost));
    if (res[1] != 0.f) return h->fail(PYA_ERR_LIMIT, (int64_t)psm, "trial count outside the score table");
    *out = res[0];
    return PYA_OK;
}

int pya_debug_table_sizes(const pya_handle *h, uint64_t out[4]) {
    if (!h || !out) return PYA_ERR_ARG;
    out[0] = (uint64_t)h->order_uploaded;
    out[1] = (uint64_t)h->lut_uploaded_n;
    out[2] = h->cfg_uploads;
    out[3] = (uint64_t)(uintptr_t)h->d_lut.p;
    return PYA_OK;
}

/* The fused body's decision for one PSM, restated (span_guard.h; fused_core.hip.h: residues, presorted, wide, no_cross): the
 * residue states as the kernel builds them -- table mass, + mod_mass, the fixed modifications added to both in list order,
 * all in float32 -- and the same guard functions. */
int pya_debug_span_guard(const pya_handle *h, const char *peptide, uint64_t len, const uint32_t *aux_pos, const float *aux_mass,
                         uint64_t n_aux, double out[3]) {
    if (!h || !peptide || len < 1 || len > 64 || (n_aux && (!aux_pos || !aux_mass))) return PYA_ERR_ARG;
    const int L = (int)len;
    const bool allow_n = h->mod_group.find('n') != std::string::npos, allow_c = h->mod_group.find('c') != std::string::npos;
    float m0[64], m1[64];
    bool modifiable[64];
    for (int r = 0; r < L; r++) {
        const char up = peptide[r];
        if (up < 'A' || up > 'Z') return PYA_ERR_ARG;
        m0[r] = std_residue_mass(up);
        m1[r] = m0[r] + h->mod_mass;
        modifiable[r] = h->mod_group.find(up) != std::string::npos || (allow_n && r == 0) || (allow_c && r == L - 1);
    }
    for (uint64_t j = 0; j < n_aux; j++) {
        const uint64_t idx = aux_pos[j] > 0 ? aux_pos[j] - 1 : 0;
        if (idx >= len) return PYA_ERR_ARG;
        m0[idx] += aux_mass[j];
        m1[idx] += aux_mass[j];
    }
    const float wide_min = 2.f * h->mz_error + 0.02f;
    bool pre = true;                                         /* presorted and wide */
    float heaviest = 0.f;
    for (int r = 0; r < L; r++) {
        pre = pre && m0[r] > 0.f && m1[r] > 0.f && m0[r] > wide_min && m1[r] > wide_min;
        const float top = m0[r] > m1[r] ? m0[r] : m1[r];
        heaviest = top > heaviest ? top : heaviest;
    }
    const SpanGuard g = span_guard_make(h->mz_error, h->mod_mass, L, heaviest);
    bool ok = pre && g.ok;
    for (int r = 0; r < L; r++) ok = ok && !span_guard_residue_fails(g, m0[r], m1[r], modifiable[r]);
    if (out) {
        out[0] = g.E;
        out[1] = g.d_min;
        out[2] = g.d_max;
    }
    return ok ? 1 : 0;
}

/* The composite keys of the common-case binning bodies (bin_key.h), by the header's own functions: the key base from the
 * largest high word of the array, as a spectrum's most intense peak gives it. */
int pya_debug_bin_keys(const double *intensity, const uint32_t *window, uint64_t n, uint32_t *keys, uint32_t *key_base) {
    if (n < 1 || !intensity || !window || !keys) return PYA_ERR_ARG;
    uint32_t maxhw = 0;
    for (uint64_t i = 0; i < n; i++) {
        uint64_t bits;
        std::memcpy(&bits, &intensity[i], 8);
        const uint32_t hw = (uint32_t)(bits >> 32);
        if (hw >= 0x7ff00000u || window[i] >= PYA_BIN_FAST_WINDOWS) return PYA_ERR_ARG;   /* negative, infinite, NaN: no fast path */
        maxhw = hw > maxhw ? hw : maxhw;
    }
    const uint32_t base = bin_key_base(maxhw);
    for (uint64_t i = 0; i < n; i++) {
        uint64_t bits;
        std::memcpy(&bits, &intensity[i], 8);
        keys[i] = bin_key_bits((uint32_t)(bits >> 32), base, window[i]);
    }
    if (key_base) *key_base = base;
    return PYA_OK;
}

int pya_debug_wave_ops(pya_handle *h, const int32_t in[64], int32_t out[263]) {
    if (!h || !in || !out) return PYA_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    DevBuf<int32_t> di, dout;
    HIPCHK(h, di.upload(in, 64));
    HIPCHK(h, dout.alloc(263));
    HIPCHK(h, hipMemset(dout.p, 0, 263 * sizeof(int32_t)));
    int e = pya_launch_debug_wave_ops(di.p, dout.p, nullptr);
    if (e) return h->hip_fail((hipError_t)e, "debug wave ops launch");
    HIPCHK(h, hipMemcpy(out, dout.p, 263 * sizeof(int32_t), hipMemcpyDeviceToHost));
    return PYA_OK;
}

/* ---- the device building blocks, one at a time (include/pyascore_debug.h; the kernels: debug_ops.hip) ---- */
int pya_debug_lookup(pya_handle *h, const float *mz, const uint32_t *rank, uint32_t n, float mz_error, const float *query, uint32_t n_query,
                     uint8_t *out, uint32_t cells[257]) {
    if (!h) return PYA_ERR_ARG;
    if (n > PYA_DEBUG_LOOKUP_MAX_N || (n && (!mz || !rank)) || (n_query && (!query || !out)) || !cells)
        return h->fail(PYA_ERR_ARG, -1, "debug lookup: a NULL array, or more than %d entries", PYA_DEBUG_LOOKUP_MAX_N);
    if (!(mz_error > 0.f) || !(mz_error < 50.f)) return h->fail(PYA_ERR_ARG, -1, "debug lookup: mz_error must be in (0, 50)");
    for (uint32_t i = 0; i < n; i++)
        if (!std::isfinite(mz[i]) || (i && mz[i] < mz[i - 1]) || rank[i] >= PYA_NO_MATCH)
            return h->fail(PYA_ERR_ARG, (int64_t)i, "debug lookup: entry %u is not one of a retained table (finite, ascending, rank < %d)", i,
                           PYA_NO_MATCH);
    /* behind the table: entries that would match if the global lookup did not mask what it reads past the last one */
    std::vector<PeakEntry> tab((size_t)n + PYA_TABLE_PAD);
    for (size_t i = 0; i < tab.size(); i++) {
        tab[i].mz = i < n ? mz[i] : (n ? mz[n - 1] : 0.f);
        tab[i].rank = i < n ? rank[i] : 0u;
    }
    DevConfig cfg;
    std::memset(&cfg, 0, sizeof cfg);
    cfg.mz_error = mz_error;
    HIPCHK(h, hipSetDevice(h->device));
    DevBuf<PeakEntry> d_tab;
    DevBuf<DevConfig> d_cfg;
    DevBuf<uint16_t> d_grid;
    DevBuf<uint32_t> d_cells;
    DevBuf<float> d_query;
    DevBuf<uint8_t> d_out;
    HIPCHK(h, d_tab.upload(tab.data(), tab.size()));
    HIPCHK(h, d_cfg.upload(&cfg, 1));
    HIPCHK(h, d_grid.alloc(PYA_GRID_CELLS));
    HIPCHK(h, d_cells.alloc(PYA_GRID_CELLS + 1));
    HIPCHK(h, d_query.upload(query, n_query));
    HIPCHK(h, d_out.alloc((size_t)n_query * 4));
    HIPCHK(h, hipMemset(d_out.p, 0xee, n_query ? (size_t)n_query * 4 : 1));
    int e = pya_launch_debug_lookup(d_tab.p, n, d_cfg.p, d_grid.p, d_cells.p, d_query.p, n_query, d_out.p, nullptr);
    if (e) return h->hip_fail((hipError_t)e, "debug lookup launch");
    HIPCHK(h, hipMemcpy(cells, d_cells.p, (PYA_GRID_CELLS + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (n_query) HIPCHK(h, hipMemcpy(out, d_out.p, (size_t)n_query * 4, hipMemcpyDeviceToHost));
    return PYA_OK;
}

int pya_debug_lane_ops(pya_handle *h, uint32_t op, const uint64_t *a, const uint64_t *b, uint64_t n, uint64_t *out) {
    if (!h) return PYA_ERR_ARG;
    if (op >= PYA_DBG_LANE_OPS || n > ((uint64_t)1 << 28) || (n && (!a || !b || !out))) return h->fail(PYA_ERR_ARG, -1, "debug lane ops: op %u, n", op);
    for (uint64_t i = 0; i < n; i++)
        if ((op == PYA_DBG_CHARGE_MZ && (b[i] < 1 || b[i] > 255)) || (op == PYA_DBG_NL_BUMP && (b[i] < 1 || b[i] > 16)))
            return h->fail(PYA_ERR_ARG, (int64_t)i, "debug lane ops: operand %llu outside the function's domain", (unsigned long long)i);
    if (n == 0) return PYA_OK;
    HIPCHK(h, hipSetDevice(h->device));
    DevBuf<uint64_t> da, db, dout;
    HIPCHK(h, da.upload(a, n));
    HIPCHK(h, db.upload(b, n));
    HIPCHK(h, dout.alloc(n));
    int e = pya_launch_debug_lane_ops(op, da.p, db.p, n, dout.p, nullptr);
    if (e) return h->hip_fail((hipError_t)e, "debug lane ops launch");
    HIPCHK(h, hipMemcpy(out, dout.p, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return PYA_OK;
}

int pya_debug_wave64(pya_handle *h, uint32_t op, const uint64_t *in, uint64_t *out) {
    if (!h) return PYA_ERR_ARG;
    if (op >= PYA_DBG_WAVE_OPS || !in || !out) return h->fail(PYA_ERR_ARG, -1, "debug wave64: op %u", op);
    HIPCHK(h, hipSetDevice(h->device));
    DevBuf<uint64_t> di, dout;
    HIPCHK(h, di.upload(in, PYA_DBG_WAVE_IN));
    HIPCHK(h, dout.alloc(PYA_DBG_WAVE_OUT));
    HIPCHK(h, hipMemset(dout.p, 0, PYA_DBG_WAVE_OUT * sizeof(uint64_t)));
    int e = op == PYA_DBG_ION_SCAN_U64 ? pya_launch_debug_ion_wave_scan(di.p, dout.p, nullptr) : pya_launch_debug_wave64(op, di.p, dout.p, nullptr);
    if (e) return h->hip_fail((hipError_t)e, "debug wave64 launch");
    HIPCHK(h, hipMemcpy(out, dout.p, PYA_DBG_WAVE_OUT * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return PYA_OK;
}

int pya_debug_block_scan(pya_handle *h, uint32_t policy, const uint32_t *in, uint32_t *out) {
    if (!h) return PYA_ERR_ARG;
    if (policy > PYA_DBG_SCAN_SEG || !in || !out) return h->fail(PYA_ERR_ARG, -1, "debug block scan: policy %u", policy);
    const size_t words = policy == PYA_DBG_SCAN_SEG ? 3 : 1;
    HIPCHK(h, hipSetDevice(h->device));
    DevBuf<uint32_t> di, dout;
    HIPCHK(h, di.upload(in, 256 * words));
    HIPCHK(h, dout.alloc(257 * words));
    int e = pya_launch_debug_block_scan(policy, di.p, dout.p, nullptr);
    if (e) return h->hip_fail((hipError_t)e, "debug block scan launch");
    HIPCHK(h, hipMemcpy(out, dout.p, 257 * words * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return PYA_OK;
}

int pya_debug_ts_scan(pya_handle *h, uint32_t policy, uint32_t *data, uint64_t n) {
    if (!h) return PYA_ERR_ARG;
    if (policy > PYA_DBG_SCAN_SEG || n > ((uint64_t)1 << 24) || (n && !data)) return h->fail(PYA_ERR_ARG, -1, "debug ts scan: policy %u, n", policy);
    if (n == 0) return PYA_OK;
    const size_t words = policy == PYA_DBG_SCAN_SEG ? 3 : 1;
    HIPCHK(h, hipSetDevice(h->device));
    DevBuf<uint32_t> d;
    HIPCHK(h, d.alloc((size_t)pya_ts_scan_entries(n) * words));
    HIPCHK(h, hipMemcpy(d.p, data, (size_t)n * words * sizeof(uint32_t), hipMemcpyHostToDevice));
    int e = pya_launch_debug_ts_scan(policy, d.p, n, nullptr);
    if (e) return h->hip_fail((hipError_t)e, "debug ts scan launch");
    HIPCHK(h, hipMemcpy(data, d.p, (size_t)n * words * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return PYA_OK;
}

int pya_debug_ions_scan(pya_handle *h, int64_t *off, uint32_t n) {
    if (!h) return PYA_ERR_ARG;
    if (!off || n < 1 || n > (1u << 24)) return h->fail(PYA_ERR_ARG, -1, "debug ions scan: n");
    HIPCHK(h, hipSetDevice(h->device));
    DevBuf<int64_t> d;
    DevBuf<uint64_t> tiles;
    HIPCHK(h, d.upload(off, (size_t)n + 1));
    HIPCHK(h, tiles.alloc(pya_ions_scan_tiles(n)));
    int e = pya_launch_ions_scan(d.p, n, tiles.p, nullptr);
    if (e) return h->hip_fail((hipError_t)e, "debug ions scan launch");
    HIPCHK(h, hipMemcpy(off, d.p, ((size_t)n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
    return PYA_OK;
}

int pya_debug_sort(pya_handle *h, const float *keys, uint32_t n, uint32_t *perm) {
    if (!h || !keys || !perm) return PYA_ERR_ARG;
    if (n == 0) return PYA_OK;
    if (n > PYA_MAX_SIGNATURES) return h->fail(PYA_ERR_LIMIT, -1, "n too large");
    HIPCHK(h, hipSetDevice(h->device));
    DevBuf<float> dk;
    DevBuf<uint32_t> dp;
    HIPCHK(h, dk.upload(keys, n));
    HIPCHK(h, dp.alloc(n));
    int e = pya_launch_debug_sort(dk.p, n, dp.p, nullptr);
    if (e) return h->hip_fail((hipError_t)e, "debug sort launch");
    HIPCHK(h, hipMemcpy(perm, dp.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return PYA_OK;
}

/* (include/pyascore_debug.h) the retained table the binning family left for one entry of a plan; p == NULL: the one-PSM
 * workspace `d`, one table at offset 0 (the one-PSM view of pya_rescore_last_keep has no offsets of its own either) */
static int debug_retained_table(pya_handle *h, const pya_plan *p, const BatchDev &d, hipStream_t last, uint64_t index, float *mz,
                                uint32_t *rank, uint64_t cap, uint64_t *n, int32_t *status) {
    *n = 0;
    *status = PYA_ST_OK;
    if (p && p->ret_off.empty()) p = nullptr;
    const bool shared = p && p->shared;
    const uint64_t entries = !p ? 1 : (shared ? p->n_spec : p->n_psm);
    if (index >= entries)
        return h->fail(PYA_ERR_ARG, -1, "retained table: entry %llu of %llu", (unsigned long long)index, (unsigned long long)entries);
    int64_t off = 0;
    if (p) {
        /* an entry the binning family never saw has no table: a PSM the host pre-pass set aside (its code is the status), a
         * shared spectrum whose PSMs were all set aside or that no PSM uses */
        bool binned = false;
        for (uint64_t i = shared ? 0 : index; i < (shared ? p->n_psm : index + 1); i++)
            binned = binned || (p->spec(i) == index && !p->pre_status[i]);
        if (!binned) {
            if (!shared) *status = p->pre_status[index];
            return h->fail(PYA_ERR_ARG, (int64_t)index, "retained table: entry %llu was not binned (set aside by the pre-pass, or a "
                           "spectrum without PSMs)", (unsigned long long)index);
        }
        off = shared ? p->sret_off[index] : p->ret_off[index];
    }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(last));
    const uint32_t *d_n = shared ? p->d_sret_n.p : d.ret_n;
    const int32_t *d_st = shared ? p->d_sstatus.p : d.status;
    uint32_t rn = 0;
    HIPCHK(h, hipMemcpy(&rn, d_n + index, sizeof rn, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(status, d_st + index, sizeof *status, hipMemcpyDeviceToHost));
    *n = rn;
    if (rn == 0) return PYA_OK;
    if (rn > cap || !mz || !rank)
        return h->fail(PYA_ERR_ARG, (int64_t)index, "retained table: %u entries, room for %llu", rn, (unsigned long long)cap);
    std::vector<PeakEntry> e(rn);
    HIPCHK(h, hipMemcpy(e.data(), d.ret + off, (size_t)rn * sizeof(PeakEntry), hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < rn; i++) {
        mz[i] = e[i].mz;
        rank[i] = e[i].rank;
    }
    return PYA_OK;
}

int pya_debug_plan_retained_table(pya_plan *p, uint64_t index, float *mz, uint32_t *rank, uint64_t cap, uint64_t *n, int32_t *status) {
    if (!p || !n || !status) return PYA_ERR_ARG;
    if (!p->ran) return p->h->fail(PYA_ERR_ARG, -1, "retained table: the plan has not run");
    return debug_retained_table(p->h, p, p->dev, p->last_stream, index, mz, rank, cap, n, status);
}

int pya_debug_retained_table(pya_handle *h, uint64_t index, float *mz, uint32_t *rank, uint64_t cap, uint64_t *n, int32_t *status) {
    if (!h || !n || !status) return PYA_ERR_ARG;
    if (h->kept) return pya_debug_plan_retained_table(h->kept, index, mz, rank, cap, n, status);
    if (!h->one.have_last || !h->one.ws.p)
        return h->fail(PYA_ERR_ARG, -1, "retained table: nothing retained and no pya_score_one call yet");
    return debug_retained_table(h, nullptr, h->one.dev, h->one.stream, index, mz, rank, cap, n, status);
}

} /* extern "C" */
