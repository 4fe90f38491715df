/* host_batch.cpp -- pya_score_batch: host arrays in, host results out; chunking and the upload / kernels / download pipeline.
 * The spectra are typed (pya_typed_spectra: float64 or float32 per array, pya_score_batch_typed); every count of their
 * bytes below is of the real ones. */
#include "host_internal.h"
#include "../../include/pyascore_debug.h"

namespace {

const size_t kChunkMin = 32u << 20;          /* spectra bytes below which a call is not worth pipelining */
const size_t kChunkTarget = 96u << 20;       /* spectra bytes per chunk when the budget allows more       */
const size_t kDefaultBudget = (size_t)6 << 30;

}  // namespace

size_t workspace_budget(const pya_handle *h) {
    if (h->ws_budget) return h->ws_budget;
    if (h->kn.workspace_mb > 0) return (size_t)std::max<int64_t>(16, h->kn.workspace_mb) << 20;
    return kDefaultBudget;
}

namespace {

/* Device bytes a chunk [lo, hi) holds while it is scored: its spectra in the upload ring (two
 * slots, so twice) and its arena (retained table, grid, per-signature scores and records, results
 * and metadata).  C(n,k) comes from the peptide letters, as in the plan's pre-pass. */
struct ChunkCost {
    std::vector<double> arena, io;             /* per PSM */
    std::vector<double> ret;                   /* shared spectra: the retained table, kept out of `arena` -- it and `io` count once per spectrum of a chunk */
    std::vector<uint8_t> sites;                /* modifiable residues per PSM, 255 = invalid letters / length */
};
ChunkCost chunk_costs(pya_handle *h, const pya_batch *b, const SpecShare *sh, uint32_t max_k, size_t peak_bytes) {
    const uint64_t n = b->n_psm;
    ChunkCost c;
    c.arena.resize(n);
    c.io.resize(n);
    if (sh) c.ret.resize(n);
    c.sites.assign(n, 255);
    auto work = [&](uint64_t lo, uint64_t hi) {
        for (uint64_t i = lo; i < hi; i++) {
            const uint64_t s = sh ? sh->spec_of[i] : i;
            const int64_t P = std::max<int64_t>(0, b->peak_off[s + 1] - b->peak_off[s]);
            const int64_t L = b->pep_off[i + 1] - b->pep_off[i];
            double sigs = 0;
            uint32_t n_sites = 0;
            if (psm_letters_ok(h, b->pep + b->pep_off[i], L, &n_sites)) {
                const uint32_t ns = n_sites;
                if (ns < 255u) c.sites[i] = (uint8_t)ns;
                uint64_t N = 0;
                if (ns <= PYA_MAX_SITES && b->n_of_mod[i] >= 0 && (uint32_t)b->n_of_mod[i] <= ns) {
                    uint64_t &cached = h->binom_cache[ns][b->n_of_mod[i]];      /* benign race: same value */
                    if (cached == 0) cached = binom(ns, (uint32_t)b->n_of_mod[i]);
                    N = cached;
                }
                sigs = N > PYA_MAX_SIGNATURES ? 0. : (double)N;
            }
            c.io[i] = (double)peak_bytes * (double)P;
            /* per site assignment: PepScore 4 + count record 4 x rec_words (6 for n_top = 10, 9 for 16); a PSM beyond the fast
             * kernels' limits (or any PSM of a scorer with n_top > 10) also has its slice of the general kernel's scratch, a
             * spectrum of more than PYA_FAST_PEAKS peaks the global binning kernel's 15 bytes per peak (sized by the largest) */
            double extra = 0.;
            const uint32_t per_type = (uint32_t)std::max<int64_t>(L - 1, 0) * (uint32_t)std::max(1, std::min(b->max_charge[i], PYA_MAX_CHARGE)) * (uint32_t)h->cfg.n_uniq;
            if (P > PYA_FAST_PEAKS || L > PYA_FAST_PEPTIDE_LEN || sigs > PYA_FAST_SIGNATURES || per_type > PYA_FAST_FRAGMENTS_PER_TYPE || h->all_general()) {
                const uint32_t ns = c.sites[i] == 255 ? 0u : c.sites[i], kk = (uint32_t)std::max(0, b->n_of_mod[i]);
                extra += (double)pya_general_scratch_bytes((uint32_t)sigs, kk <= ns ? ((kk * (ns - kk)) + 3u) & ~3u : 0u) + 256.0;
                if (P > PYA_FAST_PEAKS) extra += 16.0 * (double)PYA_MAX_PEAKS;
            }
            const double ret = 8.0 * (double)(P + 1);
            if (sh) c.ret[i] = ret;
            c.arena[i] = (sh ? 0. : ret) + 8.0 + (4.0 + 4.0 * (double)h->rec_words()) * sigs + extra + (double)L + 2.0 * PYA_GRID_CELLS + 96.0 + 12.0 * max_k;
        }
    };
    for_psm_ranges(n, work);
    return c;
}

/* "PSM 12: ..." of a chunk that starts at PSM `lo` of the caller's batch -> "PSM <12 + lo>: ..." */
void rebase_error(pya_handle *h, uint64_t lo) {
    if (h->err_index >= 0) h->err_index += (int64_t)lo;
    unsigned long long local = 0;
    int used = 0;
    if (lo && std::sscanf(h->err.c_str(), "PSM %llu%n", &local, &used) == 1)
        h->err = "PSM " + std::to_string(local + lo) + h->err.substr((size_t)used);
}

}  // namespace

/* PYA_FLAG_EVIDENCE: the evidence launch of a plan behind its kernels on `st`, and its rows on their way into the handle's
 * pinned block at PSM `lo` (asynchronous: whoever waits for the chunk's results waits for them too) */
static int evidence_behind_run(pya_handle *h, pya_plan *p, const pya_results *d_out, uint64_t lo, hipStream_t st) {
    const size_t n_rec = (size_t)p->n_psm * d_out->max_k;
    if (n_rec == 0) return PYA_OK;
    HIPCHK(h, p->d_evid.alloc(n_rec));
    const int rc = pya_plan_evidence(p, d_out, st, p->d_evid.p);
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(h->evid_host + lo * d_out->max_k, p->d_evid.p, n_rec * sizeof(pya_evidence), hipMemcpyDeviceToHost, st));
    return PYA_OK;
}

/* the handle's block for the rows of a batch of n PSMs (zeroed: a PSM no plan reaches has PYA_EV_NONE rows) */
static int evidence_host_block(pya_handle *h, uint64_t n, uint32_t mk) {
    const size_t n_rec = (size_t)n * mk;
    HIPCHK(h, hipSetDevice(h->device));
    if (h->evid_cap < n_rec) {
        if (h->evid_host) (void)hipHostFree(h->evid_host);
        h->evid_host = nullptr;
        h->evid_cap = 0;
        HIPCHK(h, hipHostMalloc((void **)&h->evid_host, std::max<size_t>(n_rec, 1) * sizeof(pya_evidence), hipHostMallocDefault));
        h->evid_cap = std::max<size_t>(n_rec, 1);
    }
    std::memset(h->evid_host, 0, n_rec * sizeof(pya_evidence));
    h->evid_n = n;
    h->evid_k = mk;
    return PYA_OK;
}

/* PYA_FLAG_IONS: count and scan behind a plan's kernels on `st`, the one wait of the stage (the number of records decides
 * what is allocated), then the fill and the records on their way into the handle's pinned block behind those of the PSMs
 * before `lo` (chunks come in PSM order).  The wait also covers whatever an earlier chunk still copied into the block,
 * which may move when it grows. */
static int ions_behind_run(pya_handle *h, pya_plan *p, const pya_results *d_out, uint64_t lo, hipStream_t st) {
    const uint64_t n = p->n_psm;
    if (n == 0) return PYA_OK;
    HIPCHK(h, p->d_ion_off.alloc(n + 1));
    int rc = pya_plan_ions_count(p, d_out, st, p->d_ion_off.p);
    if (rc) return rc;
    std::vector<int64_t> off(n + 1);
    HIPCHK(h, hipMemcpyAsync(off.data(), p->d_ion_off.p, (n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    const int64_t base = h->ions_off[lo], total = off[n];
    if (total < 0) return h->fail(PYA_ERR_HIP, -1, "corrupt ion offsets");
    for (uint64_t i = 0; i < n; i++) h->ions_off[lo + 1 + i] = base + off[i + 1];
    if (total == 0) return PYA_OK;
    const size_t need = (size_t)(base + total);
    if (h->ions_cap < need) {
        pya_ion *grown = nullptr;
        const size_t cap = need + need / 4;
        HIPCHK(h, hipHostMalloc((void **)&grown, cap * sizeof(pya_ion), hipHostMallocDefault));
        if (base) std::memcpy(grown, h->ions_host, (size_t)base * sizeof(pya_ion));
        if (h->ions_host) (void)hipHostFree(h->ions_host);
        h->ions_host = grown;
        h->ions_cap = cap;
    }
    HIPCHK(h, p->d_ions.alloc((size_t)total));
    if ((rc = pya_plan_ions(p, d_out, st, p->d_ion_off.p, p->d_ions.p, (uint64_t)total))) return rc;
    HIPCHK(h, hipMemcpyAsync(h->ions_host + base, p->d_ions.p, (size_t)total * sizeof(pya_ion), hipMemcpyDeviceToHost, st));
    return PYA_OK;
}

/* PYA_FLAG_SITES: the handle's pinned block for the site records of a batch.  A PSM has at most as many records as its
 * peptide has modifiable letters (none when it is set aside), and the chunks come in PSM order, so a block of that many
 * never has to grow -- or move -- while a chunk's copy is on its way into it. */
static int sites_host_block(pya_handle *h, const pya_batch *b) {
    size_t bound = 0;
    for (uint64_t i = 0; i < b->n_psm; i++) {
        uint32_t ns = 0;
        if (psm_letters_ok(h, b->pep + b->pep_off[i], b->pep_off[i + 1] - b->pep_off[i], &ns) && ns <= PYA_MAX_SITES) bound += ns;
    }
    HIPCHK(h, hipSetDevice(h->device));
    if (h->sites_cap < bound) {
        if (h->sites_host) (void)hipHostFree(h->sites_host);
        h->sites_host = nullptr;
        h->sites_cap = 0;
        HIPCHK(h, hipHostMalloc((void **)&h->sites_host, (bound + bound / 4) * sizeof(pya_site), hipHostMallocDefault));
        h->sites_cap = bound + bound / 4;
    }
    h->sites_off.assign(b->n_psm + 1, 0);                     /* (a PSM no plan reaches has no records) */
    return PYA_OK;
}

/* ... the site launch of a plan behind its kernels on `st`, and its records on their way into the block behind those of the
 * PSMs before `lo` (asynchronous: whoever waits for the chunk's results waits for them too) */
static int sites_behind_run(pya_handle *h, pya_plan *p, const pya_results *d_out, uint64_t lo, hipStream_t st) {
    const uint64_t n = p->n_psm;
    if (n == 0) return PYA_OK;
    std::vector<int64_t> off(n + 1);
    int rc = pya_plan_site_offsets(p, off.data());
    if (rc) return rc;
    const int64_t base = h->sites_off[lo], total = off[n];
    for (uint64_t i = 0; i < n; i++) h->sites_off[lo + 1 + i] = base + off[i + 1];
    if (total == 0) return PYA_OK;
    if ((size_t)(base + total) > h->sites_cap) return h->fail(PYA_ERR_STATE, -1, "site records beyond the block sized for them");
    HIPCHK(h, p->d_sites.alloc((size_t)total));
    if ((rc = pya_plan_sites(p, d_out, st, h->site_sig_cap, p->d_sites.p))) return rc;
    HIPCHK(h, hipMemcpyAsync(h->sites_host + base, p->d_sites.p, (size_t)total * sizeof(pya_site), hipMemcpyDeviceToHost, st));
    return PYA_OK;
}

/* PYA_FLAG_PROBS: the handle's pinned block for the probability records of a batch -- residue records bounded as the site
 * records are, then one record per PSM, zeroed (PYA_SITE_NONE until a chunk's copy lands) -- sized before the first chunk */
static int probs_host_block(pya_handle *h, const pya_batch *b) {
    size_t bound = 0;
    for (uint64_t i = 0; i < b->n_psm; i++) {
        uint32_t ns = 0;
        if (psm_letters_ok(h, b->pep + b->pep_off[i], b->pep_off[i + 1] - b->pep_off[i], &ns) && ns <= PYA_MAX_SITES) bound += ns;
    }
    HIPCHK(h, hipSetDevice(h->device));
    if (h->probs_cap < bound || h->probs_psm_cap < b->n_psm) {
        if (h->probs_host) (void)hipHostFree(h->probs_host);
        h->probs_host = nullptr;
        h->probs_cap = h->probs_psm_cap = 0;
        const size_t n_sites = bound + bound / 4, n_psms = (size_t)b->n_psm + (size_t)b->n_psm / 4;
        HIPCHK(h, hipHostMalloc((void **)&h->probs_host, n_sites * sizeof(pya_site_prob) + n_psms * sizeof(pya_psm_prob), hipHostMallocDefault));
        h->probs_cap = n_sites;
        h->probs_psm_cap = n_psms;
    }
    std::memset(h->probs_psms(), 0, (size_t)b->n_psm * sizeof(pya_psm_prob));
    h->probs_off.assign(b->n_psm + 1, 0);                     /* (a PSM no plan reaches has no records) */
    return PYA_OK;
}

/* ... the probability launches of a plan behind its kernels on `st`, and the records on their way into the block behind
 * those of the PSMs before `lo` */
static int probs_behind_run(pya_handle *h, pya_plan *p, const pya_results *d_out, uint64_t lo, hipStream_t st) {
    const uint64_t n = p->n_psm;
    if (n == 0) return PYA_OK;
    std::vector<int64_t> off(n + 1);
    int rc = pya_plan_site_offsets(p, off.data());
    if (rc) return rc;
    const int64_t base = h->probs_off[lo], total = off[n];
    for (uint64_t i = 0; i < n; i++) h->probs_off[lo + 1 + i] = base + off[i + 1];
    if ((size_t)(base + total) > h->probs_cap || lo + n > h->probs_psm_cap)
        return h->fail(PYA_ERR_STATE, -1, "probability records beyond the block sized for them");
    HIPCHK(h, p->d_prob_sites.alloc((size_t)std::max<int64_t>(total, 1)));
    HIPCHK(h, p->d_prob_psms.alloc((size_t)n));
    if ((rc = pya_plan_probs(p, d_out, st, h->site_sig_cap, p->d_prob_sites.p, p->d_prob_psms.p))) return rc;
    if (total)
        HIPCHK(h, hipMemcpyAsync(h->probs_sites() + base, p->d_prob_sites.p, (size_t)total * sizeof(pya_site_prob), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipMemcpyAsync(h->probs_psms() + lo, p->d_prob_psms.p, (size_t)n * sizeof(pya_psm_prob), hipMemcpyDeviceToHost, st));
    return PYA_OK;
}

/* PYA_FLAG_RANKED: the handle's pinned block for the ranked localisations of a batch -- ranked_k rows per PSM, zeroed
 * (PYA_RANK_NONE until a chunk's copy lands) -- sized before the first chunk; the list length is fixed for the call here */
static int ranked_host_block(pya_handle *h, const pya_batch *b) {
    const size_t need = (size_t)b->n_psm * h->ranked_k;
    HIPCHK(h, hipSetDevice(h->device));
    if (h->ranked_cap < need) {
        if (h->ranked_host) (void)hipHostFree(h->ranked_host);
        h->ranked_host = nullptr;
        h->ranked_cap = 0;
        const size_t n = need + need / 4;
        HIPCHK(h, hipHostMalloc((void **)&h->ranked_host, n * sizeof(pya_ranked), hipHostMallocDefault));
        h->ranked_cap = n;
    }
    std::memset(h->ranked_host, 0, need * sizeof(pya_ranked));
    h->ranked_n = b->n_psm;
    h->ranked_batch_k = h->ranked_k;
    return PYA_OK;
}

/* ... the ranked launches of a plan behind its kernels on `st`, and the records on their way into the block at the rows of
 * PSM `lo` */
static int ranked_behind_run(pya_handle *h, pya_plan *p, const pya_results *d_out, uint64_t lo, hipStream_t st) {
    const uint64_t n = p->n_psm;
    const uint32_t K = h->ranked_batch_k;
    if (n == 0) return PYA_OK;
    if ((size_t)(lo + n) * K > h->ranked_cap) return h->fail(PYA_ERR_STATE, -1, "ranked records beyond the block sized for them");
    HIPCHK(h, p->d_ranked.alloc((size_t)n * K));
    const int rc = pya_plan_ranked(p, d_out, st, K, h->site_sig_cap, p->d_ranked.p);
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(h->ranked_host + (size_t)lo * K, p->d_ranked.p, (size_t)n * K * sizeof(pya_ranked), hipMemcpyDeviceToHost, st));
    return PYA_OK;
}

/* PYA_FLAG_ROLLUP: the loan of pya_set_rollup becomes the call's; the device table that lives for the call is sized here and
 * cleared in front of the first chunk's launches, on their stream */
static int rollup_begin(pya_handle *h, pya_handle::RollupLoan *loan) {
    *loan = h->rollup_loan;
    h->rollup_loan = pya_handle::RollupLoan{};                /* (the loan ends with this call, whatever it returns) */
    if (!loan->set) return h->fail(PYA_ERR_ARG, -1, "PYA_FLAG_ROLLUP without slots: call pya_set_rollup before the batch call");
    HIPCHK(h, hipSetDevice(h->device));
    if (h->d_rollup.n < loan->n_slots || !h->d_rollup.p) HIPCHK(h, h->d_rollup.alloc((size_t)loan->n_slots));
    h->rollup_seen = 0;
    h->rollup_cleared = false;
    return PYA_OK;
}

/* ... the plan's slice of the caller's slots and ids on its way to the device on `st`, IN FRONT of the plan's run: the arrays
 * are the caller's pageable memory, a copy from there holds this thread until the stream gets to it, and in front of the run
 * the stream is idle (the chunk before has been waited for) -- behind the run it would keep the host pre-pass of the next
 * chunk from overlapping this chunk's kernels.  The first plan clears the call's table here too. */
static int rollup_upload(pya_handle *h, pya_plan *p, const pya_handle::RollupLoan &loan, uint64_t lo, hipStream_t st) {
    const uint64_t n = p->n_psm;
    if (!h->rollup_cleared) {
        const int rc0 = pya_rollup_clear(h, h->d_rollup.p, loan.n_slots, st);
        if (rc0) return rc0;
        h->rollup_cleared = true;
    }
    if (n == 0) return PYA_OK;
    std::vector<int64_t> off(n + 1);
    const int rc = pya_plan_site_offsets(p, off.data());
    if (rc) return rc;
    const uint64_t base = h->rollup_seen, total = (uint64_t)off[n];
    if (base + total > loan.n_records)
        return h->fail(PYA_ERR_ARG, -1, "pya_set_rollup lent %llu slots, the PSMs up to %llu have %llu residue records already",
                       (unsigned long long)loan.n_records, (unsigned long long)(lo + n), (unsigned long long)(base + total));
    h->rollup_seen = base + total;
    if (total == 0) return PYA_OK;
    HIPCHK(h, p->d_rollup_slot.alloc((size_t)total));
    HIPCHK(h, hipMemcpyAsync(p->d_rollup_slot.p, loan.slot + base, (size_t)total * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (loan.psm_id) {
        HIPCHK(h, p->d_rollup_id.alloc((size_t)n));
        HIPCHK(h, hipMemcpyAsync(p->d_rollup_id.p, loan.psm_id + lo, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    }
    return PYA_OK;
}

/* ... and the roll-up of the plan behind its probability stage on `st` (the stage of PYA_FLAG_PROBS when the call has it, its
 * own otherwise: the records stay on the device) */
static int rollup_behind_run(pya_handle *h, pya_plan *p, const pya_results *d_out, const pya_handle::RollupLoan &loan, uint32_t flags, uint64_t lo,
                             hipStream_t st) {
    const uint64_t n = p->n_psm;
    if (n == 0) return PYA_OK;
    const uint64_t total = p->d_rollup_slot.n;               /* (rollup_upload: the plan's residue records) */
    if (!(flags & PYA_FLAG_PROBS)) {
        HIPCHK(h, p->d_prob_sites.alloc((size_t)std::max<uint64_t>(total, 1)));
        HIPCHK(h, p->d_prob_psms.alloc((size_t)n));
        const int rc = pya_plan_probs(p, d_out, st, h->site_sig_cap, p->d_prob_sites.p, p->d_prob_psms.p);
        if (rc) return rc;
    }
    if (total == 0) return PYA_OK;
    return pya_plan_rollup(p, d_out, st, p->d_prob_sites.p, p->d_prob_psms.p, p->d_rollup_slot.p, loan.n_slots, loan.threshold,
                           loan.psm_id ? p->d_rollup_id.p : nullptr, (uint32_t)lo, h->d_rollup.p);
}

/* ... and the end of the call, when every chunk has been waited for: the records must have been exactly the lent ones; the
 * table comes to the host */
static int rollup_end(pya_handle *h, const pya_handle::RollupLoan &loan) {
    if (h->rollup_seen != loan.n_records)
        return h->fail(PYA_ERR_ARG, -1, "pya_set_rollup lent %llu slots, the batch has %llu residue records", (unsigned long long)loan.n_records,
                       (unsigned long long)h->rollup_seen);
    pya_site_rollup empty = {};
    empty.best_psm = PYA_ROLLUP_NO_PSM;
    h->rollup_host.assign((size_t)loan.n_slots, empty);
    if (loan.n_slots && h->rollup_cleared)
        HIPCHK(h, hipMemcpy(h->rollup_host.data(), h->d_rollup.p, (size_t)loan.n_slots * sizeof(pya_site_rollup), hipMemcpyDeviceToHost));
    h->rollup_valid = true;
    return PYA_OK;
}

/* PYA_FLAG_PEPTIDOFORMS: the loan of pya_set_peptidoforms becomes the call's; the two device lists that live for the call
 * (a list cannot be longer than the batch has PSMs) are sized here */
static int pform_begin(pya_handle *h, pya_handle::PformLoan *loan, uint64_t n_psm) {
    *loan = h->pform_loan;
    h->pform_loan = pya_handle::PformLoan{};                  /* (the loan ends with this call, whatever it returns) */
    if (!loan->set) return h->fail(PYA_ERR_ARG, -1, "PYA_FLAG_PEPTIDOFORMS without groups: call pya_set_peptidoforms before the batch call");
    if (loan->n_psm != n_psm)
        return h->fail(PYA_ERR_ARG, -1, "pya_set_peptidoforms lent the groups of %llu PSMs, the batch has %llu", (unsigned long long)loan->n_psm,
                       (unsigned long long)n_psm);
    HIPCHK(h, hipSetDevice(h->device));
    for (auto &d : h->d_pform)
        if (d.n < n_psm || !d.p) HIPCHK(h, d.alloc((size_t)n_psm));
    if (!h->d_pform_n.p) HIPCHK(h, h->d_pform_n.alloc(2));
    h->pform_len = 0;
    h->pform_cur = 0;
    return PYA_OK;
}

/* PYA_FLAG_PFORM_QUANT: the loan of pya_set_peptidoform_quant becomes the call's (h->pfq_call; pfq_active says that the
 * peptidoform hooks below carry a table); the matrix goes to the device once, the two device tables that travel with the two
 * lists are sized here.  Behind pform_begin. */
static int pfq_begin(pya_handle *h, uint64_t n_psm, uint32_t flags) {
    h->pfq_call = h->pfq_loan;
    h->pfq_loan = pya_handle::QuantLoan{};                    /* (the loan ends with this call, whatever it returns) */
    const pya_handle::QuantLoan &loan = h->pfq_call;
    if (!(flags & PYA_FLAG_PEPTIDOFORMS))
        return h->fail(PYA_ERR_ARG, -1, "PYA_FLAG_PFORM_QUANT without PYA_FLAG_PEPTIDOFORMS: the table is row-aligned with the same call's list");
    if (!loan.set) return h->fail(PYA_ERR_ARG, -1, "PYA_FLAG_PFORM_QUANT without a matrix: call pya_set_peptidoform_quant before the batch call");
    if (loan.n_psm != n_psm)
        return h->fail(PYA_ERR_ARG, -1, "pya_set_peptidoform_quant lent the rows of %llu PSMs, the batch has %llu", (unsigned long long)loan.n_psm,
                       (unsigned long long)n_psm);
    const size_t n_ch = loan.params.n_channels, n_cell = (size_t)n_psm * n_ch, n_val = (size_t)loan.n_rows * n_ch;
    HIPCHK(h, hipSetDevice(h->device));
    for (auto &d : h->d_pfq_head)
        if (d.n < n_psm || !d.p) HIPCHK(h, d.alloc((size_t)n_psm));
    for (auto &d : h->d_pfq_cell)
        if (d.n < n_cell || !d.p) HIPCHK(h, d.alloc(n_cell));
    if (h->d_pfq_values.n < n_val || !h->d_pfq_values.p) HIPCHK(h, h->d_pfq_values.alloc(n_val));
    /* (before any stream of the call has work: the chunks' streams do not wait for this one) */
    if (n_val && n_psm) HIPCHK(h, hipMemcpyAsync(h->d_pfq_values.p, loan.values, n_val * sizeof(double), hipMemcpyHostToDevice, nullptr));
    HIPCHK(h, hipStreamSynchronize(nullptr));
    h->pfq_active = true;
    return PYA_OK;
}

/* ... the plan's slice of the caller's groups and ids on its way to the device on `st`, in front of the plan's run as the
 * roll-up's slots are (rollup_upload says why), and the workspace for the plan's PSMs and the list so far, which the host
 * knows: the chunk before has been waited for */
static int pform_upload(pya_handle *h, pya_plan *p, const pya_handle::PformLoan &loan, uint64_t lo, hipStream_t st) {
    const uint64_t n = p->n_psm;
    if (n == 0) return PYA_OK;
    std::vector<int64_t> off(n + 1);
    const int rc = pya_plan_site_offsets(p, off.data());
    if (rc) return rc;
    p->pform_records = (uint64_t)off[n];
    HIPCHK(h, p->d_pform_group.alloc((size_t)n));
    HIPCHK(h, hipMemcpyAsync(p->d_pform_group.p, loan.group + lo, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (loan.psm_id) {
        HIPCHK(h, p->d_pform_id.alloc((size_t)n));
        HIPCHK(h, hipMemcpyAsync(p->d_pform_id.p, loan.psm_id + lo, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    }
    const uint64_t need = pya_peptidoform_workspace_bytes(n + h->pform_len);
    if (h->d_pform_work.n < need || !h->d_pform_work.p) HIPCHK(h, h->d_pform_work.alloc((size_t)need));
    if (h->pfq_active && h->pfq_call.row) {                   /* (the plan's slice of the caller's rows, as quant_upload sends them) */
        HIPCHK(h, p->d_pfq_row.alloc((size_t)n));
        HIPCHK(h, hipMemcpyAsync(p->d_pfq_row.p, h->pfq_call.row + lo, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    }
    return PYA_OK;
}

/* ... the stage of the plan behind its probability stage on `st` (the stage of PYA_FLAG_PROBS or of the roll-up when the call
 * has one, its own otherwise): the list so far goes in as d_prev, the other list takes the result, its length follows */
static int pform_behind_run(pya_handle *h, pya_plan *p, const pya_results *d_out, const pya_handle::PformLoan &loan, uint32_t flags, uint64_t lo,
                            hipStream_t st) {
    const uint64_t n = p->n_psm;
    if (n == 0) return PYA_OK;
    if (!(flags & (PYA_FLAG_PROBS | PYA_FLAG_ROLLUP))) {
        HIPCHK(h, p->d_prob_sites.alloc((size_t)std::max<uint64_t>(p->pform_records, 1)));
        HIPCHK(h, p->d_prob_psms.alloc((size_t)n));
        const int rc = pya_plan_probs(p, d_out, st, h->site_sig_cap, p->d_prob_sites.p, p->d_prob_psms.p);
        if (rc) return rc;
    }
    const int cur = h->pform_cur;
    /* (with PYA_FLAG_PFORM_QUANT the same list by the same launches, and the table of the list so far goes in beside it) */
    const pya_handle::QuantLoan &q = h->pfq_call;
    /* (the rows all three arrays of the result have room for; a list cannot be longer than the batch has PSMs) */
    /* ... and no more than this call's list can have, since the call clears that many rows of the table */
    const uint64_t pfq_cap = !h->pfq_active ? 0 : std::min<uint64_t>(std::min<uint64_t>(std::min<uint64_t>(h->d_pform[cur ^ 1].n, h->d_pfq_head[cur ^ 1].n),
                                                                                        h->d_pfq_cell[cur ^ 1].n / q.params.n_channels), n + h->pform_len);
    const int rc = h->pfq_active
        ? pya_plan_peptidoform_quant(p, d_out, st, p->d_prob_sites.p, p->d_prob_psms.p, p->d_pform_group.p, loan.threshold,
                                     loan.psm_id ? p->d_pform_id.p : nullptr, (uint32_t)lo, h->d_pform[cur].p, h->d_pfq_head[cur].p,
                                     h->d_pfq_cell[cur].p, h->pform_len, h->d_pfq_values.p, q.n_rows, q.row ? p->d_pfq_row.p : nullptr, (uint32_t)lo,
                                     &q.params, h->d_pform_work.p, h->d_pform_work.n, h->d_pform[cur ^ 1].p, h->d_pfq_head[cur ^ 1].p,
                                     h->d_pfq_cell[cur ^ 1].p, pfq_cap, h->d_pform_n.p)
        : pya_plan_peptidoforms(p, d_out, st, p->d_prob_sites.p, p->d_prob_psms.p, p->d_pform_group.p, loan.threshold,
                                loan.psm_id ? p->d_pform_id.p : nullptr, (uint32_t)lo, h->d_pform[cur].p, h->pform_len, h->d_pform_work.p,
                                h->d_pform_work.n, h->d_pform[cur ^ 1].p, h->d_pform[cur ^ 1].n, h->d_pform_n.p);
    if (rc) return rc;
    h->pform_cur = cur ^ 1;
    HIPCHK(h, hipMemcpyAsync(h->pform_n_host, h->d_pform_n.p, sizeof h->pform_n_host, hipMemcpyDeviceToHost, st));
    return PYA_OK;
}

/* ... once the plan's stream has been waited for: the length of the list, and the error word */
static int pform_collect(pya_handle *h, pya_plan *p, uint64_t lo) {
    if (p->n_psm == 0) return PYA_OK;
    h->pform_len = h->pform_n_host[0];
    if (h->pform_n_host[1])
        return h->fail(PYA_ERR_STATE, (int64_t)lo, "peptidoforms: %u PSMs from %llu have a best_sig that does not fit their residue records",
                       h->pform_n_host[1], (unsigned long long)lo);
    return h->pfq_active ? over_report(p, OVER_PFQ, lo) : PYA_OK;
}

/* ... and the end of the call: the list comes to the host */
static int pform_end(pya_handle *h) {
    h->pform_host.resize((size_t)h->pform_len);
    if (h->pform_len)
        HIPCHK(h, hipMemcpy(h->pform_host.data(), h->d_pform[h->pform_cur].p, (size_t)h->pform_len * sizeof(pya_peptidoform), hipMemcpyDeviceToHost));
    h->pform_valid = true;
    if (h->pfq_active) {                                      /* (the table of that list, row-aligned with it) */
        const size_t n_ch = h->pfq_call.params.n_channels;
        h->pfq_head_host.assign((size_t)h->pform_len, pya_site_quant_head{});
        h->pfq_cell_host.assign((size_t)h->pform_len * n_ch, pya_site_quant{});
        if (h->pform_len) {
            HIPCHK(h, hipMemcpy(h->pfq_head_host.data(), h->d_pfq_head[h->pform_cur].p, (size_t)h->pform_len * sizeof(pya_site_quant_head),
                                hipMemcpyDeviceToHost));
            HIPCHK(h, hipMemcpy(h->pfq_cell_host.data(), h->d_pfq_cell[h->pform_cur].p, (size_t)h->pform_len * n_ch * sizeof(pya_site_quant),
                                hipMemcpyDeviceToHost));
        }
        h->pfq_channels = (uint32_t)n_ch;
        h->pfq_valid = true;
    }
    return PYA_OK;
}

/* PYA_FLAG_MZ_PROFILE: the loan of pya_set_mz_profile becomes the call's; the device table that lives for the call is sized
 * and emptied here */
static int mzp_begin(pya_handle *h, pya_handle::MzpLoan *loan, uint64_t n_psm) {
    *loan = h->mzp_loan;
    h->mzp_loan = pya_handle::MzpLoan{};                      /* (the loan ends with this call, whatever it returns) */
    if (!loan->set) return h->fail(PYA_ERR_ARG, -1, "PYA_FLAG_MZ_PROFILE without slots: call pya_set_mz_profile before the batch call");
    if (loan->n_psm != n_psm)
        return h->fail(PYA_ERR_ARG, -1, "pya_set_mz_profile lent the run slots of %llu PSMs, the batch has %llu", (unsigned long long)loan->n_psm,
                       (unsigned long long)n_psm);
    HIPCHK(h, hipSetDevice(h->device));
    if (h->d_mzp.n < loan->n_slots || !h->d_mzp.p) HIPCHK(h, h->d_mzp.alloc((size_t)loan->n_slots));
    if (loan->n_slots) {                                      /* (before any stream of the call has work: the chunks' streams do not wait for this one) */
        HIPCHK(h, hipMemsetAsync(h->d_mzp.p, 0, (size_t)loan->n_slots * sizeof(pya_mz_profile), nullptr));
        HIPCHK(h, hipStreamSynchronize(nullptr));
    }
    return PYA_OK;
}

/* ... the plan's slice of the caller's slots on its way to the device on `st`, in front of the plan's run as the roll-up's
 * slots are (rollup_upload says why) */
static int mzp_upload(pya_handle *h, pya_plan *p, const pya_handle::MzpLoan &loan, uint64_t lo, hipStream_t st) {
    const uint64_t n = p->n_psm;
    if (n == 0 || !loan.run) return PYA_OK;
    HIPCHK(h, p->d_mzp_run.alloc((size_t)n));
    HIPCHK(h, hipMemcpyAsync(p->d_mzp_run.p, loan.run + lo, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    return PYA_OK;
}

/* ... the stage of the plan behind its run on `st`: it needs no other stage */
static int mzp_behind_run(pya_handle *h, pya_plan *p, const pya_results *d_out, const pya_handle::MzpLoan &loan, hipStream_t st) {
    if (p->n_psm == 0) return PYA_OK;
    return pya_plan_mz_profile(p, d_out, st, loan.run ? p->d_mzp_run.p : nullptr, loan.n_slots, &loan.params, h->d_mzp.p);
}

/* ... and the end of the call, when every chunk has been waited for: the table comes to the host */
static int mzp_end(pya_handle *h, const pya_handle::MzpLoan &loan) {
    h->mzp_host.assign((size_t)loan.n_slots, pya_mz_profile{});
    if (loan.n_slots) HIPCHK(h, hipMemcpy(h->mzp_host.data(), h->d_mzp.p, (size_t)loan.n_slots * sizeof(pya_mz_profile), hipMemcpyDeviceToHost));
    h->mzp_valid = true;
    return PYA_OK;
}

/* PYA_FLAG_QUANT: the loan of pya_set_site_quant becomes the call's; the matrix goes to the device once, the device table that
 * lives for the call is sized by the roll-up's n_slots and emptied here */
static int quant_begin(pya_handle *h, pya_handle::QuantLoan *loan, uint64_t n_psm, uint32_t flags, const pya_handle::RollupLoan &ru) {
    *loan = h->quant_loan;
    h->quant_loan = pya_handle::QuantLoan{};                  /* (the loan ends with this call, whatever it returns) */
    if (!(flags & PYA_FLAG_ROLLUP))
        return h->fail(PYA_ERR_ARG, -1, "PYA_FLAG_QUANT without PYA_FLAG_ROLLUP: the quantification uses the slots of the same call's roll-up");
    if (!loan->set) return h->fail(PYA_ERR_ARG, -1, "PYA_FLAG_QUANT without a matrix: call pya_set_site_quant before the batch call");
    if (loan->n_psm != n_psm)
        return h->fail(PYA_ERR_ARG, -1, "pya_set_site_quant lent the rows of %llu PSMs, the batch has %llu", (unsigned long long)loan->n_psm,
                       (unsigned long long)n_psm);
    const size_t n_ch = loan->params.n_channels, n_cell = (size_t)ru.n_slots * n_ch, n_val = (size_t)loan->n_rows * n_ch;
    HIPCHK(h, hipSetDevice(h->device));
    if (h->d_quant_head.n < ru.n_slots || !h->d_quant_head.p) HIPCHK(h, h->d_quant_head.alloc((size_t)ru.n_slots));
    if (h->d_quant_cell.n < n_cell || !h->d_quant_cell.p) HIPCHK(h, h->d_quant_cell.alloc(n_cell));
    if (h->d_quant_values.n < n_val || !h->d_quant_values.p) HIPCHK(h, h->d_quant_values.alloc(n_val));
    /* (before any stream of the call has work: the chunks' streams do not wait for this one) */
    if (ru.n_slots) {
        HIPCHK(h, hipMemsetAsync(h->d_quant_head.p, 0, (size_t)ru.n_slots * sizeof(pya_site_quant_head), nullptr));
        HIPCHK(h, hipMemsetAsync(h->d_quant_cell.p, 0, n_cell * sizeof(pya_site_quant), nullptr));
    }
    if (n_val && n_psm) HIPCHK(h, hipMemcpyAsync(h->d_quant_values.p, loan->values, n_val * sizeof(double), hipMemcpyHostToDevice, nullptr));
    HIPCHK(h, hipStreamSynchronize(nullptr));
    return PYA_OK;
}

/* ... the plan's slice of the caller's rows on its way to the device on `st`, in front of the plan's run as the roll-up's
 * slots are (rollup_upload says why) */
static int quant_upload(pya_handle *h, pya_plan *p, const pya_handle::QuantLoan &loan, uint64_t lo, hipStream_t st) {
    const uint64_t n = p->n_psm;
    if (n == 0 || !loan.row) return PYA_OK;
    HIPCHK(h, p->d_quant_row.alloc((size_t)n));
    HIPCHK(h, hipMemcpyAsync(p->d_quant_row.p, loan.row + lo, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    return PYA_OK;
}

/* ... the stage of the plan behind its roll-up on `st`: the probability records and the slots are the roll-up's */
static int quant_behind_run(pya_handle *h, pya_plan *p, const pya_results *d_out, const pya_handle::QuantLoan &loan,
                            const pya_handle::RollupLoan &ru, uint64_t lo, hipStream_t st) {
    if (p->n_psm == 0 || p->d_rollup_slot.n == 0) return PYA_OK;     /* (rollup_upload: the plan's residue records) */
    return pya_plan_site_quant(p, d_out, st, p->d_prob_sites.p, p->d_prob_psms.p, p->d_rollup_slot.p, ru.n_slots, h->d_quant_values.p, loan.n_rows,
                               loan.row ? p->d_quant_row.p : nullptr, (uint32_t)lo, &loan.params, h->d_quant_head.p, h->d_quant_cell.p);
}

/* ... and the end of the call, when every chunk has been waited for: the table comes to the host */
static int quant_end(pya_handle *h, const pya_handle::QuantLoan &loan, const pya_handle::RollupLoan &ru) {
    const size_t n_cell = (size_t)ru.n_slots * loan.params.n_channels;
    h->quant_head_host.assign((size_t)ru.n_slots, pya_site_quant_head{});
    h->quant_cell_host.assign(n_cell, pya_site_quant{});
    if (ru.n_slots) {
        HIPCHK(h, hipMemcpy(h->quant_head_host.data(), h->d_quant_head.p, (size_t)ru.n_slots * sizeof(pya_site_quant_head), hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(h->quant_cell_host.data(), h->d_quant_cell.p, n_cell * sizeof(pya_site_quant), hipMemcpyDeviceToHost));
    }
    h->quant_channels = loan.params.n_channels;
    h->quant_valid = true;
    return PYA_OK;
}

/* PYA_FLAG_RECALIBRATE: the loan of pya_set_recalibration becomes the call's.  Everything that can be refused is refused here,
 * before anything is scored: a slot outside the records, PSMs of one spectrum that name different slots.  The slot of every
 * SPECTRUM of the batch is settled once for the whole call (a spectrum whose PSMs a chunk cut separates travels with both
 * parts and must be corrected alike in both), and the records go to the device. */
static int recal_begin(pya_handle *h, pya_handle::RecalLoan *loan, const pya_batch *b, const SpecShare *sh, uint32_t flags) {
    *loan = std::move(h->recal_loan);
    h->recal_loan = pya_handle::RecalLoan{};                  /* (the loan ends with this call, whatever it returns) */
    if (!loan->set) return h->fail(PYA_ERR_ARG, -1, "PYA_FLAG_RECALIBRATE without a calibration: call pya_set_recalibration before the batch call");
    if (loan->n_psm != b->n_psm)
        return h->fail(PYA_ERR_ARG, -1, "pya_set_recalibration lent the run slots of %llu PSMs, the batch has %llu", (unsigned long long)loan->n_psm,
                       (unsigned long long)b->n_psm);
    if (flags & PYA_FLAG_KEEP)
        return h->fail(PYA_ERR_ARG, -1, "PYA_FLAG_RECALIBRATE does not go with PYA_FLAG_KEEP: correct the arrays (pya_recalibrate_spectra) and retain "
                                        "the batch without the flag");
    const uint64_t n_spec = sh ? sh->n_spectra : b->n_psm;
    loan->spec_slot.assign((size_t)n_spec, -1);
    for (uint64_t i = 0; i < b->n_psm; i++) {
        const int32_t r = loan->run ? loan->run[i] : 0;
        if (r < 0) continue;
        if ((uint64_t)r >= loan->n_slots)
            return h->fail(PYA_ERR_LIMIT, (int64_t)i, "PSM %llu: run slot %d is at or above the %llu records of pya_set_recalibration",
                           (unsigned long long)i, r, (unsigned long long)loan->n_slots);
        int32_t &slot = loan->spec_slot[sh ? sh->spec_of[i] : i];
        if (slot >= 0 && slot != r)
            return h->fail(PYA_ERR_ARG, (int64_t)i, "PSM %llu: run slot %d, another PSM of its spectrum names slot %d: a spectrum is corrected once",
                           (unsigned long long)i, r, slot);
        slot = r;
    }
    if (b->n_psm == 0) return PYA_OK;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, h->d_recal.upload(loan->cal.data(), loan->cal.size(), nullptr));
    HIPCHK(h, hipStreamSynchronize(nullptr));                 /* (the chunks' streams do not wait for the null stream) */
    return PYA_OK;
}

/* ... the plan's spectra [spec_lo, spec_lo + n_spec) corrected in place in the library's device copy on `st`, in front of the
 * plan's run: the first kernel that reads them is behind this one on the same stream.  (The slots were checked by
 * recal_begin and the records by pya_set_recalibration, so the kernel's report stays empty.) */
static int recal_before_run(pya_handle *h, pya_plan *p, const pya_handle::RecalLoan &loan, uint64_t spec_lo, uint32_t mz_type, hipStream_t st) {
    const uint64_t ns = p->n_spec;
    if (p->n_psm == 0 || ns == 0) return PYA_OK;
    HIPCHK(h, p->d_recal_slot.alloc((size_t)ns));
    HIPCHK(h, p->d_recal_over.alloc(2));
    HIPCHK(h, hipMemcpyAsync(p->d_recal_slot.p, loan.spec_slot.data() + spec_lo, (size_t)ns * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemsetAsync(p->d_recal_over.p, 0, 2 * sizeof(uint32_t), st));
    const pya_typed_spectra d_sp = {p->d_mz.p, nullptr, mz_type, PYA_F64};
    return pya_recalibrate_spectra(h, &d_sp, p->d_peak_off.p, ns, p->d_recal_slot.p, h->d_recal.p, loan.n_slots, loan.inv_band, st, p->d_mz.p,
                                   p->d_recal_over.p);
}

/* pya_score_batch_named: the handle's pinned block for the records of a call's n_q queries -- [n_q] pya_named, [n_q * n_top]
 * counts, [n_q * n_top] scores -- zeroed */
static int named_host_block(pya_handle *h, uint64_t n_q) {
    const size_t bytes = (size_t)n_q * (sizeof(pya_named) + 8 * (size_t)h->n_top);
    HIPCHK(h, hipSetDevice(h->device));
    if (h->named_cap < bytes) {
        if (h->named_host) (void)hipHostFree(h->named_host);
        h->named_host = nullptr;
        h->named_cap = 0;
        HIPCHK(h, hipHostMalloc((void **)&h->named_host, bytes + bytes / 4, hipHostMallocDefault));
        h->named_cap = bytes + bytes / 4;
    }
    if (bytes) std::memset(h->named_host, 0, bytes);
    return PYA_OK;
}

/* ... a plan's slice of the queries (the PSMs from `lo` of the call) on its way to the device on `st`, ahead of the plan's
 * kernels: the offsets rebased to the slice live in the plan, the bits are the caller's, borrowed for the call */
static int named_upload(pya_handle *h, pya_plan *p, const NamedReq *nq, uint64_t lo, hipStream_t st) {
    const uint64_t n = p->n_psm;
    const int64_t base = nq->q_off[lo], cnt = nq->q_off[lo + n] - base;
    if (n == 0 || cnt == 0) return PYA_OK;
    p->named_q_off.resize(n + 1);
    for (uint64_t i = 0; i <= n; i++) p->named_q_off[i] = nq->q_off[lo + i] - base;
    HIPCHK(h, p->d_named_q_off.alloc(n + 1));
    HIPCHK(h, p->d_named_q_bits.alloc((size_t)cnt));
    HIPCHK(h, p->d_named.alloc((size_t)cnt * (sizeof(pya_named) + 8 * (size_t)h->n_top)));
    HIPCHK(h, hipMemcpyAsync(p->d_named_q_off.p, p->named_q_off.data(), (n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(p->d_named_q_bits.p, nq->q_bits + base, (size_t)cnt * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    return PYA_OK;
}

/* ... the named launch of a plan behind its kernels on `st`, and its records on their way into the handle's pinned block at
 * the slice's first query (asynchronous: whoever waits for the chunk's results waits for them too) */
static int named_behind_run(pya_handle *h, pya_plan *p, const pya_results *d_out, const NamedReq *nq, uint64_t lo, uint64_t n_q,
                            hipStream_t st) {
    const uint64_t n = p->n_psm;
    const int64_t base = nq->q_off[lo], cnt = nq->q_off[lo + n] - base;
    if (n == 0 || cnt == 0) return PYA_OK;
    const size_t row = 4 * (size_t)h->n_top;
    unsigned char *d_rec = p->d_named.p, *d_cnt = d_rec + (size_t)cnt * sizeof(pya_named), *d_sc = d_cnt + (size_t)cnt * row;
    const int rc = pya_plan_named(p, d_out, st, p->d_named_q_off.p, p->d_named_q_bits.p, (uint64_t)cnt, (pya_named *)d_rec,
                                  nq->counts ? (int32_t *)d_cnt : nullptr, nq->scores ? (float *)d_sc : nullptr);
    if (rc) return rc;
    unsigned char *h_rec = h->named_host, *h_cnt = h_rec + (size_t)n_q * sizeof(pya_named), *h_sc = h_cnt + (size_t)n_q * row;
    HIPCHK(h, hipMemcpyAsync(h_rec + (size_t)base * sizeof(pya_named), d_rec, (size_t)cnt * sizeof(pya_named), hipMemcpyDeviceToHost, st));
    if (nq->counts) HIPCHK(h, hipMemcpyAsync(h_cnt + (size_t)base * row, d_cnt, (size_t)cnt * row, hipMemcpyDeviceToHost, st));
    if (nq->scores) HIPCHK(h, hipMemcpyAsync(h_sc + (size_t)base * row, d_sc, (size_t)cnt * row, hipMemcpyDeviceToHost, st));
    return PYA_OK;
}

/* ... and, once they have arrived, out of the block into the caller's arrays */
static void named_deliver(pya_handle *h, const NamedReq *nq, uint64_t lo, uint64_t hi, uint64_t n_q) {
    const int64_t base = nq->q_off[lo], cnt = nq->q_off[hi] - base;
    if (cnt == 0) return;
    const size_t row = 4 * (size_t)h->n_top;
    const unsigned char *h_rec = h->named_host, *h_cnt = h_rec + (size_t)n_q * sizeof(pya_named), *h_sc = h_cnt + (size_t)n_q * row;
    std::memcpy(nq->out + base, h_rec + (size_t)base * sizeof(pya_named), (size_t)cnt * sizeof(pya_named));
    if (nq->counts) std::memcpy(nq->counts + (size_t)base * h->n_top, h_cnt + (size_t)base * row, (size_t)cnt * row);
    if (nq->scores) std::memcpy(nq->scores + (size_t)base * h->n_top, h_sc + (size_t)base * row, (size_t)cnt * row);
}

/* Big pya_score_batch calls: the batch is cut into chunks of consecutive PSMs that fit the device
 * budget and the chunks are pipelined -- a helper thread streams the spectra of chunk c + 1 over
 * PCIe (the bound of this entry point: 16, 12 or 8 bytes per peak) into the other slot of a two-slot ring
 * while this thread plans chunk c, runs its kernels and brings its results back on a second
 * stream.  A call of any size completes; it never fails for lack of workspace. */
static int score_batch_chunked(pya_handle *h, const pya_batch *b, const SpecShare *sh, const pya_typed_spectra &sp,
                               uint32_t flags, const pya_results *out, const std::vector<uint64_t> &cuts,
                               const uint8_t *pre_sites, const NamedReq *nq, const pya_handle::RollupLoan &loan,
                               const pya_handle::PformLoan &pf_loan, const pya_handle::MzpLoan &mzp_loan,
                               const pya_handle::RecalLoan &recal_loan, const pya_handle::QuantLoan &quant_loan) {
    const size_t nchunk = cuts.size() - 1;
    const uint64_t n_q = nq ? (uint64_t)nq->q_off[b->n_psm] : 0;
    /* the spectra [first, last) of chunk c: its PSMs' own unless spectra are shared -- then from the first PSM's to the last
     * PSM's, each uploaded once (a group cut in two travels with both parts) */
    auto spec_lo = [&](size_t c) -> uint64_t { return sh ? sh->spec_of[cuts[c]] : cuts[c]; };
    auto spec_hi = [&](size_t c) -> uint64_t { return sh ? (uint64_t)sh->spec_of[cuts[c + 1] - 1] + 1 : cuts[c + 1]; };
    const uint32_t mk = out->max_k;
    const bool skip = (flags & PYA_FLAG_SKIP_INVALID) != 0;
    HIPCHK(h, hipSetDevice(h->device));
    if (!h->copy_stream) HIPCHK(h, hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
    if (!h->run_stream) HIPCHK(h, hipStreamCreateWithFlags(&h->run_stream, hipStreamNonBlocking));
    size_t slot_peaks = 0;
    for (size_t c = 0; c < nchunk; c++)
        slot_peaks = std::max<size_t>(slot_peaks, (size_t)(b->peak_off[spec_hi(c)] - b->peak_off[spec_lo(c)]));
    const size_t mzb = spec_elem_bytes(sp.mz_type), itb = spec_elem_bytes(sp.intensity_type);
    for (auto &slot : h->io_ring)
        if (slot.n < spec_pair_bytes(slot_peaks, sp)) HIPCHK(h, slot.alloc(spec_pair_bytes(slot_peaks, sp)));
    if (skip) h->last_status.assign(b->n_psm, 0);

    /* uploader: chunk c may be written once chunk c - 2 has been consumed */
    std::mutex mu;
    std::condition_variable cv;
    size_t uploaded = 0, consumed = 0;
    bool stop = false;
    hipError_t up_err = hipSuccess;
    const int device = h->device;
    std::thread uploader([&]() {
        hipError_t e = hipSetDevice(device);
        for (size_t c = 0; c < nchunk && e == hipSuccess; c++) {
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return stop || c < consumed + 2; });
                if (stop) break;
            }
            const int64_t p0 = b->peak_off[spec_lo(c)], np = b->peak_off[spec_hi(c)] - p0;
            unsigned char *dst = h->io_ring[c & 1].p;
            if (np > 0) {
                e = hipMemcpyAsync(dst, spec_at(sp.mz, sp.mz_type, p0), (size_t)np * mzb, hipMemcpyHostToDevice, h->copy_stream);
                if (e == hipSuccess)
                    e = hipMemcpyAsync(dst + spec_inten_offset((size_t)np, sp.mz_type), spec_at(sp.intensity, sp.intensity_type, p0),
                                       (size_t)np * itb, hipMemcpyHostToDevice, h->copy_stream);
                if (e == hipSuccess) e = hipStreamSynchronize(h->copy_stream);
            }
            std::lock_guard<std::mutex> lk(mu);
            up_err = e;
            uploaded = c + 1;
            cv.notify_all();
        }
        std::lock_guard<std::mutex> lk(mu);
        if (e != hipSuccess) up_err = e;
        uploaded = nchunk;                                   /* nobody waits for chunks that will not come */
        cv.notify_all();
    });
    auto finish = [&](int rc) {
        {
            std::lock_guard<std::mutex> lk(mu);
            stop = true;
            cv.notify_all();
        }
        uploader.join();
        return rc;
    };

    /* this thread: plan chunk c + 1 (host pre-pass) while the GPU runs the kernels and the result copy of
     * chunk c; two plans alive at a time */
    auto make_plan = [&](size_t c, pya_plan **pp) -> int {
        const uint64_t lo = cuts[c], hi = cuts[c + 1];
        const uint64_t s_lo = spec_lo(c), s_hi = spec_hi(c);
        const int64_t np = b->peak_off[s_hi] - b->peak_off[s_lo];
        pya_batch sub = *b;
        sub.n_psm = hi - lo;
        sub.peak_off = b->peak_off + s_lo;
        const SpecShare sub_sh = {sh ? sh->spec_of + lo : nullptr, s_hi - s_lo, (uint32_t)s_lo};
        sub.pep_off = b->pep_off + lo;
        sub.n_of_mod = b->n_of_mod + lo;
        sub.max_charge = b->max_charge + lo;
        if (b->aux_off) sub.aux_off = b->aux_off + lo;
        IoReq io = {sp, mk, h->io_ring[c & 1].p, h->io_ring[c & 1].p + spec_inten_offset((size_t)np, sp.mz_type), h->run_stream,
                    pre_sites ? pre_sites + lo : nullptr};
        int rc = plan_create_impl(h, &sub, flags & ~(PYA_FLAG_TIMING | PYA_FLAG_KEEP | PYA_FLAG_RECALIBRATE), &io, sh ? &sub_sh : nullptr, pp);
        if (rc) rebase_error(h, lo);
        return rc;
    };
    typedef std::unique_ptr<pya_plan, void (*)(pya_plan *)> PlanPtr;
    pya_plan *raw = nullptr;
    int rc = make_plan(0, &raw);
    if (rc) return finish(rc);
    PlanPtr cur(raw, pya_plan_destroy), next(nullptr, pya_plan_destroy);
    for (size_t c = 0; c < nchunk; c++) {
        const uint64_t lo = cuts[c], n = cuts[c + 1] - lo;
        pya_plan *p = cur.get();
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return uploaded > c; });
            if (up_err != hipSuccess) {
                lk.unlock();
                return finish(h->hip_fail(up_err, "spectrum upload"));
            }
        }
        pya_results d_out = {mk, p->d_best_score.p, p->d_best_sig.p, p->d_n_sig_out.p, p->d_ascores.p, p->d_alt.p};
        const pya_typed_spectra d_sp = {p->d_mz.p, p->d_inten.p, sp.mz_type, sp.intensity_type};
        if (nq && (rc = named_upload(h, p, nq, lo, h->run_stream))) return finish(rc);
        if ((flags & PYA_FLAG_ROLLUP) && (rc = rollup_upload(h, p, loan, lo, h->run_stream))) return finish(rc);
        if ((flags & PYA_FLAG_PEPTIDOFORMS) && (rc = pform_upload(h, p, pf_loan, lo, h->run_stream))) return finish(rc);
        if ((flags & PYA_FLAG_MZ_PROFILE) && (rc = mzp_upload(h, p, mzp_loan, lo, h->run_stream))) return finish(rc);
        if ((flags & PYA_FLAG_QUANT) && (rc = quant_upload(h, p, quant_loan, lo, h->run_stream))) return finish(rc);
        if ((flags & PYA_FLAG_RECALIBRATE) && (rc = recal_before_run(h, p, recal_loan, spec_lo(c), sp.mz_type, h->run_stream))) return finish(rc);
        rc = pya_plan_run_typed(p, &d_sp, h->run_stream, &d_out);
        if (rc) return finish(rc);
        /* status + results are adjacent in the arena: one asynchronous copy into pinned memory */
        void *&pin = h->pinned_stage[c & 1];
        if (h->pinned_bytes[c & 1] < p->d2h_bytes) {
            if (pin) (void)hipHostFree(pin);
            pin = nullptr;
            h->pinned_bytes[c & 1] = 0;
            hipError_t e0 = hipHostMalloc(&pin, p->d2h_bytes + p->d2h_bytes / 4, hipHostMallocDefault);
            if (e0 != hipSuccess) return finish(h->hip_fail(e0, "pinned result buffer"));
            h->pinned_bytes[c & 1] = p->d2h_bytes + p->d2h_bytes / 4;
        }
        unsigned char *sg = (unsigned char *)pin;
        hipError_t e = hipMemcpyAsync(sg, p->arena.p + p->o_status, p->d2h_bytes, hipMemcpyDeviceToHost, h->run_stream);
        if (e != hipSuccess) return finish(h->hip_fail(e, "results copy"));
        if ((flags & PYA_FLAG_EVIDENCE) && (rc = evidence_behind_run(h, p, &d_out, lo, h->run_stream))) return finish(rc);
        if ((flags & PYA_FLAG_IONS) && (rc = ions_behind_run(h, p, &d_out, lo, h->run_stream))) return finish(rc);
        if (nq && (rc = named_behind_run(h, p, &d_out, nq, lo, n_q, h->run_stream))) return finish(rc);
        if ((flags & PYA_FLAG_SITES) && (rc = sites_behind_run(h, p, &d_out, lo, h->run_stream))) return finish(rc);
        if ((flags & PYA_FLAG_PROBS) && (rc = probs_behind_run(h, p, &d_out, lo, h->run_stream))) return finish(rc);
        if ((flags & PYA_FLAG_RANKED) && (rc = ranked_behind_run(h, p, &d_out, lo, h->run_stream))) return finish(rc);
        if ((flags & PYA_FLAG_ROLLUP) && (rc = rollup_behind_run(h, p, &d_out, loan, flags, lo, h->run_stream))) return finish(rc);
        if ((flags & PYA_FLAG_QUANT) && (rc = quant_behind_run(h, p, &d_out, quant_loan, loan, lo, h->run_stream))) return finish(rc);
        if ((flags & PYA_FLAG_PEPTIDOFORMS) && (rc = pform_behind_run(h, p, &d_out, pf_loan, flags, lo, h->run_stream))) return finish(rc);
        if ((flags & PYA_FLAG_MZ_PROFILE) && (rc = mzp_behind_run(h, p, &d_out, mzp_loan, h->run_stream))) return finish(rc);
        if ((flags & PYA_FLAG_COVERAGE) && (rc = coverage_behind_run(h, p, &d_out, &d_sp, lo, h->run_stream))) return finish(rc);
        hipEvent_t done = nullptr;                                /* chunk c finished (kernels + copy) */
        e = hipEventCreateWithFlags(&done, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventRecord(done, h->run_stream);
        if (e != hipSuccess) return finish(h->hip_fail(e, "event"));
        int rc_next = PYA_OK;
        if (c + 1 < nchunk) {                                     /* CPU pre-pass of the next chunk meanwhile */
            raw = nullptr;
            rc_next = make_plan(c + 1, &raw);
            next.reset(raw);
        }
        e = hipEventSynchronize(done);
        (void)hipEventDestroy(done);
        p->quiesced = e == hipSuccess;
        {
            std::lock_guard<std::mutex> lk(mu);                   /* the chunk's ring slot may be overwritten now */
            consumed = c + 1;
            cv.notify_all();
        }
        if (e != hipSuccess) return finish(h->hip_fail(e, "results copy"));
        if (skip) std::memcpy(h->last_status.data() + lo, sg, n * sizeof(int32_t));
        const std::string keep_err = h->err;                      /* make_plan(c + 1) may have set a message */
        const int64_t keep_idx = h->err_index;
        rc = check_status(h, (const int32_t *)sg, n, skip);
        if (rc) {
            rebase_error(h, lo);
            return finish(rc);
        }
        if (rc_next) {
            h->err = keep_err;
            h->err_index = keep_idx;
            return finish(rc_next);
        }
        const size_t o = p->o_status;
        std::memcpy(out->best_score + lo, sg + (p->o_best_score - o), n * sizeof(float));
        std::memcpy(out->best_sig + lo, sg + (p->o_best_sig - o), n * sizeof(uint64_t));
        std::memcpy(out->n_sig + lo, sg + (p->o_n_sig_out - o), n * sizeof(int32_t));
        std::memcpy(out->ascores + lo * mk, sg + (p->o_ascores - o), n * mk * sizeof(float));
        std::memcpy(out->alt_mask + lo * mk, sg + (p->o_alt - o), n * mk * sizeof(uint64_t));
        if (nq) named_deliver(h, nq, lo, lo + n, n_q);
        /* (a slot outside the table: the report of this chunk's roll-up, whose kernels the event above waited for) */
        if ((flags & PYA_FLAG_ROLLUP) && (rc = over_report(p, OVER_ROLLUP, lo))) return finish(rc);
        if ((flags & PYA_FLAG_PEPTIDOFORMS) && (rc = pform_collect(h, p, lo))) return finish(rc);
        if ((flags & PYA_FLAG_MZ_PROFILE) && (rc = over_report(p, OVER_MZP, lo))) return finish(rc);
        if ((flags & PYA_FLAG_QUANT) && (rc = over_report(p, OVER_QUANT, lo))) return finish(rc);
        cur = std::move(next);
    }
    if ((flags & PYA_FLAG_ROLLUP) && (rc = rollup_end(h, loan))) return finish(rc);
    if ((flags & PYA_FLAG_PEPTIDOFORMS) && (rc = pform_end(h))) return finish(rc);
    if ((flags & PYA_FLAG_MZ_PROFILE) && (rc = mzp_end(h, mzp_loan))) return finish(rc);
    if ((flags & PYA_FLAG_QUANT) && (rc = quant_end(h, quant_loan, loan))) return finish(rc);
    h->evid_valid = (flags & PYA_FLAG_EVIDENCE) != 0;
    h->cov_valid = (flags & PYA_FLAG_COVERAGE) != 0;
    h->ions_valid = (flags & PYA_FLAG_IONS) != 0;
    /* (chunks behind the last PSM with records: their offsets stay at the total) */
    h->sites_valid = (flags & PYA_FLAG_SITES) != 0;
    h->probs_valid = (flags & PYA_FLAG_PROBS) != 0;
    h->ranked_valid = (flags & PYA_FLAG_RANKED) != 0;
    return finish(PYA_OK);
}

/* pya_score_batch (sh == nullptr: PSM i has spectrum i) and pya_score_batch_shared */
static int score_batch_impl(pya_handle *h, const pya_batch *b, const SpecShare *sh, const pya_typed_spectra &sp, uint32_t flags,
                            const pya_results *out, const NamedReq *nq = nullptr) {
    const uint64_t n_spec = sh ? sh->n_spectra : b->n_psm;       /* b->peak_off has n_spec + 1 entries */
    const void *mz = sp.mz, *inten = sp.intensity;
    h->last_status.clear();
    h->last_chunks = 1;
    h->evid_valid = false;
    h->ions_valid = false;
    h->sites_valid = false;
    h->probs_valid = false;
    h->ranked_valid = false;
    h->rollup_valid = false;
    h->pform_valid = false;
    h->mzp_valid = false;
    h->quant_valid = false;
    h->cov_valid = false;
    h->pfq_valid = false;
    h->pfq_active = false;
    pya_handle::RollupLoan loan;
    if (flags & PYA_FLAG_ROLLUP) {
        const int rc_ru = rollup_begin(h, &loan);
        if (rc_ru) return rc_ru;
    }
    pya_handle::PformLoan pf_loan;
    if (flags & PYA_FLAG_PEPTIDOFORMS) {
        const int rc_pf = pform_begin(h, &pf_loan, b->n_psm);
        if (rc_pf) return rc_pf;
    }
    if (flags & PYA_FLAG_PFORM_QUANT) {
        const int rc_pfq = pfq_begin(h, b->n_psm, flags);
        if (rc_pfq) return rc_pfq;
    }
    pya_handle::MzpLoan mzp_loan;
    if (flags & PYA_FLAG_MZ_PROFILE) {
        const int rc_mzp = mzp_begin(h, &mzp_loan, b->n_psm);
        if (rc_mzp) return rc_mzp;
    }
    pya_handle::QuantLoan quant_loan;
    if (flags & PYA_FLAG_QUANT) {
        const int rc_qu = quant_begin(h, &quant_loan, b->n_psm, flags, loan);
        if (rc_qu) return rc_qu;
    }
    pya_handle::RecalLoan recal_loan;
    if (flags & PYA_FLAG_RECALIBRATE) {
        if (b->n_psm && (!b->peak_off || (sh && !sh->spec_of))) return h->fail(PYA_ERR_ARG, -1, "NULL array in batch");
        const int rc_rc = recal_begin(h, &recal_loan, b, sh, flags);
        if (rc_rc) return rc_rc;
    }
    if (flags & PYA_FLAG_IONS) h->ions_off.assign(b->n_psm + 1, 0);   /* (a PSM no plan reaches has no records) */
    if (flags & PYA_FLAG_SITES) h->sites_off.assign(b->n_psm + 1, 0);
    if (flags & PYA_FLAG_PROBS) h->probs_off.assign(b->n_psm + 1, 0);
    if (b->n_psm == 0) {
        h->evid_n = 0;
        h->evid_k = out->max_k;
        h->evid_valid = (flags & PYA_FLAG_EVIDENCE) != 0;
        h->cov_n = 0;
        h->cov_valid = (flags & PYA_FLAG_COVERAGE) != 0;
        h->ions_valid = (flags & PYA_FLAG_IONS) != 0;
        h->sites_valid = (flags & PYA_FLAG_SITES) != 0;
        h->probs_valid = (flags & PYA_FLAG_PROBS) != 0;
        h->ranked_valid = (flags & PYA_FLAG_RANKED) != 0;
        h->ranked_n = 0;
        h->ranked_batch_k = h->ranked_k;
        if (flags & PYA_FLAG_PEPTIDOFORMS) {
            const int rc_pf = pform_end(h);
            if (rc_pf) return rc_pf;
        }
        if (flags & PYA_FLAG_MZ_PROFILE) {
            const int rc_mzp = mzp_end(h, mzp_loan);
            if (rc_mzp) return rc_mzp;
        }
        if (flags & PYA_FLAG_QUANT) {
            const int rc_qu = quant_end(h, quant_loan, loan);
            if (rc_qu) return rc_qu;
        }
        return (flags & PYA_FLAG_ROLLUP) ? rollup_end(h, loan) : PYA_OK;
    }
    uint32_t types = 0;
    const int rc_types = spectra_types(h, &sp, "pya_score_batch_typed", &types);
    if (rc_types) return rc_types;
    const size_t mzb = spec_elem_bytes(sp.mz_type), itb = spec_elem_bytes(sp.intensity_type);
    if (!mz || !inten) return h->fail(PYA_ERR_ARG, -1, "NULL spectrum arrays");
    if (!b->peak_off || !b->pep || !b->pep_off || !b->n_of_mod || !b->max_charge)
        return h->fail(PYA_ERR_ARG, -1, "NULL array in batch");
    if (!out->best_score || !out->best_sig || !out->n_sig || !out->ascores || !out->alt_mask)
        return h->fail(PYA_ERR_ARG, -1, "NULL array in results");
    if (b->peak_off[n_spec] < b->peak_off[0]) return h->fail(PYA_ERR_ARG, -1, "peak_off is not monotone");
    /* named localisations: the queries are checked before anything is scored; the plans take the per-stage launches */
    uint64_t n_q = 0;
    if (nq) {
        if (!nq->q_off) return h->fail(PYA_ERR_ARG, -1, "NULL query offsets");
        if (nq->q_off[0] != 0) return h->fail(PYA_ERR_ARG, 0, "PSM 0: the query offsets do not start at 0");
        for (uint64_t i = 0; i < b->n_psm; i++)
            if (nq->q_off[i + 1] < nq->q_off[i])
                return h->fail(PYA_ERR_ARG, (int64_t)i, "PSM %llu: the query offsets decrease", (unsigned long long)i);
        n_q = (uint64_t)nq->q_off[b->n_psm];
        if (n_q && (!nq->q_bits || !nq->out)) return h->fail(PYA_ERR_ARG, -1, "NULL query signatures or named records");
        const int rc_nm = named_host_block(h, n_q);
        if (rc_nm) return rc_nm;
        flags |= PYA_FLAG_NAMED;
    }
    /* (not while the records of a pya_score_one PSM are retained in the one-PSM workspace: this call would overwrite
     * what pya_get_pep_scores / pya_calculate_ambiguity still read there) */
    const bool one_view_live = h->kept && h->kept == h->one.view;
    if (flags & PYA_FLAG_EVIDENCE) {
        const int rc_ev = evidence_host_block(h, b->n_psm, out->max_k);
        if (rc_ev) return rc_ev;
    }
    if (flags & PYA_FLAG_COVERAGE) {
        const int rc_cv = coverage_host_block(h, b->n_psm);
        if (rc_cv) return rc_cv;
    }
    if (flags & PYA_FLAG_SITES) {
        if (b->pep_off[b->n_psm] < b->pep_off[0]) return h->fail(PYA_ERR_ARG, -1, "pep_off is not monotone");
        const int rc_st = sites_host_block(h, b);
        if (rc_st) return rc_st;
    }
    if (flags & PYA_FLAG_PROBS) {
        if (b->pep_off[b->n_psm] < b->pep_off[0]) return h->fail(PYA_ERR_ARG, -1, "pep_off is not monotone");
        const int rc_pb = probs_host_block(h, b);
        if (rc_pb) return rc_pb;
    }
    if (flags & PYA_FLAG_RANKED) {
        const int rc_rk = ranked_host_block(h, b);
        if (rc_rk) return rc_rk;
    }
    /* (a batch of one with PYA_FLAG_EVIDENCE, _IONS, _SITES, _PROBS, _RANKED, _ROLLUP, _PEPTIDOFORMS, _MZ_PROFILE, _COVERAGE, _QUANT, _PFORM_QUANT or _RECALIBRATE takes the plan's launches: the one-PSM kernel stays as it is) */
    if (b->n_psm == 1 && !sh && !(flags & (PYA_FLAG_SKIP_INVALID | PYA_FLAG_TIMING | PYA_FLAG_EVIDENCE | PYA_FLAG_IONS | PYA_FLAG_SITES | PYA_FLAG_PROBS | PYA_FLAG_RANKED | PYA_FLAG_ROLLUP | PYA_FLAG_PEPTIDOFORMS | PYA_FLAG_MZ_PROFILE | PYA_FLAG_COVERAGE | PYA_FLAG_QUANT | PYA_FLAG_PFORM_QUANT | PYA_FLAG_RECALIBRATE)) && !nq && !one_view_live && types == PYA_SPEC_F64_F64) {
        /* a batch of one is PyAscore.score: the low-latency path (it declines what it has no room for; float64 only) */
        const bool has_aux1 = b->aux_off && b->aux_pos && b->aux_mass;
        const int64_t a0 = has_aux1 ? b->aux_off[0] : 0, a1 = has_aux1 ? b->aux_off[1] : 0;
        const int64_t P1 = b->peak_off[1] - b->peak_off[0], L1 = b->pep_off[1] - b->pep_off[0];
        if (a1 >= a0 && P1 >= 0 && L1 >= 0) {
            int rc1 = pya_score_one(h, (const double *)mz + b->peak_off[0], (const double *)inten + b->peak_off[0], (uint64_t)P1, b->pep + b->pep_off[0], (uint64_t)L1,
                                    b->n_of_mod[0], b->max_charge[0], has_aux1 ? b->aux_pos + a0 : nullptr,
                                    has_aux1 ? b->aux_mass + a0 : nullptr, (uint64_t)(a1 - a0), flags & PYA_FLAG_KEEP, out);
            /* the one-PSM staging now holds THIS PSM: pya_rescore_last_keep must not replay it as the caller's last
             * pya_score_one PSM (it fails with PYA_ERR_STATE instead) */
            if (!(flags & PYA_FLAG_KEEP)) h->one.have_last = false;
            if (rc1 != PYA_ERR_STATE || !h->err.empty()) return rc1;
        }
    }
    {
        /* Chunking: needed when the call does not fit the device budget, worthwhile (pipelining)
         * when there is enough PCIe traffic to hide the kernels under.  A retained batch
         * (PYA_FLAG_KEEP) stays one plan: its records are queried by PSM afterwards. */
        const size_t io_total = (size_t)(b->peak_off[n_spec] - b->peak_off[0]) * (mzb + itb);
        if (!(flags & PYA_FLAG_KEEP) && io_total >= kChunkMin && !h->kn.no_chunks) {
            const size_t budget = workspace_budget(h);
            const ChunkCost cost = chunk_costs(h, b, sh, out->max_k, mzb + itb);
            double io_target = (double)kChunkTarget;
            if (h->kn.chunk_mb > 0.) io_target = h->kn.chunk_mb * 1048576.0;
            std::vector<uint64_t> cuts{0};
            double io = 0, arena = 0;
            for (uint64_t i = 0; i < b->n_psm; i++) {
                /* (shared spectra: a spectrum's bytes and its retained table count for the first of its PSMs in the chunk) */
                const bool opens = !sh || i == 0 || sh->spec_of[i] != sh->spec_of[i - 1];
                const double own = cost.arena[i] + (sh ? cost.ret[i] : 0.);
                const double io2 = io + (opens ? cost.io[i] : 0.), ar2 = arena + (opens ? own : cost.arena[i]);
                if (i > cuts.back() && (io2 > io_target || 2.0 * io2 + ar2 > (double)budget)) {
                    cuts.push_back(i);
                    io = cost.io[i];
                    arena = own;
                } else {
                    io = io2;
                    arena = ar2;
                }
            }
            cuts.push_back(b->n_psm);
            h->last_chunks = cuts.size() - 1;
            if (cuts.size() > 2) return score_batch_chunked(h, b, sh, sp, flags, out, cuts, cost.sites.data(), nq, loan, pf_loan, mzp_loan, recal_loan, quant_loan);
        }
    }
    const bool host_timing = h->kn.host_timing;
    auto t0 = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) {
        if (!host_timing) return;
        (void)hipDeviceSynchronize();
        auto t1 = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[pya host] %-14s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(t1 - t0).count());
        t0 = t1;
    };
    pya_plan *p = nullptr;
    IoReq io = {sp, out->max_k, nullptr, nullptr, nullptr, nullptr};
    /* Big batches: the spectra (16, 12 or 8 bytes per peak, PCIe-bound) go up on a helper thread while this
     * one runs the host pre-pass of the plan; small ones ride in the plan's single staged copy. */
    const int64_t peaks_lo = b->peak_off[0], n_peaks = b->peak_off[n_spec] - peaks_lo;
    std::thread uploader;
    hipError_t up_err = hipSuccess;
    if (n_peaks > 0 && (size_t)n_peaks * (mzb + itb) > kStageLimit && !h->kn.no_upload_thread) {
        HIPCHK(h, hipSetDevice(h->device));
        if (h->io_buf.n < spec_pair_bytes((size_t)n_peaks, sp)) HIPCHK(h, h->io_buf.alloc(spec_pair_bytes((size_t)n_peaks, sp)));
        io.d_mz_ext = h->io_buf.p;
        io.d_inten_ext = h->io_buf.p + spec_inten_offset((size_t)n_peaks, sp.mz_type);
        const int device = h->device;
        uploader = std::thread([&, device]() {
            up_err = hipSetDevice(device);
            if (up_err == hipSuccess)
                up_err = hipMemcpy(io.d_mz_ext, spec_at(mz, sp.mz_type, peaks_lo), (size_t)n_peaks * mzb, hipMemcpyHostToDevice);
            if (up_err == hipSuccess)
                up_err = hipMemcpy(io.d_inten_ext, spec_at(inten, sp.intensity_type, peaks_lo), (size_t)n_peaks * itb, hipMemcpyHostToDevice);
        });
    }
    int rc = plan_create_impl(h, b, flags & ~(PYA_FLAG_TIMING | PYA_FLAG_RECALIBRATE), &io, sh, &p);
    if (uploader.joinable()) uploader.join();
    if (rc) return rc;
    if (up_err != hipSuccess) {
        pya_plan_destroy(p);
        return h->hip_fail(up_err, "spectrum upload");
    }
    std::unique_ptr<pya_plan, void (*)(pya_plan *)> guard(p, pya_plan_destroy);
    lap("plan + h2d");
    const uint64_t n = b->n_psm;
    const uint32_t mk = out->max_k;
    pya_results d_out = {mk, p->d_best_score.p, p->d_best_sig.p, p->d_n_sig_out.p, p->d_ascores.p, p->d_alt.p};
    const pya_typed_spectra d_sp = {p->d_mz.p, p->d_inten.p, sp.mz_type, sp.intensity_type};
    if (nq && (rc = named_upload(h, p, nq, 0, nullptr))) return rc;
    if ((flags & PYA_FLAG_ROLLUP) && (rc = rollup_upload(h, p, loan, 0, nullptr))) return rc;
    if ((flags & PYA_FLAG_PEPTIDOFORMS) && (rc = pform_upload(h, p, pf_loan, 0, nullptr))) return rc;
    if ((flags & PYA_FLAG_MZ_PROFILE) && (rc = mzp_upload(h, p, mzp_loan, 0, nullptr))) return rc;
    if ((flags & PYA_FLAG_QUANT) && (rc = quant_upload(h, p, quant_loan, 0, nullptr))) return rc;
    if ((flags & PYA_FLAG_RECALIBRATE) && (rc = recal_before_run(h, p, recal_loan, 0, sp.mz_type, nullptr))) return rc;
    rc = pya_plan_run_typed(p, &d_sp, nullptr, &d_out);
    if (rc) return rc;
    if (p->d2h_bytes <= kStageLimit) {
        /* status and results are adjacent in the arena: one copy, which also waits for the kernels */
        h->stage.resize(std::max(h->stage.size(), p->d2h_bytes));
        unsigned char *sg = h->stage.data();
        HIPCHK(h, hipMemcpy(sg, p->arena.p + p->o_status, p->d2h_bytes, hipMemcpyDeviceToHost));
        lap("kernels + d2h");
        const bool skip = (flags & PYA_FLAG_SKIP_INVALID) != 0;
        if (skip) h->last_status.assign((const int32_t *)sg, (const int32_t *)sg + n);
        rc = check_status(h, (const int32_t *)sg, n, skip);
        if (rc) return rc;
        const size_t o = p->o_status;
        std::memcpy(out->best_score, sg + (p->o_best_score - o), n * sizeof(float));
        std::memcpy(out->best_sig, sg + (p->o_best_sig - o), n * sizeof(uint64_t));
        std::memcpy(out->n_sig, sg + (p->o_n_sig_out - o), n * sizeof(int32_t));
        std::memcpy(out->ascores, sg + (p->o_ascores - o), n * mk * sizeof(float));
        std::memcpy(out->alt_mask, sg + (p->o_alt - o), n * mk * sizeof(uint64_t));
    } else {
        rc = pya_plan_check(p);
        if (rc) return rc;
        lap("kernels");
        HIPCHK(h, hipMemcpy(out->best_score, p->d_best_score.p, n * sizeof(float), hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(out->best_sig, p->d_best_sig.p, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(out->n_sig, p->d_n_sig_out.p, n * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(out->ascores, p->d_ascores.p, n * mk * sizeof(float), hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(out->alt_mask, p->d_alt.p, n * mk * sizeof(uint64_t), hipMemcpyDeviceToHost));
    }
    if (flags & PYA_FLAG_EVIDENCE) {
        if ((rc = evidence_behind_run(h, p, &d_out, 0, nullptr))) return rc;
        HIPCHK(h, hipStreamSynchronize(nullptr));
        h->evid_valid = true;
    }
    if (flags & PYA_FLAG_IONS) {
        if ((rc = ions_behind_run(h, p, &d_out, 0, nullptr))) return rc;
        HIPCHK(h, hipStreamSynchronize(nullptr));
        h->ions_valid = true;
    }
    if (nq) {
        if ((rc = named_behind_run(h, p, &d_out, nq, 0, n_q, nullptr))) return rc;
        HIPCHK(h, hipStreamSynchronize(nullptr));
        named_deliver(h, nq, 0, n, n_q);
    }
    if (flags & PYA_FLAG_SITES) {
        if ((rc = sites_behind_run(h, p, &d_out, 0, nullptr))) return rc;
        HIPCHK(h, hipStreamSynchronize(nullptr));
        h->sites_valid = true;
    }
    if (flags & PYA_FLAG_PROBS) {
        if ((rc = probs_behind_run(h, p, &d_out, 0, nullptr))) return rc;
        HIPCHK(h, hipStreamSynchronize(nullptr));
        h->probs_valid = true;
    }
    if (flags & PYA_FLAG_RANKED) {
        if ((rc = ranked_behind_run(h, p, &d_out, 0, nullptr))) return rc;
        HIPCHK(h, hipStreamSynchronize(nullptr));
        h->ranked_valid = true;
    }
    if (flags & PYA_FLAG_ROLLUP) {
        if ((rc = rollup_behind_run(h, p, &d_out, loan, flags, 0, nullptr))) return rc;
        HIPCHK(h, hipStreamSynchronize(nullptr));
        if ((rc = over_report(p, OVER_ROLLUP, 0))) return rc;
        if ((rc = rollup_end(h, loan))) return rc;
    }
    if (flags & PYA_FLAG_QUANT) {
        if ((rc = quant_behind_run(h, p, &d_out, quant_loan, loan, 0, nullptr))) return rc;
        HIPCHK(h, hipStreamSynchronize(nullptr));
        if ((rc = over_report(p, OVER_QUANT, 0))) return rc;
        if ((rc = quant_end(h, quant_loan, loan))) return rc;
    }
    if (flags & PYA_FLAG_PEPTIDOFORMS) {
        if ((rc = pform_behind_run(h, p, &d_out, pf_loan, flags, 0, nullptr))) return rc;
        HIPCHK(h, hipStreamSynchronize(nullptr));
        if ((rc = pform_collect(h, p, 0))) return rc;
        if ((rc = pform_end(h))) return rc;
    }
    if (flags & PYA_FLAG_MZ_PROFILE) {
        if ((rc = mzp_behind_run(h, p, &d_out, mzp_loan, nullptr))) return rc;
        HIPCHK(h, hipStreamSynchronize(nullptr));
        if ((rc = over_report(p, OVER_MZP, 0))) return rc;
        if ((rc = mzp_end(h, mzp_loan))) return rc;
    }
    if (flags & PYA_FLAG_COVERAGE) {
        if ((rc = coverage_behind_run(h, p, &d_out, &d_sp, 0, nullptr))) return rc;
        HIPCHK(h, hipStreamSynchronize(nullptr));
        h->cov_valid = true;
    }
    lap("d2h");
    if (flags & PYA_FLAG_KEEP) {
        if (h->kept) pya_plan_destroy(h->kept);
        h->kept = guard.release();
    }
    return PYA_OK;
}

int pya_score_batch(pya_handle *h, const pya_batch *b, const double *mz, const double *inten, uint32_t flags,
                    const pya_results *out) {
    if (!h || !b || !out) return PYA_ERR_ARG;
    const pya_typed_spectra sp = {mz, inten, PYA_F64, PYA_F64};
    return score_batch_impl(h, b, nullptr, sp, flags, out);
}

static int score_batch_shared(pya_handle *h, const pya_batch *b, const uint32_t *spec_of, uint64_t n_spectra, const pya_typed_spectra &sp,
                              uint32_t flags, const pya_results *out, const NamedReq *nq = nullptr) {
    h->last_status.clear();
    h->evid_valid = false;
    h->ions_valid = false;
    h->sites_valid = false;
    h->probs_valid = false;
    h->ranked_valid = false;
    h->rollup_valid = false;
    h->pform_valid = false;
    h->mzp_valid = false;
    h->quant_valid = false;
    h->cov_valid = false;
    h->pfq_valid = false;
    if (b->n_psm == 0) return score_batch_impl(h, b, nullptr, sp, flags, out, nq);
    if (!b->peak_off) return h->fail(PYA_ERR_ARG, -1, "NULL array in batch");
    const int rc = check_spec_of(h, b->n_psm, spec_of, n_spectra);
    if (rc) return rc;
    const SpecShare sh = {spec_of, n_spectra, 0u};
    return score_batch_impl(h, b, &sh, sp, flags, out, nq);
}

int pya_score_batch_shared(pya_handle *h, const pya_batch *b, const uint32_t *spec_of, uint64_t n_spectra, const double *mz,
                           const double *inten, uint32_t flags, const pya_results *out) {
    if (!h || !b || !out) return PYA_ERR_ARG;
    const pya_typed_spectra sp = {mz, inten, PYA_F64, PYA_F64};
    return score_batch_shared(h, b, spec_of, n_spectra, sp, flags, out);
}

int pya_score_batch_typed(pya_handle *h, const pya_batch *b, const uint32_t *spec_of, uint64_t n_spectra, const pya_typed_spectra *spectra,
                          uint32_t flags, const pya_results *out) {
    if (!h || !b || !out) return PYA_ERR_ARG;
    if (!spectra) return h->fail(PYA_ERR_ARG, -1, "NULL spectrum arrays");
    return spec_of ? score_batch_shared(h, b, spec_of, n_spectra, *spectra, flags, out) : score_batch_impl(h, b, nullptr, *spectra, flags, out);
}

int pya_score_batch_named(pya_handle *h, const pya_batch *b, const uint32_t *spec_of, uint64_t n_spectra, const pya_typed_spectra *spectra,
                          uint32_t flags, const pya_results *out, const int64_t *q_off, const uint64_t *q_bits, pya_named *named_out,
                          int32_t *counts, float *scores) {
    if (!h || !b || !out) return PYA_ERR_ARG;
    if (!spectra) return h->fail(PYA_ERR_ARG, -1, "NULL spectrum arrays");
    const NamedReq nq = {q_off, q_bits, named_out, counts, scores};
    return spec_of ? score_batch_shared(h, b, spec_of, n_spectra, *spectra, flags, out, &nq) : score_batch_impl(h, b, nullptr, *spectra, flags, out, &nq);
}

/* (include/pyascore_debug.h) */
uint64_t pya_debug_last_chunks(const pya_handle *h) { return h ? h->last_chunks : 0; }

int pya_debug_last_probs_launch(const pya_handle *h, uint32_t front_ends[2], uint64_t lds_bytes[2]) {
    if (!h || !front_ends || !lds_bytes) return PYA_ERR_ARG;
    for (int i = 0; i < 2; i++) {
        front_ends[i] = h->last_probs_sw[i];
        lds_bytes[i] = h->last_probs_lds[i];
    }
    return PYA_OK;
}

int pya_debug_last_ranked_launch(const pya_handle *h, uint32_t front_ends[2], uint64_t lds_bytes[2]) {
    if (!h || !front_ends || !lds_bytes) return PYA_ERR_ARG;
    for (int i = 0; i < 2; i++) {
        front_ends[i] = h->last_ranked_sw[i];
        lds_bytes[i] = h->last_ranked_lds[i];
    }
    return PYA_OK;
}

int pya_debug_last_rollup_launch(const pya_handle *h, uint32_t grid[2], uint64_t *n_records) {
    if (!h || !grid || !n_records) return PYA_ERR_ARG;
    grid[0] = h->last_rollup_grid[0];
    grid[1] = h->last_rollup_grid[1];
    *n_records = h->last_rollup_records;
    return PYA_OK;
}

int pya_debug_signature_list(pya_handle *h, uint64_t psm, uint64_t *sig_bits, uint64_t cap, uint64_t *n) {
    if (!h || !n) return PYA_ERR_ARG;
    const pya_plan *p = h->kept;
    if (!p || psm >= p->n_psm) return h->fail(PYA_ERR_ARG, -1, "pya_debug_signature_list: no retained batch, or no such PSM in it");
    *n = p->n_sig[psm];
    if (cap == 0) return PYA_OK;
    if (cap < *n || !sig_bits) return h->fail(PYA_ERR_ARG, -1, "pya_debug_signature_list: room for %llu of %llu", (unsigned long long)cap, (unsigned long long)*n);
    std::memcpy(sig_bits, h->order_tab.data() + p->order_off[psm], (size_t)*n * sizeof(uint64_t));
    return PYA_OK;
}
