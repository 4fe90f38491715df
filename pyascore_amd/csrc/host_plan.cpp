/* host_plan.cpp -- creating a plan: the host pre-pass over a batch in named phases (validation, routes, id lists, fused
 * launches, descriptors), then ONE device arena laid out from one table.  Running a plan is host_run.cpp. */
#include "host_internal.h"

int check_psm_shape(const pya_handle *h, uint64_t i, int64_t P, int64_t L, int32_t k, int32_t z, const uint8_t *pep,
                    const uint32_t *aux_pos, int64_t n_aux, uint32_t *ns, char *msg) {
    const unsigned long long iu = i;
    auto say = [msg](int code, const char *fmt, auto... args) {
        std::snprintf(msg, kPsmMsg, fmt, args...);
        return code;
    };
    if (P <= 0) return say(PYA_ERR_PSM, "PSM %llu: empty spectrum", iu);
    if (P > PYA_MAX_PEAKS) return say(PYA_ERR_LIMIT, "PSM %llu: %lld peaks exceed the limit of %d", iu, (long long)P, PYA_MAX_PEAKS);
    if (L < 1 || L > PYA_MAX_PEPTIDE_LEN)
        return say(L < 1 ? PYA_ERR_PSM : PYA_ERR_LIMIT, "PSM %llu: peptide length %lld outside 1..%d", iu, (long long)L, PYA_MAX_PEPTIDE_LEN);
    if (k < 0) return say(PYA_ERR_PSM, "PSM %llu: negative n_of_mod", iu);
    if (z < 1 || z > PYA_MAX_CHARGE)
        return say(z < 1 ? PYA_ERR_PSM : PYA_ERR_LIMIT, "PSM %llu: max_fragment_charge %d outside 1..%d", iu, z, PYA_MAX_CHARGE);
    if (n_aux < 0) return say(PYA_ERR_ARG, "PSM %llu: aux_off is not monotone", iu);
    uint32_t cnt = 0;
    int64_t bad_j = -1, bad_a = -1;
    for (int64_t j = 0; j < L; j++) {
        if (!h->is_residue[pep[j]] && bad_j < 0) bad_j = j;
        if (h->letter_modifiable((char)pep[j], (size_t)j, (size_t)L)) cnt++;
    }
    for (int64_t a = 0; a < n_aux; a++)
        if (aux_pos[a] > (uint32_t)L && bad_a < 0) bad_a = a;
    if (bad_j >= 0) return say(PYA_ERR_PSM, "PSM %llu: unknown residue '%c' at position %lld", iu, (char)pep[bad_j], (long long)(bad_j + 1));
    if (bad_a >= 0) return say(PYA_ERR_PSM, "PSM %llu: aux_mod_pos %u beyond the peptide", iu, aux_pos[bad_a]);
    if (cnt > PYA_MAX_SITES) return say(PYA_ERR_LIMIT, "PSM %llu: %u modifiable residues exceed %d", iu, cnt, PYA_MAX_SITES);
    *ns = cnt;
    return PYA_OK;
}

namespace {

/* What crosses the phases of plan_create_impl, and nothing else: a phase reads and writes this and the plan. */
struct PlanBuild {
    pya_handle *h;
    const pya_batch *b;
    const IoReq *io;
    const SpecShare *sh;                 /* shared spectra (pya_plan::shared), or nullptr */
    uint32_t flags;
    pya_plan *p;
    uint64_t n;
    int64_t peak_base = 0, pep_base = 0, aux_base = 0;    /* the batch's first offsets (the plan's own start at 0) */
    int64_t total_aux = 0;
    bool has_aux;
    /* the route switches, from the settings */
    bool plain_on, both_dirs, fused_on, big_on, big_inline_ok;
    uint64_t big_inline_max;
    /* running maxima and totals of the PSM loop */
    uint32_t max_P = 1, lut_need = 0, max_k = 1;
    int64_t sig_total = 0;
    uint64_t n_skipped = 0;
    std::vector<uint8_t> bad;            /* [n] the letter scan's verdict */
    std::vector<uint32_t> caps;          /* peak classes: caps, ascending ... */
    std::vector<uint8_t> pcls;           /* ... [n] and the class of every PSM binned by the fast kernels */

    PlanBuild(pya_handle *h_, const pya_batch *b_, const IoReq *io_, const SpecShare *sh_, uint32_t flags_, pya_plan *p_)
        : h(h_), b(b_), io(io_), sh(sh_), flags(flags_), p(p_), n(b_->n_psm) {
        const DevConfig &c = h->cfg;
        const Knobs &kn = h->kn;
        has_aux = b->aux_off && b->aux_pos && b->aux_mass;
        /* (tiny batches are launch-bound: the lean instantiation's extra memset + hand-over launch cost
         * more than its occupancy gains there) */
        plain_on = c.n_nl == 0 && !(flags & PYA_FLAG_KEEP) && !kn.no_plain && n >= (uint64_t)kn.plain_min;
        both_dirs = c.n_fwd > 0 && c.n_fwd < c.n_types;
        /* fused score + localize kernel: plain settings with one ion type per direction; up to 64 site assignments (both
         * directions and 33 .. 64: the kernel walks the directions one after the other) */
        fused_on = plain_on && plain_types(c) && !kn.no_fused;
        /* score_big.hip: one PSM per 8-wave workgroup, fragment tree shared two levels deep */
        big_on = c.n_nl == 0 && both_dirs && c.n_fwd == 1 && c.n_types == 2 && h->mz_error <= 0.49f && !kn.no_big;
        /* (summary mode with the lean localize route on: the kernel localises what it scores) */
        big_inline_ok = big_on && plain_on && !kn.no_big_inline;
        big_inline_max = pya_big_inline_max();
    }
};

/* PYA_HOST_TIMING: the host time of every phase */
struct Lap {
    bool on;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void operator()(const char *what) {
        if (!on) return;
        auto t1 = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[pya plan] %-14s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(t1 - t0).count());
        t0 = t1;
    }
};

/* the batch's arrays with offsets that start at 0; where every PSM's retained table goes (shared spectra: every
 * spectrum's, and which of them every PSM reads) */
int copy_meta(PlanBuild &B) {
    pya_plan *p = B.p;
    const pya_batch *b = B.b;
    const uint64_t n = B.n;
    const uint64_t ns = p->n_spec;                      /* spectra that peak_off describes: n unless they are shared */
    p->peak_off.assign(b->peak_off, b->peak_off + ns + 1);
    p->pep_off.assign(b->pep_off, b->pep_off + n + 1);
    p->n_of_mod.assign(b->n_of_mod, b->n_of_mod + n);
    p->max_charge.assign(b->max_charge, b->max_charge + n);
    if (B.has_aux) p->aux_off.assign(b->aux_off, b->aux_off + n + 1);
    else p->aux_off.assign(n + 1, 0);
    B.peak_base = n ? p->peak_off[0] : 0;
    B.pep_base = n ? p->pep_off[0] : 0;
    B.aux_base = n ? p->aux_off[0] : 0;
    p->total_peaks = n ? p->peak_off[ns] - B.peak_base : 0;
    const int64_t total_pep = n ? p->pep_off[n] - B.pep_base : 0;
    B.total_aux = n ? p->aux_off[n] - B.aux_base : 0;
    if (p->total_peaks < 0 || total_pep < 0 || B.total_aux < 0)
        return B.h->fail(PYA_ERR_ARG, -1, "offset arrays are not monotone (the last offset is below the first)");
    p->pep.assign(b->pep + B.pep_base, b->pep + B.pep_base + total_pep);
    for (uint64_t s = 0; s <= ns; s++) p->peak_off[s] -= B.peak_base;
    for (uint64_t i = 0; i <= n; i++) {
        p->pep_off[i] -= B.pep_base;
        p->aux_off[i] -= B.aux_base;
    }
    p->ret_off.resize(n + 1);
    int64_t at = 0;                                     /* every retained table starts at an even entry */
    if (!p->shared) {
        for (uint64_t i = 0; i < n; i++) {
            p->ret_off[i] = at;
            const int64_t P = p->peak_off[i + 1] - p->peak_off[i];
            at += ((P > 0 ? P : 0) + 1) & ~(int64_t)1;
        }
    } else {
        /* one table per spectrum some PSM uses; a PSM's offset is its spectrum's */
        p->spec_of.resize(n);
        std::vector<uint8_t> used(ns, 0);
        for (uint64_t i = 0; i < n; i++) used[p->spec_of[i] = B.sh->spec_of[i] - B.sh->base] = 1;
        p->sret_off.resize(ns + 1);
        for (uint64_t s = 0; s < ns; s++) {
            p->sret_off[s] = at;
            const int64_t P = p->peak_off[s + 1] - p->peak_off[s];
            if (used[s]) at += ((P > 0 ? P : 0) + 1) & ~(int64_t)1;
        }
        p->sret_off[ns] = at;
        for (uint64_t i = 0; i < n; i++) p->ret_off[i] = p->sret_off[p->spec_of[i]];
    }
    p->ret_off[n] = at;
    return PYA_OK;
}

/* The per-letter work, threaded for big batches: is every PSM valid, and how many modifiable residues has it.  A yes or
 * no only -- route_psms asks check_psm_shape for the message of a PSM that fails here. */
void scan_letters(PlanBuild &B) {
    pya_plan *p = B.p;
    const pya_handle *h = B.h;
    const uint64_t n = B.n;
    const uint8_t *pre_sites = B.io ? B.io->pre_sites : nullptr;   /* (the caller's scan: sites per PSM, 255 = invalid) */
    const uint32_t *aux_pos = B.has_aux ? B.b->aux_pos + B.aux_base : nullptr;
    B.bad.assign(n, 0);
    auto scan = [&](uint64_t lo, uint64_t hi) {
        for (uint64_t i = lo; i < hi; i++) {
            const int64_t P = p->n_peaks(i);
            const int64_t L = p->pep_off[i + 1] - p->pep_off[i];
            const int32_t k = p->n_of_mod[i], z = p->max_charge[i];
            bool ok = P > 0 && P <= PYA_MAX_PEAKS && L >= 1 && L <= PYA_MAX_PEPTIDE_LEN && k >= 0 && z >= 1 && z <= PYA_MAX_CHARGE &&
                      p->aux_off[i + 1] >= p->aux_off[i];
            uint32_t ns = 0;
            if (ok) {
                if (pre_sites) {
                    ns = pre_sites[i];
                    ok = ns != 255u;
                } else {
                    ok = psm_letters_ok(h, p->pep.data() + p->pep_off[i], L, &ns);
                }
                for (int64_t a = p->aux_off[i]; aux_pos && a < p->aux_off[i + 1]; a++) ok = ok && aux_pos[a] <= (uint32_t)L;
                ok = ok && ns <= PYA_MAX_SITES;
            }
            B.bad[i] = ok ? 0 : 1;
            p->n_sites[i] = ok ? (uint8_t)ns : 0;
        }
    };
    for_psm_ranges(n, scan);
}

/* an invalid PSM ends the call with its message -- or, with PYA_FLAG_SKIP_INVALID, is set aside
 * (status PYA_ST_INVALID / PYA_ST_OVER_LIMIT, best_score -1, n_sig -1) while the rest is scored */
int reject(PlanBuild &B, int code, uint64_t i, const char *msg) {
    pya_plan *p = B.p;
    if (!(B.flags & PYA_FLAG_SKIP_INVALID)) return B.h->fail(code, (int64_t)i, "%s", msg);
    if (B.n_skipped == 0) (void)B.h->fail(code, (int64_t)i, "%s", msg);       /* first message is kept */
    B.n_skipped++;
    p->pre_status[i] = code == PYA_ERR_LIMIT ? PYA_ST_OVER_LIMIT : PYA_ST_INVALID;
    p->n_sites[i] = 0;
    p->n_sig[i] = 0;
    p->order_off[i] = 0;
    p->sig_off[i] = B.sig_total;
    p->buckets[0].general_ids.push_back((uint32_t)i);     /* localize writes the "no result" record */
    return PYA_OK;
}

/* the route of one valid PSM: the general kernel, or a C(n,k) class and there the fused kernel, score_big (with or without
 * its own localisation) or the two-kernel route -- and the caps of whichever launch takes it */
inline void route_one(PlanBuild &B, uint64_t i, int64_t P, int64_t L, int32_t k, int32_t z, uint32_t ns, uint64_t N, uint32_t per_type) {
    pya_plan *p = B.p;
    pya_handle *h = B.h;
    p->n_sites[i] = (uint8_t)ns;
    p->n_sig[i] = (uint32_t)N;
    uint32_t ooff = 0;
    if (N) {
        uint32_t &co = h->shape_cache[ns][k];
        if (co == 0xffffffffu) co = shape_offset(h, ns, (uint32_t)k);
        ooff = co;
    }
    p->order_off[i] = ooff;
    p->sig_off[i] = B.sig_total;
    B.sig_total += (int64_t)N;
    if (P <= PYA_FAST_PEAKS) B.max_P = std::max<uint32_t>(B.max_P, (uint32_t)P);    /* (sizes the LDS of the fast kernels) */
    B.lut_need = std::max(B.lut_need, per_type * (uint32_t)h->cfg.n_types);
    if ((uint32_t)k > B.max_k) B.max_k = (uint32_t)k;
    if (P > PYA_FAST_PEAKS || L > PYA_FAST_PEPTIDE_LEN || N > PYA_FAST_SIGNATURES || per_type > PYA_FAST_FRAGMENTS_PER_TYPE || h->all_general()) {
        /* beyond a limit of the fast kernels (or n_top > 10): the general kernel takes the PSM whole */
        p->gen[i] = 1;
        p->gen_ids.push_back((uint32_t)i);
        /* its own slice of the general kernel's scratch: sort area for ITS site assignments, room for ITS competitors */
        const uint32_t push = ((uint32_t)k <= ns ? (uint32_t)k * (ns - (uint32_t)k) : 0u);
        if (p->gen_off.empty()) p->gen_off.push_back(0);
        p->gen_off.push_back(p->gen_off.back() + ((pya_general_scratch_bytes((uint32_t)N, (push + 3u) & ~3u) + 255) & ~(size_t)255));
        p->gen_l_cap = std::max<uint32_t>(p->gen_l_cap, (uint32_t)L);
        p->gen_list_cap = std::max<uint32_t>(p->gen_list_cap, per_type);
        if (P > PYA_FAST_PEAKS) {
            /* (the id of the spectrum: the PSM's own number unless spectra are shared, then once for its consecutive PSMs) */
            const uint32_t s = (uint32_t)p->spec(i);
            if (p->bigbin_ids.empty() || p->bigbin_ids.back() != s) p->bigbin_ids.push_back(s);
            p->bigbin_cap = std::max<uint32_t>(p->bigbin_cap, ((uint32_t)P + 31u) & ~31u);
        }
        return;
    }
    if (N == 0 || (uint32_t)k >= ns) {
        Bucket &bk = p->buckets[0];                 /* unambiguous / empty: cheapest launch */
        bk.general_ids.push_back((uint32_t)i);
        bk.n_cap = std::max<uint32_t>(bk.n_cap, (uint32_t)N);
        /* (its peptide still goes through the score kernel of this class, whose residue table is sized by pos_cap) */
        bk.pos_cap = std::max<uint32_t>(bk.pos_cap, (uint32_t)std::max<int64_t>(L - 1, 1));
        return;
    }
    int bi = 0;
    while (N > kBucketLimits[bi]) bi++;
    p->ncls[i] = (uint8_t)bi;
    /* (the fused kernel's count records hold the cumulative counts as bytes: at most 255 fragments) */
    const uint32_t frags = (B.both_dirs ? 2u : 1u) * (uint32_t)(L - 1) * (uint32_t)z;
    const bool to_fused = B.fused_on && N <= 64u && frags <= 255u;
    bool inl = false;
    if (B.big_on && z == 1 && N > (uint64_t)h->kn.big_min_n && ns >= 11) { /* (its second level shares ten sites: at least eleven) */
        p->big[i] = 1;
        p->big_pos_cap = std::max(p->big_pos_cap, (uint32_t)(L - 1));
        p->big_k_max = std::max(p->big_k_max, (uint32_t)k);
        inl = B.big_inline_ok && N <= B.big_inline_max;
    }
    Bucket &bk = to_fused ? p->fusedb : (inl ? p->bigloc : p->buckets[bi]);
    if (inl) p->n_big_inline++;              /* (p->bigloc: localised by the recounting lean launch) */
    if (to_fused) {
        p->fused[i] = 1;
        p->fused_ent_cap = std::max(p->fused_ent_cap, (uint32_t)(L - 1) * (uint32_t)z);
    }
    /* lean localize instantiation: no neutral losses, charge 1, summary mode (it checks the
     * residue masses itself and hands back what it cannot do) */
    if (inl || to_fused || (B.plain_on && z == 1)) bk.ids.push_back((uint32_t)i);
    else bk.general_ids.push_back((uint32_t)i);
    bk.cover(*h, (uint32_t)N, (uint32_t)L, (uint32_t)z, (uint32_t)k, ns, per_type);
}

/* ONE serial pass in id order (the order of the ids inside every list is the order of this loop): the message of a PSM
 * the letter scan refused, the limits, the route */
int route_psms(PlanBuild &B) {
    pya_plan *p = B.p;
    pya_handle *h = B.h;
    const uint32_t n_types = (uint32_t)h->cfg.n_types;
    const uint32_t *aux_pos = B.has_aux ? B.b->aux_pos + B.aux_base : nullptr;
    char msg[kPsmMsg];
    p->pre_status.assign(B.n, 0);
    for (uint64_t i = 0; i < B.n; i++) {
        const int64_t P = p->n_peaks(i);
        const int64_t L = p->pep_off[i + 1] - p->pep_off[i];
        const int32_t k = p->n_of_mod[i], z = p->max_charge[i];
        uint32_t ns = p->n_sites[i], per_type = 0;
        uint64_t N = 0;
        int code = PYA_OK;
        if (B.bad[i]) {
            /* (without fixed modifications aux_off is all zeros: no entries, aux_pos is not read) */
            code = check_psm_shape(h, i, P, L, k, z, p->pep.data() + p->pep_off[i], aux_pos ? aux_pos + p->aux_off[i] : nullptr,
                                   p->aux_off[i + 1] - p->aux_off[i], &ns, msg);
            if (!code) {
                code = PYA_ERR_PSM;
                std::snprintf(msg, kPsmMsg, "PSM %llu: rejected by the batch scan", (unsigned long long)i);
            }
        }
        if (!code) code = check_psm_limits(h, i, L, k, z, ns, &N, &per_type, msg);
        /* (not part of check_psm: pya_score_one leaves such a PSM to ensure_lut, whose message has no PSM index) */
        if (!code && (uint64_t)per_type * n_types > PYA_MAX_LUT_N) {
            code = PYA_ERR_LIMIT;
            std::snprintf(msg, kPsmMsg, "PSM %llu: up to %llu theoretical fragments per site assignment; the score table covers %d",
                          (unsigned long long)i, (unsigned long long)per_type * n_types, PYA_MAX_LUT_N);
        }
        if (code) {
            const int rc = reject(B, code, i, msg);
            if (rc) return rc;
            continue;
        }
        route_one(B, i, P, L, k, z, ns, N, per_type);
    }
    return PYA_OK;
}

/* Two routes are taken back when the caps of the whole batch do not fit their kernel's LDS: score_big's own localisation
 * (the separate localize kernels of the PSMs' classes take them) and the fused kernel (class 0's two kernels do).  Then
 * every bucket's list is its lean PSMs followed by the general ones. */
void settle_fallbacks(PlanBuild &B) {
    pya_plan *p = B.p;
    if (p->n_big_inline) {
        Bucket &bl = p->bigloc;
        p->big_inline = pya_localize_recount_lds_bytes((B.max_P + 31u) & ~31u, bl.push_cap(), bl.pos_cap, bl.pool_cap(), bl.sb()) <= 64 * 1024;
        if (!p->big_inline) {
            /* (caps that do not fit what score_big's dead tables leave.)  bigloc spans C(n,k) classes and n_cap sizes a
             * localize launch's LDS: a class takes bigloc's other caps whole, but n_cap from its own PSMs */
            bl.n_cap = 0;
            for (uint64_t i = 0; i < B.n; i++) {
                if (!p->big[i] || p->pre_status[i] || p->n_sig[i] > B.big_inline_max) continue;
                Bucket &bk = p->buckets[p->ncls[i]];
                bk.ids.push_back((uint32_t)i);                  /* (these are charge-1 PSMs: the lean list) */
                bk.absorb(bl);
                bk.n_cap = std::max(bk.n_cap, p->n_sig[i]);
            }
            p->n_big_inline = 0;
            bl.ids.clear();
        }
    }
    for (Bucket &bk : p->buckets) {
        bk.n_plain = (uint32_t)bk.ids.size();
        bk.ids.insert(bk.ids.end(), bk.general_ids.begin(), bk.general_ids.end());
        bk.general_ids.clear();
        bk.general_ids.shrink_to_fit();
    }
    Bucket &fb = p->fusedb;
    fb.n_plain = (uint32_t)fb.ids.size();
    if (fb.ids.empty()) return;
    p->fused_both = B.both_dirs ? 1u : 0u;
    p->fused_n_cap = (fb.n_cap + 3u) & ~3u;
    p->fused_stride = (B.both_dirs ? 2u : 1u) * p->fused_n_cap + 4u;
    const uint32_t cap_all = (B.max_P + 31u) & ~31u;
    if (pya_fused_lds_bytes(cap_all, p->fused_n_cap, p->fused_stride, fb.pos_cap, p->fused_ent_cap, fb.push_cap(), p->fused_both, 1u) <= 64 * 1024 &&
        pya_localize_lds_bytes(fb.push_cap(), fb.n_cap, fb.pos_cap, fb.pool_cap(), fb.sb()) <= kMaxLds)
        return;
    Bucket &b0 = p->buckets[0];                             /* (huge spectra) back to the two-kernel route */
    std::vector<uint32_t> lean, general;                    /* charge 1 -> lean localize instantiation */
    for (uint32_t id : fb.ids) (p->max_charge[id] == 1 ? lean : general).push_back(id);
    b0.ids.insert(b0.ids.begin(), lean.begin(), lean.end());
    b0.n_plain += (uint32_t)lean.size();
    b0.ids.insert(b0.ids.end(), general.begin(), general.end());
    b0.absorb(fb);
    fb.ids.clear();
    fb.n_plain = 0;
    std::fill(p->fused.begin(), p->fused.end(), 0);
}

/* bin_spectra and the scoring kernels are launched per peak class (pya_plan::bin_lists): the classes, then the id lists
 * of every launch, filled by counting */
void peak_classes_and_lists(PlanBuild &B) {
    pya_plan *p = B.p;
    const pya_handle *h = B.h;
    const uint64_t n = B.n;
    std::vector<uint32_t> &caps = B.caps;
    /* peak classes: the median, 90th and 99th percentile and the maximum of the peak counts,
     * rounded up to 32 (one class for small batches) */
    if (n >= 2048 && !h->kn.one_peak_class) {
        /* (the order statistics from a histogram of the counts -- they are at most PYA_FAST_PEAKS here --: one pass
         * instead of three std::nth_element over the batch) */
        std::vector<uint32_t> hist(PYA_FAST_PEAKS + 2, 0);
        std::vector<uint8_t> global_bin(p->bigbin_ids.empty() ? 0 : p->n_spec, 0);
        for (uint32_t id : p->bigbin_ids) global_bin[id] = 1;      /* (binned by their own kernel) */
        for (uint64_t i = 0; i < n; i++) {
            uint32_t v = p->pre_status[i] ? 1u : (uint32_t)p->n_peaks(i);
            if (!global_bin.empty() && global_bin[p->spec(i)]) v = 1u;
            hist[v > PYA_FAST_PEAKS ? PYA_FAST_PEAKS + 1 : v]++;
        }
        for (double q : {0.5, 0.9, 0.99}) {
            const size_t at = (size_t)(q * (double)(n - 1));
            size_t acc = 0;
            uint32_t v = 0;
            for (; v < hist.size(); v++) {
                acc += hist[v];
                if (acc > at) break;
            }
            caps.push_back((v + 31u) & ~31u);
        }
    }
    /* classes only pay when the tail is long: every extra launch has its own ramp-up and tail */
    if (!caps.empty() && p->peak_cap < 2 * caps[0] && !h->kn.peak_classes) caps.clear();
    caps.push_back(p->peak_cap);
    std::sort(caps.begin(), caps.end());
    caps.erase(std::unique(caps.begin(), caps.end()), caps.end());
    const size_t nc = caps.size();
    std::vector<uint32_t> cnt_bin(nc, 0), cnt_score(nc * kNumBuckets, 0), cnt_big(nc, 0);
    B.pcls.resize(n);
    /* the binning lists hold spectra: PSM numbers unless spectra are shared, then a spectrum once for its consecutive PSMs
     * (the first of them that is not set aside lists it) */
    int64_t listed = -1;
    for (uint64_t i = 0; i < n; i++) {
        if (p->pre_status[i]) continue;                  /* set aside: neither binned nor scored */
        const uint32_t P = (uint32_t)p->n_peaks(i);
        if (P > PYA_FAST_PEAKS) continue;               /* (pya_bin_global_kernel; scored by the general kernel) */
        size_t c = 0;
        while (caps[c] < P) c++;
        B.pcls[i] = (uint8_t)c;
        if ((int64_t)p->spec(i) != listed) cnt_bin[c]++;
        listed = (int64_t)p->spec(i);
        if (p->fused[i] || p->gen[i]) continue;
        if (p->big[i]) cnt_big[c]++;
        else cnt_score[p->ncls[i] * nc + c]++;
    }
    uint32_t n_bin = 0, n_score = 0, n_big = 0;
    for (size_t c = 0; c < nc; c++) {
        p->bin_lists.push_back({n_bin, 0u, caps[c], 0u});
        n_bin += cnt_bin[c];
    }
    for (size_t g = 0; g < nc * kNumBuckets; g++) {
        p->score_lists.push_back({n_score, 0u, caps[g % nc], (uint32_t)(g / nc)});
        n_score += cnt_score[g];
    }
    for (size_t c = 0; c < nc; c++) {
        p->big_lists.push_back({n_big, 0u, caps[c], 0u});
        n_big += cnt_big[c];
    }
    p->bin_ids.resize(n_bin);
    p->score_ids.resize(n_score);
    p->big_ids.resize(n_big);
    listed = -1;
    for (uint64_t i = 0; i < n; i++) {
        if (p->pre_status[i]) continue;
        if (p->n_peaks(i) > PYA_FAST_PEAKS) continue;
        pya_plan::IdList &bl = p->bin_lists[B.pcls[i]];
        if ((int64_t)p->spec(i) != listed) p->bin_ids[bl.off + bl.n++] = (uint32_t)p->spec(i);
        listed = (int64_t)p->spec(i);
        if (p->fused[i] || p->gen[i]) continue;         /* (listed by fused_launches / in gen_ids) */
        pya_plan::IdList &sl = p->big[i] ? p->big_lists[B.pcls[i]] : p->score_lists[p->ncls[i] * nc + B.pcls[i]];
        (p->big[i] ? p->big_ids : p->score_ids)[sl.off + sl.n++] = (uint32_t)i;
    }
}

struct FusedItem {
    uint32_t id, group;                  /* group = peak class * 2 + (charge > 1) */
    size_t need;                         /* the LDS it would need in a launch of its own */
    uint32_t n_cap, pos, ent, push;
};

/* order: (group, LDS need, id).  The items come in id order and (group, need) takes a few hundred values at most, so
 * a stable counting sort over the distinct pairs (kept sorted, found by bisection) does it in O(n log pairs) with
 * eight-byte keys -- r06: std::sort over 100 000 forty-byte items was 3 of the 7 ms of a cfg2 batch's pre-pass */
void sort_fused_items(std::vector<FusedItem> &items) {
    std::vector<std::pair<uint64_t, uint32_t>> keys;     /* (group << 40 | need, class id), sorted by key */
    keys.reserve(256);
    std::vector<uint32_t> cls(items.size());
    std::vector<size_t> cnt;
    uint64_t last_key = ~0ull;
    uint32_t last_cls = 0;
    for (size_t t = 0; t < items.size(); t++) {
        const uint64_t key = ((uint64_t)items[t].group << 40) | (uint64_t)items[t].need;
        if (key != last_key) {
            auto it = std::lower_bound(keys.begin(), keys.end(), std::make_pair(key, 0u));
            if (it == keys.end() || it->first != key) {
                it = keys.insert(it, std::make_pair(key, (uint32_t)cnt.size()));
                cnt.push_back(0);
            }
            last_key = key;
            last_cls = it->second;
        }
        cls[t] = last_cls;
        cnt[last_cls]++;
    }
    std::vector<size_t> at(cnt.size());
    size_t acc = 0;
    for (const auto &kc : keys) {                        /* ascending (group, need) */
        at[kc.second] = acc;
        acc += cnt[kc.second];
    }
    std::vector<FusedItem> sorted(items.size());
    for (size_t t = 0; t < items.size(); t++) sorted[at[cls[t]]++] = items[t];     /* (stable: ids stay ascending) */
    items.swap(sorted);
}

/* launches of the fused kernel: per peak class and charge class (a group), and inside a group per LDS class */
void fused_launches(PlanBuild &B) {
    pya_plan *p = B.p;
    const uint32_t ndir = B.both_dirs ? 2u : 1u;
    std::vector<FusedItem> items;
    for (uint64_t i = 0; i < B.n; i++) {
        if (!p->fused[i] || p->pre_status[i]) continue;
        FusedItem it;
        it.id = (uint32_t)i;
        const uint32_t z = (uint32_t)p->max_charge[i], Lm1 = (uint32_t)(p->pep_off[i + 1] - p->pep_off[i] - 1);
        const uint32_t kk = (uint32_t)p->n_of_mod[i], ns = p->n_sites[i];
        it.group = (uint32_t)B.pcls[i] * 2 + (z > 1 ? 1u : 0u);
        it.n_cap = (p->n_sig[i] + 3u) & ~3u;
        it.pos = std::max(Lm1, 1u);
        it.ent = std::max(Lm1 * z, 1u);
        it.push = std::min<uint32_t>(PYA_MAX_PUSHED, (kk * (ns - kk) + 7u) & ~7u);
        if (it.push < 8) it.push = 8;
        it.need = pya_fused_lds_bytes(B.caps[B.pcls[i]], it.n_cap, ndir * it.n_cap + 4, it.pos, it.ent, it.push, p->fused_both, z > 1 ? 1u : 0u);
        items.push_back(it);
    }
    p->n_fused_total = (uint32_t)items.size();
    sort_fused_items(items);
    p->fused_ids.resize(items.size());
    size_t g0 = 0;
    while (g0 < items.size()) {
        size_t g1 = g0;
        while (g1 < items.size() && items[g1].group == items[g0].group) g1++;
        /* LDS classes inside the group: cut at the median and the 85th percentile of the footprint when
         * that buys at least a fifth of the largest footprint (every launch has its own ramp-up and tail) */
        std::vector<size_t> cuts{g0};
        if (g1 - g0 >= 8192 && !B.h->kn.one_lds_class) {
            const size_t need_max = items[g1 - 1].need;
            for (double q : {0.5, 0.85}) {
                const size_t at = g0 + (size_t)(q * (double)(g1 - g0));
                size_t cut = at;
                while (cut < g1 && items[cut].need == items[at].need) cut++;    /* equal footprints stay together */
                if (cut < g1 && cut > cuts.back() && items[at].need * 5 <= need_max * 4) cuts.push_back(cut);
            }
        }
        cuts.push_back(g1);
        for (size_t c = 0; c + 1 < cuts.size(); c++) {
            pya_plan::FusedLaunch fl = {(uint32_t)cuts[c], (uint32_t)(cuts[c + 1] - cuts[c]), B.caps[items[g0].group / 2],
                                        items[g0].group & 1u, 4, 4, 1, 1, 8};
            for (size_t t = cuts[c]; t < cuts[c + 1]; t++) {
                fl.n_cap = std::max(fl.n_cap, items[t].n_cap);
                fl.pos_cap = std::max(fl.pos_cap, items[t].pos);
                fl.ent_cap = std::max(fl.ent_cap, items[t].ent);
                fl.push_cap = std::max(fl.push_cap, items[t].push);
                p->fused_ids[t] = items[t].id;
            }
            fl.stride = ndir * fl.n_cap + 4;            /* + a spare column for lanes without a walker */
            p->fused_launches.push_back(fl);
        }
        g0 = g1;
    }
}

/* packed descriptors: what a kernel needs to know about a PSM before it can fetch anything else,
 * in one cache line (fetched ahead by the fused kernel) */
void pack_descriptors(PlanBuild &B) {
    pya_plan *p = B.p;
    p->desc.resize((size_t)B.n * PYA_DESC_WORDS);
    for (uint64_t i = 0; i < B.n; i++) {
        uint64_t *w = &p->desc[(size_t)i * PYA_DESC_WORDS];
        const uint64_t L = (uint64_t)std::max<int64_t>(0, std::min<int64_t>(p->pep_off[i + 1] - p->pep_off[i], 0xffff));
        const uint64_t na = (uint64_t)std::max<int64_t>(0, std::min<int64_t>(p->aux_off[i + 1] - p->aux_off[i], 0xffff));
        w[0] = (uint64_t)p->ret_off[i];
        w[1] = (uint64_t)p->pep_off[i];
        w[2] = (uint64_t)p->sig_off[i];
        w[3] = (uint64_t)p->aux_off[i];
        pack_desc_tail(L, na, p->n_of_mod[i], p->n_sites[i], p->max_charge[i], p->n_sig[i], p->order_off[i], w);
    }
}

int check_lds_budgets(PlanBuild &B) {
    pya_plan *p = B.p;
    pya_handle *h = B.h;
    if (B.io && B.io->max_k < B.max_k)
        return h->fail(PYA_ERR_ARG, -1, "results.max_k (%u) is smaller than the largest n_of_mod (%u)", B.io->max_k, B.max_k);
    for (Bucket &bk : p->buckets) {
        if (bk.ids.empty()) continue;
        size_t need = pya_localize_lds_bytes(bk.push_cap(), bk.n_cap, bk.pos_cap, bk.pool_cap(), bk.sb());
        if (need > kMaxLds)
            return h->fail(PYA_ERR_LIMIT, (int64_t)bk.ids[0], "LDS budget exceeded (%zu bytes) for the bucket of PSM %u",
                           need, bk.ids[0]);
    }
    if (!p->gen_ids.empty() && pya_general_lds_bytes(p->gen_l_cap, p->gen_list_cap) > kMaxLds)
        return h->fail(PYA_ERR_LIMIT, (int64_t)p->gen_ids[0], "LDS budget exceeded for the general kernel (PSM %u)", p->gen_ids[0]);
    return PYA_OK;
}

/* The plan's arena as ONE table: a buffer is named once -- add(its DevBuf, elements of its own type, where they are
 * uploaded from, if at all) -- in layout order.  add() hands out offsets at 256-byte boundaries and notes the upload;
 * after the single allocation adopt_all() points every DevBuf at its place. */
class ArenaLayout {
    struct Slot { void *buf; void (*adopt)(void *buf, void *at, size_t count); size_t off, count; };
    std::vector<Slot> slots;

public:
    struct Up { size_t off; const void *src; size_t bytes; };
    std::vector<Up> ups;
    size_t total = 0;
    template <typename T>
    size_t add(DevBuf<T> &b, size_t count, const T *src = nullptr) {
        const size_t off = total, bytes = count * sizeof(T);
        total += (bytes + 255) & ~(size_t)255;
        slots.push_back({&b, [](void *buf, void *at, size_t c) { static_cast<DevBuf<T> *>(buf)->adopt(at, c); }, off, count});
        if (src && bytes) ups.push_back({off, src, bytes});
        return off;
    }
    void adopt_all(unsigned char *base) const {
        for (const Slot &s : slots) s.adopt(s.buf, base + s.off, s.count);
    }
};

/* One device allocation for everything (hipMalloc is ~100 us a call), laid out so that what goes up and what comes back
 * are each one contiguous range: [uploaded metadata (+ spectra) | status (+ results) | workspace]. */
int layout_and_upload(PlanBuild &B) {
    pya_plan *p = B.p;
    pya_handle *h = B.h;
    const pya_batch *b = B.b;
    const IoReq *io = B.io;
    const size_t n = B.n, n_aux = (size_t)B.total_aux, n_sigs = (size_t)B.sig_total, n_peaks = (size_t)p->total_peaks;
    ArenaLayout A;
    A.add(p->d_ret_off, n + 1, p->ret_off.data());
    A.add(p->d_peak_off, p->peak_off.size(), p->peak_off.data());
    A.add(p->d_pep_off, n + 1, p->pep_off.data());
    A.add(p->d_aux_off, n + 1, p->aux_off.data());
    A.add(p->d_sig_off, n + 1, p->sig_off.data());
    A.add(p->d_pep, p->pep.size(), p->pep.data());
    A.add(p->d_n_sites, n, p->n_sites.data());
    A.add(p->d_n_of_mod, n, p->n_of_mod.data());
    A.add(p->d_max_charge, n, p->max_charge.data());
    A.add(p->d_n_sig, n, p->n_sig.data());
    A.add(p->d_order_off, n, p->order_off.data());
    A.add(p->d_aux_pos, n_aux, B.has_aux ? b->aux_pos + B.aux_base : nullptr);
    A.add(p->d_aux_mass, n_aux, B.has_aux ? b->aux_mass + B.aux_base : nullptr);
    A.add(p->d_bin_ids, p->bin_ids.size(), p->bin_ids.data());
    A.add(p->d_score_ids, p->score_ids.size(), p->score_ids.data());
    A.add(p->d_fused_ids, p->fused_ids.size(), p->fused_ids.data());
    A.add(p->d_desc, p->desc.size(), p->desc.data());
    A.add(p->d_big_ids, p->big_ids.size(), p->big_ids.data());
    A.add(p->bigloc.d_ids, p->bigloc.ids.size(), p->bigloc.ids.data());
    A.add(p->d_gen_ids, p->gen_ids.size(), p->gen_ids.data());
    A.add(p->d_gen_off, p->gen_off.size(), p->gen_off.data());
    A.add(p->d_bigbin_ids, p->bigbin_ids.size(), p->bigbin_ids.data());
    for (Bucket &bk : p->buckets) A.add(bk.d_ids, bk.ids.size(), bk.ids.data());
    std::vector<uint32_t> fan_spec;                   /* (uploaded before this function returns) */
    if (p->shared) {
        fan_spec = p->spec_of;
        for (size_t i = 0; i < n; i++)
            if (p->pre_status[i]) fan_spec[i] = 0xffffffffu;    /* set aside: the fan-out leaves its status alone */
        A.add(p->d_spec_of, n, fan_spec.data());
        A.add(p->d_sret_off, p->sret_off.size(), p->sret_off.data());
    }
    if (io && !io->d_mz_ext) {                        /* pya_score_batch: the spectra ride in the same copy ... */
        const size_t mzb = spec_elem_bytes(io->sp.mz_type), itb = spec_elem_bytes(io->sp.intensity_type);   /* (real bytes) */
        A.add(p->d_mz, n_peaks * mzb, spec_at(io->sp.mz, io->sp.mz_type, B.peak_base));
        A.add(p->d_inten, n_peaks * itb, spec_at(io->sp.intensity, io->sp.intensity_type, B.peak_base));
    } else if (io) {                                  /* ... unless the caller uploads them itself */
        p->d_mz.adopt(io->d_mz_ext, n_peaks * spec_elem_bytes(io->sp.mz_type));
        p->d_inten.adopt(io->d_inten_ext, n_peaks * spec_elem_bytes(io->sp.intensity_type));
    }
    const size_t h2d_bytes = A.total;
    p->o_status = A.add(p->d_status, n);
    if (io) {
        const size_t mk = p->io_max_k = io->max_k;
        p->o_best_score = A.add(p->d_best_score, n);
        p->o_best_sig = A.add(p->d_best_sig, n);
        p->o_n_sig_out = A.add(p->d_n_sig_out, n);
        p->o_ascores = A.add(p->d_ascores, n * mk);
        p->o_alt = A.add(p->d_alt, n * mk);
    }
    p->d2h_bytes = A.total - p->o_status;
    A.add(p->d_ret_n, n);
    if (p->shared) {
        A.add(p->d_sret_n, (size_t)p->n_spec);
        A.add(p->d_sstatus, (size_t)p->n_spec);
    }
    A.add(p->d_ret, (size_t)p->ret_off[n] + 8);      /* (eight entries of slack behind the last table) */
    A.add(p->d_grid, n * PYA_GRID_CELLS);
    A.add(p->d_redo, kRedoHead + n);
    A.add(p->d_redo3, kRedoHead + 2 * n);
    A.add(p->d_redo4, kRedoHead + p->n_fused_total);
    A.add(p->d_redo5, kRedoHead + p->n_big_inline);
    A.add(p->d_ws_top, n * 4);
    A.add(p->d_ws, n_sigs);
    A.add(p->d_rec, n_sigs * h->rec_words());
    if (B.flags & PYA_FLAG_KEEP) A.add(p->d_sorted, n_sigs);
    A.add(p->d_gen_scratch, p->gen_off.empty() ? 0 : (size_t)p->gen_off.back());
    p->bigbin_stride = p->bigbin_ids.empty() ? 0 : (pya_bin_global_scratch_bytes(p->bigbin_cap) + 255) & ~(size_t)255;
    A.add(p->d_bigbin_scratch, p->bigbin_ids.size() * p->bigbin_stride);
    if (!p->arena.take_if_fits(h->spare_arena, A.total) && !p->arena.take_if_fits(h->spare_arena2, A.total))
        HIPCHK(h, p->arena.alloc(A.total));
    unsigned char *base = p->arena.p;
    A.adopt_all(base);
    if (h2d_bytes <= kStageLimit) {
        /* small batch: HIP call overhead dominates, so gather on the host and copy once */
        h->stage.resize(std::max(h->stage.size(), h2d_bytes));
        for (const ArenaLayout::Up &u : A.ups) std::memcpy(h->stage.data() + u.off, u.src, u.bytes);
        HIPCHK(h, hipMemcpy(base, h->stage.data(), h2d_bytes, hipMemcpyHostToDevice));
        /* (a null-stream copy from pageable memory; the plan may run on a non-blocking stream, which does not wait for it) */
        HIPCHK(h, hipStreamSynchronize(nullptr));
    } else {
        hipStream_t ust = io ? io->stream : nullptr;
        for (const ArenaLayout::Up &u : A.ups) HIPCHK(h, hipMemcpyAsync(base + u.off, u.src, u.bytes, hipMemcpyHostToDevice, ust));
        if (ust) HIPCHK(h, hipStreamSynchronize(ust));
        else HIPCHK(h, hipDeviceSynchronize());
    }
    if (B.n_skipped) {      /* bin_spectra never touches these entries, so they keep their code for every run */
        HIPCHK(h, hipMemcpy(p->d_status.p, p->pre_status.data(), n * sizeof(int32_t), hipMemcpyHostToDevice));
        HIPCHK(h, hipStreamSynchronize(nullptr));
    }
    return PYA_OK;
}

/* what a run needs besides the arena: the side stream and its two events when the run forks, the timing ring */
int make_run_resources(PlanBuild &B) {
    pya_plan *p = B.p;
    pya_handle *h = B.h;
    /* the fused family beside the others (host_internal.h: pya_plan::fork) when the batch has both */
    const bool others = !p->gen_ids.empty() || pya_plan::any_ids(p->score_lists) || pya_plan::any_ids(p->big_lists);
    p->fork = !h->kn.no_fork && p->n_fused_total != 0 && others;
    if (p->fork) {
        if (!h->side_stream) HIPCHK(h, hipStreamCreateWithFlags(&h->side_stream, hipStreamNonBlocking));
        p->side = h->side_stream;
        HIPCHK(h, hipEventCreateWithFlags(&p->ev_fork, hipEventDisableTiming));
        HIPCHK(h, hipEventCreateWithFlags(&p->ev_join, hipEventDisableTiming));
    }
    if (B.flags & PYA_FLAG_TIMING) {
        p->evring.assign(pya_plan::kEvPerRun * pya_plan::kEvRing, nullptr);
        p->evalias.assign(pya_plan::kEvPerRun * pya_plan::kEvRing, 0);
        /* (timing only: nothing synchronises-with the work through these events, so no system-scope fence per record) */
        for (auto &e : p->evring) HIPCHK(h, hipEventCreateWithFlags(&e, hipEventDisableSystemFence));
    }
    return PYA_OK;
}

/* the plan's buffers as the kernels see them (BatchDev: common.h) */
void fill_dev(pya_plan *p) {
    pya_handle *h = p->h;
    BatchDev &d = p->dev;
    std::memset(&d, 0, sizeof d);
    d.peak_off = p->d_peak_off.p;
    d.pep = p->d_pep.p;
    d.pep_off = p->d_pep_off.p;
    d.n_of_mod = p->d_n_of_mod.p;
    d.max_charge = p->d_max_charge.p;
    d.aux_pos = p->d_aux_pos.p;
    d.aux_mass = p->d_aux_mass.p;
    d.aux_off = p->d_aux_off.p;
    d.n_sites = p->d_n_sites.p;
    d.n_sig = p->d_n_sig.p;
    d.order_off = p->d_order_off.p;
    d.sig_off = p->d_sig_off.p;
    d.desc = p->d_desc.p;
    shared_tables(h, d);
    d.ret = p->d_ret.p;
    d.ret_off = p->d_ret_off.p;
    d.ret_n = p->d_ret_n.p;
    d.grid = p->d_grid.p;
    d.redo_count = p->d_redo.p;
    d.redo_ids = p->d_redo.p + kRedoHead;
    d.redo3_count = p->d_redo3.p;
    d.redo3_ids = p->d_redo3.p + kRedoHead;
    d.redo3b_count = p->d_redo3.p + 1;
    d.redo3b_ids = p->d_redo3.p + kRedoHead + p->n_psm;
    /* (the hand-over counts share the head of d_redo: two sets, taken in turn by the runs -- pya_plan_run, host_run.cpp) */
    d.redo4_count = p->d_redo.p + 1;
    d.redo4_ids = p->d_redo4.p + kRedoHead;
    d.ws = p->d_ws.p;
    d.ws_top = p->d_ws_top.p;
    d.rec = p->d_rec.p;
    d.sorted_idx = p->d_sorted.p;
    d.status = p->d_status.p;
    d.max_k = p->max_k;
    d.keep = (p->flags & PYA_FLAG_KEEP) ? 1u : 0u;
    d.debug = h->kn.debug;
    if (h->kn.stamps) {
        if (!p->d_stamps.p) {
            (void)p->d_stamps.alloc(64);
            (void)hipMemset(p->d_stamps.p, 0, 64 * 8);
        }
        d.stamps = p->d_stamps.p;
    }
}

}  // namespace

int spectra_types(pya_handle *h, const pya_typed_spectra *s, const char *who, uint32_t *types) {
    if (!spec_elem_bytes(s->mz_type) || !spec_elem_bytes(s->intensity_type))
        return h->fail(PYA_ERR_ARG, -1, "%s: spectrum types (%u, %u) are not PYA_F64 (%u) / PYA_F32 (%u)", who, s->mz_type, s->intensity_type,
                       PYA_F64, PYA_F32);
    if (s->mz_type == PYA_F32 && s->intensity_type == PYA_F64)
        return h->fail(PYA_ERR_ARG, -1, "%s: float32 m/z with float64 intensities is not supported (pass both as float32 or widen the m/z)", who);
    *types = s->mz_type == PYA_F32 ? PYA_SPEC_F32_F32 : s->intensity_type == PYA_F32 ? PYA_SPEC_F64_F32 : PYA_SPEC_F64_F64;
    return PYA_OK;
}

int check_spec_of(pya_handle *h, uint64_t n_psm, const uint32_t *spec_of, uint64_t n_spectra) {
    h->err.clear();
    h->err_index = -1;
    if (n_psm == 0) return PYA_OK;
    if (!spec_of) return h->fail(PYA_ERR_ARG, -1, "NULL spec_of");
    if (n_spectra == 0) return h->fail(PYA_ERR_ARG, 0, "PSM 0: the batch has PSMs and no spectra (n_spectra is 0)");
    if (n_spectra >= 0xffffffffull) return h->fail(PYA_ERR_LIMIT, -1, "more than 2^32 - 2 spectra in one batch");
    for (uint64_t i = 0; i < n_psm; i++) {
        if (spec_of[i] >= n_spectra)
            return h->fail(PYA_ERR_ARG, (int64_t)i, "PSM %llu: spec_of is %u, the batch has %llu spectra", (unsigned long long)i, spec_of[i],
                           (unsigned long long)n_spectra);
        if (i && spec_of[i] < spec_of[i - 1])
            return h->fail(PYA_ERR_ARG, (int64_t)i, "PSM %llu: spec_of decreases (%u after %u); the PSMs of a spectrum must be consecutive",
                           (unsigned long long)i, spec_of[i], spec_of[i - 1]);
    }
    return PYA_OK;
}

int plan_create_impl(pya_handle *h, const pya_batch *b, uint32_t flags, const IoReq *io, const SpecShare *sh, pya_plan **out) {
    if (!h || !b || !out) return PYA_ERR_ARG;
    *out = nullptr;
    h->err.clear();
    h->err_index = -1;
    HIPCHK(h, hipSetDevice(h->device));
    int rc = sync_config(h);
    if (rc) return rc;
    const uint64_t n = b->n_psm;
    if (n > 0 && (!b->peak_off || !b->pep || !b->pep_off || !b->n_of_mod || !b->max_charge))
        return h->fail(PYA_ERR_ARG, -1, "NULL array in batch");
    if (n >= (1ull << 31)) return h->fail(PYA_ERR_LIMIT, -1, "more than 2^31 PSMs in one batch");
    Lap lap{h->kn.host_timing};
    std::unique_ptr<pya_plan> p(new pya_plan);
    p->h = h;
    p->settings_gen = h->settings_gen;                       /* (sync_config above: the device has this generation's DevConfig) */
    for (Bucket &bk : p->buckets) bk.take_knobs(h->kn);      /* (PYA_SB / PYA_GTP / PYA_HASH_PP of THIS handle) */
    p->fusedb.take_knobs(h->kn);
    p->bigloc.take_knobs(h->kn);
    p->flags = flags;
    p->n_psm = n;
    p->shared = sh != nullptr && n != 0;
    p->n_spec = p->shared ? sh->n_spectra : n;
    PlanBuild B(h, b, io, sh, flags, p.get());
    if ((rc = copy_meta(B))) return rc;
    lap("copy meta");
    p->n_sites.resize(n);
    p->n_sig.resize(n);
    p->order_off.resize(n);
    p->sig_off.resize(n + 1);
    p->ncls.assign(n, 0);
    p->fused.assign(n, 0);
    p->big.assign(n, 0);
    p->gen.assign(n, 0);
    scan_letters(B);
    lap("letter scan");
    if ((rc = route_psms(B))) return rc;
    settle_fallbacks(B);
    lap("psm loop");
    p->n_skipped = B.n_skipped;
    p->sig_off[n] = B.sig_total;
    p->total_sigs = B.sig_total;
    p->max_k = B.max_k;
    p->peak_cap = (B.max_P + 31u) & ~31u;
    peak_classes_and_lists(B);
    fused_launches(B);
    pack_descriptors(B);
    lap("id lists");
    if ((rc = ensure_lut(h, B.lut_need))) return rc;
    if ((rc = upload_shared_tables(h))) return rc;
    if ((rc = check_lds_budgets(B))) return rc;
    lap("tables");
    if ((rc = layout_and_upload(B))) return rc;
    lap("arena+upload");
    if ((rc = make_run_resources(B))) return rc;
    fill_dev(p.get());
    *out = p.release();
    return PYA_OK;
}

/* a plan never sees host spectra: its user corrects their own device arrays (pya_recalibrate_spectra) before pya_plan_run_typed */
static int refuse_recalibrate(pya_handle *h, uint32_t flags, pya_plan **out) {
    if (!h || !(flags & PYA_FLAG_RECALIBRATE)) return PYA_OK;
    if (out) *out = nullptr;
    return h->fail(PYA_ERR_ARG, -1, "pya_plan_create does not take PYA_FLAG_RECALIBRATE: call pya_recalibrate_spectra on the device arrays before "
                                    "pya_plan_run_typed");
}

int pya_plan_create(pya_handle *h, const pya_batch *b, uint32_t flags, pya_plan **out) {
    const int rc_flag = refuse_recalibrate(h, flags, out);
    if (rc_flag) return rc_flag;
    return plan_create_impl(h, b, flags, nullptr, nullptr, out);
}

int pya_plan_create_shared(pya_handle *h, const pya_batch *b, const uint32_t *spec_of, uint64_t n_spectra, uint32_t flags,
                           pya_plan **out) {
    if (!h || !b || !out) return PYA_ERR_ARG;
    *out = nullptr;
    const int rc_flag = refuse_recalibrate(h, flags, out);
    if (rc_flag) return rc_flag;
    const int rc = check_spec_of(h, b->n_psm, spec_of, n_spectra);
    if (rc) return rc;
    const SpecShare sh = {spec_of, n_spectra, 0u};
    return plan_create_impl(h, b, flags, nullptr, &sh, out);
}

uint64_t pya_plan_workspace_bytes(const pya_plan *p) { return p ? p->workspace_bytes() : 0; }
uint64_t pya_plan_total_signatures(const pya_plan *p) { return p ? (uint64_t)p->total_sigs : 0; }

void pya_plan_destroy(pya_plan *p) {
    if (!p) return;
    (void)hipSetDevice(p->h->device);
    if (p->d_stamps.p) {
        unsigned long long v[64];
        (void)hipDeviceSynchronize();
        (void)hipMemcpy(v, p->d_stamps.p, sizeof v, hipMemcpyDeviceToHost);
        unsigned long long tot = 0;
        for (int i = 0; i < 64; i++) tot += v[i];
        std::fprintf(stderr, "[pya stamps] total %llu\n", tot);
        for (int i = 0; i < 64; i++)
            if (v[i]) std::fprintf(stderr, "[pya stamps] phase %2d: %12llu  %5.1f%%\n", i, v[i], 100.0 * v[i] / tot);
    }
    if (p->h->kept == p) p->h->kept = nullptr;
    if (p->h->one.view == p) p->h->one.view = nullptr;       /* (pya_score_one's retained view of its workspace) */
    if (!p->quiesced) (void)hipDeviceSynchronize();     /* nothing may still be using the buffers */
    if (!p->h->spare_arena.p) p->arena.give_to(p->h->spare_arena);
    else if (!p->h->spare_arena2.p) p->arena.give_to(p->h->spare_arena2);
    else if (p->h->spare_arena.n <= p->h->spare_arena2.n) p->arena.give_to(p->h->spare_arena);
    else p->arena.give_to(p->h->spare_arena2);
    delete p;
}
