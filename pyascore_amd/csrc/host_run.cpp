/* host_run.cpp -- running a plan: the launch families of pya_plan_run, the fork onto the side stream and the ONE way back
 * from it, the timing ring, the per-PSM status. */
#include "host_internal.h"

namespace {

/* which scoring kernel a list of one C(n,k) class gets, and with what caps -- decided at every run from the handle's
 * settings and switches as they are then */
struct ScoreRoute {
    enum Kind { kCountNodes, kCountNodesGeneral, kSignatures } kind;
    uint32_t prefix, compact, kc, node_cap, node_cols, res_cap, nl_cap;
};

ScoreRoute pick_score_route(const pya_handle *h, const Bucket &bk, uint32_t ncls, uint32_t peak_cap) {
    const DevConfig &c = h->cfg;
    ScoreRoute r = {ScoreRoute::kSignatures, score_prefix(h, bk.n_cap), score_compact(c, bk.z_max), 8u, 0u, 0u, 0u, nl_cap(c)};
    const bool general = general_settings(c);
    /* the count-node tables: fragment tolerance below half a unit, room for the launch's k and site counts */
    const bool cnt_ok = h->mz_error <= 0.49f && bk.k_max + 1u <= 31u && bk.ns_max <= 32u && !h->kn.no_cnt && !(h->kn.debug & 0x8000u);
    /* many site assignments (classes above 64) under the plain settings with both directions, charge 1: the count-node
     * table decides the fragments (score_cnt.hip) */
    if (ncls >= 1 && !general && c.n_fwd == 1 && c.n_types == 2 && bk.z_max == 1 && cnt_ok) {
        while (r.kc < bk.k_max + 1u) r.kc <<= 1;
        if (pya_score_cnt_lds_bytes(peak_cap, bk.pos_cap, r.kc, bk.k_max, bk.ns_max) <= 64u * 1024u) {
            r.kind = ScoreRoute::kCountNodes;
            return r;
        }
    }
    /* general settings: the count nodes carry over when the loss variants depend on the count too (score_cntg.hip; the
     * kernel checks that per peptide and walks what does not qualify) */
    if (general && cnt_ok && pya_score_cntg_lds_bytes(peak_cap, bk.pos_cap, bk.k_max, bk.ns_max, r.nl_cap) <= 64u * 1024u) {
        r.kind = ScoreRoute::kCountNodesGeneral;
        return r;
    }
    /* score_signatures -- under general settings with one lookup set per distinct node of the assignment tree instead of
     * one per signature (score_core.hip.h: score_nodes_dir).  The node kernel's LDS decides its occupancy: residue and
     * loss-state tables by the launch, room for 320 nodes per direction -- cfg4's shape needs 186 on average, 328 at
     * most; a direction with more is walked */
    r.node_cols = std::max<uint32_t>(8u, (bk.node_cols + 7u) & ~7u);
    r.res_cap = std::min<uint32_t>(64u, (bk.pos_cap + 1u + 3u) & ~3u);
    if (general && !r.prefix && !h->kn.no_nodes && bk.node_words) {
        r.node_cap = std::min<uint32_t>(320u, (bk.pos_cap * std::min<uint32_t>(bk.n_cap, 64u) + 1u) & ~1u);
        if (h->kn.node_cap >= 0) r.node_cap = (uint32_t)h->kn.node_cap & ~1u;
        if (pya_score_node_lds_bytes(peak_cap, with_nl(c), r.node_cap, r.node_cols, bk.node_words, r.res_cap, r.nl_cap) > 64u * 1024u)
            r.node_cap = 0;
    }
    return r;
}

/* PYA_FLAG_TIMING: the events of this run in the plan's ring (without the flag mark() does nothing) */
struct RunMarks {
    pya_handle *h;
    hipStream_t st;
    hipEvent_t *ev;
    uint8_t *alias;
    /* boundary i of the run: a new event if the family before it launched anything, else the previous boundary's */
    int operator()(int i, bool launched) const {
        if (!ev) return PYA_OK;
        if (i > 0 && !launched) {
            alias[i] = alias[i - 1];
            return PYA_OK;
        }
        alias[i] = (uint8_t)i;
        if (hipEventRecord(ev[i], st) != hipSuccess) return h->hip_fail(hipGetLastError(), "hipEventRecord");
        return PYA_OK;
    }
};

/* A handful of PSMs (PyAscore.score is a batch of one) is launch-bound: one fused launch, one wavefront per PSM, instead of
 * the five of the three-kernel path (tiny_batch.hip).  *done = whether the batch went that way. */
int run_tiny(pya_plan *p, const BatchDev &d, uint32_t types, hipStream_t st, bool *done) {
    pya_handle *h = p->h;
    *done = false;
    /* (the tiny kernel bins per PSM from the PSM's own float64 peaks: a shared batch and a batch with float32 arrays,
     * however small, take the plan's launches) */
    if ((p->flags & (PYA_FLAG_TIMING | PYA_FLAG_EVIDENCE | PYA_FLAG_IONS | PYA_FLAG_NAMED | PYA_FLAG_ROLLUP | PYA_FLAG_PEPTIDOFORMS | PYA_FLAG_MZ_PROFILE | PYA_FLAG_COVERAGE | PYA_FLAG_QUANT | PYA_FLAG_PFORM_QUANT | PYA_FLAG_SITES | PYA_FLAG_PROBS | PYA_FLAG_RANKED)) || p->n_psm > (uint64_t)h->kn.tiny_max || p->n_skipped != 0 || h->kn.no_tiny || !p->gen_ids.empty() ||
        p->shared || types != PYA_SPEC_F64_F64)
        return PYA_OK;
    /* caps that cover every PSM of the batch (the PSMs the fused kernel would take are accounted in their own bucket: its
     * caps count too -- leaving them out sized this launch's work areas for the other PSMs only) */
    Bucket m;
    m.take_knobs(h->kn);
    for (const Bucket &bk : p->buckets)
        if (!bk.ids.empty()) m.absorb(bk);
    if (!p->fusedb.ids.empty()) m.absorb(p->fusedb);
    if (p->n_big_inline != 0) m.absorb(p->bigloc);
    const uint32_t prefix = score_prefix(h, m.n_cap), compact = score_compact(h->cfg, m.z_max);
    /* the merged caps (maxima over the buckets) can ask for more LDS than any single bucket does:
     * such a batch takes the three-kernel path, whose launches are sized per bucket */
    if (pya_tiny_lds_bytes(p->peak_cap, prefix, with_nl(h->cfg), compact, m.push_cap(), m.n_cap, m.pos_cap, m.pool_cap(), m.sb()) > kMaxLds)
        return PYA_OK;
    int e = pya_launch_tiny(&d, (uint32_t)p->n_psm, p->peak_cap, prefix, with_nl(h->cfg), compact, m.push_cap(), m.n_cap, m.pos_cap,
                            m.pool_cap(), m.sb(), m.gtp(), st);
    if (e) return h->hip_fail((hipError_t)e, "tiny_batch launch");
    *done = true;
    return PYA_OK;
}

/* `types`: the element types of d.mz / d.inten (PYA_SPEC_*) -- every launch of the family, the exact kernel that works off what
 * the others hand over included, is the instantiation for them */
int run_binning(pya_plan *p, const BatchDev &d, uint32_t types, hipStream_t st) {
    pya_handle *h = p->h;
    int e = 0;
    for (const pya_plan::IdList &l : p->bin_lists) {
        /* dense classes: selection first (bin_select.hip.h); the all-pairs ranking of bin_fast is O(window^2) and holds 13 bytes
         * of LDS per raw peak */
        const uint32_t scap = (uint32_t)std::min<int64_t>(std::max<int64_t>(h->kn.bin_select_scap, 64), 4096) & ~31u;
        if ((int64_t)l.cap > h->kn.bin_select_min)
            e = pya_launch_bin_select(&d, p->d_bin_ids.p + l.off, l.n, scap, types, st);
        else
            e = pya_launch_bin(&d, p->d_bin_ids.p + l.off, l.n, l.cap, types, st);
        if (e) return h->hip_fail((hipError_t)e, "bin_spectra launch");
    }
    e = pya_launch_bin_exact(&d, (uint32_t)p->n_psm, p->peak_cap, types, st);
    if (e) return h->hip_fail((hipError_t)e, "bin_spectra (exact) launch");
    e = pya_launch_bin_global(&d, p->d_bigbin_ids.p, (uint32_t)p->bigbin_ids.size(), p->d_bigbin_scratch.p, p->bigbin_stride, p->bigbin_cap, types, st);
    if (e) return h->hip_fail((hipError_t)e, "bin_spectra (global) launch");
    return PYA_OK;
}

/* Shared spectra: the binning family over SPECTRUM ids with the spectrum-side view of the plan (peak_off is the spectra's
 * already; ret_off, ret_n and status by spectrum), then the fan-out that gives every PSM its spectrum's ret_n and status --
 * behind it every kernel reads by PSM number, as in an unshared plan. */
int run_binning_shared(pya_plan *p, const BatchDev &d, uint32_t types, hipStream_t st) {
    BatchDev sd = d;
    sd.ret_off = p->d_sret_off.p;
    sd.ret_n = p->d_sret_n.p;
    sd.status = p->d_sstatus.p;
    const int rc = run_binning(p, sd, types, st);
    if (rc) return rc;
    const int e = pya_launch_fan_out(p->d_spec_of.p, p->d_sret_n.p, p->d_sstatus.p, d.ret_n, d.status, (uint32_t)p->n_psm, st);
    if (e) return p->h->hip_fail((hipError_t)e, "fan-out launch");
    return PYA_OK;
}

/* the fused family: few site assignments, plain settings, scored and localised in one pass (score_localize.hip), one PSM
 * per wavefront; what it hands over goes through the general localize instantiation.  On `fs`: the plan's side stream when
 * the run forks (every other family is independent of it: other PSMs, other hand-over lists), else the caller's. */
int run_fused_family(pya_plan *p, const BatchDev &d, hipStream_t fs) {
    pya_handle *h = p->h;
    const Bucket &fb = p->fusedb;
    for (const pya_plan::FusedLaunch &l : p->fused_launches) {
        int fe = pya_launch_fused(&d, p->d_fused_ids.p + l.off, l.n, l.cap, l.n_cap, l.stride, l.pos_cap, l.ent_cap, l.push_cap,
                                  p->fused_both, l.multi_z, d.redo4_count, d.redo4_ids, fs);
        if (fe) return h->hip_fail((hipError_t)fe, "score_localize launch");
    }
    int fe = pya_launch_localize_redo(&d, d.redo4_count, d.redo4_ids, p->n_fused_total, fb.push_cap(), fb.n_cap,
                                      fb.pos_cap, fb.pool_cap(), fb.sb(), fb.gtp(), fs);
    if (fe) return h->hip_fail((hipError_t)fe, "localize (hand-over) launch");
    return PYA_OK;
}

/* the scoring kernels of every PSM that is not fused and not general: per C(n,k) class and peak class, then score_big's */
int run_scoring(pya_plan *p, const BatchDev &d, hipStream_t st) {
    pya_handle *h = p->h;
    int e = 0;
    for (const pya_plan::IdList &l : p->score_lists) {
        const Bucket &bk = p->buckets[l.ncls];
        const uint32_t *ids = p->d_score_ids.p + l.off;
        const ScoreRoute r = pick_score_route(h, bk, l.ncls, l.cap);
        switch (r.kind) {
            case ScoreRoute::kCountNodes:
                e = pya_launch_score_cnt(&d, ids, l.n, l.cap, bk.pos_cap, r.kc, bk.k_max, bk.ns_max, st);
                if (e) return h->hip_fail((hipError_t)e, "score_cnt launch");
                break;
            case ScoreRoute::kCountNodesGeneral:
                e = pya_launch_score_cntg(&d, ids, l.n, l.cap, bk.pos_cap, bk.k_max, bk.ns_max, r.nl_cap, st);
                if (e) return h->hip_fail((hipError_t)e, "score_cntg launch");
                break;
            case ScoreRoute::kSignatures:
                e = pya_launch_score(&d, ids, l.n, l.cap, r.prefix, with_nl(h->cfg), r.compact, r.node_cap, r.node_cols, bk.node_words,
                                     r.res_cap, r.nl_cap, st);
                if (e) return h->hip_fail((hipError_t)e, "score_signatures launch");
                break;
        }
    }
    for (const pya_plan::IdList &l : p->big_lists) {
        e = pya_launch_score_big(&d, p->d_big_ids.p + l.off, l.n, l.cap, p->big_pos_cap, p->big_kc(), p->big_inline ? 1u : 0u, st);
        if (e) return h->hip_fail((hipError_t)e, "score_big launch");
    }
    return PYA_OK;
}

/* what score_big scored in its summary mode: the lean body with recounted signatures and the winner score_big
 * named; what that declines is scored again with count records and goes to the general localize body */
int run_big_inline(pya_plan *p, const BatchDev &d, hipStream_t st) {
    pya_handle *h = p->h;
    const Bucket &bl = p->bigloc;
    uint32_t *count = d.redo_count + 2, *ids = p->d_redo5.p + kRedoHead;
    int e = pya_launch_localize_recount(&d, bl.d_ids.p, (uint32_t)bl.ids.size(), 0u, bl.push_cap(), bl.pos_cap, bl.pool_cap(),
                                        bl.sb(), bl.gtp(), count, ids, st);
    if (e) return h->hip_fail((hipError_t)e, "localize (recount) launch");
    e = pya_launch_score_big_list(&d, count, ids, p->n_big_inline, p->peak_cap, p->big_pos_cap, p->big_kc(), st);
    if (e) return h->hip_fail((hipError_t)e, "score_big (hand-over) launch");
    e = pya_launch_localize_redo(&d, count, ids, p->n_big_inline, bl.push_cap(), (uint32_t)pya_big_inline_max(),
                                 bl.pos_cap, bl.pool_cap(), bl.sb(), bl.gtp(), st);
    if (e) return h->hip_fail((hipError_t)e, "localize (score_big hand-over) launch");
    return PYA_OK;
}

/* every class: the lean instantiation for its plain PSMs, then the general one (hash route where its tables fit) */
int run_localize(pya_plan *p, const BatchDev &d, hipStream_t st) {
    pya_handle *h = p->h;
    const uint32_t nnl = (uint32_t)h->cfg.n_nl;
    for (Bucket &bk : p->buckets) {
        /* more than sort_room_max signatures: the lean launch without room for the sort emulation (LDS ->
         * occupancy); PSMs with a tie at the top go through the hand-over list to a second lean pass that has it */
        const uint32_t sort_room = (bk.n_cap <= h->kn.sort_room_max || h->kn.sort_room) ? 1u : 0u;
        int e = pya_launch_localize(&d, bk.d_ids.p, bk.n_plain, bk.push_cap(), bk.n_cap, bk.pos_cap, bk.pool_cap(), bk.sb(),
                                    bk.gtp(), 1u, sort_room, st);
        if (e) return h->hip_fail((hipError_t)e, "localize launch");
        if (h->kn.host_timing && !bk.ids.empty() && p->n_runs == 1)    /* diagnostics: what decides the general route's occupancy */
            std::fprintf(stderr, "[pya plan] localize bucket: %zu PSMs, LDS hash route %zu B (vc %u hs %u pp %u sb %u push %u), list route %zu B\n",
                         bk.ids.size(), pya_localize_hash_lds_bytes(bk.push_cap(), bk.n_cap, bk.pos_cap, bk.sb(), bk.hash_vc(), bk.hash_hs(),
                                                                    bk.hash_pp(), p->max_k, nnl),
                         bk.hash_vc(), bk.hash_hs(), bk.hash_pp(), bk.sb(), bk.push_cap(),
                         pya_localize_lds_bytes(bk.push_cap(), bk.n_cap, bk.pos_cap, bk.pool_cap(), bk.sb()));
        const uint32_t *general_ids = bk.d_ids.p + bk.n_plain, n_general = (uint32_t)bk.ids.size() - bk.n_plain;
        if (!h->kn.no_loc_hash && bk.hash_ok(p->max_k, nnl))
            e = pya_launch_localize_hash(&d, general_ids, n_general, bk.push_cap(), bk.n_cap, bk.pos_cap, bk.pool_cap(), bk.sb(),
                                         bk.gtp(), bk.hash_vc(), bk.hash_hs(), bk.hash_pp(), nnl, st);
        else
            e = pya_launch_localize(&d, general_ids, n_general, bk.push_cap(), bk.n_cap, bk.pos_cap, bk.pool_cap(), bk.sb(),
                                    bk.gtp(), 0u, 1u, st);
        if (e) return h->hip_fail((hipError_t)e, "localize launch");
    }
    return PYA_OK;
}

int run_general(pya_plan *p, const BatchDev &d, hipStream_t st) {
    int e = pya_launch_general(&d, p->d_gen_ids.p, (uint32_t)p->gen_ids.size(), p->d_gen_scratch.p, p->d_gen_off.p, p->gen_l_cap,
                               p->gen_list_cap, st);
    if (e) return p->h->hip_fail((hipError_t)e, "general kernel launch");
    return PYA_OK;
}

/* Everything of a run behind the binning.  A forked run has recorded ev_fork on `st` by now and pya_plan_run joins the
 * side stream whatever this returns: nothing in here leaves pya_plan_run on its own. */
int run_behind_binning(pya_plan *p, const BatchDev &d, hipStream_t st, const RunMarks &mark) {
    pya_handle *h = p->h;
    int rc;
    if (mark.alias) mark.alias[5] = 0;
    if (p->fork) {
        HIPCHK(h, hipStreamWaitEvent(p->side, p->ev_fork, 0));
        if (mark.ev) {
            mark.alias[5] = 1;
            HIPCHK(h, hipEventRecord(mark.ev[5], p->side));
        }
        if ((rc = run_fused_family(p, d, p->side))) return rc;
        if (mark.ev) HIPCHK(h, hipEventRecord(mark.ev[6], p->side));
    }
    if ((rc = run_scoring(p, d, st))) return rc;
    if ((rc = mark(2, pya_plan::any_ids(p->score_lists) || pya_plan::any_ids(p->big_lists)))) return rc;
    const bool fused_here = p->n_fused_total != 0 && !p->fork;
    if (fused_here && (rc = run_fused_family(p, d, st))) return rc;
    if ((rc = mark(3, fused_here))) return rc;
    const bool big_inline = p->big_inline && !p->bigloc.ids.empty();
    if (big_inline && (rc = run_big_inline(p, d, st))) return rc;
    if ((rc = run_localize(p, d, st))) return rc;
    if (!p->gen_ids.empty() && (rc = run_general(p, d, st))) return rc;
    if (mark.ev) {
        bool loc = big_inline || !p->gen_ids.empty();
        for (const Bucket &bk : p->buckets) loc = loc || !bk.ids.empty();
        if ((rc = mark(4, loc))) return rc;
        p->ev_runs++;
        if (p->ev_runs - p->ev_read > pya_plan::kEvRing) p->ev_read = p->ev_runs - pya_plan::kEvRing;   /* (overwritten) */
    }
    return PYA_OK;
}

}  // namespace

int pya_plan_run(pya_plan *p, const double *d_mz, const double *d_inten, void *hip_stream,
                 const pya_results *o) {
    const pya_typed_spectra sp = {d_mz, d_inten, PYA_F64, PYA_F64};
    return pya_plan_run_typed(p, &sp, hip_stream, o);
}

int pya_plan_run_typed(pya_plan *p, const pya_typed_spectra *sp, void *hip_stream, const pya_results *o) {
    if (!p || !o) return PYA_ERR_ARG;
    pya_handle *h = p->h;
    if (const int rc_gen = plan_settings_stale(p, "pya_plan_run")) return rc_gen;
    if (p->n_psm == 0) return PYA_OK;
    if (!sp) return h->fail(PYA_ERR_ARG, -1, "NULL device pointer passed to pya_plan_run");
    uint32_t types = 0;
    const int rc_types = spectra_types(h, sp, "pya_plan_run_typed", &types);
    if (rc_types) return rc_types;
    const void *d_mz = sp->mz, *d_inten = sp->intensity;
    if (!d_mz || !d_inten || !o->best_score || !o->best_sig || !o->n_sig || !o->ascores || !o->alt_mask)
        return h->fail(PYA_ERR_ARG, -1, "NULL device pointer passed to pya_plan_run");
    if (o->max_k < p->max_k)
        return h->fail(PYA_ERR_ARG, -1, "results.max_k (%u) is smaller than the largest n_of_mod (%u)",
                       o->max_k, p->max_k);
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)hip_stream;
    shared_tables(h, p->dev);
    BatchDev d = p->dev;
    d.mz = d_mz;
    d.inten = d_inten;
    d.best_score = o->best_score;
    d.best_sig = o->best_sig;
    d.n_sig_out = o->n_sig;
    d.ascores = o->ascores;
    d.alt_mask = o->alt_mask;
    d.max_k = o->max_k;
    bool tiny = false;
    int rc = run_tiny(p, d, types, st, &tiny);
    if (rc) return rc;
    if (!tiny) {
        const bool timing = p->flags & PYA_FLAG_TIMING;
        const RunMarks mark = {h, st, timing ? p->ev_set(p->ev_runs) : nullptr, timing ? p->ev_alias(p->ev_runs) : nullptr};
        if ((rc = mark(0, true))) return rc;
        /* hand-over counts (bin_spectra's, the fused kernel's, the recount's): two sets at the head of d_redo, taken in turn;
         * the binning kernel of a run zeroes the set of the next (bin_spectra.hip), so only a plan without such a launch --
         * every spectrum binned by the global kernel, or set aside -- and the first run need a memset */
        uint32_t *cnt = p->d_redo.p + 8 * (p->n_runs & 1u);
        d.redo_count = cnt;
        d.redo4_count = cnt + 1;
        d.zero_next = p->d_redo.p + 8 * ((p->n_runs + 1u) & 1u);
        if (p->n_runs == 0 || !pya_plan::any_ids(p->bin_lists)) HIPCHK(h, hipMemsetAsync(p->d_redo.p, 0, 16 * sizeof(uint32_t), st));
        p->n_runs++;
        if ((rc = p->shared ? run_binning_shared(p, d, types, st) : run_binning(p, d, types, st))) return rc;
        if ((rc = mark(1, true))) return rc;
        if (!p->fork) {
            if ((rc = run_behind_binning(p, d, st, mark))) return rc;
        } else {
            /* From the fork to the join there is ONE way out, failing or not: whatever the caller enqueues behind this run
             * -- the plan's next run included -- waits for the side stream too (after boundary 4, so that the localize
             * family's interval does not include the wait).  The first error is what the call returns. */
            HIPCHK(h, hipEventRecord(p->ev_fork, st));
            rc = run_behind_binning(p, d, st, mark);
            hipError_t ej = hipEventRecord(p->ev_join, p->side);
            if (ej == hipSuccess) ej = hipStreamWaitEvent(st, p->ev_join, 0);
            if (ej != hipSuccess && !rc) rc = h->hip_fail(ej, "joining the side stream");
        }
    }
    p->last_stream = st;
    p->ran = true;
    p->ions_state = 0;                       /* (counts, offsets and the overflow report belonged to the run before) */
    for (OverReport &o : p->over) o.asked = false;
    p->dev = d;
    return rc;
}

namespace {
/* The four intervals of the runs [r0, r1) added to ms[] (waits for the latest of them): boundary to boundary on the caller's
 * stream, and the fused family's own interval on the side stream when a run forked (boundaries 2 and 3 are then one event). */
int add_run_intervals(pya_plan *p, uint64_t r0, uint64_t r1, double ms[4]) {
    pya_handle *h = p->h;
    HIPCHK(h, hipEventSynchronize(p->ev_set(r1 - 1)[p->ev_alias(r1 - 1)[4]]));
    if (p->ev_alias(r1 - 1)[5]) HIPCHK(h, hipEventSynchronize(p->ev_set(r1 - 1)[6]));
    for (uint64_t r = r0; r < r1; r++) {
        hipEvent_t *ev = p->ev_set(r);
        const uint8_t *al = p->ev_alias(r);
        for (int i = 0; i < 4; i++) {
            float t = 0.f;
            if (al[i] != al[i + 1]) HIPCHK(h, hipEventElapsedTime(&t, ev[al[i]], ev[al[i + 1]]));
            ms[i] += (double)t;
        }
        float side = 0.f;
        if (al[5]) HIPCHK(h, hipEventElapsedTime(&side, ev[5], ev[6]));
        ms[2] += (double)side;
    }
    return PYA_OK;
}
}  // namespace

int pya_plan_timings(pya_plan *p, float ms[4]) {
    if (!p || !ms) return PYA_ERR_ARG;
    if (!(p->flags & PYA_FLAG_TIMING) || p->ev_runs == 0) return p->h->fail(PYA_ERR_STATE, -1, "plan has no timing events");
    double sum[4] = {0., 0., 0., 0.};
    const int rc = add_run_intervals(p, p->ev_runs - 1, p->ev_runs, sum);
    for (int i = 0; i < 4; i++) ms[i] = (float)sum[i];
    return rc;
}

int pya_plan_timings_sum(pya_plan *p, double ms[4], uint32_t *n_runs) {
    if (!p || !ms || !n_runs) return PYA_ERR_ARG;
    if (!(p->flags & PYA_FLAG_TIMING)) return p->h->fail(PYA_ERR_STATE, -1, "plan has no timing events");
    for (int i = 0; i < 4; i++) ms[i] = 0.;
    *n_runs = (uint32_t)(p->ev_runs - p->ev_read);
    if (*n_runs == 0) return PYA_OK;
    const int rc = add_run_intervals(p, p->ev_read, p->ev_runs, ms);
    if (rc) return rc;
    p->ev_read = p->ev_runs;
    return PYA_OK;
}

int check_status(pya_handle *h, const int32_t *st, uint64_t n, bool skip_invalid) {
    if (skip_invalid) return PYA_OK;                    /* codes are reported per PSM instead */
    for (uint64_t i = 0; i < n; i++) {
        switch (st[i]) {
            case PYA_ST_OK: break;
            case PYA_ST_INVALID:
            case PYA_ST_OVER_LIMIT:
                return h->fail(st[i] == PYA_ST_INVALID ? PYA_ERR_PSM : PYA_ERR_LIMIT, (int64_t)i,
                               "PSM %llu was set aside by the host pre-pass", (unsigned long long)i);
            case PYA_ST_NO_BINS:
                return h->fail(PYA_ERR_PSM, (int64_t)i, "PSM %llu: all peaks sit on one multiple of 100 m/z; the "
                               "spectrum has no windows", (unsigned long long)i);
            case PYA_ST_TOO_MANY_BINS:
                return h->fail(PYA_ERR_LIMIT, (int64_t)i, "PSM %llu: more than 65535 m/z windows", (unsigned long long)i);
            case PYA_ST_LUT_RANGE:
                return h->fail(PYA_ERR_LIMIT, (int64_t)i, "PSM %llu: trial count outside the score table", (unsigned long long)i);
            case PYA_ST_PUSHED_OVERFLOW:
                return h->fail(PYA_ERR_LIMIT, (int64_t)i, "PSM %llu: more than %d tied competitors", (unsigned long long)i, PYA_MAX_PUSHED);
            case PYA_ST_ROUTE_CAPS:
                return h->fail(PYA_ERR_STATE, (int64_t)i, "PSM %llu reached a kernel whose launch was not sized for it (modifications or "
                               "modifiable residues beyond the launch's caps): a routing error of this library", (unsigned long long)i);
            default:
                return h->fail(PYA_ERR_HIP, (int64_t)i, "PSM %llu: unexpected kernel status %d", (unsigned long long)i, st[i]);
        }
    }
    return PYA_OK;
}

/* The last call of stage `which` behind this run: what it wrote nothing of, because it was not inside the room of the call
 * (the query range of a PSM; the slot of a record, of a PSM's run; the slot or the row of a record; the row of a PSM). */
int over_report(pya_plan *p, int which, uint64_t psm_lo) {
    static const char *const kText[OVER_COUNT] = {
        "pya_plan_named: the query ranges of %u PSMs (PSM %llu the first) are not inside the n_q records of the call; nothing of them was "
        "written",
        "pya_plan_rollup: %u residue records (PSM %llu the first) name a slot at or above the n_slots of the call; nothing of them was "
        "written",
        "pya_plan_mz_profile: %u PSMs (PSM %llu the first) name a run slot at or above the n_slots of the call; nothing of them was written",
        "pya_plan_site_quant: %u residue records (PSM %llu the first) name a slot at or above the n_slots or a row at or above the n_rows "
        "of the call; nothing of them was written",
        "pya_plan_peptidoform_quant: %u PSMs (PSM %llu the first) name a row at or above the n_rows of the call; nothing of them was "
        "written to the table",
    };
    uint32_t count = 0u, id = 0u;
    const int rc = p->over[which].read(p->h, &count, &id);
    if (rc || !count) return rc;
    const uint64_t first = psm_lo + id;
    return p->h->fail(PYA_ERR_LIMIT, (int64_t)first, kText[which], count, (unsigned long long)first);
}

int pya_plan_check(pya_plan *p) {
    if (!p) return PYA_ERR_ARG;
    pya_handle *h = p->h;
    if (!p->ran || p->n_psm == 0) return PYA_OK;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(p->last_stream));
    std::vector<int32_t> st(p->n_psm);
    HIPCHK(h, hipMemcpy(st.data(), p->d_status.p, p->n_psm * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (h->kn.host_timing) {                               /* diagnostics: how many PSMs the lean kernels handed over */
        uint32_t r3 = 0, r4 = 0;
        (void)hipMemcpy(&r3, p->d_redo3.p, 4, hipMemcpyDeviceToHost);
        (void)hipMemcpy(&r4, p->d_redo.p + 8 * ((p->n_runs + 1u) & 1u) + 1, 4, hipMemcpyDeviceToHost);   /* (the last run's set) */
        std::fprintf(stderr, "[pya plan] handed over: %u by the lean localize instantiation (last bucket), %u of %u by the fused kernel\n",
                     r3, r4, p->n_fused_total);
    }
    const bool skip = (p->flags & PYA_FLAG_SKIP_INVALID) != 0;
    if (skip) h->last_status = st;
    const int rc = check_status(h, st.data(), p->n_psm, skip);
    if (rc) return rc;
    for (int which = 0; which < OVER_COUNT; which++)     /* (named, rollup, mzp, quant, pfq: the order of the enum) */
        if (const int rc_over = over_report(p, which, 0)) return rc_over;
    if (p->ions_state != 2) return PYA_OK;
    /* the last pya_plan_ions of this run: PSMs whose records would have passed the caller's cap */
    uint32_t over[2] = {0u, 0u};
    HIPCHK(h, hipEventSynchronize(p->ev_ions));
    HIPCHK(h, hipMemcpy(over, p->d_ions_over.p, sizeof(over), hipMemcpyDeviceToHost));
    if (over[0])
        return h->fail(PYA_ERR_LIMIT, (int64_t)(0xffffffffu - over[1]), "pya_plan_ions: the records of %u PSMs (PSM %u the first) pass the "
                       "cap of the call; nothing of them was written", over[0], 0xffffffffu - over[1]);
    return PYA_OK;
}

namespace {
/* Makes `st` wait for the last run.  The run's own stream has joined the side stream already (pya_plan_run_typed); another
 * stream waits for an event recorded behind it. */
int wait_for_run(pya_plan *p, hipStream_t st) {
    pya_handle *h = p->h;
    if (st == p->last_stream) return PYA_OK;
    if (!p->ev_evid) HIPCHK(h, hipEventCreateWithFlags(&p->ev_evid, hipEventDisableTiming));
    HIPCHK(h, hipEventRecord(p->ev_evid, p->last_stream));
    HIPCHK(h, hipStreamWaitEvent(st, p->ev_evid, 0));
    return PYA_OK;
}

/* What a stage behind a run does before it launches.  Two launches: one for the PSMs inside the fast limits, sized by THEIR
 * longest peptide and fragment list, one for the plan's general PSMs with the general kernel's caps (a single 400-residue
 * peptide must not set the LDS, hence the occupancy, of a batch of 20-mers).  This sets the caps of the first (once per plan
 * and set of loss sums), asks whether `lds_bytes` of either fits a compute unit, and makes `st` wait for the last run. */
int stage_behind_run(pya_plan *p, hipStream_t st, const char *who, const char *kernel, size_t (*lds_bytes)(uint32_t, uint32_t)) {
    pya_handle *h = p->h;
    const uint32_t n_uniq = (uint32_t)h->cfg.n_uniq;
    if (!p->evid_caps || p->evid_uniq != n_uniq) {
        std::vector<uint32_t> fast_ids;
        uint32_t l_cap = 1, list_cap = 1;
        const bool listed = !p->gen_ids.empty();
        for (uint64_t i = 0; i < p->n_psm; i++) {
            if (!p->gen.empty() && p->gen[i]) continue;
            if (listed) fast_ids.push_back((uint32_t)i);
            if (!p->pre_status.empty() && p->pre_status[i]) continue;       /* (set aside: nothing of it is read) */
            const int64_t L = p->pep_off[i + 1] - p->pep_off[i];
            if (L < 1 || L > PYA_MAX_PEPTIDE_LEN || p->max_charge[i] < 1) continue;
            l_cap = std::max(l_cap, (uint32_t)L);
            list_cap = std::max(list_cap, (uint32_t)(L - 1) * (uint32_t)p->max_charge[i] * n_uniq);
        }
        p->evid_n_fast = listed ? (uint32_t)fast_ids.size() : (uint32_t)p->n_psm;
        if (listed && !fast_ids.empty()) {
            /* (a blocking copy: the vector does not outlive this call) */
            HIPCHK(h, p->d_evid_ids.alloc(fast_ids.size()));
            HIPCHK(h, hipMemcpy(p->d_evid_ids.p, fast_ids.data(), fast_ids.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        }
        p->evid_l_cap = l_cap;
        p->evid_list_cap = list_cap;
        p->evid_uniq = n_uniq;
        p->evid_caps = true;
    }
    if (lds_bytes(p->evid_l_cap, p->evid_list_cap) > kMaxLds || (!p->gen_ids.empty() && lds_bytes(p->gen_l_cap, p->gen_list_cap) > kMaxLds))
        return h->fail(PYA_ERR_LIMIT, -1, "%s: %u fragments per ion type exceed the %s kernel's room", who,
                       std::max(p->evid_list_cap, p->gen_ids.empty() ? 0u : p->gen_list_cap), kernel);
    return wait_for_run(p, st);
}
}  // namespace

/* The evidence stage (csrc/evidence.hip) */
int pya_plan_evidence(pya_plan *p, const pya_results *r, void *hip_stream, pya_evidence *d_out) {
    if (!p || !r) return PYA_ERR_ARG;
    pya_handle *h = p->h;
    if (const int rc_gen = plan_settings_stale(p, "pya_plan_evidence")) return rc_gen;
    if (p->n_psm == 0) return PYA_OK;
    if (!p->ran) return h->fail(PYA_ERR_STATE, -1, "pya_plan_evidence: the plan has not been run");
    if (!d_out || !r->best_score || !r->best_sig || !r->n_sig || !r->ascores || !r->alt_mask)
        return h->fail(PYA_ERR_ARG, -1, "NULL device pointer passed to pya_plan_evidence");
    if (r->max_k < p->max_k)
        return h->fail(PYA_ERR_ARG, -1, "results.max_k (%u) is smaller than the largest n_of_mod (%u)", r->max_k, p->max_k);
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const int rc = stage_behind_run(p, st, "pya_plan_evidence", "evidence", pya_evidence_lds_bytes);
    if (rc) return rc;
    shared_tables(h, p->dev);
    BatchDev d = p->dev;
    d.best_score = r->best_score;
    d.best_sig = r->best_sig;
    d.n_sig_out = r->n_sig;
    d.ascores = r->ascores;
    d.alt_mask = r->alt_mask;
    d.max_k = r->max_k;
    int e = pya_launch_evidence(&d, p->gen_ids.empty() ? nullptr : p->d_evid_ids.p, p->evid_n_fast, d_out, p->evid_l_cap,
                                p->evid_list_cap, st);
    if (!e && !p->gen_ids.empty())
        e = pya_launch_evidence(&d, p->d_gen_ids.p, (uint32_t)p->gen_ids.size(), d_out, p->gen_l_cap, p->gen_list_cap, st);
    if (e) return h->hip_fail((hipError_t)e, "evidence launch");
    return PYA_OK;
}

/* The named stage (csrc/named.hip): the same two launches behind the same wait.  It reads best_sig and n_sig of the caller's
 * results structure and nothing else of it. */
int pya_plan_named(pya_plan *p, const pya_results *r, void *hip_stream, const int64_t *d_q_off, const uint64_t *d_q_bits, uint64_t n_q,
                   pya_named *d_out, int32_t *d_counts, float *d_scores) {
    if (!p || !r) return PYA_ERR_ARG;
    pya_handle *h = p->h;
    if (const int rc_gen = plan_settings_stale(p, "pya_plan_named")) return rc_gen;
    if (p->n_psm == 0 || n_q == 0) return PYA_OK;
    if (!p->ran) return h->fail(PYA_ERR_STATE, -1, "pya_plan_named: the plan has not been run");
    if (!d_q_off || !d_q_bits || !d_out || !r->best_score || !r->best_sig || !r->n_sig)
        return h->fail(PYA_ERR_ARG, -1, "NULL device pointer passed to pya_plan_named");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)hip_stream;
    OverReport &over = p->over[OVER_NAMED];
    int rc = stage_behind_run(p, st, "pya_plan_named", "named", pya_named_lds_bytes);
    if (rc || (rc = over.begin(h, st))) return rc;
    shared_tables(h, p->dev);
    BatchDev d = p->dev;
    d.best_score = r->best_score;
    d.best_sig = r->best_sig;
    d.n_sig_out = r->n_sig;
    int e = pya_launch_named(&d, p->gen_ids.empty() ? nullptr : p->d_evid_ids.p, p->evid_n_fast, d_q_off, d_q_bits, n_q, d_out, d_counts,
                             d_scores, over.d_over.p, p->evid_l_cap, p->evid_list_cap, st);
    if (!e && !p->gen_ids.empty())
        e = pya_launch_named(&d, p->d_gen_ids.p, (uint32_t)p->gen_ids.size(), d_q_off, d_q_bits, n_q, d_out, d_counts, d_scores,
                             over.d_over.p, p->gen_l_cap, p->gen_list_cap, st);
    if (e) return h->hip_fail((hipError_t)e, "named launch");
    return over.end(h, st);
}

/* The site stage (csrc/sites.hip).  The offsets are the pre-pass's: a PSM has as many records as modifiable residues, a PSM
 * that was set aside none. */
static void site_offsets(pya_plan *p) {
    if (p->site_off.size() == p->n_psm + 1) return;
    p->site_off.assign(p->n_psm + 1, 0);
    for (uint64_t i = 0; i < p->n_psm; i++) p->site_off[i + 1] = p->site_off[i] + (int64_t)p->n_sites[i];
}

/* ... and their copy on the device for a stage on `st`: uploaded by the first call (from the plan's own vector, which
 * outlives the copy), waited for by a later call, which may be on another stream */
static int site_offsets_on_device(pya_plan *p, hipStream_t st) {
    pya_handle *h = p->h;
    if (!p->ev_sites) HIPCHK(h, hipEventCreateWithFlags(&p->ev_sites, hipEventDisableTiming));
    if (!p->site_off_sent) {
        HIPCHK(h, p->d_site_off.alloc(p->n_psm + 1));
        HIPCHK(h, hipMemcpyAsync(p->d_site_off.p, p->site_off.data(), (p->n_psm + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
        HIPCHK(h, hipEventRecord(p->ev_sites, st));
        p->site_off_sent = true;
    } else {
        HIPCHK(h, hipStreamWaitEvent(st, p->ev_sites, 0));
    }
    return PYA_OK;
}

int pya_plan_site_offsets(const pya_plan *plan, int64_t *site_off) {
    if (!plan || !site_off) return PYA_ERR_ARG;
    pya_plan *p = const_cast<pya_plan *>(plan);              /* (the offsets are made once and kept) */
    site_offsets(p);
    std::memcpy(site_off, p->site_off.data(), (p->n_psm + 1) * sizeof(int64_t));
    return PYA_OK;
}

/* ... the same two launches behind the same wait as the evidence stage.  It reads best_sig and n_sig of the caller's results
 * structure and nothing else of it. */
int pya_plan_sites(pya_plan *p, const pya_results *r, void *hip_stream, uint32_t sig_cap, pya_site *d_out) {
    if (!p || !r) return PYA_ERR_ARG;
    pya_handle *h = p->h;
    if (const int rc_gen = plan_settings_stale(p, "pya_plan_sites")) return rc_gen;
    if (p->n_psm == 0) return PYA_OK;
    if (!p->ran) return h->fail(PYA_ERR_STATE, -1, "pya_plan_sites: the plan has not been run");
    site_offsets(p);
    const uint64_t n_out = (uint64_t)p->site_off[p->n_psm];
    if (n_out == 0) return PYA_OK;
    if (!d_out || !r->best_score || !r->best_sig || !r->n_sig) return h->fail(PYA_ERR_ARG, -1, "NULL device pointer passed to pya_plan_sites");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const int rc = stage_behind_run(p, st, "pya_plan_sites", "site", pya_sites_lds_bytes);
    if (rc) return rc;
    const int rc_off = site_offsets_on_device(p, st);
    if (rc_off) return rc_off;
    shared_tables(h, p->dev);
    BatchDev d = p->dev;
    d.best_score = r->best_score;
    d.best_sig = r->best_sig;
    d.n_sig_out = r->n_sig;
    int e = pya_launch_sites(&d, p->gen_ids.empty() ? nullptr : p->d_evid_ids.p, p->evid_n_fast, p->d_site_off.p, n_out, sig_cap, d_out,
                             p->evid_l_cap, st);
    if (!e && !p->gen_ids.empty())
        e = pya_launch_sites(&d, p->d_gen_ids.p, (uint32_t)p->gen_ids.size(), p->d_site_off.p, n_out, sig_cap, d_out, p->gen_l_cap, st);
    if (e) return h->hip_fail((hipError_t)e, "site launch");
    HIPCHK(h, hipEventRecord(p->ev_sites, st));
    return PYA_OK;
}

/* The probability stage (csrc/probs.hip): the site stage's offsets, wait and two launches.  Each launch carves the front
 * ends its PSMs need: the count-node tables (probs_cnt.hip.h) with the caps of the PSMs that qualify for them, the general
 * front end when a PSM of the list does not -- or none does: other settings, PYA_NO_PROB_CNT.
 * The host's test of a PSM is the kernel's (probs_cnt.hip.h: pc_fits) term for term, with the spectrum's peak count standing
 * for the retained table's (a table never has more entries than its spectrum has peaks; the plan's peak_cap is NOT that
 * bound: it leaves out the spectra above PYA_FAST_PEAKS), so a list whose PSMs all pass can be launched with the tables
 * alone.  Like a score_cnt bucket the tables are held to 64 KiB: the shapes of the qualifying PSMs fix everything but the
 * staged peak table, what is left of the 64 KiB is the room for peaks, and a PSM with a larger spectrum takes the general
 * front end instead of setting the footprint of the whole launch.  PSMs that no front end will see -- set aside, more
 * modifications than sites, no site assignment -- neither qualify nor stand in the way. */
static const size_t kProbCntLds = 64u * 1024u;
static void prob_lists(pya_plan *p) {
    if (p->prob_lists_made) return;
    auto list_of = [&](uint64_t i) -> pya_plan::ProbList & { return p->prob_lists[!p->gen.empty() && p->gen[i] ? 1 : 0]; };
    auto shape_ok = [&](uint64_t i) {
        const int64_t L = p->pep_off[i + 1] - p->pep_off[i];
        const int32_t k = p->n_of_mod[i];
        return L >= 2 && L <= 64 && p->max_charge[i] == 1 && k + 1 <= 31 && p->n_sites[i] <= 32u;
    };
    auto scored = [&](uint64_t i) {
        return (p->pre_status.empty() || !p->pre_status[i]) && p->n_of_mod[i] >= 0 && (uint32_t)p->n_of_mod[i] <= p->n_sites[i] && p->n_sig[i] > 0;
    };
    for (uint64_t i = 0; i < p->n_psm; i++) {
        if (!scored(i)) continue;
        pya_plan::ProbList &l = list_of(i);
        l.n_scored++;
        if (!shape_ok(i)) continue;
        l.pos_max = std::max(l.pos_max, (uint32_t)(p->pep_off[i + 1] - p->pep_off[i] - 1));
        l.k_max = std::max(l.k_max, (uint32_t)p->n_of_mod[i]);
        l.ns_max = std::max(l.ns_max, (uint32_t)p->n_sites[i]);
    }
    for (pya_plan::ProbList &l : p->prob_lists) {
        PcCaps c = {0u, l.pos_max, 8u, l.k_max, l.ns_max};
        while (c.kc < c.k_cap + 1u) c.kc <<= 1;
        l.kc = c.kc;
        const size_t fixed = pya_probs_cnt_bytes(&c) + 64u * 16u;            /* (with the slice's 64 pairs) */
        l.peak_room = fixed < kProbCntLds ? (uint32_t)((kProbCntLds - fixed) / sizeof(PeakEntry)) & ~31u : 0u;
    }
    for (uint64_t i = 0; i < p->n_psm; i++) {
        if (!scored(i) || !shape_ok(i)) continue;
        pya_plan::ProbList &l = list_of(i);
        const uint64_t P = ((uint64_t)p->n_peaks(i) + 31u) & ~(uint64_t)31u;
        if (P > l.peak_room) continue;
        l.n_fit++;
        l.peak_max = std::max(l.peak_max, (uint32_t)P);
    }
    p->prob_lists_made = true;
}

/* ... and what the two launches of a stage that scores with these front ends carve (slice_score.hip.h: PB_CNT 1, PB_GEN 2):
 * caps[li], sw[li] for the PSMs inside the fast limits (0) and the general list (1) */
static void prob_front_ends(pya_plan *p, PcCaps caps[2], uint32_t sw[2]) {
    pya_handle *h = p->h;
    prob_lists(p);
    const DevConfig &c = h->cfg;
    const bool plain = c.n_nl == 0 && c.n_types == 2 && c.n_fwd == 1 && c.n_top == PYA_NTOP && h->mz_error <= 0.49f && !h->kn.no_prob_cnt;
    for (int li = 0; li < 2; li++) {
        const pya_plan::ProbList &l = p->prob_lists[li];
        caps[li] = PcCaps{};
        sw[li] = 2u;
        if (!plain || l.n_fit == 0) continue;
        const PcCaps k = {l.peak_max, l.pos_max, l.kc, l.k_max, l.ns_max};
        caps[li] = k;
        /* the tables alone only for the list of the PSMs inside the fast limits, and only when every PSM of it that will be
         * scored passed the kernel's own test on the host: whatever else is in a list needs the general front end */
        sw[li] = li == 0 && l.n_fit == l.n_scored ? 1u : 3u;
    }
}

int pya_plan_probs(pya_plan *p, const pya_results *r, void *hip_stream, uint32_t sig_cap, pya_site_prob *d_sites, pya_psm_prob *d_psms) {
    if (!p || !r) return PYA_ERR_ARG;
    pya_handle *h = p->h;
    if (const int rc_gen = plan_settings_stale(p, "pya_plan_probs")) return rc_gen;
    if (p->n_psm == 0) return PYA_OK;
    if (!p->ran) return h->fail(PYA_ERR_STATE, -1, "pya_plan_probs: the plan has not been run");
    site_offsets(p);
    const uint64_t n_out = (uint64_t)p->site_off[p->n_psm];
    if (!d_psms || (n_out && !d_sites) || !r->best_score || !r->best_sig || !r->n_sig)
        return h->fail(PYA_ERR_ARG, -1, "NULL device pointer passed to pya_plan_probs");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)hip_stream;
    if (!p->ev_sites) HIPCHK(h, hipEventCreateWithFlags(&p->ev_sites, hipEventDisableTiming));
    PcCaps caps[2] = {};
    uint32_t sw[2] = {2u, 2u};
    prob_front_ends(p, caps, sw);
    /* (stage_behind_run sizes the general front end's LDS: l_cap alone counts, the stage keeps no fragment list) */
    struct Room {
        static size_t general(uint32_t l_cap, uint32_t) {
            const PcCaps none = {};
            return pya_probs_lds_bytes(l_cap, &none, 2u);
        }
    };
    const int rc = stage_behind_run(p, st, "pya_plan_probs", "probability", Room::general);
    if (rc) return rc;
    if (pya_probs_lds_bytes(p->evid_l_cap, &caps[0], sw[0]) > kMaxLds) sw[0] = 2u;
    if (pya_probs_lds_bytes(p->gen_l_cap, &caps[1], sw[1]) > kMaxLds) sw[1] = 2u;
    const int rc_off = site_offsets_on_device(p, st);
    if (rc_off) return rc_off;
    shared_tables(h, p->dev);
    BatchDev d = p->dev;
    d.best_score = r->best_score;
    d.best_sig = r->best_sig;
    d.n_sig_out = r->n_sig;
    int e = pya_launch_probs(&d, p->gen_ids.empty() ? nullptr : p->d_evid_ids.p, p->evid_n_fast, p->d_site_off.p, n_out, sig_cap, d_sites, d_psms,
                             p->evid_l_cap, &caps[0], sw[0], st);
    if (!e && !p->gen_ids.empty())
        e = pya_launch_probs(&d, p->d_gen_ids.p, (uint32_t)p->gen_ids.size(), p->d_site_off.p, n_out, sig_cap, d_sites, d_psms, p->gen_l_cap,
                             &caps[1], sw[1], st);
    if (e) return h->hip_fail((hipError_t)e, "probability launch");
    for (int li = 0; li < 2; li++) {                            /* (pya_debug_last_probs_launch) */
        const bool launched = li == 0 ? p->evid_n_fast != 0 : !p->gen_ids.empty();
        h->last_probs_sw[li] = launched ? sw[li] : 0u;
        h->last_probs_lds[li] = launched ? pya_probs_lds_bytes(li == 0 ? p->evid_l_cap : p->gen_l_cap, &caps[li], sw[li]) : 0u;
    }
    return PYA_OK;
}

/* The ranked stage (csrc/ranked.hip): the probability stage's front ends, offsets (a PSM's modifiable residues are the
 * difference of two), wait and two launches; the list it keeps lives in registers, so its LDS is the front ends' alone. */
int pya_plan_ranked(pya_plan *p, const pya_results *r, void *hip_stream, uint32_t top_k, uint32_t sig_cap, pya_ranked *d_out) {
    if (!p || !r) return PYA_ERR_ARG;
    pya_handle *h = p->h;
    if (const int rc_gen = plan_settings_stale(p, "pya_plan_ranked")) return rc_gen;
    if (top_k < 1u || top_k > PYA_MAX_RANKED)
        return h->fail(PYA_ERR_ARG, -1, "pya_plan_ranked: top_k %u is not in 1 .. %d", top_k, PYA_MAX_RANKED);
    if (p->n_psm == 0) return PYA_OK;
    if (!p->ran) return h->fail(PYA_ERR_STATE, -1, "pya_plan_ranked: the plan has not been run");
    if (!d_out || !r->best_score || !r->best_sig || !r->n_sig) return h->fail(PYA_ERR_ARG, -1, "NULL device pointer passed to pya_plan_ranked");
    site_offsets(p);
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)hip_stream;
    if (!p->ev_sites) HIPCHK(h, hipEventCreateWithFlags(&p->ev_sites, hipEventDisableTiming));
    PcCaps caps[2] = {};
    uint32_t sw[2] = {2u, 2u};
    prob_front_ends(p, caps, sw);
    struct Room {
        static size_t general(uint32_t l_cap, uint32_t) {
            const PcCaps none = {};
            return pya_ranked_lds_bytes(l_cap, &none, 2u);
        }
    };
    const int rc = stage_behind_run(p, st, "pya_plan_ranked", "ranked", Room::general);
    if (rc) return rc;
    if (pya_ranked_lds_bytes(p->evid_l_cap, &caps[0], sw[0]) > kMaxLds) sw[0] = 2u;
    if (pya_ranked_lds_bytes(p->gen_l_cap, &caps[1], sw[1]) > kMaxLds) sw[1] = 2u;
    const int rc_off = site_offsets_on_device(p, st);
    if (rc_off) return rc_off;
    shared_tables(h, p->dev);
    BatchDev d = p->dev;
    d.best_score = r->best_score;
    d.best_sig = r->best_sig;
    d.n_sig_out = r->n_sig;
    int e = pya_launch_ranked(&d, p->gen_ids.empty() ? nullptr : p->d_evid_ids.p, p->evid_n_fast, p->d_site_off.p, top_k, sig_cap, d_out,
                              p->evid_l_cap, &caps[0], sw[0], st);
    if (!e && !p->gen_ids.empty())
        e = pya_launch_ranked(&d, p->d_gen_ids.p, (uint32_t)p->gen_ids.size(), p->d_site_off.p, top_k, sig_cap, d_out, p->gen_l_cap, &caps[1],
                              sw[1], st);
    if (e) return h->hip_fail((hipError_t)e, "ranked launch");
    for (int li = 0; li < 2; li++) {                            /* (pya_debug_last_ranked_launch) */
        const bool launched = li == 0 ? p->evid_n_fast != 0 : !p->gen_ids.empty();
        h->last_ranked_sw[li] = launched ? sw[li] : 0u;
        h->last_ranked_lds[li] = launched ? pya_ranked_lds_bytes(li == 0 ? p->evid_l_cap : p->gen_l_cap, &caps[li], sw[li]) : 0u;
    }
    return PYA_OK;
}

/* The roll-up stage (csrc/rollup.hip): no kernel of it reads a retained table, a fragment list or LDS, so it takes nothing of
 * stage_behind_run but the wait for the run; the offsets are the site stage's.  Two launches, one thread per residue record,
 * into the caller's table; the report of slots outside the table goes the way of pya_plan_named's. */
int pya_plan_rollup(pya_plan *p, const pya_results *r, void *hip_stream, const pya_site_prob *d_site_probs, const pya_psm_prob *d_psm_probs,
                    const int32_t *d_slot, uint64_t n_slots, double threshold, const uint32_t *d_psm_id, uint32_t psm_base,
                    pya_site_rollup *d_table) {
    if (!p || !r) return PYA_ERR_ARG;
    pya_handle *h = p->h;
    if (const int rc_gen = plan_settings_stale(p, "pya_plan_rollup")) return rc_gen;
    if (n_slots > 0x7fffffffull) return h->fail(PYA_ERR_ARG, -1, "pya_plan_rollup: %llu slots are more than an int32 slot can name", (unsigned long long)n_slots);
    if (p->n_psm == 0) return PYA_OK;
    if (!p->ran) return h->fail(PYA_ERR_STATE, -1, "pya_plan_rollup: the plan has not been run");
    site_offsets(p);
    const uint64_t n_rec = (uint64_t)p->site_off[p->n_psm];
    if (!d_psm_probs || (n_rec && (!d_site_probs || !d_slot)) || (n_slots && !d_table) || !r->best_sig || !r->ascores)
        return h->fail(PYA_ERR_ARG, -1, "NULL device pointer passed to pya_plan_rollup");
    if (r->max_k < p->max_k)
        return h->fail(PYA_ERR_ARG, -1, "results.max_k (%u) is smaller than the largest n_of_mod (%u)", r->max_k, p->max_k);
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)hip_stream;
    OverReport &over = p->over[OVER_ROLLUP];
    int rc;
    if ((rc = wait_for_run(p, st)) || (rc = site_offsets_on_device(p, st)) || (rc = over.begin(h, st))) return rc;
    const int e = pya_launch_rollup(p->d_site_off.p, p->n_psm, n_rec, d_site_probs, d_psm_probs, d_slot, n_slots, threshold, d_psm_id, psm_base,
                                    r->best_sig, r->ascores, r->max_k, d_table, over.d_over.p, h->last_rollup_grid, st);
    if (e) return h->hip_fail((hipError_t)e, "roll-up launch");
    h->last_rollup_records = n_rec;
    return over.end(h, st);
}

/* The site quantification (csrc/site_quant.hip): the roll-up's wait for the run and its offsets, one launch into the caller's
 * table; the argument checks are host_site_quant.cpp's, the report of slots and rows outside goes the way of pya_plan_rollup's. */
int pya_plan_site_quant(pya_plan *p, const pya_results *r, void *hip_stream, const pya_site_prob *d_site_probs, const pya_psm_prob *d_psm_probs,
                        const int32_t *d_slot, uint64_t n_slots, const double *d_values, uint64_t n_rows, const int32_t *d_row, uint32_t row_base,
                        const pya_site_quant_params *prm, pya_site_quant_head *d_head, pya_site_quant *d_cell) {
    if (!p || !r) return PYA_ERR_ARG;
    pya_handle *h = p->h;
    if (const int rc_gen = plan_settings_stale(p, "pya_plan_site_quant")) return rc_gen;
    const int rc_arg = quant_check(h, "pya_plan_site_quant", n_slots, n_rows, prm);
    if (rc_arg) return rc_arg;
    if (p->n_psm == 0) return PYA_OK;
    if (!p->ran) return h->fail(PYA_ERR_STATE, -1, "pya_plan_site_quant: the plan has not been run");
    site_offsets(p);
    const uint64_t n_rec = (uint64_t)p->site_off[p->n_psm];
    if (!d_psm_probs || (n_rec && (!d_site_probs || !d_slot)) || (n_slots && (!d_head || !d_cell)) || (n_rows && !d_values) || !r->best_sig)
        return h->fail(PYA_ERR_ARG, -1, "NULL device pointer passed to pya_plan_site_quant");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)hip_stream;
    OverReport &over = p->over[OVER_QUANT];
    int rc;
    if ((rc = wait_for_run(p, st)) || (rc = site_offsets_on_device(p, st)) || (rc = over.begin(h, st))) return rc;
    const int e = pya_launch_site_quant(p->d_site_off.p, p->n_psm, n_rec, d_site_probs, d_psm_probs, d_slot, n_slots, d_values, n_rows, d_row,
                                        row_base, prm, std::ldexp(1.0, prm->scale_log2), r->best_sig, d_head, d_cell, over.d_over.p, st);
    if (e) return h->hip_fail((hipError_t)e, "site quantification launch");
    return over.end(h, st);
}

/* The peptidoform stage (csrc/peptidoforms.hip): like the roll-up it takes nothing of stage_behind_run but the wait for the
 * run, and the offsets are the site stage's.  The argument checks and the launches are host_peptidoforms.cpp's. */
int pya_plan_peptidoforms(pya_plan *p, const pya_results *r, void *hip_stream, const pya_site_prob *d_site_probs, const pya_psm_prob *d_psm_probs,
                          const int32_t *d_group, double threshold, const uint32_t *d_psm_id, uint32_t psm_base, const pya_peptidoform *d_prev,
                          uint64_t n_prev, void *d_work, uint64_t work_bytes, pya_peptidoform *d_out, uint64_t cap, uint32_t *d_n) {
    if (!p || !r) return PYA_ERR_ARG;
    pya_handle *h = p->h;
    if (const int rc_gen = plan_settings_stale(p, "pya_plan_peptidoforms")) return rc_gen;
    bool run;
    const int rc = pform_check(h, "pya_plan_peptidoforms", p->n_psm, d_prev, n_prev, d_work, work_bytes, d_out, cap, d_n, &run);
    if (rc) return rc;
    uint64_t n_rec = 0;
    if (p->n_psm) {
        if (!p->ran) return h->fail(PYA_ERR_STATE, -1, "pya_plan_peptidoforms: the plan has not been run");
        site_offsets(p);
        n_rec = (uint64_t)p->site_off[p->n_psm];
        if (!d_psm_probs || !d_group || (n_rec && !d_site_probs) || !r->best_sig || !r->ascores)
            return h->fail(PYA_ERR_ARG, -1, "NULL device pointer passed to pya_plan_peptidoforms");
        if (r->max_k < p->max_k)
            return h->fail(PYA_ERR_ARG, -1, "results.max_k (%u) is smaller than the largest n_of_mod (%u)", r->max_k, p->max_k);
    }
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)hip_stream;
    if (p->n_psm) {
        int rc_run;
        if ((rc_run = wait_for_run(p, st)) || (rc_run = site_offsets_on_device(p, st))) return rc_run;
    }
    return pform_run(h, p->n_psm ? p->d_site_off.p : nullptr, p->n_psm, d_site_probs, d_psm_probs, d_group, threshold, d_psm_id, psm_base,
                     r->best_sig, r->ascores, r->max_k, d_prev, n_prev, nullptr, 0, d_work, d_out, cap, d_n, run, st);
}

/* The peptidoform quantification (csrc/pform_quant.hip): pya_plan_peptidoforms' checks, wait and offsets, the list by the same
 * launches, the table behind them; the report of rows outside the matrix goes the way of pya_plan_site_quant's. */
int pya_plan_peptidoform_quant(pya_plan *p, const pya_results *r, void *hip_stream, const pya_site_prob *d_site_probs, const pya_psm_prob *d_psm_probs,
                               const int32_t *d_group, double threshold, const uint32_t *d_psm_id, uint32_t psm_base, const pya_peptidoform *d_prev,
                               const pya_site_quant_head *d_prev_head, const pya_site_quant *d_prev_cell, uint64_t n_prev, const double *d_values,
                               uint64_t n_rows, const int32_t *d_row, uint32_t row_base, const pya_site_quant_params *prm, void *d_work,
                               uint64_t work_bytes, pya_peptidoform *d_out, pya_site_quant_head *d_head, pya_site_quant *d_cell, uint64_t cap,
                               uint32_t *d_n) {
    if (!p || !r) return PYA_ERR_ARG;
    pya_handle *h = p->h;
    if (const int rc_gen = plan_settings_stale(p, "pya_plan_peptidoform_quant")) return rc_gen;
    const char *who = "pya_plan_peptidoform_quant";
    int rc = quant_check(h, who, 0, n_rows, prm);
    if (rc) return rc;
    bool run;
    if ((rc = pform_check(h, who, p->n_psm, d_prev, n_prev, d_work, work_bytes, d_out, cap, d_n, &run))) return rc;
    if ((rc = pfq_check(h, who, d_prev_head, d_prev_cell, nullptr, nullptr, d_head, d_cell, cap))) return rc;
    uint64_t n_rec = 0;
    if (p->n_psm) {
        if (!p->ran) return h->fail(PYA_ERR_STATE, -1, "%s: the plan has not been run", who);
        site_offsets(p);
        n_rec = (uint64_t)p->site_off[p->n_psm];
        if (!d_psm_probs || !d_group || (n_rec && !d_site_probs) || !r->best_sig || !r->ascores || (n_rows && !d_values))
            return h->fail(PYA_ERR_ARG, -1, "NULL device pointer passed to %s", who);
        if (r->max_k < p->max_k)
            return h->fail(PYA_ERR_ARG, -1, "results.max_k (%u) is smaller than the largest n_of_mod (%u)", r->max_k, p->max_k);
    }
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)hip_stream;
    OverReport &over = p->over[OVER_PFQ];                       /* (of the PSMs: a call without them reports nothing) */
    if (p->n_psm && ((rc = wait_for_run(p, st)) || (rc = site_offsets_on_device(p, st)) || (rc = over.begin(h, st)))) return rc;
    rc = pfq_run(h, p->n_psm ? p->d_site_off.p : nullptr, p->n_psm, d_site_probs, d_psm_probs, d_group, threshold, d_psm_id, psm_base, r->best_sig,
                 r->ascores, r->max_k, d_prev, d_prev_head, d_prev_cell, n_prev, nullptr, nullptr, nullptr, 0, d_values, n_rows, d_row, row_base, prm,
                 d_work, d_out, d_head, d_cell, cap, d_n, p->n_psm ? over.d_over.p : nullptr, run, st);
    if (rc || !p->n_psm) return rc;
    return over.end(h, st);
}

/* The mass-error profile (csrc/mz_profile.hip): the wait and the two lists of the evidence stage, with the longest peptide of
 * either list as the only cap -- the kernel keeps no fragment list.  The argument checks are host_mz_profile.cpp's; the report
 * of slots outside the table goes the way of pya_plan_rollup's. */
int pya_plan_mz_profile(pya_plan *p, const pya_results *r, void *hip_stream, const int32_t *d_run, uint64_t n_slots,
                        const pya_mz_profile_params *prm, pya_mz_profile *d_table) {
    if (!p || !r) return PYA_ERR_ARG;
    pya_handle *h = p->h;
    if (const int rc_gen = plan_settings_stale(p, "pya_plan_mz_profile")) return rc_gen;
    const int rc_arg = mzp_check(h, "pya_plan_mz_profile", n_slots, prm);
    if (rc_arg) return rc_arg;
    if (p->n_psm == 0) return PYA_OK;
    if (!p->ran) return h->fail(PYA_ERR_STATE, -1, "pya_plan_mz_profile: the plan has not been run");
    if ((n_slots && !d_table) || !r->best_sig || !r->n_sig) return h->fail(PYA_ERR_ARG, -1, "NULL device pointer passed to pya_plan_mz_profile");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)hip_stream;
    OverReport &over = p->over[OVER_MZP];
    /* (the LDS condition of pya_plan_evidence, and this kernel's own room, which only a peptide length could exceed) */
    struct Room {
        static size_t both(uint32_t l_cap, uint32_t list_cap) {
            return std::max(pya_evidence_lds_bytes(l_cap, list_cap), pya_mz_profile_lds_bytes(l_cap));
        }
    };
    int rc = stage_behind_run(p, st, "pya_plan_mz_profile", "evidence", Room::both);
    if (rc || (rc = over.begin(h, st))) return rc;
    shared_tables(h, p->dev);
    BatchDev d = p->dev;
    d.best_sig = r->best_sig;
    d.n_sig_out = r->n_sig;
    int e = pya_launch_mz_profile(&d, p->gen_ids.empty() ? nullptr : p->d_evid_ids.p, p->evid_n_fast, d_run, n_slots, prm, d_table,
                                  over.d_over.p, p->evid_l_cap, st);
    if (!e && !p->gen_ids.empty())
        e = pya_launch_mz_profile(&d, p->d_gen_ids.p, (uint32_t)p->gen_ids.size(), d_run, n_slots, prm, d_table, over.d_over.p, p->gen_l_cap, st);
    if (e) return h->hip_fail((hipError_t)e, "mass-error profile launch");
    return over.end(h, st);
}

namespace {
/* the raw peak caps of pya_plan_coverage's two launches, for the Room of its stage_behind_run (which hands over l_cap and
 * list_cap only; the larger of the two caps stands for both lists there, the launches take their own) */
thread_local uint32_t cov_room_peaks = 1;
}  // namespace

/* The coverage stage (csrc/coverage.hip): the wait and the two lists of the evidence stage, each launch with the longest
 * peptide and the largest spectrum of ITS list as caps -- the kernel keeps two bit planes over the retained table, and
 * retained <= raw.  The raw arrays are the caller's: what the run scored. */
int pya_plan_coverage(pya_plan *p, const pya_results *r, const pya_typed_spectra *sp, void *hip_stream, pya_coverage *d_out) {
    if (!p || !r) return PYA_ERR_ARG;
    pya_handle *h = p->h;
    if (const int rc_gen = plan_settings_stale(p, "pya_plan_coverage")) return rc_gen;
    if (p->n_psm == 0) return PYA_OK;
    if (!p->ran) return h->fail(PYA_ERR_STATE, -1, "pya_plan_coverage: the plan has not been run");
    if (!d_out || !sp || !sp->mz || !sp->intensity || !r->best_sig || !r->n_sig)
        return h->fail(PYA_ERR_ARG, -1, "NULL device pointer passed to pya_plan_coverage");
    uint32_t types = 0;
    const int rc_types = spectra_types(h, sp, "pya_plan_coverage", &types);
    if (rc_types) return rc_types;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)hip_stream;
    if (!p->ev_cov) HIPCHK(h, hipEventCreateWithFlags(&p->ev_cov, hipEventDisableTiming));
    if (!p->cov_caps) {
        uint32_t fast = 1, gen = 1;
        for (uint64_t i = 0; i < p->n_psm; i++) {
            if (!p->pre_status.empty() && p->pre_status[i]) continue;       /* (set aside: nothing of it is read) */
            const int64_t np = p->n_peaks(i);
            uint32_t &cap = (!p->gen.empty() && p->gen[i]) ? gen : fast;
            cap = std::max(cap, (uint32_t)std::min<int64_t>(std::max<int64_t>(np, 1), 0xffffffffll));
        }
        p->cov_peak_fast = fast;
        p->cov_peak_gen = gen;
        p->cov_caps = true;
    }
    /* (the LDS condition of pya_plan_evidence, and this kernel's own room) */
    struct Room {
        static size_t both(uint32_t l_cap, uint32_t list_cap) {
            return std::max(pya_evidence_lds_bytes(l_cap, list_cap), pya_coverage_lds_bytes(l_cap, cov_room_peaks));
        }
    };
    cov_room_peaks = std::max(p->cov_peak_fast, p->gen_ids.empty() ? 1u : p->cov_peak_gen);
    const int rc = stage_behind_run(p, st, "pya_plan_coverage", "evidence", Room::both);
    if (rc) return rc;
    /* (behind an earlier call's kernels, on whatever stream they were: they may write the same records) */
    if (p->cov_asked) HIPCHK(h, hipStreamWaitEvent(st, p->ev_cov, 0));
    shared_tables(h, p->dev);
    BatchDev d = p->dev;
    d.best_sig = r->best_sig;
    d.n_sig_out = r->n_sig;
    d.mz = sp->mz;
    d.inten = sp->intensity;
    const uint32_t *d_spec_of = p->shared ? p->d_spec_of.p : nullptr;
    int e = pya_launch_coverage(&d, p->gen_ids.empty() ? nullptr : p->d_evid_ids.p, p->evid_n_fast, d_spec_of, types, d_out, p->evid_l_cap,
                                p->cov_peak_fast, st);
    if (!e && !p->gen_ids.empty())
        e = pya_launch_coverage(&d, p->d_gen_ids.p, (uint32_t)p->gen_ids.size(), d_spec_of, types, d_out, p->gen_l_cap, p->cov_peak_gen, st);
    if (e) return h->hip_fail((hipError_t)e, "coverage launch");
    HIPCHK(h, hipEventRecord(p->ev_cov, st));
    p->cov_asked = true;
    return PYA_OK;
}

namespace {
/* the results of the caller's structure in place of the run's (pya_plan_evidence does the same) */
BatchDev ions_view(pya_plan *p, const pya_results *r) {
    BatchDev d = p->dev;
    d.best_score = r->best_score;
    d.best_sig = r->best_sig;
    d.n_sig_out = r->n_sig;
    d.ascores = r->ascores;
    d.alt_mask = r->alt_mask;
    d.max_k = r->max_k;
    return d;
}

/* the two launches of pya_plan_evidence, with their caps (d_out NULL: the count pass) */
int ions_launches(pya_plan *p, const BatchDev &d, int64_t *d_off, pya_ion *d_out, uint64_t cap, hipStream_t st) {
    int e = pya_launch_ions(&d, p->gen_ids.empty() ? nullptr : p->d_evid_ids.p, p->evid_n_fast, p->d_ions_evid.p, d_off, d_out, cap,
                            p->d_ions_over.p, p->evid_l_cap, p->evid_list_cap, st);
    if (!e && !p->gen_ids.empty())
        e = pya_launch_ions(&d, p->d_gen_ids.p, (uint32_t)p->gen_ids.size(), p->d_ions_evid.p, d_off, d_out, cap, p->d_ions_over.p,
                            p->gen_l_cap, p->gen_list_cap, st);
    return e;
}
}  // namespace

/* The ion stage, first half: the evidence rows of the results into the plan's own block (competitor and depth of every
 * counted column; pya_plan_evidence waits for the run and sets the caps of the two launches), the count pass on the same
 * two launches, the scan.  Nothing waits on the host. */
int pya_plan_ions_count(pya_plan *p, const pya_results *r, void *hip_stream, int64_t *d_ion_off) {
    if (!p || !r) return PYA_ERR_ARG;
    pya_handle *h = p->h;
    if (const int rc_gen = plan_settings_stale(p, "pya_plan_ions_count")) return rc_gen;
    if (!d_ion_off) return h->fail(PYA_ERR_ARG, -1, "NULL device pointer passed to pya_plan_ions_count");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)hip_stream;
    if (p->n_psm == 0) {
        HIPCHK(h, hipMemsetAsync(d_ion_off, 0, sizeof(int64_t), st));
        return PYA_OK;
    }
    if (!p->ran) return h->fail(PYA_ERR_STATE, -1, "pya_plan_ions_count: the plan has not been run");
    const size_t n_rows = (size_t)p->n_psm * r->max_k;
    if (p->d_ions_evid.n < std::max<size_t>(n_rows, 1)) HIPCHK(h, p->d_ions_evid.alloc(std::max<size_t>(n_rows, 1)));
    const uint32_t tiles = pya_ions_scan_tiles((uint32_t)p->n_psm);
    if (p->d_ions_tiles.n < tiles) HIPCHK(h, p->d_ions_tiles.alloc(tiles));
    if (!p->d_ions_over.p) HIPCHK(h, p->d_ions_over.alloc(2));
    if (!p->ev_ions) HIPCHK(h, hipEventCreateWithFlags(&p->ev_ions, hipEventDisableTiming));
    p->ions_state = 0;
    const int rc = pya_plan_evidence(p, r, hip_stream, p->d_ions_evid.p);
    if (rc) return rc;
    if (pya_ions_lds_bytes(p->evid_l_cap, p->evid_list_cap) > kMaxLds ||
        (!p->gen_ids.empty() && pya_ions_lds_bytes(p->gen_l_cap, p->gen_list_cap) > kMaxLds))
        return h->fail(PYA_ERR_LIMIT, -1, "pya_plan_ions_count: %u fragments per ion type exceed the ion kernel's room",
                       std::max(p->evid_list_cap, p->gen_ids.empty() ? 0u : p->gen_list_cap));
    const BatchDev d = ions_view(p, r);
    int e = ions_launches(p, d, d_ion_off, nullptr, 0, st);
    if (!e) e = pya_launch_ions_scan(d_ion_off, (uint32_t)p->n_psm, p->d_ions_tiles.p, st);
    if (e) return h->hip_fail((hipError_t)e, "ion count launch");
    HIPCHK(h, hipEventRecord(p->ev_ions, st));
    p->ions_max_k = r->max_k;
    p->ions_state = 1;
    return PYA_OK;
}

/* ... second half: the fill pass behind the count (whatever stream that was on) */
int pya_plan_ions(pya_plan *p, const pya_results *r, void *hip_stream, const int64_t *d_ion_off, pya_ion *d_out, uint64_t cap) {
    if (!p || !r) return PYA_ERR_ARG;
    pya_handle *h = p->h;
    if (const int rc_gen = plan_settings_stale(p, "pya_plan_ions")) return rc_gen;
    if (p->n_psm == 0) return PYA_OK;
    if (!p->ran) return h->fail(PYA_ERR_STATE, -1, "pya_plan_ions: the plan has not been run");
    if (p->ions_state == 0) return h->fail(PYA_ERR_STATE, -1, "pya_plan_ions: pya_plan_ions_count has not been called for this run");
    if (!d_ion_off || !d_out || !r->best_score || !r->best_sig || !r->n_sig || !r->ascores || !r->alt_mask)
        return h->fail(PYA_ERR_ARG, -1, "NULL device pointer passed to pya_plan_ions");
    if (r->max_k != p->ions_max_k)
        return h->fail(PYA_ERR_ARG, -1, "results.max_k (%u) is not the one pya_plan_ions_count was given (%u)", r->max_k, p->ions_max_k);
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)hip_stream;
    HIPCHK(h, hipStreamWaitEvent(st, p->ev_ions, 0));
    HIPCHK(h, hipMemsetAsync(p->d_ions_over.p, 0, 2 * sizeof(uint32_t), st));
    const BatchDev d = ions_view(p, r);
    const int e = ions_launches(p, d, const_cast<int64_t *>(d_ion_off), d_out, cap, st);
    if (e) return h->hip_fail((hipError_t)e, "ion fill launch");
    HIPCHK(h, hipEventRecord(p->ev_ions, st));
    p->ions_state = 2;
    return PYA_OK;
}

int pya_pack_records(pya_handle *h, const pya_results *d_res, uint64_t n_psm, uint32_t k, int32_t *d_out, void *hip_stream) {
    if (!h) return PYA_ERR_ARG;
    if (!d_res || !d_out || !d_res->best_score || !d_res->best_sig || !d_res->n_sig || !d_res->ascores || !d_res->alt_mask)
        return h->fail(PYA_ERR_ARG, -1, "pya_pack_records: null result array");
    if (k < d_res->max_k || k > 64 || d_res->max_k == 0)
        return h->fail(PYA_ERR_ARG, -1, "pya_pack_records: record width k = %u is narrower than the results' rows (%u) or above 64", k,
                       d_res->max_k);
    HIPCHK(h, hipSetDevice(h->device));
    const int e = pya_launch_pack_records(d_res->best_score, d_res->n_sig, d_res->best_sig, d_res->ascores, d_res->alt_mask, k,
                                          d_res->max_k, n_psm, d_out, (hipStream_t)hip_stream);
    if (e) return h->fail(PYA_ERR_HIP, -1, "pya_pack_records: launch failed (%d)", e);
    return PYA_OK;
}
