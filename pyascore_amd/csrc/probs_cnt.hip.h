/* probs_cnt.hip.h -- the count-node front end of a stage that needs the PepScore of EVERY site assignment of a PSM behind
 * a run (probs.hip and ranked.hip today, through slice_score.hip.h; sites.hip may adopt it): under the plain settings of score_cnt.hip (no neutral loss, fragment
 * charge 1, one ion type per direction, both directions, mz_error <= 0.49, n_top = PYA_NTOP) the tables of walk_core.hip.h
 * are built ONCE per PSM in LDS from the retained table the run left, and a site assignment then costs k reads of the
 * (t, site) table and the ten score reads instead of a binary search per fragment.
 *   pc_setup   staged peak table and grid, envelopes (cnt_envelopes), one lookup per node (cnt_table_entry), the prefix sums
 *              at the sites' steps and the (t, site) table in score_cnt.hip's compact layout -- cnt_prefix_sums keeps all L
 *              columns of a row, twice the bytes of the envelopes it would have to replace, and the stage is bound to the
 *              LDS score_cnt.hip has for the same caps -- the marked nodes in the high half of the third word.
 *   pc_score   the lane's site assignment: cnt_eval_sites, a walk with its own sums when its path crosses a marked node
 *              (walk_cnt_both), the depth scores and the weighted sum of Ascore.cpp:123-139.
 * The PepScore has the bits score_cnt.hip writes to the run's ws array, which are the bits of every other route.
 * One wavefront per PSM; nothing is written to global memory. */
#ifndef PYA_PROBS_CNT_H
#define PYA_PROBS_CNT_H
#include "score_core.hip.h"

/* (PcCaps, the caps of a launch: common.h) */
struct PcLds {
    uint16_t *grid;
    float2 *resd;
    PeakEntry *t_e;
    uint4 *cum_lut;
    uint8_t *T;          /* [2][pos_cap][kc] */
    uint8_t *site_pos;   /* [64] */
    float2 *env;         /* [2][k_cap + 1][pos_cap]          } the same bytes: the envelopes are dead */
    uint4 *psite;        /* [2][k_cap + 1][n_cap + 1]        } when the prefix sums are written      */
    uint4 *G;            /* [k_cap * n_cap + 1] */
};
/* (term for term the bytes of score_cnt.hip: score_cnt_lds_bytes) */
__host__ __device__ static inline size_t pc_lds_bytes(const PcCaps &c) {
    const size_t env = (size_t)2 * (c.k_cap + 1) * c.pos_cap * sizeof(float2);
    const size_t tabs = ((size_t)2 * (c.k_cap + 1) * (c.n_cap + 1) + (size_t)c.k_cap * c.n_cap + 1) * sizeof(uint4);
    return PYA_GRID_CELLS * 2 + ((((size_t)c.pos_cap + 1) * 8 + 15) & ~(size_t)15) + ((size_t)c.cap + PYA_TABLE_PAD) * 8 + 16 * sizeof(uint4) +
           (((size_t)2 * c.pos_cap * c.kc + 15) & ~(size_t)15) + 64 + (env > tabs ? env : tabs) + 16;
}
DEV PcLds pc_carve(unsigned char *raw, const PcCaps &c) {
    PcLds l;
    l.grid = (uint16_t *)raw;
    size_t o = PYA_GRID_CELLS * 2;
    l.resd = (float2 *)(raw + o);
    o += (((size_t)c.pos_cap + 1) * 8 + 15) & ~(size_t)15;
    l.t_e = (PeakEntry *)(raw + o);
    o += ((size_t)c.cap + PYA_TABLE_PAD) * 8;
    l.cum_lut = (uint4 *)(raw + o);
    o += 16 * sizeof(uint4);
    l.T = raw + o;
    o += ((size_t)2 * c.pos_cap * c.kc + 15) & ~(size_t)15;
    l.site_pos = raw + o;
    o += 64;
    l.env = (float2 *)(raw + o);
    l.psite = (uint4 *)(raw + o);
    l.G = l.psite + (size_t)2 * (c.k_cap + 1) * (c.n_cap + 1);
    return l;
}

/* what pc_setup leaves for pc_score (wave-uniform but for the residue registers) */
struct PcPsm {
    PcLds l;
    PeakTable tab;
    WalkEnv env;
    Residues res;
    PcCaps caps;
    int L, k, n_sites;
};

/* do the scorer's settings and this PSM's shape fit the count-node tables of a launch with `caps`? (wave-uniform) */
DEV bool pc_fits(const DevConfig *cfg, const PcCaps &c, int L, int k, int n_sites, int zmax, int R) {
    return cfg->n_nl == 0 && cfg->n_types == 2 && cfg->n_fwd == 1 && cfg->n_top == PYA_NTOP && !(cfg->mz_error > 0.49f) && zmax == 1 &&
           L >= 2 && L <= 64 && k >= 0 && k + 1 <= 31 && n_sites <= 32 && (uint32_t)k <= c.k_cap && (uint32_t)k + 1u <= c.kc &&
           (uint32_t)n_sites <= c.n_cap && (uint32_t)(L - 1) <= c.pos_cap && R >= 0 && (uint32_t)R <= c.cap;
}

/* P(d, j, e) at the steps the sites enter at, and the row totals (score_cnt.hip: site_prefix_sums, one row at a time) */
DEV void pc_prefix_sums(const PcLds &c, const PcCaps &caps, int L, int k, int n_sites) {
    const int lane = lane_id();
    const int Lm1 = L - 1;
    const int pos = lane < n_sites ? (int)c.site_pos[lane] : 0;
    for (int row = 0; row < 2 * (k + 1); row++) {
        const int d = row / (k + 1), j = row - d * (k + 1);
        uint32_t x = 0, y = 0, z = 0;
        if (lane < Lm1) {
            const uint32_t ent = c.T[((size_t)d * caps.pos_cap + lane) * caps.kc + j];
            const uint4 inc = c.cum_lut[ent & 15u];
            x = inc.x;
            y = inc.y;
            z = inc.z | ((ent >> 7) << 16);
        }
        x = wave_incl_scan_u32<false>(x);
        y = wave_incl_scan_u32<false>(y);
        z = wave_incl_scan_u32<false>(z);
        /* lane i: the sum over the steps below e = min(step of site i, L - 1) = the inclusive value of step e - 1 */
        const int st = d ? Lm1 - pos : pos;
        const int e = st < Lm1 ? st : Lm1;
        const int src = e > 0 ? e - 1 : 0, last = Lm1 > 0 ? Lm1 - 1 : 0;
        uint32_t px = (uint32_t)__shfl((int)x, src, 64), py = (uint32_t)__shfl((int)y, src, 64), pz = (uint32_t)__shfl((int)z, src, 64);
        if (e == 0) px = py = pz = 0u;
        const uint32_t tx = (uint32_t)__shfl((int)x, last, 64), ty = (uint32_t)__shfl((int)y, last, 64), tz = (uint32_t)__shfl((int)z, last, 64);
        uint4 *out = c.psite + (size_t)row * (n_sites + 1);
        if (lane < n_sites) out[lane] = make_uint4(px, py, pz, 0u);
        if (lane == 0) out[n_sites] = make_uint4(tx, ty, tz, 0u);
    }
}

/* G(t, site) and the constant (walk_core.hip.h: cnt_site_table) from the prefix sums at the sites */
DEV void pc_site_table(const PcLds &c, int k, int n_sites) {
    const int W = n_sites + 1;
    for (int i = lane_id(); i <= k * n_sites; i += 64) {
        uint4 g;
        if (i == k * n_sites) {
            const uint4 a = c.psite[(size_t)k * W + n_sites], q = c.psite[(size_t)(k + 1 + k) * W + n_sites];
            g = make_uint4(a.x + q.x, a.y + q.y, a.z + q.z, 0u);
        } else {
            const int t = i / n_sites + 1, site = i - (t - 1) * n_sites, tb = k + 1 - t;
            const uint4 f0 = c.psite[(size_t)(t - 1) * W + site], f1 = c.psite[(size_t)t * W + site];
            const uint4 b0 = c.psite[(size_t)(k + 1 + tb - 1) * W + site], b1 = c.psite[(size_t)(k + 1 + tb) * W + site];
            g = make_uint4((f0.x - f1.x) + (b0.x - b1.x), (f0.y - f1.y) + (b0.y - b1.y), (f0.z - f1.z) + (b0.z - b1.z), 0u);
        }
        c.G[i] = g;
    }
}

/* The tables of PSM `psm`, whose retained table has R peaks at b.ret + ret0.  The caller has checked pc_fits with the
 * launch's caps.  Returns false (wave-uniform) when the letters give another number of modifiable residues than n_sites. */
DEV bool pc_setup(const BatchDev &b, uint32_t psm, unsigned char *lds_raw, const PcCaps &caps, int64_t ret0, int R, int k, int n_sites, PcPsm &p) {
    const int lane = lane_id();
    const DevConfig *cfg = b.cfg;
    p.caps = caps;
    p.l = pc_carve(lds_raw, caps);
    const PcLds &c = p.l;
    p.res = load_residues(b, cfg, psm);
    const Residues &res = p.res;
    const int L = res.L;
    p.L = L;
    p.k = k;
    p.n_sites = n_sites;
    if (__popcll(res.site_mask) != n_sites) return false;
    stage_peak_table_at(b, ret0, R, c.t_e, &p.tab);
    stage_residues(res, c.resd, nullptr);
    if (lane < 16) c.cum_lut[lane] = fused_cum_entry((uint32_t)lane);
    if ((res.site_mask >> lane) & 1ull) c.site_pos[mask_rank(res.site_mask)] = (uint8_t)lane;
    for (uint32_t i = lane; i < (uint32_t)((2 * caps.pos_cap * caps.kc + 15) & ~15u) / 4u; i += 64) ((uint32_t *)c.T)[i] = 0x0f0f0f0fu;
    wave_lds_sync();
    grid_build(&p.tab, c.grid);
    wave_lds_sync();
    /* envelopes, then one lookup per node */
    cnt_envelopes(res, k, caps.pos_cap, c.env);
    wave_lds_sync();
    double A0 = 0., B0 = 0., A1 = 0., B1 = 0.;
    type_constants(cfg->types[0], &A0, &B0);
    type_constants(cfg->types[cfg->n_fwd], &A1, &B1);
    const uint32_t per_dir = (uint32_t)(k + 1) * (uint32_t)(L - 1);
    const FastDiv divL = fastdiv_make((uint32_t)(L - 1));
    for (uint32_t i = (uint32_t)lane; i < 2u * per_dir; i += 64) {
        const uint32_t d = i >= per_dir ? 1u : 0u, r = i - d * per_dir, j = fastdiv(r, divL), st = r - j * (uint32_t)(L - 1);
        const float2 lh = c.env[(size_t)(d * (uint32_t)(k + 1) + j) * caps.pos_cap + st];
        uint32_t ent = cnt_table_entry(p.tab, lh.x, lh.y, d ? A1 : A0, d ? B1 : B0);
        if ((b.debug & 0x40000000u) && lh.x <= lh.y) ent |= CNT_MARK;       /* (every node marked: every assignment is walked) */
        c.T[((size_t)d * caps.pos_cap + st) * caps.kc + j] = (uint8_t)ent;
    }
    wave_lds_sync();
    pc_prefix_sums(c, caps, L, k, n_sites);
    wave_lds_sync();
    pc_site_table(c, k, n_sites);
    wave_lds_sync();
    p.env.cfg = cfg;
    p.env.n_nl = 0;
    p.env.nl_present = nullptr;
    p.env.nl_uniq = nullptr;
    p.env.resd = c.resd;
    p.env.resn = nullptr;
    p.env.cnt = nullptr;
    p.env.L = L;
    p.env.zmax = 1;
    return true;
}

/* The PepScore of the lane's site assignment `bits` (bit j = the j-th modifiable residue; k bits set), -1 when the score
 * table has no row for the peptide's fragment count.  Every lane of the wavefront calls it; `active` lanes have one. */
DEV float pc_score(const BatchDev &b, const PcPsm &p, uint64_t bits, bool active) {
    uint32_t marks = 0;
    CumCounts cc = {0u, 0u, 0u};
    if (active) {
        cc = cnt_eval_sites(p.l.G, (uint32_t)bits, p.k, p.n_sites, &marks);
        marks = cc.c >> 16;
        cc.c &= 0xffffu;
    }
    const bool marked = active && marks != 0u;
    if (__any(marked)) {                                     /* (rare: a peak within a few ulps of some window end) */
        float run0 = 0.f, run1 = 0.f;
        CumCounts cw = {0u, 0u, 0u};
        walk_cnt_both(p.env, p.tab, p.l.cum_lut, p.l.T, p.caps.pos_cap, p.caps.kc, deposit_sites(bits, p.res.site_mask), 0, p.L - 1, run0, 0u, 0,
                      p.L - 1, run1, 0u, cw);
        if (marked) cc = cw;
    }
    const uint32_t nfrag = 2u * (uint32_t)(p.L - 1);
    if (!active || nfrag > b.lut_n_max) return -1.f;
    double sum = 0.;
#pragma unroll
    for (int d = 0; d < PYA_NTOP; d++) {
        const float sc = lut_score(b, (uint32_t)d, cc.at(d), nfrag);
        const float prod = b.cfg->weights[d] * sc;           /* float product ... */
        sum = sum + (double)prod;                            /* ... double sum    */
    }
    return (float)sum;
}

#endif
