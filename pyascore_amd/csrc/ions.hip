/* ions.hip -- WHICH ions stand behind a scored plan: 16-byte records (pya_ion, include/pyascore_hip.h), CSR per PSM, one PSM
 * per wavefront, launched BEHIND a run like evidence.hip and on the same body (the general route's device functions).
 *
 * No kernel of a run reads anything written here.  The kernel reads what the run left -- the retained peak tables where
 * they lie, best_sig, status -- and the evidence rows of the same results (competitor and depth of every counted column):
 *   section 1, the winner's annotation         every fragment Ascore::accumulateCounts visits for the best localisation
 *                                              (cpp/Ascore.cpp:53-121) that has a retained peak in its window
 *                                              (ModifiedPeptide::consumePeak, cpp/ModifiedPeptide.cpp:126-142):
 *                                              ion_walk_winner (ion_match.hip.h), the lanes over 64 consecutive prefixes,
 *                                              the table INDEX of the match, records placed by ballot / mask_rank
 *   section 2, site-determining ions           for every PYA_EV_COUNTED column the two lists that survive the greedy walk
 *                                              (cpp/ModifiedPeptide.cpp:259-320) of the winner against that row's
 *                                              competitor: the pair routine of general_core.hip.h with every ion's identity
 *                                              carried through the rank sort in a parallel index array; lane 0 walks and
 *                                              marks the survivors, the wavefront writes them
 * One template, launched twice: COUNT (the emission compiled out; section 2 is the row's two `possible` fields) writes
 * the number of records of every PSM, FILL writes the records at the offsets the scan below made of the counts.  A PSM
 * whose records would pass `cap` writes nothing and is reported through over[] (count, 0xffffffff - the smallest PSM).
 */
#include "ion_match.hip.h"

#define ION_WINNER 255u
#define ION_LOSS 1u
#define ION_COMP 2u
#define ION_COUNTED 4u
#define ION_SURVIVES 0x80000000u
#define ION_EV_COUNTED 1u

/* behind the general route's LDS, per list entry: the identity of the unsorted ion and of the sorted ion of either list
 * (size | charge << 16 | loss << 24; bit 31: it survived the walk) */
__host__ __device__ static inline size_t ions_lds_bytes(uint32_t l_cap, uint32_t list_cap) {
    return gen_own_off(l_cap, list_cap) + (size_t)list_cap * 3 * 4;
}

DEV uint4 ion_rec(float theo, float peak, uint32_t size, uint32_t type, uint32_t charge, uint32_t rank, uint32_t site, uint32_t flags) {
    return make_uint4(__float_as_uint(theo), __float_as_uint(peak), (size & 0xffffu) | (type & 0xffu) << 16 | (charge & 0xffu) << 24,
                      (rank & 0xffu) | (site & 0xffu) << 8 | (flags & 0xffu) << 16);
}

/* the survivors of one sorted list, in m/z order, from `at` on (never at or past `end`); returns how many there were */
DEV uint32_t ion_write_list(uint4 *out, uint64_t at, uint64_t end, const float *theo, const float *peak, const uint32_t *ident,
                            const uint8_t *rank, int n, uint32_t type, uint32_t site, uint32_t side_flag, int depth) {
    uint32_t done = 0;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane_id();
        const uint32_t id = i < n ? ident[i] : 0u;
        const bool lives = (id & ION_SURVIVES) != 0u;
        const uint64_t m = __ballot(lives);
        const uint64_t pos = at + done + (uint64_t)mask_rank(m);
        if (lives && pos < end) {
            const uint32_t rk = rank[i];
            const uint32_t flags = side_flag | ((id >> 24) & 1u ? ION_LOSS : 0u) | ((int)rk <= depth ? ION_COUNTED : 0u);
            out[pos] = ion_rec(theo[i], peak[i], id & 0xffffu, type, (id >> 16) & 0xffu, rk, site, flags);
        }
        done += (uint32_t)__popcll(m);
    }
    return done;
}

/* Section 2 of one column: gen_ascore_pair's steps (Ascore.cpp:177-197) with the ions kept apart.  The winner's survivors
 * go to [at_ref, end_ref), the competitor's to [end_ref, end_oth), ion type after ion type, ascending m/z inside a type. */
DEV void ion_pair_emit(const DevConfig *cfg, const GenLds &g, uint32_t *ident_u, uint32_t *ident_a, uint32_t *ident_b, uint64_t ref_bits,
                       uint64_t oth_bits, int depth, int L, int zmax, uint32_t lc, uint32_t list_cap, const PeakEntry *tab, int R,
                       uint4 *out, uint64_t at_ref, uint64_t end_ref, uint64_t end_oth, uint32_t site) {
    const int lane = lane_id();
    const float err = cfg->mz_error;
    const bool half_check = err > 0.49f;
    const int T = cfg->n_types, n_fwd = cfg->n_fwd;
    const uint64_t types64 = load_types64(cfg);
    uint64_t at_oth = end_ref;
    int tables_dir = -1;
    uint32_t npairs_a = 0, npairs_b = 0;
    for (int t = 0; t < T; t++) {
        const int dir = t < n_fwd ? 0 : 1;
        if (dir != tables_dir) {
            gen_pair_tables(g, cfg, ref_bits, oth_bits, L, dir, lc, &npairs_a, &npairs_b);
            tables_dir = dir;
        }
        const int na = (int)npairs_a * zmax, nb = (int)npairs_b * zmax;
        if ((uint32_t)na > list_cap || (uint32_t)nb > list_cap) return;   /* (the evidence row would not be a counted one: not reached) */
        const uint32_t type = type_at(types64, t);
        double A, B;
        type_constants((uint8_t)type, &A, &B);
        gen_fill_list(g, cfg, L, zmax, 0, lc, A, B, g.la, ident_u);
        gen_sync();
        gen_rank_sort(g.la, g.sa, na, ident_u, ident_a);
        gen_sync();
        gen_fill_list(g, cfg, L, zmax, 1, lc, A, B, g.lb, ident_u);
        gen_sync();
        gen_rank_sort(g.lb, g.sb, nb, ident_u, ident_b);
        gen_sync();
        /* the match of every sorted ion: its rank beside it, the peak's m/z where the unsorted value was */
        for (int i = lane; i < na; i += 64) {
            int rk;
            const int at = gen_match_index(tab, R, g.sa[i], err, half_check, &rk);
            g.ha[i] = (uint8_t)rk;
            g.la[i] = at >= 0 ? tab[at].mz : 0.f;
        }
        for (int i = lane; i < nb; i += 64) {
            int rk;
            const int at = gen_match_index(tab, R, g.sb[i], err, half_check, &rk);
            g.hb[i] = (uint8_t)rk;
            g.lb[i] = at >= 0 ? tab[at].mz : 0.f;
        }
        gen_sync();
        if (lane == 0) gen_greedy_walk(g.sa, na, g.sb, nb, err, [&](int side, int i) { (side ? ident_b : ident_a)[i] |= ION_SURVIVES; });
        gen_sync();
        at_ref += ion_write_list(out, at_ref, end_ref, g.sa, g.la, ident_a, g.ha, na, type, site, 0u, depth);
        at_oth += ion_write_list(out, at_oth, end_oth, g.sb, g.lb, ident_b, g.hb, nb, type, site, ION_COMP, depth);
        gen_sync();
    }
}

/* ids == NULL: block i takes PSM i.  COUNT: off[psm] = the records of the PSM.  FILL: off[] are the scanned offsets. */
template <bool FILL>
__global__ __launch_bounds__(64) void pya_ions_kernel(BatchDev b, const uint32_t *ids, uint32_t n_ids, const uint4 *evid, int64_t *off, uint4 *out,
                                                       uint64_t cap, uint32_t *over, uint32_t l_cap, uint32_t list_cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    if (blockIdx.x >= n_ids) return;
    const uint32_t psm = ids ? ids[blockIdx.x] : blockIdx.x;
    const int lane = lane_id();
    const DevConfig *cfg = b.cfg;
    const GenLds g = gen_carve(lds_raw, l_cap, list_cap);
    const uint32_t lc = (l_cap + 3u) & ~3u;
    uint32_t *ident_u = (uint32_t *)(lds_raw + gen_own_off(l_cap, list_cap));
    uint32_t *ident_a = ident_u + list_cap, *ident_b = ident_a + list_cap;

    /* no records: not scored (set aside, rejected by a kernel, no site assignment) */
    const int N = b.status[psm] == PYA_ST_OK ? b.n_sig_out[psm] : -1;
    const int64_t pep0 = b.pep_off[psm];
    const int L = (int)(b.pep_off[psm + 1] - pep0);
    int n_sites = -1;
    if (N > 0 && L >= 1 && (uint32_t)L <= l_cap) n_sites = gen_setup_residues(b, cfg, g, psm, pep0, L);
    if (n_sites < 0 || n_sites > GEN_MAX_SITES) {
        if (!FILL && lane == 0) off[psm] = 0;
        return;
    }
    uint64_t base = 0, end = 0;
    if (FILL) {
        base = (uint64_t)off[psm];
        end = (uint64_t)off[psm + 1];
        if (end == base) return;
        if (end > cap || end < base) {                              /* nothing of the PSM is written */
            if (lane == 0) report_over(over, psm);
            return;
        }
    }

    const int k = b.n_of_mod[psm];
    const uint32_t max_k = b.max_k;
    const int zmax = b.max_charge[psm];
    const uint64_t best_bits = b.best_sig[psm];
    const PeakEntry *tab = b.ret + b.ret_off[psm];
    const int R = (int)b.ret_n[psm];
    const bool pairs = k > 0 && k < n_sites;                        /* (an unambiguous PSM has no section 2) */

    /* section 2 is as long as its counted rows say */
    uint64_t n2 = 0;
    if (pairs)
        for (int a = 0; a < k && a < (int)max_k && a < 64; a++) {
            const uint4 row = evid[(size_t)psm * max_k + a];
            if ((row.y >> 24) == ION_EV_COUNTED) n2 += (uint64_t)(row.z >> 16) + (uint64_t)(row.w >> 16);
        }
    if (FILL && end - base < n2) return;                            /* (offsets that are not this count's: not reached) */
    const uint64_t end1 = end - n2;

    /* ---- section 1: the winner's matched fragments in the order of ion_walk_winner, placed by ballot / mask_rank ---- */
    uint64_t n1 = 0;
    ion_walk_winner(g, cfg, best_bits, L, zmax, lc, tab, R, [&](int, int step, int v, uint32_t type, int z, float f, int at, int rk) {
        const uint64_t hit = __ballot(at >= 0);
        if (FILL) {
            const uint64_t pos = base + n1 + (uint64_t)mask_rank(hit);
            if (at >= 0 && pos < end1)
                out[pos] = ion_rec(f, tab[at].mz, (uint32_t)(step + 1), type, (uint32_t)z, (uint32_t)rk, ION_WINNER, v ? ION_LOSS : 0u);
        }
        n1 += (uint64_t)__popcll(hit);
    });
    if (!FILL) {
        if (lane == 0) off[psm] = (int64_t)(n1 + n2);
        return;
    }
    if (!pairs) return;
    gen_sync();

    /* ---- section 2: column after column, the winner's list, then the competitor's ---- */
    uint64_t at = end1;
    for (int a = 0; a < k && a < (int)max_k && a < 64; a++) {
        const uint4 row = evid[(size_t)psm * max_k + a];
        if ((row.y >> 24) != ION_EV_COUNTED) continue;
        const uint32_t n_ref = row.z >> 16, n_oth = row.w >> 16;
        const int pos_a = nth_set_bit(best_bits, a);
        const int comp = (int)(row.y & 0xffffu) - 1;
        if (pos_a < 64 && comp >= 0 && comp < L && g.sor[comp] != 255u) {
            const uint64_t oth = (best_bits & ~(1ull << pos_a)) | (1ull << (g.sor[comp] & 63u));
            ion_pair_emit(cfg, g, ident_u, ident_a, ident_b, best_bits, oth, (int)((row.y >> 16) & 0xffu), L, zmax, lc, list_cap, tab, R, out, at,
                          at + n_ref, at + n_ref + n_oth, (uint32_t)a);
        }
        at += (uint64_t)n_ref + n_oth;
    }
}

/* ---- the exclusive scan of the counts: a tile of 1 024 PSMs per wavefront, 16 consecutive ones per lane ---- */
#define ION_SCAN_ITEMS 16
#define ION_SCAN_TILE (64 * ION_SCAN_ITEMS)

/* exclusive prefix sum of a 64-bit value over the 64 lanes (all active) on the 32-bit DPP scan: the low 24 bits and the
 * rest are scanned apart (64 x 2^24 fits a word; values below 2^50) */
DEV uint64_t ion_wave_excl_scan_u64(uint64_t v, uint64_t *total) {
    int t_lo, t_hi;
    const int lo = wave_excl_scan_i32((int)(v & 0xffffffull), &t_lo);
    const int hi = wave_excl_scan_i32((int)((v >> 24) & 0x3ffffffull), &t_hi);
    *total = ((uint64_t)(uint32_t)t_hi << 24) + (uint64_t)(uint32_t)t_lo;
    return ((uint64_t)(uint32_t)hi << 24) + (uint64_t)(uint32_t)lo;
}

__global__ __launch_bounds__(64) void pya_ions_tile_sums_kernel(const int64_t *cnt, uint32_t n, uint64_t *tile_sum) {
    const uint64_t i0 = (uint64_t)blockIdx.x * ION_SCAN_TILE + (uint64_t)lane_id() * ION_SCAN_ITEMS;
    uint64_t s = 0;
    for (int j = 0; j < ION_SCAN_ITEMS; j++)
        if (i0 + j < n) s += (uint64_t)cnt[i0 + j];
    uint64_t total;
    (void)ion_wave_excl_scan_u64(s, &total);
    if (lane_id() == 0) tile_sum[blockIdx.x] = total;
}

/* in place: off[i] = counts before PSM i, off[n] = all of them */
__global__ __launch_bounds__(64) void pya_ions_scan_kernel(int64_t *off, uint32_t n, const uint64_t *tile_sum) {
    const int lane = lane_id();
    uint64_t before = 0;
    for (uint32_t t = lane; t < blockIdx.x; t += 64) before += tile_sum[t];
    uint64_t carry;
    (void)ion_wave_excl_scan_u64(before, &carry);
    const uint64_t i0 = (uint64_t)blockIdx.x * ION_SCAN_TILE + (uint64_t)lane * ION_SCAN_ITEMS;
    uint64_t v[ION_SCAN_ITEMS], s = 0;
    for (int j = 0; j < ION_SCAN_ITEMS; j++) {
        v[j] = i0 + j < n ? (uint64_t)off[i0 + j] : 0ull;
        s += v[j];
    }
    uint64_t total;
    uint64_t run = carry + ion_wave_excl_scan_u64(s, &total);
    for (int j = 0; j < ION_SCAN_ITEMS; j++) {
        if (i0 + j < n) off[i0 + j] = (int64_t)run;
        run += v[j];
    }
    if (blockIdx.x == gridDim.x - 1 && lane == 63) off[n] = (int64_t)(carry + total);
}

/* test-only: ion_wave_excl_scan_u64 by one full wavefront (include/pyascore_debug.h: pya_debug_wave64, PYA_DBG_ION_SCAN_U64):
 * out[0 .. 63] the exclusive sums, out[64 .. 127] the total as every lane has it */
__global__ __launch_bounds__(64) void pya_debug_ion_wave_scan_kernel(const uint64_t *in, uint64_t *out) {
    uint64_t total;
    out[lane_id()] = ion_wave_excl_scan_u64(in[lane_id()], &total);
    out[64 + lane_id()] = total;
}
extern "C" int pya_launch_debug_ion_wave_scan(const uint64_t *d_in, uint64_t *d_out, hipStream_t stream) {
    hipLaunchKernelGGL(pya_debug_ion_wave_scan_kernel, dim3(1), dim3(64), 0, stream, d_in, d_out);
    return (int)hipGetLastError();
}

extern "C" size_t pya_ions_lds_bytes(uint32_t l_cap, uint32_t list_cap) { return ions_lds_bytes(l_cap, list_cap); }
extern "C" uint32_t pya_ions_scan_tiles(uint32_t n) { return (n + ION_SCAN_TILE - 1) / ION_SCAN_TILE; }

/* d_ids (n_ids PSM numbers) or NULL: the PSMs 0 .. n_ids - 1; d_evid: [n_psm * b->max_k] evidence rows of the same results.
 * d_out == NULL: the count pass (d_off[psm] = records of the PSM); else the fill pass at the scanned offsets d_off */
extern "C" int pya_launch_ions(const BatchDev *b, const uint32_t *d_ids, uint32_t n_ids, const void *d_evid, int64_t *d_off, void *d_out,
                               uint64_t cap, uint32_t *d_over, uint32_t l_cap, uint32_t list_cap, hipStream_t stream) {
    if (n_ids == 0) return 0;
    const size_t lds = ions_lds_bytes(l_cap, list_cap);
    if (d_out) {
        hipError_t e = PYA_ENSURE_MAX_LDS(pya_ions_kernel<true>);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(pya_ions_kernel<true>, dim3(n_ids), dim3(64), lds, stream, *b, d_ids, n_ids, (const uint4 *)d_evid, d_off,
                           (uint4 *)d_out, cap, d_over, l_cap, list_cap);
    } else {
        hipError_t e = PYA_ENSURE_MAX_LDS(pya_ions_kernel<false>);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(pya_ions_kernel<false>, dim3(n_ids), dim3(64), lds, stream, *b, d_ids, n_ids, (const uint4 *)d_evid, d_off,
                           (uint4 *)nullptr, cap, d_over, l_cap, list_cap);
    }
    return (int)hipGetLastError();
}

/* d_off[0 .. n): counts in, offsets out; d_off[n] = their sum; d_tiles: room for pya_ions_scan_tiles(n) words of 8 bytes */
extern "C" int pya_launch_ions_scan(int64_t *d_off, uint32_t n, uint64_t *d_tiles, hipStream_t stream) {
    const uint32_t tiles = (n + ION_SCAN_TILE - 1) / ION_SCAN_TILE;
    if (tiles == 0) return 0;
    hipLaunchKernelGGL(pya_ions_tile_sums_kernel, dim3(tiles), dim3(64), 0, stream, (const int64_t *)d_off, n, d_tiles);
    hipLaunchKernelGGL(pya_ions_scan_kernel, dim3(tiles), dim3(64), 0, stream, d_off, n, (const uint64_t *)d_tiles);
    return (int)hipGetLastError();
}
