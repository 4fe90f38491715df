/*
 * pyascore_hip.h -- C ABI of the MI355X-native Ascore scorer (libpyascore_hip.so).
 *
 * This is the drop-in boundary for pyAscore's ptm_scoring hot path.  Every entry point
 * replaces a piece of the reference's Cython/C++ interface (citations are into the reference
 * tree, pyascore/ptm_scoring/):
 *
 *   pya_create / pya_destroy      PyAscore.__cinit__/__dealloc__      Ascore.pyx:64-79
 *   pya_add_neutral_loss          PyAscore.add_neutral_loss           Ascore.pyx:81-99
 *   pya_score_batch               PyAscore.score, batched             Ascore.pyx:103-152
 *                                 (= BinnedSpectra::consumeSpectra cpp/Spectra.cpp:43-68,
 *                                    ModifiedPeptide::consumePeptide/consumePeak
 *                                    cpp/ModifiedPeptide.cpp:105-142, Ascore::score
 *                                    cpp/Ascore.cpp:256-271)
 *   pya_score_batch_shared /      the hit_depth loop of the command line: every hit of a scan is scored against
 *   pya_plan_create_shared        the scan's ONE spectrum           pyascore/__main__.py (groupby(psms, scan), hit_depth)
 *   pya_results fields            best_score / ascores / alt_sites / best signature
 *                                                                     Ascore.pyx:232-288
 *   pya_get_pep_scores            PyAscore.pep_scores                 Ascore.pyx:241-252
 *   pya_get_pep_scores_range      the same for a range of PSMs of a retained batch (bulk export)
 *   pya_calculate_ambiguity       PyAscore.calculate_ambiguity        Ascore.pyx:208-230
 *   pya_format_peptide(s)         ModifiedPeptide::getPeptide         cpp/ModifiedPeptide.cpp:199-253
 *   pya_plan_*                    (new) device-resident variant of pya_score_batch for callers
 *                                 that keep spectra in HBM and own a HIP stream
 *   pya_evidence / pya_plan_evidence /   what Ascore::calculateAmbiguity holds while it works and drops
 *   pya_last_batch_evidence       (max_score_depth, ion_counts, ion_trials)      cpp/Ascore.cpp:157-210
 *   pya_ion / pya_plan_ions_count /      the matched fragments of the best localisation and the site-determining ions
 *   pya_plan_ions / pya_last_batch_ions  of every counted pair, one record per ion (per PSM: ModifiedPeptide::getMatch,
 *                                 getSiteDeterminingIons, FragmentGraph)         cpp/ModifiedPeptide.cpp:126-150, :259-320
 *   pya_named / pya_plan_named /         PyAscore.pep_scores and PyAscore.calculate_ambiguity(pep_scores[0], rec) for the
 *   pya_score_batch_named         site assignments the CALLER names, in bulk     Ascore.pyx:208-252, cpp/Ascore.cpp:53-210
 *
 * Conventions
 *   - plain pointers and sizes only; no C++ or framework types cross the boundary;
 *   - inputs are borrowed for the duration of the call (for pya_plan_run: until the stream
 *     has drained); outputs are caller-allocated; the library never frees caller memory;
 *   - every function returns PYA_OK (0) or a negative status; pya_last_error() gives the
 *     message and pya_error_index() the offending PSM (or -1);
 *   - a handle is single-owner (one handle <-> one device); different handles may be used
 *     from different threads;
 *   - there is NO CPU fallback: without a HIP device pya_create fails with PYA_ERR_HIP.
 *
 * Signature bit sets ("sig bits"): bit j is the j-th modifiable residue counted from the
 * N-terminus, 1 = modified.  Alternative-site masks: bit (p-1) = 1-based peptide position p.
 */
#ifndef PYASCORE_HIP_H
#define PYASCORE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PYA_OK 0
#define PYA_ERR_ARG (-1)    /* invalid configuration / argument                          */
#define PYA_ERR_HIP (-2)    /* HIP runtime failure or no device                          */
#define PYA_ERR_PSM (-3)    /* a PSM is invalid (unknown residue, empty spectrum, ...)   */
#define PYA_ERR_LIMIT (-4)  /* a PSM exceeds a documented limit of this implementation   */
#define PYA_ERR_STATE (-5)  /* call sequence error (e.g. no retained batch)              */

/* documented limits (DESIGN.md "Limits").  The FAST_* values are what the fast kernels take; a PSM beyond one of
 * them (and inside the limits above it) is scored by the general kernel (csrc/general_psm.hip): same results, the
 * reference's algorithm at a fraction of the speed. */
#define PYA_MAX_PEPTIDE_LEN 511               /* (the general kernel; the reference takes any length) */
#define PYA_MAX_SITES 63                   /* (the reference's own limit: cpp/Ascore.cpp:91-94 keys a signature by a long) */
#define PYA_MAX_SIGNATURES (1 << 22)       /* C(n_sites, n_of_mod) */
#define PYA_MAX_FRAGMENTS_PER_TYPE 8192    /* (L - 1) x charges x neutral-loss sums */
#define PYA_FAST_PEPTIDE_LEN 64
#define PYA_FAST_SIGNATURES 15000
#define PYA_FAST_FRAGMENTS_PER_TYPE 2048
#define PYA_MAX_PEAKS 65535                /* peaks of one spectrum */
#define PYA_FAST_PEAKS 8192
#define PYA_MAX_FRAGMENT_TYPES 8
#define PYA_MAX_CHARGE 255                 /* max_fragment_charge (the fragments per ion type above bound it long before) */
#define PYA_MAX_NL_VALUES 8                /* distinct neutral-loss masses; more than 4: every PSM through the general kernel */
#define PYA_N_TOP 10                       /* the value everything is built for (the reference's command line passes 10) */
#define PYA_MAX_N_TOP 16                   /* 11..16: every PSM of the scorer goes through the general kernel            */

#define PYA_FLAG_KEEP 1u    /* retain per-signature records for pya_get_pep_scores /     */
                            /* pya_calculate_ambiguity                                    */
#define PYA_FLAG_TIMING 2u  /* record HIP events around every kernel of pya_plan_run     */
#define PYA_FLAG_SKIP_INVALID 4u /* a PSM that is invalid, exceeds a limit or is rejected by a  */
                            /* kernel does not fail the call: it gets best_score -1, n_sig -1, */
                            /* and its code in pya_last_batch_status(); the rest is scored      */
#define PYA_FLAG_EVIDENCE 8u /* pya_score_batch*: the evidence records of every site as well       */
                            /* (pya_last_batch_evidence); pya_plan_create*: the plan's runs take   */
                            /* the per-stage launches whatever its size (pya_plan_evidence)        */
#define PYA_FLAG_IONS 16u   /* pya_score_batch*: the ion records of every PSM as well              */
                            /* (pya_last_batch_ions); pya_plan_create*: as PYA_FLAG_EVIDENCE       */
                            /* (pya_plan_ions_count / pya_plan_ions)                               */
#define PYA_FLAG_NAMED 32u  /* pya_plan_create*: as PYA_FLAG_EVIDENCE, for pya_plan_named;          */
                            /* pya_score_batch*: no effect (pya_score_batch_named takes the queries) */
#define PYA_FLAG_SITES 64u  /* pya_score_batch* / pya_score_batch_named: the site table of every PSM as */
                            /* well (pya_last_batch_sites); pya_plan_create*: as PYA_FLAG_EVIDENCE      */
                            /* (pya_plan_site_offsets / pya_plan_sites)                                 */
#define PYA_FLAG_PROBS 128u /* pya_score_batch* / pya_score_batch_named: the site probabilities of every PSM as */
                            /* well (pya_last_batch_probs); pya_plan_create*: as PYA_FLAG_EVIDENCE              */
                            /* (pya_plan_site_offsets / pya_plan_probs)                                         */
#define PYA_FLAG_RANKED 256u /* pya_score_batch* / pya_score_batch_named: the ranked localisations of every PSM as */
                             /* well (pya_last_batch_ranked, pya_set_ranked_k); pya_plan_create*: as               */
                             /* PYA_FLAG_EVIDENCE (pya_plan_ranked)                                                */
#define PYA_FLAG_ROLLUP 512u /* pya_score_batch* / pya_score_batch_named: the site roll-up of the batch as well, into the */
                             /* slots lent by pya_set_rollup (pya_last_batch_rollup); the library runs the probability    */
                             /* stage for itself; pya_plan_create*: as PYA_FLAG_EVIDENCE (pya_plan_rollup)                */
#define PYA_FLAG_PEPTIDOFORMS 1024u /* pya_score_batch* / pya_score_batch_named: the peptidoform list of the batch as well, */
                                    /* over the groups lent by pya_set_peptidoforms (pya_last_batch_peptidoforms); the       */
                                    /* library runs the probability stage for itself; pya_plan_create*: as                  */
                                    /* PYA_FLAG_EVIDENCE (pya_plan_peptidoforms)                                            */
#define PYA_FLAG_MZ_PROFILE 2048u /* pya_score_batch* / pya_score_batch_named: the fragment mass-error profile of the batch as  */
                                  /* well, into the run slots lent by pya_set_mz_profile (pya_last_batch_mz_profile); it needs  */
                                  /* no other stage; pya_plan_create*: as PYA_FLAG_EVIDENCE (pya_plan_mz_profile)               */
#define PYA_FLAG_RECALIBRATE 4096u /* pya_score_batch* / pya_score_batch_named: the m/z of every spectrum corrected with the      */
                                   /* calibration lent by pya_set_recalibration, in the library's own device copy, before the    */
                                   /* first kernel reads it; refused by pya_score_one, by pya_plan_create* (a plan's user calls  */
                                   /* pya_recalibrate_spectra on their own arrays) and together with PYA_FLAG_KEEP               */
#define PYA_FLAG_COVERAGE 8192u /* pya_score_batch* / pya_score_batch_named: the coverage record of every PSM as well           */
                                /* (pya_last_batch_coverage), taken on the spectra that were scored -- with                    */
                                /* PYA_FLAG_RECALIBRATE the corrected copy; it needs no other stage; pya_plan_create*: as      */
                                /* PYA_FLAG_EVIDENCE (pya_plan_coverage)                                                       */
#define PYA_FLAG_QUANT 16384u /* pya_score_batch* / pya_score_batch_named: the site quantification of the batch as well, over the */
                              /* slots of the same call's PYA_FLAG_ROLLUP (without it: PYA_ERR_ARG) and the channel matrix lent   */
                              /* by pya_set_site_quant (pya_last_batch_site_quant); pya_plan_create*: as PYA_FLAG_EVIDENCE        */
                              /* (pya_plan_site_quant)                                                                            */
#define PYA_FLAG_PFORM_QUANT 32768u /* pya_score_batch* / pya_score_batch_named: the peptidoform quantification of the batch as well, */
                                    /* row-aligned with the list of the same call's PYA_FLAG_PEPTIDOFORMS (without it: PYA_ERR_ARG)  */
                                    /* over the channel matrix lent by pya_set_peptidoform_quant (pya_last_batch_peptidoform_quant);  */
                                    /* pya_plan_create*: as PYA_FLAG_EVIDENCE (pya_plan_peptidoform_quant)                            */

/* per-PSM codes of pya_last_batch_status */
#define PYA_PSM_OK 0
#define PYA_PSM_NO_WINDOWS 1       /* all peaks on one multiple of 100 m/z (reference: UB)      */
#define PYA_PSM_TOO_MANY_WINDOWS 2
#define PYA_PSM_TABLE_RANGE 3      /* trial count outside the score table                        */
#define PYA_PSM_TIED_OVERFLOW 4
#define PYA_PSM_INVALID 16         /* unknown residue, empty spectrum, bad charge, ...           */
#define PYA_PSM_OVER_LIMIT 17      /* beyond a documented limit (length, sites, C(n,k), peaks)   */

/* What stands behind one Ascore: the depth it was taken at, the site-determining ions of the winning localisation and of
 * the competitor it was measured against, and that competitor.  Ascore::calculateAmbiguity computes all of it and returns
 * the one float (cpp/Ascore.cpp:157-210: max_score_depth :164-172, ion_counts / ion_trials :177-197); the reference never
 * exposes the competitor's PepScore (AscoreContainer.pep_scores).  One record per (PSM, modified site of the winner), in the
 * order of pya_results.ascores / alt_mask, row stride max_k.
 *   The competitors of site j are the positions in alt_mask[j] (the single-move competitors that share the site's best
 *   PepScore, Ascore.cpp:212-250); that PepScore is comp_score.
 *   PYA_EV_TIED     it is within 1e-6 of the winner's: the reference returns 0 before it looks at an ion (:159-161); depth
 *                   and counts are 0, comp_pos is the smallest alternative position.
 *   PYA_EV_COUNTED  the row belongs to the competitor whose ambiguity IS ascores[j] (getAscores takes the minimum; among
 *                   equal ones the smallest position), and
 *                       score(depth, ref_possible, ref_matched) - score(depth, comp_possible, comp_matched)
 *                   has the bit pattern of ascores[j], score(d, n, k) = |-10 log10 P(X >= k)|, X ~ Binomial(n, 2 mz_error
 *                   (d + 1) / 100) in the reference's float chain (Ascore.cpp:28-33, :199-207).
 *   PYA_EV_NONE     nothing to compare: ascores[j] is +inf, the PSM was not scored (status != 0, n_sig <= 0), or the column
 *                   is >= the PSM's n_of_mod.  Every other field is 0.
 * comp_pos is a 1-based peptide position for every peptide length (alt_mask switches to modifiable-residue bits above 64
 * residues; this does not). */
#define PYA_EV_NONE 0
#define PYA_EV_COUNTED 1
#define PYA_EV_TIED 2
typedef struct pya_evidence {      /* 16 bytes */
    float comp_score;              /* PepScore of the competitor */
    uint16_t comp_pos;             /* 1-based peptide position the modification moves to; 0 = none */
    uint8_t depth;                 /* 0-based peak depth the Ascore was taken at */
    uint8_t kind;                  /* PYA_EV_* */
    uint16_t ref_matched, ref_possible;    /* site-determining ions of the winner: matched at `depth`, all (ion_counts[0], ion_trials[0]) */
    uint16_t comp_matched, comp_possible;  /* ... of the competitor (ion_counts[1], ion_trials[1]) */
} pya_evidence;

/* Which ions stand behind a PSM: one record per ion, the records of a PSM in one range (ion_off[psm] .. ion_off[psm + 1])
 * of two sections.
 *   1. The winner's annotation (site == PYA_ION_WINNER): every theoretical fragment of the best localisation that has a
 *      match among the retained peaks -- one record per fragment Ascore::accumulateCounts visits (cpp/Ascore.cpp:53-121:
 *      every ion type of the scorer, charges 1 .. max_charge, neutral-loss variants; two fragments of one m/z are two
 *      records).  The match is ModifiedPeptide::consumePeak's (cpp/ModifiedPeptide.cpp:126-142, the mz - .5 lower bound for
 *      mz_error > 0.49 included): the lowest rank inside the open window and, among equal ranks, the lowest m/z.  Fragments
 *      without a match are not listed.  The number of records with rank <= d is the winner's count at depth d (pep_scores).
 *      PYA_ION_COUNTED is never set here (there is no row and no depth).
 *   2. Site-determining ions, for every column j of ascores / evidence whose evidence row is PYA_EV_COUNTED: the two lists
 *      that survive the greedy walk (cpp/ModifiedPeptide.cpp:259-320) of the winner against that row's competitor
 *      (comp_pos), matched or not (rank 255, peak_mz 0 when not).  There are ref_possible records of the winner, of which
 *      ref_matched carry PYA_ION_COUNTED, and comp_possible / comp_matched of the competitor (PYA_ION_COMP).  PYA_EV_TIED
 *      and PYA_EV_NONE columns have no records.
 * PSMs that were set aside or rejected have no records; a PSM without a competing localisation has section 1 only.
 * Order (fixed: two runs, every route and every cut into chunks give the same bytes).  Section 1: N-terminal ion types (b, c)
 * before C-terminal ones (y, z, Z); inside a direction blocks of 64 consecutive fragment sizes, inside a block by loss sum
 * (none first, then ascending), ion type in the scorer's order, charge, size.  Section 2: column after column; inside a
 * column the winner's records, then the competitor's; inside a side ion type after ion type in the scorer's order, ascending
 * theo_mz inside a type (equal m/z: size, loss sum, charge). */
#define PYA_ION_WINNER 255   /* pya_ion.site of section 1 */
#define PYA_ION_LOSS 1       /* pya_ion.flags: a neutral-loss variant */
#define PYA_ION_COMP 2       /* ... belongs to the competitor's list (else the winner's) */
#define PYA_ION_COUNTED 4    /* ... matched with rank <= the row's depth */
typedef struct pya_ion {     /* 16 bytes, one store */
    float theo_mz;           /* the fragment's m/z as the float32 the reference keys its match cache by */
    float peak_mz;           /* the retained peak it matched ((float)mz of the table); 0 when none */
    uint16_t size;           /* residues in the fragment, 1 .. L-1 */
    uint8_t type;            /* 'b' 'y' 'c' 'z' 'Z' */
    uint8_t charge;
    uint8_t rank;            /* 0-based rank of that peak in its window = first depth it counts at; 255: no match */
    uint8_t site;            /* PYA_ION_WINNER, or the column j of ascores / evidence the ion is site-determining for */
    uint8_t flags;           /* PYA_ION_* */
    uint8_t reserved;        /* 0 */
} pya_ion;

/* Localisations the caller names.  The evidence and ion records answer for the competitor the library picked; a user asks
 * about a site assignment of their own: the search engine's reported sites, the known site of a synthetic peptide, a
 * runner-up.  The reference answers per PSM with PyAscore.pep_scores (the ScoreContainer of every site assignment,
 * Ascore.pyx:241-252, cpp/Ascore.cpp:53-139) and PyAscore.calculate_ambiguity(ref, other) (Ascore.pyx:208-230,
 * cpp/Ascore.cpp:157-210); this is both, in bulk, for exactly the signatures asked for.
 *   Queries: a CSR list per PSM of sig bits (above: bit j = the j-th modifiable residue from the N-terminus, for every
 *   peptide length): q_off[n_psm + 1] (q_off[0] == 0, non-decreasing), q_bits[q_off[n_psm]].  A PSM may have no query,
 *   many, or the same one twice.  One record per query, in query order; sig_bits echoes the query in every record.
 *   Tests, in this order:
 *   PYA_NAMED_NONE     the PSM was not scored (status != 0, or n_sig <= 0: that includes n_of_mod above the number of
 *                      modifiable residues).  Every field but sig_bits is 0.
 *   PYA_NAMED_WINNER   the query IS best_sig: pep_score has the bits of best_score, ambiguity 0, no ion is looked at.
 *   PYA_NAMED_INVALID  the bits do not name exactly n_of_mod of the PSM's modifiable residues (popcount, or a bit at or above
 *                      the number of sites).  Every field but sig_bits and kind is 0.  Never an error of the call.
 *   PYA_NAMED_TIED     its PepScore is within 1e-6 of the winner's: the reference returns 0 before it looks at an ion
 *                      (cpp/Ascore.cpp:159-161); ambiguity 0.
 *   PYA_NAMED_COUNTED  ambiguity = Ascore::calculateAmbiguity(winner, query) for any number of moved modifications (it can
 *                      be negative: it is what the reference returns), and
 *                          score(depth, ref_possible, ref_matched) - score(depth, comp_possible, comp_matched)
 *                      has its bit pattern (score as for pya_evidence); depth follows cpp/Ascore.cpp:164-172 (strict > from
 *                      0: depth 0 when no depth favours the winner).
 *   WINNER, TIED and COUNTED carry the container: pep_score, total_fragments, n_moved and the rows of the two optional
 *   arrays are bit-equal to the record with the same sig_bits that pya_get_pep_scores* returns from a PYA_FLAG_KEEP batch.
 *   depth and the four ion counts are 0 unless COUNTED; the optional rows of NONE and INVALID are zero; reserved is 0, so
 *   records compare as 32 raw bytes.
 *   The winner with site j moved to an evidence row's comp_pos gives that row's depth and four counts, and ambiguity ==
 *   ascores[j] when the row is PYA_EV_COUNTED (PYA_NAMED_TIED when it is PYA_EV_TIED). */
#define PYA_NAMED_NONE 0
#define PYA_NAMED_INVALID 1
#define PYA_NAMED_WINNER 2
#define PYA_NAMED_TIED 3
#define PYA_NAMED_COUNTED 4
typedef struct pya_named {         /* 32 bytes, two 16-byte stores */
    uint64_t sig_bits;             /* the query, echoed */
    float pep_score;               /* ScoreContainer.weighted_score of that site assignment */
    float ambiguity;               /* Ascore::calculateAmbiguity(winner, this) */
    uint32_t total_fragments;      /* ScoreContainer.total_fragments */
    uint8_t kind, depth, n_moved, reserved;   /* PYA_NAMED_*; n_moved = n_of_mod - |winner AND query| */
    uint16_t ref_matched, ref_possible, comp_matched, comp_possible;   /* as in pya_evidence; COUNTED only */
} pya_named;

/* Site tables.  Everything above answers for one localisation (the winner), for the competitor the library picked per
 * modified site, or for signatures the caller names; a site-level table has a row for EVERY modifiable residue of the
 * peptide, and a delta score needs the runner-up.  Both are reductions over all site assignments of the PSM -- the
 * reference's pep_scores list (Ascore.pyx:241-252, cpp/Ascore.cpp:53-139) -- done on the device: per PSM and modifiable
 * residue, the best PepScore among the site assignments that modify the residue and the best among those that leave it
 * unmodified (the two max-marginals).  One record per (PSM, modifiable residue), the residues of a PSM from the N- to the
 * C-terminus, which is the bit order of sig bits; CSR per PSM through site_off[n_psm + 1], offsets the host knows from its
 * pre-pass.  A PSM the host pre-pass set aside (PYA_FLAG_SKIP_INVALID) has an empty range.
 *   Every score is the maximum of ScoreContainer.weighted_score over the matching records of the PSM's pep_scores, bit for
 *   bit (what pya_get_pep_scores* returns from a PYA_FLAG_KEEP batch).
 *   Which assignment is named when several attain the maximum ("attain" is float equality): best_sig if it is one of them,
 *   otherwise the numerically smallest sig bits.  The rule does not depend on the reference's std::sort order.
 *   So a residue of best_sig has with_score == best_score (bits) and with_sig == best_sig; any other residue has
 *   without_score == best_score and without_sig == best_sig; the largest without_score among the residues of best_sig is
 *   the runner-up localisation's PepScore, its without_sig the runner-up.  With n_of_mod == 1, without_score of the modified
 *   residue has the bits of the PSM's evidence comp_score; for any n_of_mod, comp_score of modified site j is <= the
 *   without_score of that site and <= the with_score of the residue at comp_pos (the Ascore looks at single moves only).
 *   PYA_SITE_NONE    the PSM was not scored (status != 0, n_sig <= 0): every field but pos is 0.
 *   PYA_SITE_OVER    n_sig is above the sig_cap of the call: pos and PYA_SITE_IN_BEST only, the rest 0.
 *   PYA_SITE_SCORED  otherwise.  n_of_mod == 0: nothing modifies a residue, with_score -1 and with_sig 0. */
#define PYA_SITE_NONE   0
#define PYA_SITE_SCORED 1
#define PYA_SITE_OVER   2
#define PYA_SITE_IN_BEST       1   /* flags: best_sig modifies this residue                                  */
#define PYA_SITE_WITH_TIED     2   /* more than one site assignment attains with_score                       */
#define PYA_SITE_WITHOUT_TIED  4   /* ... without_score                                                      */
#define PYA_SITE_NO_WITHOUT    8   /* n_of_mod == n_sites: nothing leaves it unmodified; without_score -1    */
typedef struct pya_site {          /* 32 bytes, two 16-byte stores */
    uint64_t with_sig;             /* a best site assignment that modifies the residue (sig bits)            */
    uint64_t without_sig;          /* a best one that leaves it unmodified; 0 with PYA_SITE_NO_WITHOUT       */
    float with_score;              /* its PepScore = max over the assignments that modify the residue        */
    float without_score;           /* max over those that do not; -1 with PYA_SITE_NO_WITHOUT                */
    uint16_t pos;                  /* peptide position, numbered as pya_evidence.comp_pos                    */
    uint8_t kind, flags;           /* PYA_SITE_*                                                             */
    uint32_t reserved;             /* 0: records compare as 32 raw bytes                                     */
} pya_site;

/* Site probabilities.  The site table above holds the two MAX-marginals of a PSM's PepScores; these are the two
 * SUM-marginals: the posterior over the site assignments that their PepScores imply, summed per modifiable residue -- the
 * localisation probability phosphoproteomics pipelines filter on ("class I site: p >= 0.75") -- and the posterior of the
 * reported localisation.  It is a PepScore-based posterior, MaxQuant's construction (a PepScore is -10 log10 of a chance
 * probability, so 10^(s / 10) is read as a likelihood ratio); it is NOT part of the Ascore publication and the reference
 * has no counterpart.  For a scored PSM with site assignments i = 0 .. n_sig - 1 in the order of its shape's signature
 * list (the list every route scores from; NOT the order of pya_get_pep_scores*' records, which is the reference's sorted
 * one), PepScores s_i (float32, bit-equal to the pep_scores records) and s* = best_score:
 *   w_i = exp2(((double)s_i - (double)s*) * C),  C = 0.33219280948873623 (log2(10) / 10): the likelihood ratio
 *         10^((s_i - s*) / 10).  The subtraction is exact in double; w of the winner is exactly 1.
 *   Z = sum w_i;  W_with[r] = sum of w_i over the assignments that modify residue r,  W_without[r] over those that do not.
 *         Each is a SEQUENTIAL double sum in list order (i ascending): given the w_i a host loop reproduces the sums bit
 *         for bit, and they do not depend on the route that scored the PSM, on chunk cuts or on batch neighbours.
 *   pya_site_prob  per modifiable residue, N- to C-terminus, at the offsets of the site table (pya_plan_site_offsets,
 *         site_off): with_prob = W_with / Z, without_prob = W_without / Z.  Both are kept: 1 - p loses everything near 1.
 *   pya_psm_prob   per PSM: z = Z (the posterior of the reported localisation is 1 / z), n_summed = n_sig, kind:
 *         PYA_SITE_NONE    the PSM was not scored (set aside, status != 0, n_sig <= 0): all zeros, residue records 0 / 0;
 *         PYA_SITE_OVER    n_sig is above the sig_cap of the call: z = 0, n_summed = 0, residue records -1 / -1;
 *         PYA_SITE_SCORED  otherwise.  n_of_mod == 0: z = 1, every residue 0 / 1.  n_of_mod == n_sites: every residue 1 / 0.
 * Only exp2 separates the device from a host restatement of this: floats agree to a few ulps, everything else exactly. */
typedef struct pya_site_prob {     /* 16 bytes, one store */
    double with_prob;              /* P(the residue is modified | spectrum, n_of_mod)                          */
    double without_prob;           /* P(it is not)                                                             */
} pya_site_prob;
typedef struct pya_psm_prob {      /* 16 bytes, one store */
    double z;                      /* sum of the likelihood ratios against the winner; 1 / z = its posterior   */
    uint32_t n_summed;             /* site assignments summed (n_sig)                                          */
    uint8_t kind;                  /* PYA_SITE_NONE / _SCORED / _OVER                                          */
    uint8_t pad[3];                /* 0                                                                        */
} pya_psm_prob;

/* Site roll-up.  Everything above is a view of ONE PSM; this is the first reduction ACROSS PSMs: the probability records of
 * many PSMs collapsed onto a dense table of caller-defined slots -- "one site" in whatever key the caller uses (peptide +
 * position, protein + position, ...) --, the site-level table of a phosphoproteomics report (MaxQuant's Phospho (STY)Sites,
 * the "class I sites" of a paper).  The caller names the slot of every residue record (slot[site_off[n_psm]], int32, in the
 * records' order; negative: the record is left out) and the number a PSM is known by (psm_id); the stage accumulates into
 * table[n_slots].  A record CONTRIBUTES when its PSM's pya_psm_prob.kind is PYA_SITE_SCORED and its slot lies in
 * [0, n_slots); PYA_SITE_NONE and PYA_SITE_OVER PSMs, PSMs that were set aside (they have no records) and negative slots
 * contribute nothing, a slot at or above n_slots writes nothing and is reported by pya_plan_check.  Two records of one PSM may
 * name one slot: both contribute.  Per slot, over its contributing records:
 *   best_prob    the largest with_prob, compared as the uint64 bit pattern (non-negative doubles order like their bits);
 *   best_psm     the smallest psm_id among the records whose with_prob has exactly those bits;
 *   n_psm        their number;  n_confident  ... of them with with_prob >= threshold (compared as doubles);
 *   n_in_best    ... of them whose PSM's best_sig modifies the residue (record r of a PSM is its r-th modifiable residue,
 *                bit r of best_sig);
 *   best_ascore  the largest Ascore of those: ascores[psm * max_k + popcount(best_sig & ((1 << r) - 1))], the column of the
 *                residue among the modified ones.  Largest under the total order of the bit patterns, -NaN < -inf < ... < -0
 *                < +0 < ... < +inf < +NaN: the float order wherever floats have one (an Ascore may be negative, and is
 *                +inf for a localisation without a competitor).
 * THE TABLE IS A FUNCTION OF THE MULTISET OF CONTRIBUTING RECORDS (slot, with_prob, psm_id, in-best, Ascore) AND OF NOTHING
 * ELSE: every field is an integer count, a max over bit patterns or a min over ids.  It does not depend on the order of the
 * atomics, on the route that scored a PSM, on shared or typed input, on chunk cuts, or on whether the PSMs came in one call
 * or were accumulated over several -- the table a caller holds between calls IS this record, and rolling more PSMs into it
 * gives the bytes of one call over all of them.  For the same reason two tables over the same slots can be merged on the
 * host: max / min / sum per field (best_psm: of the side with the larger best_prob, the smaller id on equal bits; best_ascore
 * only among sides with n_in_best != 0).  The empty slot is NOT all-zero bytes: pya_rollup_clear writes it.  Counts are
 * 32-bit and are not checked for overflow. */
#define PYA_ROLLUP_NO_PSM 0xffffffffu
typedef struct pya_site_rollup {   /* 32 bytes; records compare as raw bytes */
    double best_prob;              /* max with_prob over the contributing records; 0 when none                 */
    uint32_t best_psm;             /* psm_id of a PSM attaining it: the smallest such id; PYA_ROLLUP_NO_PSM none */
    uint32_t n_psm;                /* contributing records (scored PSMs that cover the slot)                   */
    uint32_t n_confident;          /* ... of them with with_prob >= threshold                                  */
    uint32_t n_in_best;            /* ... of them whose best_sig modifies the residue                          */
    float best_ascore;             /* max Ascore over those n_in_best records; 0 when n_in_best == 0           */
    uint32_t reserved;             /* 0                                                                        */
} pya_site_rollup;

/* Site quantification: the roll-up's slots joined with the channel intensities of a labelled experiment (TMT / iTRAQ reporters,
 * pya_marker above or any matrix of the caller's) -- per slot and channel the summed intensity of the PSMs that place the
 * modification on the site confidently.  The reference has no counterpart.  Input: the residue records of the probability
 * stage and best_sig of the results; slot[site_off[n_psm]] exactly as the roll-up takes it; a channel matrix
 * values[n_rows * n_channels], doubles, row-major, one row per spectrum (or whatever the caller keys rows by); row[n_psm], the
 * row of every PSM (int32; NULL: PSM i has row row_base + i; negative: the PSM has no channel data and is left out).
 * A residue record r of PSM p CONTRIBUTES iff the roll-up's rule holds (pya_psm_prob.kind == PYA_SITE_SCORED, slot in
 * [0, n_slots)), bit r of best_sig[p] is set, with_prob >= threshold (compared as doubles) and the PSM's row is in
 * [0, n_rows).  A negative slot or a negative row contributes nothing, silently.  A record that meets every other condition
 * and whose slot is at or above n_slots, or whose row is at or above n_rows, writes nothing and is reported by pya_plan_check
 * (PYA_ERR_LIMIT), as the roll-up reports its slots.  Two records of one PSM may name one slot: both contribute.
 * A value v is USABLE iff v == v && v > 0.0: NaN, zeros and negatives are "no reading".  Its QUANTUM q(v): t = v * 2^scale_log2,
 * one double multiplication by an exactly representable power of two; t >= 281474976710656.0 (2^48, +inf included): q = 2^48
 * and the reading is SATURATED; otherwise q = (uint64_t)t, by truncation (it may be 0: the reading still counts).  A
 * contributing record is COMPLETE when all n_channels values of its row are usable.
 * Per slot, head.n_records counts the contributing records and head.n_complete the complete ones among them.  Per cell
 * [slot * n_channels + c], over the contributing records whose value in channel c is usable -- with PYA_QUANT_COMPLETE_ONLY:
 * over the complete records only --: sum is the sum of q, n their number, n_saturated the saturated readings among them.
 * THE TABLE IS A FUNCTION OF THE MULTISET OF CONTRIBUTING RECORDS (slot, the row's values) AND OF NOTHING ELSE: every field is
 * an integer sum.  It does not depend on the order of the atomics, on how the records were grouped before they reached memory,
 * on the route that scored a PSM, on shared or typed input, on chunk cuts, or on whether the PSMs came in one call or were
 * accumulated over several plans, calls and files.  Two tables over the same slots and channels MERGE BY ADDING EVERY FIELD.
 * The empty table is all-zero bytes (hipMemsetAsync clears it).  Counts are 32-bit and sums 64-bit, neither checked for
 * overflow: a reading is at most 2^48, so a sum stays below 2^64 for up to 65 535 contributing records per slot.
 * csrc/site_quant.hip; the library is built without fast-math. */
#define PYA_QUANT_COMPLETE_ONLY 1u /* pya_site_quant_params.flags: only complete records are summed */
#define PYA_QUANT_MAX_CHANNELS 64
typedef struct pya_site_quant_params {  /* 24 bytes */
    double threshold;              /* a record contributes when with_prob >= threshold (not a NaN)              */
    int32_t scale_log2;            /* -64 .. 64: a quantum is 2^-scale_log2 intensity units                     */
    uint32_t n_channels;           /* 1 .. PYA_QUANT_MAX_CHANNELS: the columns of values and of the table       */
    uint32_t flags;                /* PYA_QUANT_COMPLETE_ONLY or 0                                              */
    uint32_t reserved;             /* 0                                                                        */
} pya_site_quant_params;
typedef struct pya_site_quant_head {   /* 8 bytes per slot; one 64-bit add */
    uint32_t n_records;            /* contributing records                                                     */
    uint32_t n_complete;           /* ... of them whose row has a usable value in every channel                */
} pya_site_quant_head;
typedef struct pya_site_quant {    /* 16 bytes per (slot, channel), at [slot * n_channels + c]; two 64-bit adds */
    uint64_t sum;                  /* sum of q over the summed records with a usable value in this channel     */
    uint32_t n;                    /* their number                                                             */
    uint32_t n_saturated;          /* ... of them with q = 2^48                                                */
} pya_site_quant;

/* Site FLR.  The roll-up says how good every site's best localisation is; this says which sites may be reported at a given
 * false-localisation rate: the slots sorted by best_prob, the expected errors 1 - p accumulated down the list and, with decoy
 * residues in the modification group (Ala / Pro / Gly beside STY), the decoys above every cut turned into a q-value.  Input:
 * a table in any state pya_plan_rollup or a host merge can leave it in, and optionally a class byte per slot, cls[n_slots] --
 * PYA_FLR_TARGET, PYA_FLR_DECOY, PYA_FLR_LEFT_OUT; NULL: every slot is a target.  A slot is RANKED when n_psm != 0, its class
 * is target or decoy and, with PYA_FLR_REPORTED_ONLY, n_in_best != 0.  The ranked slots are ordered by best_prob descending,
 * compared as the uint64 bit pattern (as the roll-up orders them), equal bits by ascending slot index.  A TIE GROUP is the set
 * of ranked slots with identical best_prob bits; every member of a group gets the same values, the cumulative ones at the END
 * of its group.  THE RECORD OF A SLOT IS A FUNCTION OF THE MULTISET OF (best_prob bits, class) OF THE RANKED SLOTS AND OF
 * NOTHING ELSE: rank and n_decoy are integer counts, err_sum is a sum of integers -- err(p) = (uint64_t)(max(0.0, 1.0 - p) *
 * 4294967296.0), one double subtraction, an exact scaling by 2^32, truncation; below 2^63 for n_slots <= 2^31 - 1 --, flr and
 * decoy_q are one correctly rounded division each of exactly converted integers.  Permuting the slots permutes the records.
 * flr needs no running minimum: the running mean of a non-decreasing sequence is non-decreasing.  An unranked slot's record
 * is 32 zero bytes.  csrc/flr.hip; the library is built without fast-math. */
#define PYA_FLR_TARGET 0u
#define PYA_FLR_DECOY 1u
#define PYA_FLR_LEFT_OUT 2u
#define PYA_FLR_REPORTED_ONLY 1u   /* flag: slots with n_in_best == 0 are not ranked */
#define PYA_FLR_TILE 1024u         /* slots per workgroup and sort pass (the sizes a test of the stage wants to straddle) */
typedef struct pya_site_flr {      /* 32 bytes; records compare as raw bytes */
    uint32_t rank;                 /* ranked slots whose best_prob bits are >= this slot's; 0: the slot is not ranked  */
    uint32_t n_decoy;              /* ... of them with class PYA_FLR_DECOY                                             */
    uint64_t err_sum;              /* sum of err(best_prob) over them                                                  */
    double flr;                    /* (double)err_sum / (double)((uint64_t)rank << 32): the model-based FLR of the cut  */
                                   /* "this site and everything at least as good"                                      */
    double decoy_q;                /* min over this group and every group with SMALLER best_prob of (double)n_decoy /   */
                                   /* (double)max(rank - n_decoy, 1): the q-value of the raw decoy / target ratio (the  */
                                   /* caller multiplies by the target-to-decoy residue frequency ratio, a positive      */
                                   /* constant that commutes with the minimum); 0 when no slot is a decoy              */
} pya_site_flr;

/* Peptidoform roll-up.  The site roll-up has one record per caller-keyed SITE; this is the second reduction across PSMs: one
 * record per localised PEPTIDOFORM, a peptide together with the site assignment reported for it -- MaxQuant's
 * modification-specific peptides, a "class I peptidoforms" list, the positional isomers seen for one peptide.  Its key holds
 * best_sig, which exists only after the run, so the records are a sorted LIST, not a dense table.  The caller names the
 * peptide of every PSM (group[n_psm], any non-negative int32, not dense; negative: the PSM is left out) and the number a PSM
 * is known by (psm_id).  A PSM CONTRIBUTES when its pya_psm_prob.kind is PYA_SITE_SCORED and its group is not negative;
 * PYA_SITE_NONE and PYA_SITE_OVER PSMs and PSMs that were set aside contribute nothing.  Per contributing PSM:
 *   min_prob    the smallest with_prob among its residue records r with bit r of best_sig set, compared as the uint64 bit
 *               pattern; exactly 1.0 for best_sig == 0;
 *   min_ascore  the smallest of ascores[psm * max_k + c], c = 0 .. popcount(best_sig) - 1, under the total order of bit
 *               patterns pya_site_rollup.best_ascore documents; +inf for popcount == 0.
 * THE LIST is one record per distinct (group, sig_bits) among the contributing PSMs, ordered by group ascending as uint32,
 * then by sig_bits ascending as uint64.  IT IS A FUNCTION OF THE MULTISET OF CONTRIBUTING (group, sig, min_prob, z,
 * min_ascore, psm_id) TUPLES AND OF NOTHING ELSE: the stage does no floating-point arithmetic (it copies and compares bits and
 * counts; only n_confident compares two doubles), so it does not depend on the order of the PSMs, on the route that scored a
 * PSM, on shared or typed input, on chunk cuts, or on how the PSMs were spread over calls -- a list fed back as d_prev with
 * more PSMs gives the bytes of one call over all of them, and two lists merge by pya_peptidoform_reduce or on the host:
 * counts add, best_min_prob the max over bits (best_psm of the side with the larger bits, the smaller id on equal bits),
 * best_z the min over bits, best_min_ascore the max under the total order, n_isomers recomputed.  A PSM is a record with
 * n_psm == 1.  Counts are 32-bit and are not checked for overflow.  csrc/peptidoforms.hip. */
#define PYA_PFORM_TILE 1024u       /* entries per workgroup and sort pass (the sizes a test of the stage wants to straddle) */
typedef struct pya_peptidoform {   /* 48 bytes, three 16-byte stores; records compare as raw bytes */
    uint64_t sig_bits;             /* the site assignment: best_sig of the PSMs behind the record              */
    uint32_t group;                /* the caller's key of the peptide                                          */
    uint32_t n_psm;                /* contributing PSMs                                                        */
    uint32_t n_confident;          /* ... of them with min_prob >= threshold (compared as doubles)             */
    uint32_t best_psm;             /* smallest psm_id among the PSMs whose min_prob has exactly the best bits  */
    double best_min_prob;          /* max over the PSMs of min_prob, compared as uint64 bit patterns           */
    double best_z;                 /* min over the PSMs of pya_psm_prob.z, compared as uint64 bit patterns     */
    float best_min_ascore;         /* max over the PSMs of min_ascore, under the roll-up's total order of bits */
    uint32_t n_isomers;            /* distinct sig_bits among the records of this group (same in all of them)  */
} pya_peptidoform;

/* Peptidoform quantification: the peptidoform list joined with the channel intensities of a labelled experiment -- per
 * modification-specific peptide and channel the summed intensity of the PSMs that report it confidently.  A site table adds
 * the intensities of species that are regulated independently (a doubly modified peptide and its singly modified forms share
 * sites); this one does not.  The reference has no counterpart.  THE RESULT IS A PAIR: a peptidoform list, pya_peptidoform[n],
 * byte for byte what pya_plan_peptidoforms gives for the same inputs, and a table ROW-ALIGNED with it, pya_site_quant_head
 * head[n] and pya_site_quant cell[n * n_channels]: row j belongs to list record j.  No new record types: the two structs and
 * pya_site_quant_params are the site quantification's.  Input: what pya_plan_peptidoforms takes (probability records,
 * best_sig, ascores, group, psm_id, the list's threshold, an earlier list), what pya_plan_site_quant takes for the channels
 * (values[n_rows * n_channels], row[n_psm] or NULL with row_base, params), and optionally the table of the earlier list.
 * A PSM CONTRIBUTES TO THE TABLE iff it contributes to the list (kind == PYA_SITE_SCORED, group not negative, best_sig inside
 * the plan's residue records and max_k), its min_prob -- the same bits the list stage computes -- satisfies min_prob >=
 * params->threshold compared as doubles, and its row is in [0, n_rows).  A negative row is left out silently.  A row at or
 * above n_rows writes nothing to the table and is reported by pya_plan_check (PYA_ERR_LIMIT), as the site quantification
 * reports it; the PSM is still in the list.  params->threshold is the table's own and independent of the list's threshold.
 * Usable value, quantum q(v), saturation at 2^48, COMPLETE and PYA_QUANT_COMPLETE_ONLY are pya_site_quant's above, word for
 * word (csrc/quant_rule.hip.h is the one place both stages take them from).  Per list record, head.n_records counts the
 * contributing PSMs of that key and head.n_complete the complete ones, plus the same fields of the earlier table's row for
 * the same key.  Per cell, sum, n and n_saturated over those PSMs with a usable value in the channel -- with
 * PYA_QUANT_COMPLETE_ONLY over the complete ones only --, plus the earlier table's cell for the same key.  A record of the
 * list none of whose PSMs contributes to the table has an all-zero row.
 * THE PAIR IS A FUNCTION OF THE MULTISET OF CONTRIBUTING TUPLES (group, sig, min_prob, z, min_ascore, psm_id, the row's
 * values) AND OF NOTHING ELSE: the list is, and every field of the table is an integer sum.  It does not depend on the order of
 * the PSMs, on the route that scored a PSM, on shared or typed input, on chunk cuts, or on how the PSMs were spread over calls.
 * A pair fed back as the earlier list and table together with more PSMs gives the bytes of one call over all of them.  Two
 * pairs merge by pya_peptidoform_quant_reduce: the keys' union, rows of equal keys added field by field.  A record with
 * n_psm == 0 in an input list is skipped, as the list stage skips it, and its table row with it.  THE CALLER KEEPS
 * params->threshold, scale_log2, n_channels and flags THE SAME across everything that is merged or fed forward: the table does
 * not record them.  Counts are 32-bit and sums 64-bit, neither checked for overflow.
 * cap: d_n[0] is the true length of the list; rows [0, min(length, cap)) of list and table are written; the call clears
 * head[0 .. cap) and cell[0 .. cap * n_channels) itself on the stream, so rows behind the list are zero bytes; a key whose
 * place in the list is at or above cap writes nothing; the result for a smaller cap is the byte prefix of the result for a
 * larger one.  csrc/pform_quant.hip; the library is built without fast-math. */

/* Channel correction: what stands between the raw reporter intensities of a labelled experiment and sums that are reported --
 * the isotope impurities of the reagent lot taken out per spectrum, and the columns brought to equal totals because the
 * channels were not loaded with equal amounts.  Both act on the channel matrix values[n_rows * n_channels] (doubles, row-major,
 * n_channels 1 .. PYA_QUANT_MAX_CHANNELS: what pya_marker_values writes and pya_plan_site_quant reads) BEFORE the tables sum it;
 * afterwards they cannot be done, because a sum of clamped values is not the clamp of a sum, the quanta are truncated per reading
 * and a "no reading" must stay one.  The reference has no counterpart.  Usable value and quantum q(v) are pya_site_quant's
 * above, word for word (csrc/quant_rule.hip.h is the one place the stages take them from).  With C = n_channels:
 * APPLY (pya_channel_correct), with a matrix m[C * C] (row-major: the inverse of the lot's spill matrix S, observed = S true;
 * the caller inverts) or a factor f[C] or both.  For every row v[0 .. C) and channel c:
 *   u[j]   = usable(v[j]) ? v[j] : +0.0
 *   v[c] not usable:  out[c] = v[c], bits copied -- a missing reading stays the missing reading it was, a zero stays a zero;
 *   otherwise         x = +0.0; for j = 0 .. C - 1 ascending: x = x + m[c * C + j] * u[j]    (with a matrix: one rounded double
 *                                                     multiplication and one rounded double addition per term, never fused)
 *                     x = v[c]                                                               (without a matrix)
 *                     x = x * f[c]                                                           (with a factor: one multiplication)
 *                     out[c] = (x == x && x > 0.0) ? x : +0.0
 * A corrected reading that is not positive is clamped to +0.0, which the quant stages take as "no reading" and the caller can
 * tell from a NaN; so is the NaN of inf * 0.  THE STAGE HAS ONE DEFINED ORDER OF ARITHMETIC, so its bytes are those of a host
 * restatement with the same doubles: no matrix instruction (v_mfma_f64_* fuses and reorders), no butterfly sum, no atomics.
 * SUMS (pya_channel_sums): one table row, pya_site_quant cell[C] -- per channel, over the selected rows (select[row] != 0, or
 * all) with a usable value in the channel: sum of q, n their number, n_saturated the saturated ones.  The result is ADDED into
 * cell; the empty row is zero bytes, so it accumulates over calls and files and rows merge by adding.  Integer sums: the bytes
 * depend on no order.
 * FACTORS (pya_channel_factors): M the largest sum of the C cells; f[c] = sum[c] == 0 ? 1.0 : (double)M / (double)sum[c], both
 * conversions to nearest and one correctly rounded division.  Every column's total is brought to the largest one -- an
 * order-free integer, and ratios between channels do not depend on the target.
 * csrc/channel_correct.hip; the library is built without fast-math. */
#define PYA_CHANNEL_NORMALIZE 1u   /* pya_channel_correct_host flags: equal column totals after the matrix pass */
#define PYA_CHANNEL_TILE 128u      /* rows per workgroup of the apply kernel (the sizes a test of the stage wants to straddle) */

/* Fragment mass-error profile.  The third reduction across PSMs, and the one that speaks about a SETTING rather than about a
 * localisation: per run (file, fraction, instrument -- a slot the caller names per PSM) the distribution of the m/z errors of
 * the matched fragments the scores counted, in Da and in ppm, resolved over bands of m/z.  The reference has no counterpart.
 * A PSM CONTRIBUTES when its status is OK, its n_sig > 0 and its slot run[psm] (int32, the caller's) is not negative.  THE
 * IONS of a contributing PSM are exactly its section-1 ion records, the winner's matched fragments as pya_plan_ions emits them
 * (site 255): the same match rule -- the lowest rank inside the open window of mz_error, not the nearest peak --, the same
 * fragments, and two fragments of one m/z are two ions.  Per ion with rank <= max_rank, in double and in this order:
 *   d    = (double)peak_mz - (double)theo_mz
 *   p    = d * 1e6 / (double)theo_mz                        one multiplication, then one division
 *   band = min(PYA_MZP_BANDS - 1, (int)floor((double)theo_mz * inv_band))
 *   q    = (int)floor(d * inv_da) + PYA_MZP_BINS / 2        counted in da[band][q] when 0 <= q < PYA_MZP_BINS, else in
 *                                                           out_da[0] (below the axis) or out_da[1] (at or above it)
 *   the same with p, inv_ppm, ppm[band][q] and out_ppm.
 * Bins are half-open, [j w, (j + 1) w) around 0: d == 0 lands in bin PYA_MZP_BINS / 2.  inv_da, inv_ppm and inv_band are the
 * CALLER's doubles, e.g. (PYA_MZP_BINS / 2) / half_width; the device never computes them, there is no multiply-add to contract
 * and double division is correctly rounded, so a host restatement with the same doubles gives EQUAL counts, not close ones.
 * Every word of a record is an integer count: THE TABLE IS A FUNCTION OF THE MULTISET OF (slot, ion) PAIRS AND OF NOTHING
 * ELSE -- not of the order of the PSMs, the route that scored them, shared or typed input, chunk cuts or how the PSMs were
 * spread over calls.  Two tables merge by adding every word.  Per slot
 *   sum(da) + out_da[0] + out_da[1] == n_ions, the same for ppm, and
 *   n_ions + n_rank_skipped == the section-1 ion records of the slot's PSMs.
 * Counts are 32-bit and are not checked for overflow.  What the profile cannot show: an error outside +-mz_error of the run
 * (such a peak was never matched), and the nearest peak where a lower-ranked one shares the window; random matches form a flat
 * floor under the peak.  The use is: run wide, read the profile, re-run narrow.  csrc/mz_profile.hip. */
#define PYA_MZP_BANDS 8
#define PYA_MZP_BINS 64
#define PYA_MZP_CHUNK 128u         /* PSMs per workgroup (the sizes a test of the stage wants to straddle) */
typedef struct pya_mz_profile {    /* 4 128 bytes; the empty record is all-zero bytes (hipMemsetAsync clears a table) */
    uint32_t n_psm;                /* contributing PSMs                                                        */
    uint32_t n_ions;               /* their ions with rank <= max_rank                                         */
    uint32_t n_rank_skipped;       /* their ions with rank > max_rank                                          */
    uint32_t out_da[2], out_ppm[2];
    uint32_t reserved;             /* 0                                                                        */
    uint32_t da[PYA_MZP_BANDS][PYA_MZP_BINS];
    uint32_t ppm[PYA_MZP_BANDS][PYA_MZP_BINS];
} pya_mz_profile;
typedef struct pya_mz_profile_params {
    double inv_da, inv_ppm, inv_band;  /* bins per Da, bins per ppm, bands per m/z unit: finite and positive   */
    uint32_t max_rank, reserved;       /* 0 .. 15: the deepest peak rank counted; 0                            */
} pya_mz_profile_params;

/* Fragment m/z recalibration: what turns a profile into a correction.  A profile that shows a SYSTEMATIC error -- +30 ppm at low
 * m/z fading to 0 at high m/z -- makes the narrow re-run useless: the true peaks lie outside the narrow window.  The FIT reads
 * one systematic error per band of m/z off the ppm axis of a profile, the APPLY corrects the m/z of spectra with it on the
 * device.  The reference has no counterpart.
 * THE FIT, per slot and band b, over the band's 64 ppm-axis counts h[0..63], every integer 64-bit:
 *   floor4 = h[0] + h[1] + h[62] + h[63]             the four outermost bins: the flat floor of random matches, times four
 *   ex[i]  = max(0, 4 h[i] - floor4),  E = sum ex[i]
 *   the band is FITTED when E >= 4 min_ions; n_signal[b] = floor(E / 4) (saturating at 2^32 - 1)
 *   for num in 16, 50, 84: j = the smallest bin with 100 cum[j] >= num E (cum the inclusive sum; ex[j] > 0 follows),
 *                          pos = j + (double)(num E - 100 (cum[j] - ex[j])) / (double)(100 ex[j])
 *   ppm[b] = (pos50 - 32) / inv_ppm,  spread_ppm[b] = (float)(0.5 (pos84 - pos16) / inv_ppm)
 *   a band that is not fitted has spread_ppm 0 and copies ppm from the nearest fitted band, the lower index on a tie; a slot
 *   without a fitted band is all zero apart from n_signal.
 * Integer sums, one double division per quantile and one per scaling: a host restatement gives EQUAL bytes
 * (pyascore_amd.rollup.fit_mz_calibration).
 * THE APPLY, per peak x of a spectrum whose slot is not negative, in double and in this order (ppm[] the slot's knots, which
 * sit at the CENTRES of the bands; inv_band the caller's double, bands per m/z unit, as in pya_mz_profile_params):
 *   u = x inv_band - 0.5,  j = clamp(floor(u), 0, 6),  t = clamp(u - j, 0, 1)
 *   e = ppm[j] + (ppm[j + 1] - ppm[j]) t,  c = e 1e-6,  x' = x - x c
 * float32 m/z is widened, corrected and rounded once back to float32.  A value that is not finite or not positive is copied
 * bit for bit, so the all-zero record leaves every byte as it was.  With |knots| <= PYA_MZC_MAX_PPM the map is increasing: an
 * ascending spectrum stays non-descending.  csrc/mz_calibrate.hip. */
#define PYA_MZC_MAX_PPM 1000
typedef struct pya_mz_calibration {   /* 128 bytes per run slot; the empty record is all-zero bytes = "no correction" */
    double   ppm[PYA_MZP_BANDS];        /* systematic error (observed - theoretical) at the CENTRE of band b, in ppm */
    float    spread_ppm[PYA_MZP_BANDS]; /* half of (q84 - q16) of the band's excess, in ppm; 0 where the band was not fitted */
    uint32_t n_signal[PYA_MZP_BANDS];   /* floor(E / 4): ions above the flat floor; fitted <=> n_signal >= min_ions */
} pya_mz_calibration;

/* Explained ion current: how much of the spectrum the reported localisation explains.  The PSM quality column of the field
 * (MS-GF+: ExplainedIonCurrentRatio, NTermIonCurrentRatio, CTermIonCurrentRatio, MS2IonCurrent; MaxQuant: intensity coverage,
 * peak coverage), and the number that shows on a caller's own spectra whether a transform in front of the run helped.  One
 * record per PSM, written BEHIND a run; no kernel of a run reads it.  The reference has no counterpart.
 * THE FRAGMENTS of a scored PSM are exactly its section-1 ion records (pya_ion, site 255): every theoretical fragment of
 * best_sig -- all ion types of the scorer, charges 1 .. max_charge, loss variants -- that has a retained peak in its window,
 * matched by the rule of the ion stage.  n_fragments is their number, so it equals the winner's cumulative count at depth
 * n_top - 1 in pep_scores.
 * EXPLAINED.  Raw peak i of the PSM's spectrum is explained iff (float)mz[i] equals, bit for bit as a float32 value (a float32
 * m/z is taken as it is), the peak_mz of at least one fragment; N-terminal-explained if such a fragment has a forward ion type
 * (b, c: the first types of the configuration), C-terminal-explained if such a fragment has a backward type (y, z, Z).  A peak
 * can be both.  A NaN m/z is never explained.  TWO RAW PEAKS WITH THE SAME float32 m/z ARE BOTH EXPLAINED when one is: the
 * price of a definition that does not depend on the order of the raw peaks -- spectra out of m/z order are scored (the exact
 * binning route) and are covered here.
 * THE FOUR SUMS are in double, in this order and no other, over the spectrum's peaks by local index: lane l = 0 .. 63
 * accumulates p[l] = ((0.0 + x[l]) + x[l + 64]) + ..., then s = (((0.0 + p[0]) + p[1]) + ...) + p[63].  In a restricted sum a
 * peak outside the set contributes + 0.0: added, not skipped.  float32 intensities widen exactly; NaN and infinities propagate
 * by IEEE.  No multiply-add exists to contract, so a host restatement gives EQUAL bytes (pyascore_amd.rollup.coverage).
 * SIZES.  A forward fragment of size s covers bond s, a backward one of size s bond L - s (L the peptide's length, bonds
 * 1 .. L - 1).  nterm_sizes / cterm_sizes count the distinct s with a fragment of that direction, over any type, charge and
 * loss variant; *_run is the longest run of consecutive s in that set; bonds the size of the union of the covered bonds.
 * PYA_COV_NONE: the PSM was not scored (status != 0 or n_sig <= 0) or was set aside; every other byte of the record is 0.
 * The record is a function of the PSM, its spectrum and the scorer: not of the route, shared or typed input or chunk cuts.
 * csrc/coverage.hip. */
#define PYA_COV_NONE 0
#define PYA_COV_SCORED 1
typedef struct pya_coverage {      /* 64 bytes, four 16-byte stores; records compare as raw bytes */
    double total_current;          /* sum of the intensities of every raw peak of the PSM's spectrum            */
    double explained_current;      /* ... of the explained peaks                                                */
    double nterm_current;          /* ... of the peaks explained by a forward ion type                          */
    double cterm_current;          /* ... of the peaks explained by a backward ion type                         */
    uint32_t n_peaks;              /* raw peaks of the spectrum                                                 */
    uint32_t n_retained;           /* peaks the binning kept (the retained table)                               */
    uint32_t n_explained;          /* raw peaks that are explained                                              */
    uint32_t n_fragments;          /* section-1 ion records of the PSM                                          */
    uint16_t nterm_sizes, cterm_sizes;   /* distinct fragment sizes with a forward / backward fragment          */
    uint16_t nterm_run, cterm_run;       /* longest run of consecutive sizes among them                         */
    uint16_t bonds;                /* bonds 1 .. L - 1 covered from either side                                 */
    uint8_t kind;                  /* PYA_COV_NONE / PYA_COV_SCORED                                             */
    uint8_t pad[5];                /* 0                                                                         */
} pya_coverage;

/* Deisotoping: the one step in front of a run that REMOVES peaks.  High-resolution MS2 spectra carry isotope envelopes; every
 * M+1 / M+2 satellite that makes the cut of the ten most intense peaks per 100 m/z takes a slot from a real fragment and offers
 * one more random match.  The filter is a transform of spectra that runs before a plan exists (a plan reads the peak counts on
 * the host); no kernel of a run knows of it.  The reference has no counterpart.
 * THE RULE is local and order-free; every spectrum is handled on its own and the output is a subset of its peaks, bits copied.
 * A spectrum has ascending m/z x[] and intensities y[] (float32 is widened at the load).  Peak j is REMOVED iff there is a peak
 * i of the same spectrum and a charge z in 1 .. max_charge with, in double and in this order of operations:
 *   d = x[j] - x[i],  e = d - spacing[z - 1],  fabs(e) <= tol
 *   m = x[i] (double)z,  b = ratio0 + ratio_per_mz m,  y[j] <= y[i] b
 * The parent i may itself be a removed peak (M+2 goes because of M+1): no greedy claiming, no dependence on the order peaks are
 * visited in.  A comparison with a NaN is false, so a peak with a NaN intensity stays and removes nothing.  spacing[] are the
 * caller's doubles (the Python helper fills step / z on the host: the kernel divides nothing and a host restatement reads the
 * same bits, pyascore_amd.rollup.deisotope).  The parameters must satisfy: tol finite and >= 0; ratio0 and ratio_per_mz finite;
 * 1 <= max_charge <= PYA_DEISO_MAX_CHARGE; reserved == 0; spacing[0 .. max_charge) finite, positive and strictly decreasing;
 * spacing[max_charge - 1] > 2 tol.  So a parent has a strictly lower m/z, hence a lower index, e is monotone in i, and the
 * lowest peak of a spectrum is always kept: a spectrum that is not empty stays so.
 * A spectrum that is NOT ASCENDING -- an adjacent pair without x[k - 1] <= x[k]: a descending pair, or a NaN m/z, which no order
 * holds -- is copied unchanged and reported. */
#define PYA_DEISO_MAX_CHARGE 8
typedef struct pya_deisotope_params {   /* 96 bytes */
    double tol;                             /* half width of the match on the isotope spacing, in m/z units (Da)            */
    double ratio0, ratio_per_mz;            /* a satellite is at most (ratio0 + ratio_per_mz x[i] z) times its parent        */
    double spacing[PYA_DEISO_MAX_CHARGE];   /* the isotope spacing at charge z in [z - 1]; entries at and above max_charge  */
                                            /* are not read                                                                  */
    uint32_t max_charge, reserved;          /* 1 .. PYA_DEISO_MAX_CHARGE; 0                                                  */
} pya_deisotope_params;

/* Charge deconvolution: deisotoping, and the fragments that the removed satellites show to be multiply charged reduced to 1+.
 * The satellites of a peak are the only evidence of its charge; deisotoping alone throws it away and leaves a 2+ or 3+ fragment
 * at its multiply-charged m/z, where a run with b/y at 1+ never finds it.  Like deisotoping a transform of spectra in front of a
 * plan (the peak counts change); no kernel of a run knows of it.  The reference has no counterpart.
 * THE RULE.  Every spectrum is handled on its own; x[], y[], "in double" and R are those of pya_deisotope_params above: for
 * peaks i, j and a charge z, R(i, j, z) holds iff, in double and in this order of operations,
 *   d = x[j] - x[i],  e = d - iso.spacing[z - 1],  fabs(e) <= iso.tol
 *   m = x[i] (double)z,  b = iso.ratio0 + iso.ratio_per_mz m,  y[j] <= y[i] b
 * so that peak j is removed by deisotoping iff R(i, j, z) for some i and some z in 1 .. iso.max_charge.
 * KEPT SET: the kept peaks are exactly those deisotoping keeps under iso.
 * CHARGE: c(i) of kept peak i is the largest z in 2 .. iso.max_charge for which some peak j has R(i, j, z) and
 * y[j] >= y[i] witness (the product in double); 1 when there is no such z.  The child j is always a removed peak (R removes it);
 * a child testifies for every z it matches; z = 1 needs no witness.  witness is the least share of the parent's intensity a
 * child must have to be believed: on spectra whose fragments are all 1+, a chance peak half a spacing above a fragment testifies
 * to a false 2+, and a real M+1 is seldom that weak.
 * MOVED VALUE, in double and in this order, then rounded once to the m/z element type:
 *   t = x[i] (double)c,  u = (double)(c - 1) carrier,  v = t - u
 * If c >= 2 and the stored (rounded) value is finite and greater than x[i], the peak's m/z becomes it and its charge is c.
 * Otherwise the peak stays and its charge is reported as 1 (so a peak with x[i] <= carrier never moves).  Intensities are copied
 * bit for bit, and so is the m/z of every peak that does not move.
 * carrier is the mass one charge adds.  Its default, PYA_DECHARGE_CARRIER, is the value the scoring kernels themselves add per
 * charge -- the literal 1.007825 of charge_mz() in csrc/device_common.hip.h and of the walks in csrc/walk_core.hip.h, the
 * reference's PROTON: the mass of a hydrogen atom to six places, not the proton's 1.00728 --, so that a reduced peak lands where
 * a run computes the fragment at 1+.
 * OUTPUT ORDER: the kept peaks of a spectrum ordered by stored m/z as numbers, equal values by raw index (a stable sort of the
 * kept peaks in raw order).  Moving only raises m/z, so a moved peak precedes every unmoved peak of equal value.
 * A spectrum that is NOT ASCENDING in pya_deisotope_params' sense is copied unchanged and reported; all its charges are 1.
 * With iso.max_charge == 1 the output is byte for byte that of pya_deisotope_spectra.
 * The parameters must satisfy: iso as at pya_deisotope_params; carrier finite and > 0; witness finite and >= 0. */
#define PYA_DECHARGE_CARRIER 1.007825
typedef struct pya_decharge_params {   /* 112 bytes */
    pya_deisotope_params iso;   /* the deisotoping rule, unchanged, with its conditions                                      */
    double carrier;             /* mass of one charge carrier; finite, > 0                                                   */
    double witness;             /* a child testifies to a charge only with y[j] >= y[i] witness; finite, >= 0                */
} pya_decharge_params;

/* Precursor stripping: the peaks of an MS2 spectrum that are no fragments at all -- the unfragmented precursor, its
 * neutral-loss forms (precursor - H3PO4 is usually the base peak of a phosphopeptide's CID spectrum), under ETD the
 * charge-reduced precursors [M + zH]^(z')+, z' < z, and their losses, in TMT runs the reporter region -- removed before a run.
 * Each of them is the most intense peak of its 100 m/z window: it takes the first of the n_top ranks there, moves every real
 * fragment of the window one rank down at every depth, and is one more target for a random match.  Like deisotoping a transform
 * of spectra in front of a plan (the peak counts change); no kernel of a run knows of it.  The reference has no counterpart.
 * THE RULE.  Every spectrum s is handled on its own, with its precursor prec_mz[s] (double) and prec_z[s] (int32).
 * NO WINDOWS: a spectrum whose prec_z is outside 1 .. PYA_STRIP_MAX_CHARGE, or whose prec_mz is not finite or not positive,
 * has no windows; the range cut below still applies to it.
 * THE WINDOWS: otherwise C = prec_z when reduced, else 1.  For the charge index c = 0 .. C - 1 let z' = prec_z - c; for the
 * loss index l = 0 .. n_loss, window w = c (n_loss + 1) + l is, in double, every operation rounded on its own, in this order:
 *   M    = prec_mz (double)prec_z
 *   cen  = (M - loss[l]) / (double)z'
 *   span = (double)isotopes (step / (double)z')
 *   lo   = cen - tol
 *   hi   = (cen + span) + tol
 * At most 8 x 8 = 64 windows.  A window whose cen is not finite or not positive is INACTIVE.  loss[0] is always 0.0: window
 * c (n_loss + 1) is the (charge-reduced) precursor itself.
 * WHICH PEAKS GO: a peak with m/z x (float32 is widened at the load) is REMOVED iff x < mz_lo, or x > mz_hi, or some active
 * window has lo <= x && x <= hi.  A comparison with a NaN is false, so a peak with a NaN m/z stays.  Intensities are never
 * looked at.  The rule is per peak and order-free: a spectrum need not be ascending and there is no "not ascending" path.
 * The output is the kept peaks in input order, bits copied.
 * THE REPORT: per spectrum one pya_strip_report.  Bit w of hit is set iff at least one peak of the spectrum lies in active
 * window w, whether or not the range cut removes that peak too; n_windows is the number of active windows; n_removed the
 * number of peaks removed by any part of the rule.  "Precursor - 98 seen" is the classic pS/pT-versus-pY hint.
 * The parameters must satisfy: tol finite and >= 0; step finite and > 0; mz_lo and mz_hi not NaN with mz_lo <= mz_hi (the
 * defaults -inf and +inf cut nothing); n_loss <= PYA_STRIP_MAX_LOSS; loss[0] == 0.0 and loss[1 .. n_loss] finite and >= 0
 * (entries above n_loss are not read); reduced 0 or 1; isotopes 0 .. PYA_STRIP_MAX_ISOTOPES; reserved == 0. */
#define PYA_STRIP_MAX_CHARGE 8
#define PYA_STRIP_MAX_LOSS 7
#define PYA_STRIP_MAX_ISOTOPES 4
#define PYA_STRIP_STEP 1.0033548378
typedef struct pya_strip_params {   /* 112 bytes */
    double tol;                             /* half width of a window beyond its centre (and its isotopes), in m/z (Da)      */
    double step;                            /* the isotope spacing at charge 1; a window reaches isotopes step / z' upwards  */
    double mz_lo, mz_hi;                    /* the range cut: peaks below mz_lo or above mz_hi go                            */
    double loss[PYA_STRIP_MAX_LOSS + 1];    /* neutral masses taken off M; [0] is 0.0, [1 .. n_loss] the caller's            */
    uint32_t n_loss;                        /* 0 .. PYA_STRIP_MAX_LOSS                                                       */
    uint32_t reduced;                       /* 1: windows at every charge prec_z, prec_z - 1, .. 1 (ETD); 0: at prec_z only  */
    uint32_t isotopes;                      /* isotope peaks above the centre a window covers, 0 .. PYA_STRIP_MAX_ISOTOPES   */
    uint32_t reserved;                      /* 0                                                                             */
} pya_strip_params;
typedef struct pya_strip_report {   /* 16 bytes per spectrum */
    uint64_t hit;                           /* bit w: a peak lay in active window w = c (n_loss + 1) + l                     */
    uint32_t n_removed;                     /* peaks removed, by a window or by the range cut                                */
    uint32_t n_windows;                     /* active windows                                                                */
} pya_strip_report;

/* Marker ions: the intensities of reporter and diagnostic ions per spectrum -- the isobaric-label reporters a site is
 * quantified with, the pY immonium ion, the precursor's - H3PO4 and - HPO3 peaks -- read off the peaks pya_strip_params is there
 * to remove.  A READ-ONLY stage: it looks up at most PYA_MARKER_MAX_TARGETS target windows per spectrum and writes records; the
 * spectra and their peak counts stay as they are, so there is no workspace, no scan and no fill, and no kernel of a run knows
 * of it.  The reference has no counterpart.
 * THE RULE.  Every spectrum s is handled on its own; x is the m/z of a peak and y its intensity (float32 is widened at the
 * load); all arithmetic is in double, every operation rounded on its own, in the order written; a comparison with a NaN is
 * false.
 * THE CENTRE c of target t: a FIXED target (bit t of loss_mask clear) has c = value[t] and is always active.  A LOSS target
 * (bit t set) applies only to a spectrum with a usable precursor -- strip's test: prec_z[s] in 1 .. PYA_STRIP_MAX_CHARGE,
 * prec_mz[s] finite and > 0 --, where
 *   c = (prec_mz (double)prec_z - value[t]) / (double)prec_z
 * and the target is ACTIVE iff c is finite and > 0.  Without a usable precursor a loss target is inactive.
 * THE WINDOW of an active target:
 *   w  = tol + (tol_ppm 1e-6) c
 *   lo = c - w,  hi = c + w
 * A peak is INSIDE iff lo <= x && x <= hi; a NaN m/z is never inside.  n_peaks of the record counts every peak inside.
 * THE PICK: a peak inside is ELIGIBLE iff y == y.  Among the eligible peaks the larger y wins; with equal y the smaller
 * fabs(x - c); with that equal too the smaller x.  That is a total order up to peaks with equal (x, y), so the record does not
 * depend on the order of the peaks.  The record holds x + 0.0 and y + 0.0 of the pick (no -0.0 reaches a record) and 0.0 / 0.0
 * when no peak is eligible.  A peak inside the windows of two targets counts for both and may be picked by both.
 * PER SPECTRUM: tic is the sum of (y == y ? y : 0.0) over the peaks: 64 partials from 0.0, peak k (counted from the spectrum's
 * first) into partial k mod 64 in index order, the partials then added in order from 0.0 (pya_coverage's sum).  base_peak is
 * the largest y with y == y of the whole spectrum, + 0.0; 0.0 when there is none.  n_peaks is the (clipped) peak count, n_active
 * the number of active targets, bit t of hit is set iff target t picked a peak.
 * An INACTIVE target's record is all zero; every record of a call is written.
 * The parameters must satisfy: tol and tol_ppm finite and >= 0; n_targets in 1 .. PYA_MARKER_MAX_TARGETS; no bit of loss_mask
 * at or above n_targets; value[t], t < n_targets, finite, > 0 for a fixed target and >= 0 for a loss target (entries from
 * n_targets on are not looked at); reserved == 0. */
#define PYA_MARKER_MAX_TARGETS 64
typedef struct pya_marker_params {     /* 544 bytes */
    double tol;                                    /* half width of a window in m/z (Da); finite, >= 0                       */
    double tol_ppm;                                /* and in ppm of the centre, added to it; finite, >= 0                    */
    double value[PYA_MARKER_MAX_TARGETS];          /* fixed target: its m/z; loss target: the neutral mass off the precursor */
    uint64_t loss_mask;                            /* bit t: target t is relative to the precursor; no bit >= n_targets      */
    uint32_t n_targets;                            /* 1 .. PYA_MARKER_MAX_TARGETS                                            */
    uint32_t reserved;                             /* 0                                                                      */
} pya_marker_params;
typedef struct pya_marker {            /* 24 bytes per (spectrum, target), at [s * n_targets + t] */
    double mz, intensity;                          /* the picked peak, widened; 0.0 / 0.0 when none                          */
    uint32_t n_peaks;                              /* peaks of the spectrum inside the window                                */
    uint32_t flags;                                /* bit 0: the target is active for this spectrum; bit 1: a peak was picked */
} pya_marker;
#define PYA_MARKER_ACTIVE 1u
#define PYA_MARKER_PICKED 2u
typedef struct pya_marker_spectrum {   /* 32 bytes per spectrum */
    double tic, base_peak;                         /* the ion current and the largest intensity of the spectrum              */
    uint64_t hit;                                  /* bit t: target t picked a peak                                          */
    uint32_t n_peaks, n_active;                    /* peaks of the spectrum; active targets                                  */
} pya_marker_spectrum;

/* Precursor purity: the share of an MS2 scan's isolation window that belonged to the identified precursor, read off the survey
 * (MS1) scan in front of it -- MaxQuant's PIF, Proteome Discoverer's "isolation interference".  A reporter reading is only as
 * good as that share: what else was isolated adds its own signal to every channel and compresses the ratios.  A READ-ONLY
 * stage over the survey spectra, as the marker stage is over the MS2 spectra: records out, no workspace, and no kernel of a
 * run knows of it.  The reference has no counterpart.
 * THE RULE.  n_survey survey spectra (pya_typed_spectra + int64 offsets) and n_query queries, one per MS2 spectrum, row-aligned
 * with the matrix pya_marker_values writes.  Per query q: survey[q] (int64, the survey spectrum to read), prec_mz[q] (double),
 * prec_z[q] (int32), win_lo[q] and win_hi[q] (double, the ABSOLUTE m/z bounds of the isolation window).  All arithmetic is in
 * double, every operation rounded on its own, in the order written; a comparison with a NaN is false; float32 is widened at
 * the load.
 * INACTIVE: a query with survey[q] < 0, or whose precursor fails strip's test (prec_z in 1 .. PYA_STRIP_MAX_CHARGE, prec_mz
 * finite and > 0), or for which win_lo <= win_hi is false, or one of whose bounds is not finite.  Its record is all zero and
 * nothing is read for it.
 * survey[q] >= n_survey: the record is all zero and the query is reported through d_over as a clipped spectrum is (counted in
 * d_over[0], the smallest such q in d_over[1] as 0xffffffff - q); nothing is read.  An active query whose survey spectrum's
 * offsets had to be clipped to the elements the arrays hold is reported the same way; its record is that of the clipped peaks.
 * THE CENTRES of an active query:
 *   d = step / (double)prec_z
 *   for i = -below .. isotopes:
 *     c_i  = prec_mz + (double)i d
 *     w_i  = tol + (tol_ppm 1e-6) c_i
 *     lo_i = c_i - w_i,  hi_i = c_i + w_i
 * THE PEAKS: peak (x, y) of the survey spectrum, in index order, is
 *   INSIDE    iff win_lo <= x && x <= win_hi
 *   ELIGIBLE  iff inside and y > 0.0
 *   PRECURSOR iff eligible and lo_i <= x && x <= hi_i for some i.
 * A centre outside the isolation window gets nothing; a peak in two centre windows counts once.
 * THE RECORD: window is the sum of y over the eligible peaks and precursor the sum of y over the precursor peaks, each
 * SEQUENTIAL from 0.0 in index order -- the two sums have ONE defined order, the survey spectrum's own.  other_mz /
 * other_intensity: the most intense eligible peak that is no precursor peak; the larger y wins, then the smaller x -- total up
 * to equal (x, y) --, stored + 0.0, and 0.0 / 0.0 when there is none.  n_window and n_precursor count the eligible and the
 * precursor peaks; bit i + below of iso_hit is set iff centre i holds an eligible peak; flags is PYA_PURITY_ACTIVE, with
 * PYA_PURITY_SEEN iff n_precursor > 0.  The ratio is not stored: precursor / window where window > 0.  Every record of a call
 * is written.
 * The parameters must satisfy: tol and tol_ppm finite and >= 0; step finite and > 0; below 0 .. 4;
 * n_c = below + 1 + isotopes in 1 .. PYA_PURITY_MAX_CENTRES; reserved == 0.  The defaults of the Python layer (tol 0, tol_ppm
 * 10, isotopes 3, below 0, step PYA_STRIP_STEP) are choices, not measurements.
 * THE GATE (pya_purity_gate): threshold finite in [0, 1], keep_unknown 0 or 1.  Row r is KNOWN iff its record is ACTIVE and
 * window > 0.0.  It PASSES iff known ? precursor >= threshold window : keep_unknown -- one multiplication, no division.
 * select[r] = 1 / 0; in the matrix a passing row's readings have their bits copied and a failing row's readings become the NaN
 * pya_marker_values writes for "no reading" (0x7ff8000000000000). */
#define PYA_PURITY_MAX_CENTRES 16
#define PYA_PURITY_MAX_BELOW 4
typedef struct pya_purity_params {     /* 40 bytes */
    double tol;                                    /* half width of a centre's window in m/z (Da); finite, >= 0              */
    double tol_ppm;                                /* and in ppm of the centre, added to it; finite, >= 0                    */
    double step;                                   /* the isotope spacing at charge 1 (PYA_STRIP_STEP); finite, > 0          */
    uint32_t below;                                /* isotope positions under the selected m/z, 0 .. PYA_PURITY_MAX_BELOW    */
    uint32_t isotopes;                             /* positions above it; below + 1 + isotopes <= PYA_PURITY_MAX_CENTRES     */
    uint32_t reserved[2];                          /* 0                                                                      */
} pya_purity_params;
typedef struct pya_purity {            /* 48 bytes per query */
    double window;                                 /* sum of y over the eligible peaks, in index order                       */
    double precursor;                              /* sum of y over the precursor peaks, in index order                      */
    double other_mz, other_intensity;              /* the most intense eligible peak that is no precursor peak; 0.0 / 0.0    */
    uint32_t n_window, n_precursor;                /* eligible peaks; precursor peaks                                        */
    uint32_t iso_hit;                              /* bit i + below: centre i holds an eligible peak                         */
    uint32_t flags;                                /* PYA_PURITY_ACTIVE; PYA_PURITY_SEEN iff n_precursor > 0                 */
} pya_purity;
#define PYA_PURITY_ACTIVE 1u
#define PYA_PURITY_SEEN 2u

/* Precursor XIC: the MS1 intensity of an identified precursor for LABEL-FREE quantification -- the area, the apex and the sum
 * of its extracted ion chromatogram over the survey scans around the identification, what a search engine or MaxQuant reports
 * per PSM.  A READ-ONLY stage over the survey spectra beside the purity stage: records out, no workspace, and no kernel of a
 * run knows of it.  The reference has no counterpart.  Positional phospho-isomers share a precursor m/z and elute a few scans
 * apart: a trace that is not split at the valley between them credits each isomer's PSMs with both peaks, so the peak rule
 * has a valley split.
 * THE RULE.  n_survey survey spectra (pya_typed_spectra + int64 offsets, float32 widened at the load), rt[n_survey] (double,
 * seconds; not checked, its arithmetic is taken as it is), scan_ok[n_survey] (uint8, what pya_xic_survey_check writes: 1 iff
 * x[j] <= x[j + 1] for every adjacent pair of the scan's m/z -- a NaN among two or more fails, 0 or 1 peaks pass) and n_query
 * queries, one per MS2 spectrum: seed[q], scan_lo[q], scan_hi[q] (int64 indices into the survey list; the window is
 * [scan_lo, scan_hi)), prec_mz[q] (double), prec_z[q] (int32).  All arithmetic is in double, every operation rounded on its
 * own, in the order written; a comparison with a NaN is false.
 * SILENT: seed < 0.  The record is all zero bytes and nothing is read.
 * ACTIVE iff 0 <= scan_lo <= seed < scan_hi <= n_survey, scan_hi - scan_lo <= PYA_XIC_MAX_SCANS, prec_z in
 * 1 .. PYA_STRIP_MAX_CHARGE and prec_mz finite and > 0.  A query that is not active has an all-zero record.  One with
 * seed >= 0 that fails the first two conditions (the RANGE) is counted in d_over[0], the smallest such q in d_over[1] as
 * 0xffffffff - q, as purity reports a survey index beyond the spectra.  An active query one of whose scans had its offsets
 * clipped to the elements the arrays hold is reported the same way; its record is that of the clipped peaks.
 * THE TRACE of scan s of the window, for i = 0 .. isotopes:
 *   d    = step / (double)prec_z
 *   c_i  = prec_mz + (double)i d
 *   w_i  = tol + (tol_ppm 1e-6) c_i
 *   lo_i = c_i - w_i,  hi_i = c_i + w_i
 *   p_i[s] = the largest y among ALL peaks (x, y) of scan s with lo_i <= x && x <= hi_i && y > 0.0, +0.0 when there is none
 * -- a maximum over a set: order-free, no tie rule; a NaN x or y never qualifies; an infinite y takes part as arithmetic has
 * it.  A scan with scan_ok[s] == 0 has no peaks for this purpose, and the record of an active query with such a scan in its
 * window gets PYA_XIC_UNSORTED.
 *   present[s] iff p_0[s] > 0.0
 *   t[s] = p_0[s], then t = t + p_i[s] for i = 1 .. isotopes ascending; +0.0 where s is not present.
 * START: a0 = seed if present, else the nearest present scan with |s - seed| <= max_gap + 1, the earlier one on a tie.  None:
 * the record is ACTIVE without SEEN -- flags (ACTIVE, UNSORTED where it applies) and n_present are filled, the rest is zero.
 * REGION [r_lo, r_hi]: the largest interval around a0 inside the window with no run of more than max_gap consecutive absent
 * scans in it and both ends present.  Absent scans inside it are skipped by everything below.
 * VALLEYS, on the present scans v != a0 of the region.  L[v]: the largest t from a0 to v inclusive.  F[v]: the largest t
 * strictly beyond v, away from a0, inside the region.  n(v): the next present scan beyond v.  v is a VALLEY iff n(v) exists,
 * t[v] <= t[n(v)], rise t[v] < L[v] and rise t[v] < F[v] (one rounded product).  e_r: the smallest valley above a0, else
 * r_hi; e_l: the largest valley below a0, else r_lo.  A valley scan belongs to both neighbouring peaks.
 * THE PEAK, over the present scans of [e_l, e_r] ascending: apex the largest t, the smaller scan on a tie;
 *   sum:  S = +0.0; S = S + t[u]
 *   area: A = +0.0; for consecutive present scans u < v: A = A + (0.5 (t[u] + t[v])) (rt[v] - rt[u])
 * each operation rounded, no contraction -- ONE defined order, the scans'.  (A NaN that the rt arithmetic makes is stored as
 * the device makes it; its sign and payload are not part of the rule.)
 * THE RECORD: seed_intensity is t[seed]; the four scans are absolute survey indices; n_points the present scans of the peak,
 * n_present those of the window; bit i of iso_hit iff p_i[apex] > 0.  Flags: ACTIVE, SEEN (a start was found), SEED_PRESENT,
 * LEFT_VALLEY / RIGHT_VALLEY (the bound is a valley), LEFT_OPEN iff e_l == scan_lo and it is no valley, RIGHT_OPEN iff
 * e_r == scan_hi - 1 and it is no valley: the peak may go on outside the window.  No -0.0 reaches a record.
 * By hand: rt = 0, 1, 2, ..; one peak per scan with intensities 10 100 300 100 20 150 400 150 10; rise 2, isotopes 0, window
 * [0, 9).  Seed 2: the peak [0, 4], apex scan 2, RIGHT_VALLEY | LEFT_OPEN, area 515.0, sum 530.0.  Seed 6: the peak [4, 8],
 * apex scan 6, LEFT_VALLEY | RIGHT_OPEN, area 715.0.
 * The parameters must satisfy: tol and tol_ppm finite and >= 0; step finite and > 0; rise finite and >= 1; isotopes 0 ..
 * PYA_XIC_MAX_ISOTOPES; max_gap 0 .. PYA_XIC_MAX_GAP.  The defaults of the Python layer (tol 0, tol_ppm 10, isotopes 2, step
 * PYA_STRIP_STEP, rise 2, max_gap 1) are choices, not measurements.
 * KNOWN WEAKNESS of the valley rule: a noise dip on a slope that faces a second, higher peak is a valley, and cuts early. */
#define PYA_XIC_MAX_SCANS 64
#define PYA_XIC_MAX_ISOTOPES 3
#define PYA_XIC_MAX_GAP 8
typedef struct pya_xic_params {        /* 40 bytes */
    double tol;                                    /* half width of an isotope's window in m/z (Da); finite, >= 0            */
    double tol_ppm;                                /* and in ppm of its centre, added to it; finite, >= 0                    */
    double step;                                   /* the isotope spacing at charge 1 (PYA_STRIP_STEP); finite, > 0          */
    double rise;                                   /* a valley lies below 1 / rise of the maxima on both sides; finite, >= 1 */
    uint32_t isotopes;                             /* isotope positions above the selected m/z, 0 .. PYA_XIC_MAX_ISOTOPES    */
    uint32_t max_gap;                              /* absent scans a trace may bridge, 0 .. PYA_XIC_MAX_GAP                  */
} pya_xic_params;
typedef struct pya_xic {               /* 64 bytes per query */
    double area;                                   /* trapezoids over the present scans of the peak, in scan order           */
    double apex_intensity;                         /* the largest t of the peak                                              */
    double seed_intensity;                         /* t[seed]; 0.0 where the seed scan is absent                             */
    double sum_intensity;                          /* t summed over the present scans of the peak, in scan order             */
    uint32_t apex_scan, left_scan, right_scan;     /* apex, e_l and e_r as survey indices                                    */
    uint32_t start_scan;                           /* a0 as a survey index                                                   */
    uint32_t n_points, n_present;                  /* present scans of the peak; of the window                               */
    uint32_t iso_hit;                              /* bit i: isotope i held a peak in the apex scan                          */
    uint32_t flags;                                /* PYA_XIC_*                                                              */
} pya_xic;
#define PYA_XIC_ACTIVE 1u
#define PYA_XIC_SEEN 2u
#define PYA_XIC_SEED_PRESENT 4u
#define PYA_XIC_LEFT_VALLEY 8u
#define PYA_XIC_RIGHT_VALLEY 16u
#define PYA_XIC_UNSORTED 32u
#define PYA_XIC_LEFT_OPEN 64u
#define PYA_XIC_RIGHT_OPEN 128u
#define PYA_XIC_AREA 0u                /* `which` of pya_xic_values */
#define PYA_XIC_APEX 1u
#define PYA_XIC_SEED 2u
#define PYA_XIC_SUM 3u

/* Centroiding (peak picking): the first of the transforms in front of a run.  Everything behind it -- the top-N-per-100-m/z
 * binning, the match window, deisotoping's tol, the strip windows -- takes one (m/z, intensity) pair for one peak.  A
 * profile-mode spectrum (msconvert without a peak-picking filter, older QTOF exports, "profile MS2" methods) has 10 to 20
 * samples per peak: the ranks of a window fill with the flanks of its tallest peaks and every flank sample is one more target
 * for a random match.  Like deisotoping a transform of spectra in front of a plan (the peak counts change); no kernel of a run
 * knows of it.  The reference has no counterpart.
 * THE RULE.  Every spectrum is handled on its own.  x[] is its m/z and y[] its intensities (float32 is widened at the load);
 * all arithmetic is in double, every operation rounded on its own, in the order written; a comparison with a NaN is false.
 * CONNECTED: points k - 1 and k are connected iff
 *   g = x[k] - x[k - 1],  lim = gap0 + gap_per_mz x[k - 1],  g <= lim
 * APEX: point i is an apex iff y[i] > 0 and y[i] >= min_height, and it has no connected left neighbour or y[i - 1] < y[i], and
 * it has no connected right neighbour or y[i + 1] <= y[i].  So the first point of a plateau is the apex; a NaN intensity is no
 * apex and lets neither connected neighbour be one.  Two apexes are never adjacent and connected.
 * FOOTPRINT [l, r] of apex i: l is the smallest index >= i - half_width such that every step k - 1 -> k, l < k <= i, is
 * connected and has y[k - 1] < y[k]; r is the largest index <= i + half_width such that every step k -> k + 1, i <= k < r, is
 * connected and has y[k + 1] <= y[k].  The two comparisons are the apex test's own: a run of equal intensities belongs to the
 * peak on its LEFT, as a plateau belongs to its first point.  (With <= on both sides the footprints of two neighbours would
 * share every point of a flat valley, y = 3 1 1 3, and the bound below would not hold.)  A valley point may lie in both
 * neighbours' footprints: it is then r of the left one and l of the right one, and is added to both.
 * CENTROID, sequentially for k = l .. r, from sw = 0, s = 0:
 *   sw = sw + y[k],  d = x[k] - x[i],  p = d y[k],  s = s + p
 * then
 *   q = s / sw,  c = x[i] + q,  c = (c >= x[l]) ? c : x[l],  c = (c <= x[r]) ? c : x[r]
 * (so a NaN becomes x[l]), and c is rounded once to the m/z element type.  When l == r the bits of x[i] are copied instead
 * (c is x[i] but for the sign of a zero).  The output intensity is y[i] with its bits copied when area == 0, and sw rounded
 * once to the intensity element type when area == 1.
 * OUTPUT: one pair per apex, in index order.  It is ascending (not strictly) whenever the input is.  Proof: let i < j be
 * consecutive apexes with footprints [l_i, r_i] and [l_j, r_j].  (1) r_i < j: otherwise the step j - 1 -> j is one of i's right
 * flank, connected with y[j] <= y[j - 1], and j with a connected left neighbour needs y[j - 1] < y[j].  (2) r_i <= l_j:
 * otherwise k = l_j + 1 <= r_i < j, and the step k - 1 -> k lies in i's right flank (y[k] <= y[k - 1]) and in j's left flank
 * (y[k - 1] < y[k]).  (3) The two selects leave x[l] <= c <= x[r] whatever q is (x[l] <= x[r]: the input ascends), and x[l], x[r]
 * are values of the element type, so rounding, which is monotone, keeps c inside.  Hence c_i <= x[r_i] <= x[l_j] <= c_j.
 * PASS-THROUGH: a spectrum in which no two adjacent points are connected comes out as its points with y > 0 && y >= min_height,
 * every byte copied (l == r everywhere).  So an already centroided spectrum survives the transform, and with min_height == 0
 * and positive intensities it is unchanged.
 * A spectrum that is NOT ASCENDING in pya_deisotope_params' sense is copied unchanged and reported.
 * SELECT: an optional byte per spectrum; a spectrum whose byte is 0 is copied unchanged and is not reported.
 * The parameters must satisfy: gap0 and gap_per_mz finite, >= 0 and not both 0; min_height finite and >= 0; half_width in
 * 1 .. PYA_CENTROID_MAX_HALF_WIDTH; area 0 or 1; reserved == 0. */
#define PYA_CENTROID_MAX_HALF_WIDTH 8
typedef struct pya_centroid_params {   /* 40 bytes */
    double gap0, gap_per_mz;                /* two adjacent points are of one peak iff they are at most gap0 + gap_per_mz x apart */
    double min_height;                      /* an apex is at least this intense (and above 0)                                 */
    uint32_t half_width;                    /* points on either side of the apex a centroid may take in, 1 .. 8              */
    uint32_t area;                          /* 0: the output intensity is the apex's; 1: the sum over the footprint          */
    uint64_t reserved;                      /* 0                                                                             */
} pya_centroid_params;

/* Ranked localisations.  The site table holds the winner and the runner-up of a PSM, the probabilities a sum over all of its
 * site assignments; this is the list itself: the K best site assignments by PepScore, in order -- the positional isomers a
 * report lists (LuciPHOr-style top-two permutations, MaxQuant-style score differences over all isoforms), "everything within
 * 3 PepScore units of the winner", "how many assignments tie the best score".  The reference has no counterpart but a sort
 * of its pep_scores records.  The stage writes K records per PSM at a fixed stride, out[psm * K + r], r = 0 .. K - 1,
 * 1 <= K <= PYA_MAX_RANKED.  For a scored PSM with n_sig site assignments the rows 0 .. min(n_sig, K) - 1 hold:
 *   row 0        the reported localisation: sig_bits == best_sig, pep_score has the bits of best_score.  It is the
 *                reference's winner with the reference's own tie-break and is not decided again here.
 *   rows 1 ..    every OTHER site assignment by PepScore descending, compared as float32; equal floats by numerically
 *                ascending sig_bits.  The rule does not depend on the reference's std::sort order, on the route that scored
 *                the PSM, on chunk cuts, on batch neighbours or on K: for K' < K the K' list is bytewise the prefix of the K
 *                list, and no field says "last row" or anything else that depends on K.
 * No assignment scores above best_score.  Every pep_score is bit-equal to ScoreContainer.weighted_score of the record with
 * the same sig bits from a PYA_FLAG_KEEP batch.  n_of_mod == 0 is one assignment with sig 0 and n_of_mod == n_sites one with
 * every site: row 0 only.  kind:
 *   PYA_RANK_NONE    the PSM was not scored (set aside, status != 0, n_sig <= 0), or the row is at or beyond n_sig: all 16
 *                    bytes 0;
 *   PYA_RANK_OVER    n_sig is above the sig_cap of the call (as for pya_plan_sites; 0: no cap): row 0 only, with best_sig,
 *                    best_score and the kind (flags 0), the rows behind it zero;
 *   PYA_RANK_SCORED  otherwise.  flags: PYA_RANK_TIED_PREV the pep_score is float-equal to the row above's,
 *                    PYA_RANK_IN_BEST_TIE it is float-equal to best_score (row 0 carries it too). */
#define PYA_MAX_RANKED 64
#define PYA_RANK_NONE 0
#define PYA_RANK_SCORED 1
#define PYA_RANK_OVER 2
#define PYA_RANK_TIED_PREV 1
#define PYA_RANK_IN_BEST_TIE 2
typedef struct pya_ranked {        /* 16 bytes, one store; records compare as raw bytes */
    uint64_t sig_bits;             /* the site assignment: bit j = the j-th modifiable residue is modified    */
    float pep_score;               /* its PepScore                                                            */
    uint16_t rank;                 /* = r, the row                                                            */
    uint8_t kind;                  /* PYA_RANK_NONE / _SCORED / _OVER                                         */
    uint8_t flags;                 /* PYA_RANK_TIED_PREV | PYA_RANK_IN_BEST_TIE                               */
} pya_ranked;

typedef struct pya_handle pya_handle;
typedef struct pya_plan pya_plan;

typedef struct pya_config {
    float bin_size;             /* m/z width of a peak window                            */
    uint32_t n_top;             /* peaks retained per window = depths scored: 10..16     */
    const char *mod_group;      /* e.g. "STY"; 'n' / 'c' allow the termini               */
    float mod_mass;
    float mz_error;             /* Da                                                    */
    const char *fragment_types; /* subset of "bycz Z", e.g. "by"                         */
    int32_t device;             /* HIP device ordinal                                    */
} pya_config;

/* host-side CSR description of a batch of PSMs (all arrays borrowed) */
typedef struct pya_batch {
    uint64_t n_psm;
    const int64_t *peak_off;    /* [n_psm+1] offsets into mz / intensity                 */
    const uint8_t *pep;         /* peptide letters of all PSMs, back to back             */
    const int64_t *pep_off;     /* [n_psm+1]                                             */
    const int32_t *n_of_mod;    /* [n_psm] unlocalised modifications                     */
    const int32_t *max_charge;  /* [n_psm] max fragment charge (>= 1)                    */
    const uint32_t *aux_pos;    /* fixed mods: 0 = n-term, else 1-based position; or NULL */
    const float *aux_mass;
    const int64_t *aux_off;     /* [n_psm+1] or NULL                                     */
} pya_batch;

/* caller-allocated structure-of-arrays results; host pointers for pya_score_batch,
 * device pointers for pya_plan_run */
typedef struct pya_results {
    uint32_t max_k;             /* row stride of ascores / alt_mask (>= max n_of_mod)    */
    float *best_score;          /* [n_psm]  PepScore of the best localisation, -1 if none */
    uint64_t *best_sig;         /* [n_psm]  sig bits of the best localisation            */
    int32_t *n_sig;             /* [n_psm]  number of localisations scored               */
    float *ascores;             /* [n_psm * max_k]  +inf where unambiguous               */
    uint64_t *alt_mask;         /* [n_psm * max_k] alternative sites of every modified site: bit p = residue p of the
                                 * peptide (0-based) for peptides of up to 64 residues; for longer ones (general
                                 * kernel) bit j = the j-th modifiable residue (pya_count_sites gives its position) */
} pya_results;

int pya_create(const pya_config *cfg, pya_handle **out);
void pya_destroy(pya_handle *h);
/* PyAscore.add_neutral_loss.  Changes what every later call scores under -- and ENDS THE LAUNCHING LIFE of every plan the
 * handle has made so far, the retained batch of a PYA_FLAG_KEEP call included (see pya_plan_create): the handle's settings
 * generation goes up with every call, a repeated identical one and one that fails with PYA_ERR_LIMIT too.  Results already
 * produced stay readable (pya_get_pep_scores*, pya_plan_check, the timing ring): they are those of the old settings. */
int pya_add_neutral_loss(pya_handle *h, const char *group, float mass);
/* PyAscore.score for ONE PSM with the lowest latency (Ascore.pyx:103-152; the reference's own command line
 * calls it once per PSM, pyascore/__main__.py:129-164): no plan, no copies -- the spectrum is staged in pinned
 * host memory the device reads directly, the PSM's scalars travel in the kernel's arguments, one wavefront runs
 * the whole path and writes the results straight back into pinned host memory.  Results as row 0 of `out`
 * (out->max_k <= 64).  flags: PYA_FLAG_KEEP retains the per-signature records at once; without it
 * pya_rescore_last_keep() retains them on demand (the properties only a few callers read).  PYA_FLAG_EVIDENCE and
 * PYA_FLAG_IONS are refused with PYA_ERR_ARG: those records come from the batch path (a batch of one with the flag).  Returns
 * PYA_ERR_STATE without an error message when the PSM needs the batch path (more than 8 fixed
 * modifications): call pya_score_batch then. */
int pya_score_one(pya_handle *h, const double *mz, const double *intensity, uint64_t n_peaks, const uint8_t *peptide,
                  uint64_t peptide_len, int32_t n_of_mod, int32_t max_fragment_charge, const uint32_t *aux_pos,
                  const float *aux_mass, uint64_t n_aux, uint32_t flags, const pya_results *out);
int pya_rescore_last_keep(pya_handle *h);

/* The environment reaches a handle through four variables, read once in pya_create: PYA_WORKSPACE_MB and
 * PYA_CHUNK_MB (sizes of pya_score_batch's device budget and chunks), PYA_HOST_TIMING and PYA_STAMPS (diagnostics that
 * change no result and no route).  This re-reads them and puts every debug switch (include/pyascore_debug.h) back to
 * its production default.  No reference counterpart. */
int pya_reload_env(pya_handle *h);
/* diagnostics: average microseconds per pya_score_one call since the last call of this function, by stage (checks
 * and tables, spectrum into the pinned block, launch, wait for the kernel, results out); us[5] = calls averaged;
 * us[6..9] = inside the kernel by its own clock (scalars into place, binning, scoring, the rest), us[10] = the
 * kernel's shader clock cycles */
int pya_one_times(pya_handle *h, double us[12]);

const char *pya_last_error(const pya_handle *h);
int64_t pya_error_index(const pya_handle *h);

/* host buffers in, host buffers out: H2D copy + kernels + D2H copy, synchronous (big batches are
 * chunked and pipelined, see pya_set_workspace_budget; a PYA_FLAG_KEEP batch is always one plan) */
int pya_score_batch(pya_handle *h, const pya_batch *batch, const double *mz,
                    const double *intensity, uint32_t flags, const pya_results *out);

/* Several PSMs against one spectrum -- the reference's command line groups the identifications by scan and scores the first
 * --hit_depth of every group against the scan's spectrum (pyascore/__main__.py, the groupby(psms, scan) loop); ranked hits of
 * a search engine and co-isolated peptides of a chimeric spectrum are the same case.  pya_score_batch with
 *   - batch->peak_off of n_spectra + 1 entries: it describes the SPECTRA (mz / intensity hold every spectrum once),
 *   - spec_of[i] = the spectrum of PSM i, 0 <= spec_of[i] < n_spectra, NON-DECREASING in i: the PSMs of a spectrum are
 *     consecutive.
 * Every spectrum is uploaded and binned once, and its retained peaks are held once.  The binning depends on the peaks and
 * the scorer's bin_size / n_top alone (cpp/Spectra.cpp:43-68), so every result is bit-equal to what pya_score_batch gives
 * for the same PSMs with the spectrum repeated, whatever the cut into chunks.
 *   - spec_of out of range or decreasing, or n_spectra == 0 with PSMs present: PYA_ERR_ARG, the message names the PSM;
 *   - a spectrum no PSM refers to is legal: it is uploaded with the rest and neither binned nor given workspace;
 *   - what belongs to the spectrum (empty, more than PYA_MAX_PEAKS peaks, PYA_PSM_NO_WINDOWS, PYA_PSM_TOO_MANY_WINDOWS)
 *     hits EVERY PSM of that spectrum with the code the repeated-spectrum batch gives it; an invalid peptide hits its own
 *     PSM only, its siblings are scored.  Flags as for pya_score_batch; pya_last_batch_status, pya_get_pep_scores* and
 *     pya_calculate_ambiguity go by PSM number. */
int pya_score_batch_shared(pya_handle *h, const pya_batch *batch, const uint32_t *spec_of, uint64_t n_spectra,
                           const double *mz, const double *intensity, uint32_t flags, const pya_results *out);

/* Typed spectra (no reference counterpart -- the reference's one entry point, PyAscore.score, takes two float64 buffers
 * and raises on anything else, Ascore.pyx:103; pya_score_one / PyAscore.score keep that contract).  The batch entry points
 * take the arrays in the precision their source holds them in: mzML as msconvert writes it has 64-bit m/z and 32-bit
 * intensities, mzXML 32-bit pairs, and widening them on the host only adds bytes to the PCIe copy that bounds
 * pya_score_batch.  float32 -> float64 is exact and the binning kernels widen every value where they load it, so the
 * results are bit-equal to those of the same arrays widened by the caller and sent through pya_score_batch /
 * pya_score_batch_shared / pya_plan_run; no widened copy is made on the host or on the device.
 *   (mz_type, intensity_type) = (PYA_F64, PYA_F64): 16 bytes per peak, behaves as the float64 entry points (which are
 *                                                   thin wrappers of these two);
 *                               (PYA_F64, PYA_F32): 12 bytes per peak;
 *                               (PYA_F32, PYA_F32):  8 bytes per peak;
 *                               (PYA_F32, PYA_F64): REFUSED with PYA_ERR_ARG and a message (no file format stores it);
 *   any other type value: PYA_ERR_ARG.
 * (The struct is not called pya_spectra: that is pyascore_aux.h's PyBinnedSpectra counterpart.) */
#define PYA_F64 0u
#define PYA_F32 1u
typedef struct pya_typed_spectra {  /* host pointers for pya_score_batch_typed, device pointers for pya_plan_run_typed */
    const void *mz, *intensity;
    uint32_t mz_type, intensity_type;   /* PYA_F64 / PYA_F32 */
} pya_typed_spectra;
/* pya_score_batch (spec_of == NULL; n_spectra is ignored) or pya_score_batch_shared (spec_of != NULL) for typed arrays:
 * same validation, messages, per-PSM status codes, flags and retained records (PYA_FLAG_KEEP).  Upload ring, chunk cuts
 * (PYA_CHUNK_MB, the workspace budget) and the spectra in the plan's arena count the arrays' real bytes.  A batch of one PSM
 * takes pya_score_one's low-latency kernel only when both arrays are float64. */
int pya_score_batch_typed(pya_handle *h, const pya_batch *batch, const uint32_t *spec_of, uint64_t n_spectra,
                          const pya_typed_spectra *spectra, uint32_t flags, const pya_results *out);

/* pya_score_batch_typed with named localisations (pya_named above): the queries q_off[n_psm + 1] / q_bits[q_off[n_psm]] in, one
 * record per query out in named_out[q_off[n_psm]], and, where not NULL, the containers' cumulative counts and depth scores in
 * counts / scores [q_off[n_psm] * n_top], laid out like pya_get_pep_scores.  spec_of NULL: private spectra.  Every flag of
 * pya_score_batch keeps its meaning, and pya_results, status, evidence and ions are byte for byte what the call without
 * queries gives.  The stage (csrc/named.hip) runs behind the kernels of every chunk with that chunk's slice of the queries
 * and its records come back behind the chunk's results; they do not depend on the cut into chunks, on the route a PSM took
 * or on shared / typed input.  A batch of one or a handful takes the plan's launches.  The PSMs PYA_FLAG_SKIP_INVALID sets
 * aside have PYA_NAMED_NONE records.  q_off[0] != 0 or a decreasing q_off: PYA_ERR_ARG, the message names the PSM; a
 * malformed signature is a PYA_NAMED_INVALID record, never an error.  (PyAscore.pep_scores, PyAscore.calculate_ambiguity:
 * Ascore.pyx:208-252.) */
int pya_score_batch_named(pya_handle *h, const pya_batch *batch, const uint32_t *spec_of, uint64_t n_spectra,
                          const pya_typed_spectra *spectra, uint32_t flags, const pya_results *out, const int64_t *q_off,
                          const uint64_t *q_bits, pya_named *named_out, int32_t *counts, float *scores);

/* Device memory one pya_score_batch call may hold at a time (upload ring + workspace; default 6 GiB,
 * or PYA_WORKSPACE_MB).  Calls that need more -- and every call with more than 32 MB of spectra -- are
 * cut into chunks of consecutive PSMs and pipelined: the upload of chunk c + 1 runs under the kernels
 * and the result copy of chunk c.  Results do not depend on the cut.  (pya_score_batch_shared: a chunk holds each of its
 * spectra once; a group of PSMs bigger than a chunk is cut, its spectrum then travels with both parts.) */
int pya_set_workspace_budget(pya_handle *h, uint64_t bytes);
/* the budget in force (the value set, PYA_WORKSPACE_MB, or the default of 6 GiB) */
uint64_t pya_get_workspace_budget(const pya_handle *h);

/* per-PSM status codes (PYA_PSM_*) of the last pya_score_batch call on this handle; n must equal
 * that batch's n_psm.  All zeros unless PYA_FLAG_SKIP_INVALID let PSMs be set aside. */
int pya_last_batch_status(pya_handle *h, int32_t *status, uint64_t n);

/* The evidence records of the last pya_score_batch / _shared / _typed call on this handle that was given
 * PYA_FLAG_EVIDENCE: out[n_psm * max_k], n_psm and max_k as in that call (anything else: PYA_ERR_ARG).  PYA_ERR_STATE when
 * the last batch was scored without the flag.  The rows of a PSM that was set aside (PYA_FLAG_SKIP_INVALID) are all zero;
 * rows do not depend on how the batch was cut into chunks.  What it answers for in the reference: see pya_evidence. */
int pya_last_batch_evidence(pya_handle *h, pya_evidence *out, uint64_t n_psm, uint32_t max_k);

/* The ion records (pya_ion above) of the last pya_score_batch / _shared / _typed call on this handle that was given
 * PYA_FLAG_IONS, with the size-query convention of pya_get_pep_scores_range: ion_off[n_psm + 1] always (n_psm of that
 * batch; ion_off[n_psm] = the number of records), the records when cap is not 0 -- cap below that number: PYA_ERR_ARG.
 * PYA_ERR_STATE when the last batch was scored without the flag.  The records do not depend on how the batch was cut into
 * chunks.  The flag makes the library compute the evidence rows it needs; pya_last_batch_evidence still answers only when
 * PYA_FLAG_EVIDENCE was given. */
int pya_last_batch_ions(pya_handle *h, int64_t *ion_off, pya_ion *out, uint64_t cap);

/* The site records (pya_site above) of the last pya_score_batch / _shared / _typed / _named call on this handle that was
 * given PYA_FLAG_SITES, with the size-query convention of pya_last_batch_ions: site_off[n_psm + 1] always (site_off[n_psm]
 * = the number of records), the records when cap is not 0 -- cap below that number: PYA_ERR_ARG.  PYA_ERR_STATE when the
 * last batch was scored without the flag.  The records do not depend on the route that scored a PSM, on how the batch was
 * cut into chunks, or on shared / typed input. */
int pya_last_batch_sites(pya_handle *h, int64_t *site_off, pya_site *out, uint64_t cap);
/* The most site assignments of a PSM the site stage of a batch call enumerates (PYA_SITE_OVER above it); 0: no cap.  The
 * general kernel takes up to PYA_MAX_SIGNATURES per PSM, and the stage scores every one of them a second time.  The default
 * is PYA_FAST_SIGNATURES. */
int pya_set_site_sig_cap(pya_handle *h, uint32_t sig_cap);
uint32_t pya_get_site_sig_cap(const pya_handle *h);
/* The site probabilities (pya_site_prob / pya_psm_prob above) of the last pya_score_batch / _shared / _typed / _named call on
 * this handle that was given PYA_FLAG_PROBS, with the size-query convention of pya_last_batch_sites: site_off[n_psm + 1]
 * always (the offsets of the site table), sites[site_off[n_psm]] and psms[n_psm] when cap is not 0 -- cap below
 * site_off[n_psm]: PYA_ERR_ARG, as is a NULL array then.  PYA_ERR_STATE when the last batch was scored without the flag.  A
 * PSM that was set aside has an empty range and a PYA_SITE_NONE record.  The cap on site assignments per PSM is
 * pya_set_site_sig_cap's.  The records do not depend on the route that scored a PSM, on how the batch was cut into chunks,
 * or on shared / typed input. */
int pya_last_batch_probs(pya_handle *h, int64_t *site_off, pya_site_prob *sites, pya_psm_prob *psms, uint64_t cap);
/* The ranked localisations (pya_ranked above) of the last pya_score_batch / _shared / _typed / _named call on this handle
 * that was given PYA_FLAG_RANKED: out[n_psm * top_k], the rows of PSM i at out[i * top_k].  n_psm and top_k must be those of
 * the call (top_k: what pya_get_ranked_k returned when it was made), anything else is PYA_ERR_ARG, as is a NULL array for a
 * batch that has PSMs.  PYA_ERR_STATE when the last batch was scored without the flag.  A PSM that was set aside has
 * PYA_RANK_NONE rows.  The cap on site assignments per PSM is pya_set_site_sig_cap's.  The records do not depend on the route
 * that scored a PSM, on how the batch was cut into chunks, or on shared / typed input. */
int pya_last_batch_ranked(pya_handle *h, pya_ranked *out, uint64_t n_psm, uint32_t top_k);
/* The list length K of the batch calls with PYA_FLAG_RANKED (the counterpart of pya_set_site_sig_cap; pya_plan_ranked takes
 * its own): 1 .. PYA_MAX_RANKED, anything else is PYA_ERR_ARG and changes nothing.  The default is 5. */
int pya_set_ranked_k(pya_handle *h, uint32_t top_k);
uint32_t pya_get_ranked_k(const pya_handle *h);
/* Lends the library what the NEXT pya_score_batch / _shared / _typed / _named call with PYA_FLAG_ROLLUP rolls its PSMs into
 * (pya_site_rollup above): slot[n_records], host memory that must stay valid until that call returns -- one entry per
 * residue record of the batch in the records' order, n_records = the batch's site_off[n_psm] (what pya_last_batch_probs or
 * pya_plan_site_offsets report: the modifiable residues of every PSM that is not set aside, summed); n_slots, the size of
 * the table; threshold, the "confident" cut of n_confident (e.g. 0.75); psm_id[n_psm] or NULL: PSM i of the batch is known as
 * i.  The batch call computes the probability records for itself (pya_last_batch_probs still answers only with
 * PYA_FLAG_PROBS; the cap is pya_set_site_sig_cap's), uploads a chunk's slice of slot and psm_id with the chunk and runs the
 * stage behind every chunk's probability stage into one device table that lives for the call.  The loan ends with the first
 * batch call with the flag that gets as far as its PSMs, whatever that call returns.  A batch whose records are not n_records
 * (checked chunk by chunk BEFORE anything is read past the array, and at the end), or a flag without a loan: PYA_ERR_ARG with a
 * message; a slot at or above n_slots: PYA_ERR_LIMIT.
 * NULL slot with n_records != 0, or n_slots above 2^31 - 1: PYA_ERR_ARG. */
int pya_set_rollup(pya_handle *h, const int32_t *slot, uint64_t n_records, uint64_t n_slots, double threshold, const uint32_t *psm_id);
/* The table of the last batch call on this handle that was given PYA_FLAG_ROLLUP: out[n_slots], n_slots as lent
 * (anything else: PYA_ERR_ARG, as is a NULL array for a table that has slots).  PYA_ERR_STATE when the last batch was scored
 * without the flag. */
int pya_last_batch_rollup(pya_handle *h, pya_site_rollup *out, uint64_t n_slots);
/* Puts a DEVICE table of n_slots records into the empty state (best_psm = PYA_ROLLUP_NO_PSM, everything else 0), on
 * hip_stream, stream-ordered, no host synchronisation inside. */
int pya_rollup_clear(pya_handle *h, pya_site_rollup *d_table, uint64_t n_slots, void *hip_stream);

/* The device bytes pya_rollup_flr needs as its workspace for a table of n_slots (keys and payloads double-buffered, digit
 * histograms, tile sums: about 25 bytes per slot); 0 for an empty table. */
uint64_t pya_flr_workspace_bytes(uint64_t n_slots);
/* Site FLR (pya_site_flr above) of the DEVICE table d_table[n_slots]: d_out[n_slots] the records, d_order[n_slots] (or NULL)
 * the ranked slots in order, then the unranked ones by ascending index, d_n_ranked[2] the number of ranked slots and an error
 * word -- the number of class bytes that are none of 0, 1, 2 (such a slot is treated as left out).  d_cls[n_slots] or NULL;
 * flags: PYA_FLR_REPORTED_ONLY or 0.  Everything is stream-ordered on hip_stream: no host synchronisation and no allocation
 * inside, the caller lends d_work (work_bytes >= pya_flr_workspace_bytes(n_slots), 16-byte aligned as d_table and d_out are)
 * and reads the results after the stream reaches them.  The table is only read.  No write lies outside d_out[0 .. n_slots),
 * d_order[0 .. n_slots), d_n_ranked[0 .. 2) and d_work[0 .. pya_flr_workspace_bytes(n_slots)).  n_slots == 0 is valid and
 * launches nothing (d_n_ranked is zeroed).  PYA_ERR_ARG, with nothing launched: n_slots above 2^31 - 1, unknown flag bits, a
 * workspace that is too small, NULL or misaligned where an array is needed. */
int pya_rollup_flr(pya_handle *h, const pya_site_rollup *d_table, uint64_t n_slots, const uint8_t *d_cls, uint32_t flags, void *hip_stream,
                   void *d_work, uint64_t work_bytes, pya_site_flr *d_out, uint32_t *d_order, uint32_t *d_n_ranked);
/* The same for a HOST table (a table merged over several files, ...): uploads, runs pya_rollup_flr on the handle's stream
 * with a workspace of its own, downloads and checks the error word.  order may be NULL.  A class byte above 2: PYA_ERR_ARG
 * (pya_error_index names the slot), before anything is uploaded. */
int pya_rollup_flr_host(pya_handle *h, const pya_site_rollup *table, uint64_t n_slots, const uint8_t *cls, uint32_t flags, pya_site_flr *out,
                        uint32_t *order, uint32_t *n_ranked);

/* Lends the library what the NEXT batch call with PYA_FLAG_PEPTIDOFORMS lists its PSMs by (pya_peptidoform above):
 * group[n_psm] and psm_id[n_psm] (or NULL: PSM i of the batch is known as i), host memory that must stay valid until that
 * call returns; threshold, the "confident" cut of n_confident.  The lifetime rules are pya_set_rollup's: the loan ends with
 * the first batch call with the flag that gets as far as its PSMs, whatever it returns; a batch of another size or a flag
 * without a loan is PYA_ERR_ARG.  The batch call computes the probability records for itself and feeds every chunk's list
 * into the next chunk's call as d_prev.  NULL group with n_psm != 0, or n_psm above 2^31 - 1: PYA_ERR_ARG. */
int pya_set_peptidoforms(pya_handle *h, const int32_t *group, uint64_t n_psm, double threshold, const uint32_t *psm_id);
/* The list of the last batch call on this handle that was given PYA_FLAG_PEPTIDOFORMS: *n its length, the first
 * min(*n, cap) records into out (out may be NULL with cap == 0: the length alone).  PYA_ERR_STATE when the last batch was
 * scored without the flag. */
int pya_last_batch_peptidoforms(pya_handle *h, pya_peptidoform *out, uint64_t cap, uint64_t *n);
/* Lends the library what the NEXT batch call with PYA_FLAG_MZ_PROFILE profiles its PSMs into (pya_mz_profile above):
 * run[n_psm], one slot per PSM (negative: left out), or NULL: every PSM is of slot 0; host memory that must stay valid until
 * that call returns; n_slots, the size of the table; params, copied.  Lifetime and refusals are pya_set_peptidoforms's: the loan
 * ends with the first batch call with the flag that gets as far as its PSMs, a batch of another size or a flag without a loan
 * is PYA_ERR_ARG.  The batch call uploads a chunk's slice of run with the chunk and runs the stage behind every chunk into one
 * device table that lives for the call; it needs neither the probability nor the evidence stage.  A slot at or above n_slots:
 * PYA_ERR_LIMIT.  PYA_ERR_ARG: n_psm or n_slots above 2^31 - 1, NULL params, max_rank >= 16, an inv_* that is not finite and
 * positive. */
int pya_set_mz_profile(pya_handle *h, const int32_t *run, uint64_t n_psm, uint64_t n_slots, const pya_mz_profile_params *params);
/* The table of the last batch call on this handle that was given PYA_FLAG_MZ_PROFILE: out[n_slots], n_slots as lent (anything
 * else: PYA_ERR_ARG).  PYA_ERR_STATE when the last batch was scored without the flag. */
int pya_last_batch_mz_profile(pya_handle *h, pya_mz_profile *out, uint64_t n_slots);
/* Lends the library what the NEXT batch call with PYA_FLAG_QUANT quantifies its sites with (pya_site_quant above):
 * values[n_rows * params->n_channels] and row[n_psm] (or NULL: PSM i of the batch has row i), host memory that must stay valid
 * until that call returns; params, copied.  The slots and n_slots are those of the same call's PYA_FLAG_ROLLUP
 * (pya_set_rollup): the flag without PYA_FLAG_ROLLUP is PYA_ERR_ARG with a message.  Lifetime and refusals are
 * pya_set_mz_profile's: the loan ends with the first batch call with the flag that gets as far as its PSMs, a batch of another
 * size or a flag without a loan is PYA_ERR_ARG.  The batch call uploads the matrix once, a chunk's slice of row with the chunk,
 * and runs the stage behind every chunk's roll-up into one device table that lives for the call.  A row at or above n_rows:
 * PYA_ERR_LIMIT.  PYA_ERR_ARG: n_psm or n_rows above 2^31 - 1, NULL params, NULL values with n_rows != 0, scale_log2 outside
 * -64 .. 64, n_channels outside 1 .. 64, unknown flag bits, a threshold that is a NaN, reserved != 0. */
int pya_set_site_quant(pya_handle *h, const double *values, uint64_t n_rows, const int32_t *row, uint64_t n_psm,
                       const pya_site_quant_params *params);
/* The table of the last batch call on this handle that was given PYA_FLAG_QUANT: head[n_slots] and cell[n_slots * n_channels],
 * n_slots and n_channels as lent (anything else: PYA_ERR_ARG, as is a NULL array for a table that has slots).  PYA_ERR_STATE
 * when the last batch was scored without the flag. */
int pya_last_batch_site_quant(pya_handle *h, pya_site_quant_head *head, pya_site_quant *cell, uint64_t n_slots, uint32_t n_channels);
/* Lends the library what the NEXT batch call with PYA_FLAG_PFORM_QUANT quantifies its peptidoforms with (peptidoform
 * quantification above): values[n_rows * params->n_channels] and row[n_psm] (or NULL: PSM i of the batch has row i), host
 * memory that must stay valid until that call returns; params, copied.  The list is that of the same call's
 * PYA_FLAG_PEPTIDOFORMS (pya_set_peptidoforms): the flag without PYA_FLAG_PEPTIDOFORMS is PYA_ERR_ARG with a message.  Lifetime
 * and refusals are pya_set_site_quant's.  The batch call uploads the matrix once, a chunk's slice of row with the chunk, and
 * feeds every chunk's pair into the next chunk's call as the earlier list and table, as it does for the list alone; with the
 * flag pya_last_batch_peptidoforms returns exactly what it returns without it.  A row at or above n_rows: PYA_ERR_LIMIT. */
int pya_set_peptidoform_quant(pya_handle *h, const double *values, uint64_t n_rows, const int32_t *row, uint64_t n_psm,
                              const pya_site_quant_params *params);
/* The table of the last batch call on this handle that was given PYA_FLAG_PFORM_QUANT, row-aligned with the list of
 * pya_last_batch_peptidoforms: head[n] and cell[n * n_channels], n the length of that list and n_channels as lent (anything
 * else: PYA_ERR_ARG, as is a NULL array for a table that has rows).  PYA_ERR_STATE when the last batch was scored without the
 * flag. */
int pya_last_batch_peptidoform_quant(pya_handle *h, pya_site_quant_head *head, pya_site_quant *cell, uint64_t n, uint32_t n_channels);
/* The coverage records (pya_coverage above) of the last batch call on this handle that was given PYA_FLAG_COVERAGE: out[n_psm],
 * n_psm as in that call (anything else: PYA_ERR_ARG).  PYA_ERR_STATE when the last batch was scored without the flag.  The
 * record of a PSM that was set aside (PYA_FLAG_SKIP_INVALID) is all zero; records do not depend on the cut into chunks. */
int pya_last_batch_coverage(pya_handle *h, pya_coverage *out, uint64_t n_psm);
/* Fits d_table[n_slots] (device memory, pya_mz_profile) into d_cal[n_slots] (device memory; every byte of every record is
 * written): one launch of csrc/mz_calibrate.hip on hip_stream, one wavefront per slot, stream-ordered, no host wait and no
 * allocation.  Of params only inv_ppm is used.  PYA_ERR_ARG, with nothing launched: NULL where an array is needed with
 * n_slots > 0, n_slots above 2^31 - 1, params that pya_plan_mz_profile would refuse, min_ions == 0.  n_slots == 0 is a no-op. */
int pya_mz_profile_fit(pya_handle *h, const pya_mz_profile *d_table, uint64_t n_slots, const pya_mz_profile_params *params,
                       uint32_t min_ions, void *hip_stream, pya_mz_calibration *d_cal);
/* The same for a table on the host: uploads, runs on the handle's stream, downloads and waits (as pya_rollup_flr_host). */
int pya_mz_profile_fit_host(pya_handle *h, const pya_mz_profile *table, uint64_t n_slots, const pya_mz_profile_params *params,
                            uint32_t min_ions, pya_mz_calibration *out);
/* Corrects the m/z of n_spectra spectra on the device (the APPLY above): d_spectra->mz of d_spectra->mz_type (device memory;
 * the intensities are not touched and may be NULL), d_peak_off[n_spectra + 1], d_run[n_spectra] the slot of every spectrum
 * (NULL: slot 0; negative: left as it is), d_cal[n_slots], inv_band (finite and positive), d_mz_out of the same element type
 * (may equal d_spectra->mz), d_over two words zeroed by the caller.  One launch on hip_stream, stream-ordered, no host wait and
 * no allocation.  A spectrum whose slot is at or above n_slots, or whose record has a knot that is not finite or exceeds
 * PYA_MZC_MAX_PPM in magnitude, is copied unchanged and counted in d_over[0], the smallest such spectrum in d_over[1] as
 * 0xffffffff - spectrum.  No write lies outside d_mz_out[0 .. peak_off[n_spectra]).  PYA_ERR_ARG, with nothing launched: NULL
 * where an array is needed, an unknown mz_type, n_spectra above 2^32 - 2, n_slots above 2^31 - 1, an inv_band that is not
 * finite and positive.  n_spectra == 0 is a no-op. */
int pya_recalibrate_spectra(pya_handle *h, const pya_typed_spectra *d_spectra, const int64_t *d_peak_off, uint64_t n_spectra,
                            const int32_t *d_run, const pya_mz_calibration *d_cal, uint64_t n_slots, double inv_band, void *hip_stream,
                            void *d_mz_out, uint32_t *d_over);
/* Lends the library what the NEXT batch call with PYA_FLAG_RECALIBRATE corrects its spectra with: run[n_psm], one slot per PSM
 * (negative: the PSM asks for no correction), or NULL: slot 0, host memory that must stay valid until that call returns;
 * cal[n_slots], host memory, copied; inv_band.  The batch call corrects every chunk's spectra in place in the library's own
 * device copy on the run stream, before the first kernel that reads them; the caller's arrays are never written.  With shared
 * spectra a spectrum takes the slot of its PSMs: PSMs of one spectrum that name different non-negative slots are PYA_ERR_ARG
 * naming the PSM; a spectrum whose PSMs are all negative, or that no PSM refers to, is left alone.  A slot at or above n_slots:
 * PYA_ERR_LIMIT.  Every result of the flagged batch is bit-equal to the same batch scored without the flag on arrays corrected
 * by the definition above, whatever the route or the cut into chunks; with PYA_FLAG_MZ_PROFILE the profile is that of the
 * corrected spectra (the residual errors).  PYA_FLAG_KEEP with this flag is PYA_ERR_ARG.  Lifetime and the remaining refusals
 * are pya_set_mz_profile's.  PYA_ERR_ARG here: n_psm or n_slots above 2^31 - 1, NULL cal with n_slots > 0, a knot that is not
 * finite or exceeds PYA_MZC_MAX_PPM in magnitude, an inv_band that is not finite and positive. */
int pya_set_recalibration(pya_handle *h, const int32_t *run, uint64_t n_psm, const pya_mz_calibration *cal, uint64_t n_slots,
                          double inv_band);
/* The device bytes pya_deisotope_spectra needs as its workspace for n_spectra spectra of n_peaks peaks together: one keep bit
 * per peak in 64-bit words that no two spectra share, and the tile sums of the offset scan; 8 bytes at the least. */
uint64_t pya_deisotope_workspace_bytes(uint64_t n_spectra, uint64_t n_peaks);
/* Deisotopes n_spectra spectra on the device (THE RULE at pya_deisotope_params above; csrc/deisotope.hip): d_in the m/z and
 * intensity arrays (device memory, laid out by d_peak_off[n_spectra + 1]), d_out arrays of the same element types and the
 * input's capacity, d_new_off[n_spectra + 1] the offsets of the filtered spectra (d_new_off[0] = 0), d_over two words zeroed
 * by the caller.  Three passes on hip_stream -- mark and count, an exclusive scan of the counts, fill --, stream-ordered, no
 * host wait and no allocation; the caller lends d_work (8-byte aligned, work_bytes >= pya_deisotope_workspace_bytes(n_spectra,
 * d_peak_off[n_spectra])).  The kept peaks of spectrum s are d_out[d_new_off[s] .. d_new_off[s + 1]), in their order, bit for
 * bit.  A spectrum that is not ascending is copied unchanged and counted in d_over[0], the smallest such spectrum in d_over[1]
 * as 0xffffffff - spectrum (as pya_recalibrate_spectra reports).  No write lies outside out[0 .. d_new_off[n_spectra]),
 * d_new_off[0 .. n_spectra], d_over[0 .. 2) and d_work[0 .. work_bytes): the out elements from d_new_off[n_spectra] up to the
 * input's length stay as they were.  There is no limit on the peaks of a spectrum beyond int64 offsets: a spectrum over the
 * scorer's 65 535 peaks may come out under it.  The peak count is on the device, so the host can only check the workspace
 * against pya_deisotope_workspace_bytes(n_spectra, 0); the kernels clip the offsets to the peaks the lent workspace has bits
 * for, and a spectrum that reaches beyond them is reported in d_over as well.
 * PYA_ERR_ARG, with nothing launched: NULL where an array is needed, an out array that is an in array, unknown element types
 * or types that differ between in and out, float32 m/z beside float64 intensities, a workspace that is misaligned or too
 * small, parameters outside the conditions above, n_spectra above 2^32 - 2.  n_spectra == 0 writes d_new_off[0] = 0 and
 * nothing else. */
int pya_deisotope_spectra(pya_handle *h, const pya_typed_spectra *d_in, const int64_t *d_peak_off, uint64_t n_spectra,
                          const pya_deisotope_params *params, void *hip_stream, void *d_work, uint64_t work_bytes,
                          const pya_typed_spectra *d_out, int64_t *d_new_off, uint32_t *d_over);
/* The same over HOST arrays: uploads, runs on the handle's stream with a workspace of its own, downloads
 * out[0 .. new_off[n_spectra]), new_off and over, and waits (as pya_mz_profile_fit_host).  peak_off[0] must not be
 * negative and the offsets must not descend (PYA_ERR_ARG); the arrays are read from element 0 to peak_off[n_spectra]. */
int pya_deisotope_spectra_host(pya_handle *h, const pya_typed_spectra *in, const int64_t *peak_off, uint64_t n_spectra,
                               const pya_deisotope_params *params, const pya_typed_spectra *out, int64_t *new_off, uint32_t *over);
/* The device bytes pya_decharge_spectra needs as its workspace for n_spectra spectra of n_peaks peaks together: per group of 64
 * peaks a keep word, a moved word, a running count and 64 entries of 16 bytes for the moved peaks (about 16.4 bytes a peak),
 * per spectrum 32 bytes, and the tile sums of the offset scan. */
uint64_t pya_decharge_workspace_bytes(uint64_t n_spectra, uint64_t n_peaks);
/* Charge-deconvolves n_spectra spectra on the device (THE RULE at pya_decharge_params above; csrc/decharge.hip).  The arguments
 * are those of pya_deisotope_spectra, one for one, and d_charge beside them: one byte per OUTPUT peak with its charge (1 for a
 * peak that did not move), device memory of the input's capacity, or NULL when it is not wanted.  Three passes on hip_stream --
 * mark (keep, charge, moved value; counts), an exclusive scan of the kept counts, place (every kept peak computes its position
 * in the sorted output and writes itself there) --, stream-ordered, no host wait and no allocation; the caller lends d_work
 * (8-byte aligned, work_bytes >= pya_decharge_workspace_bytes(n_spectra, d_peak_off[n_spectra])).  The peaks of spectrum s are
 * d_out[d_new_off[s] .. d_new_off[s + 1]), ascending.  d_new_off equals what pya_deisotope_spectra gives under params->iso.  A
 * spectrum that is not ascending is copied unchanged and counted in d_over[0], the smallest such spectrum in d_over[1] as
 * 0xffffffff - spectrum.  No write lies outside out[0 .. d_new_off[n_spectra]), d_charge[0 .. d_new_off[n_spectra]),
 * d_new_off[0 .. n_spectra], d_over[0 .. 2) and d_work[0 .. work_bytes): the out elements from d_new_off[n_spectra] up to the
 * input's length stay as they were.  The peak count is on the device, so the host can only check the workspace against
 * pya_decharge_workspace_bytes(n_spectra, 0); the kernels clip the offsets to the peaks the lent workspace has room for (whole
 * groups of 64), and a spectrum that reaches beyond them is reported in d_over as well.
 * PYA_ERR_ARG, with nothing launched: everything pya_deisotope_spectra refuses (of params->iso for the parameters), a carrier
 * that is not finite and positive, a witness that is not finite or negative, a d_charge that is one of the spectrum arrays.
 * n_spectra == 0 writes d_new_off[0] = 0 and nothing else. */
int pya_decharge_spectra(pya_handle *h, const pya_typed_spectra *d_in, const int64_t *d_peak_off, uint64_t n_spectra,
                         const pya_decharge_params *params, void *hip_stream, void *d_work, uint64_t work_bytes,
                         const pya_typed_spectra *d_out, int64_t *d_new_off, uint8_t *d_charge, uint32_t *d_over);
/* The same over HOST arrays, as pya_deisotope_spectra_host: uploads, runs on the handle's stream with a workspace of its own,
 * downloads out[0 .. new_off[n_spectra]), charge[0 .. new_off[n_spectra]) (charge may be NULL), new_off and over, and waits.
 * peak_off[0] must not be negative and the offsets must not descend (PYA_ERR_ARG). */
int pya_decharge_spectra_host(pya_handle *h, const pya_typed_spectra *in, const int64_t *peak_off, uint64_t n_spectra,
                              const pya_decharge_params *params, const pya_typed_spectra *out, int64_t *new_off, uint8_t *charge,
                              uint32_t *over);
/* Diagnostic: which of the three passes pya_decharge_spectra launches from now on, in every handle (bit 0 mark, bit 1 scan,
 * bit 2 place; 7 is the default).  For scripts/decharge_probe.py, which times the passes apart; not thread-safe. */
void pya_debug_decharge_passes(uint32_t passes);
/* The device bytes pya_strip_spectra needs as its workspace for n_spectra spectra of n_peaks peaks together: what
 * pya_deisotope_workspace_bytes gives (one keep bit per peak in 64-bit words that no two spectra share, and the tile sums of
 * the offset scan; 8 bytes at the least). */
uint64_t pya_strip_workspace_bytes(uint64_t n_spectra, uint64_t n_peaks);
/* Strips the precursor-derived peaks from n_spectra spectra on the device (THE RULE at pya_strip_params above;
 * csrc/strip.hip).  The arguments are those of pya_deisotope_spectra, one for one, with the precursors and the report beside
 * them: d_prec_mz[n_spectra] (double) and d_prec_z[n_spectra] (int32) in device memory, d_report[n_spectra] one
 * pya_strip_report per spectrum (device memory, 8-byte aligned), or NULL when it is not wanted.  Three passes on hip_stream
 * -- mark and count (every lane of a wavefront holds one window of the spectrum, every peak is tested against all of them),
 * an exclusive scan of the counts, deisotoping's fill --, stream-ordered, no host wait and no allocation; the caller lends
 * d_work (8-byte aligned, work_bytes >= pya_strip_workspace_bytes(n_spectra, d_peak_off[n_spectra])).  The kept peaks of
 * spectrum s are d_out[d_new_off[s] .. d_new_off[s + 1]), in their order, bit for bit.  No write lies outside
 * out[0 .. d_new_off[n_spectra]), d_new_off[0 .. n_spectra], d_report[0 .. n_spectra), d_over[0 .. 2) and
 * d_work[0 .. work_bytes): the out elements from d_new_off[n_spectra] up to the input's length stay as they were.  The peak
 * count is on the device, so the host can only check the workspace against pya_strip_workspace_bytes(n_spectra, 0); the
 * kernels clip the offsets to the peaks the lent workspace has bits for, and a spectrum that reaches beyond them is counted
 * in d_over[0], the smallest such spectrum in d_over[1] as 0xffffffff - spectrum (its report is that of the clipped peaks).
 * Nothing else is reported in d_over: no spectrum is "not ascending" under this rule.
 * PYA_ERR_ARG, with nothing launched: everything pya_deisotope_spectra refuses about its arrays, its workspace and n_spectra,
 * a NULL d_prec_mz or d_prec_z, a d_report that is not 8-byte aligned, parameters outside the conditions above.
 * n_spectra == 0 writes d_new_off[0] = 0 and nothing else. */
int pya_strip_spectra(pya_handle *h, const pya_typed_spectra *d_in, const int64_t *d_peak_off, uint64_t n_spectra,
                      const double *d_prec_mz, const int32_t *d_prec_z, const pya_strip_params *params, void *hip_stream,
                      void *d_work, uint64_t work_bytes, const pya_typed_spectra *d_out, int64_t *d_new_off,
                      pya_strip_report *d_report, uint32_t *d_over);
/* The same over HOST arrays, as pya_deisotope_spectra_host: uploads, runs on the handle's stream with a workspace of its own,
 * downloads out[0 .. new_off[n_spectra]), new_off, report[0 .. n_spectra) (report may be NULL) and over, and waits.
 * peak_off[0] must not be negative and the offsets must not descend (PYA_ERR_ARG). */
int pya_strip_spectra_host(pya_handle *h, const pya_typed_spectra *in, const int64_t *peak_off, uint64_t n_spectra,
                           const double *prec_mz, const int32_t *prec_z, const pya_strip_params *params,
                           const pya_typed_spectra *out, int64_t *new_off, pya_strip_report *report, uint32_t *over);
/* Looks up the marker ions of n_spectra spectra on the device (THE RULE at pya_marker_params above; csrc/markers.hip).  d_in,
 * d_peak_off and n_spectra as pya_deisotope_spectra takes them; n_peaks: the elements the arrays of d_in hold -- the offsets
 * are clipped to it, as the transforms clip theirs to their workspace, so nothing beyond it is read whatever the offsets say;
 * d_prec_mz[n_spectra] (double) and d_prec_z[n_spectra] (int32) in device memory, both of which may be NULL iff
 * params->loss_mask == 0.  d_markers[n_spectra * params->n_targets]: one pya_marker per (spectrum, target), at
 * [s * n_targets + t]; d_spectra[n_spectra]: one pya_marker_spectrum per spectrum, or NULL when it is not wanted (both device
 * memory, 8-byte aligned); d_over[2] (zeroed by the caller): the spectra whose offsets were clipped are counted in d_over[0],
 * the smallest of them in d_over[1] as 0xffffffff - spectrum (its records are those of the clipped peaks).  One launch on
 * hip_stream, stream-ordered, no host wait, no allocation and no workspace.  The spectra are only read; no write lies
 * outside d_markers[0 .. n_spectra * n_targets), d_spectra[0 .. n_spectra) and d_over[0 .. 2).
 * PYA_ERR_ARG, with nothing launched: element types that are neither PYA_F64 nor PYA_F32, float32 m/z beside float64
 * intensities, more than 2^32 - 2 spectra, a NULL array, parameters outside the conditions above, a NULL precursor array
 * while loss_mask != 0, records that are not 8-byte aligned.  n_spectra == 0 is a call that writes nothing. */
int pya_marker_spectra(pya_handle *h, const pya_typed_spectra *d_in, const int64_t *d_peak_off, uint64_t n_spectra,
                       uint64_t n_peaks, const double *d_prec_mz, const int32_t *d_prec_z, const pya_marker_params *params,
                       void *hip_stream, pya_marker *d_markers, pya_marker_spectrum *d_spectra, uint32_t *d_over);
/* The same over HOST arrays: uploads the spectra once, runs on the handle's stream, downloads only the records -- markers,
 * spectra (may be NULL) and over -- and waits.  peak_off[0] must not be negative and the offsets must not descend
 * (PYA_ERR_ARG); n_peaks is peak_off[n_spectra]. */
int pya_marker_spectra_host(pya_handle *h, const pya_typed_spectra *in, const int64_t *peak_off, uint64_t n_spectra,
                            const double *prec_mz, const int32_t *prec_z, const pya_marker_params *params,
                            pya_marker *markers, pya_marker_spectrum *spectra, uint32_t *over);
/* Turns the marker records d_markers[n_spectra * n_targets] (device memory, as pya_marker_spectra wrote them) into the channel
 * matrix pya_plan_site_quant takes: d_values[n_spectra * popcount(channel_mask)] (device memory, doubles, row-major), the
 * channels being the targets whose bit of channel_mask is set, in ascending order -- the picked intensity, or a NaN where
 * PYA_MARKER_PICKED is clear.  One launch of csrc/site_quant.hip on hip_stream, stream-ordered, no host wait, no allocation;
 * the records are only read and no write lies outside d_values[0 .. n_spectra * popcount(channel_mask)).  PYA_ERR_ARG, with
 * nothing launched: n_targets outside 1 .. PYA_MARKER_MAX_TARGETS, an empty channel_mask or one with a bit at or above
 * n_targets, more than 2^32 - 2 spectra, a NULL array.  n_spectra == 0 is a call that writes nothing. */
int pya_marker_values(pya_handle *h, const pya_marker *d_markers, uint64_t n_spectra, uint32_t n_targets, uint64_t channel_mask,
                      void *hip_stream, double *d_values);
/* The precursor purity of n_query queries over n_survey survey spectra on the device (THE RULE at pya_purity_params above;
 * csrc/purity.hip).  d_survey_spectra, d_survey_off[n_survey + 1] and n_survey as pya_marker_spectra takes its spectra;
 * n_survey_peaks: the elements the arrays hold -- the offsets are clipped to it, so nothing beyond it is read whatever they
 * say; d_survey[n_query] (int64), d_prec_mz[n_query] (double), d_prec_z[n_query] (int32), d_win_lo[n_query] and
 * d_win_hi[n_query] (double) in device memory; d_purity[n_query]: one pya_purity per query (device memory, 8-byte aligned);
 * d_over[2] (zeroed by the caller): the queries with survey[q] >= n_survey or a clipped survey spectrum are counted in
 * d_over[0], the smallest of them in d_over[1] as 0xffffffff - q.  One launch on hip_stream, one wavefront per query,
 * stream-ordered, no host wait, no allocation and no workspace.  The inputs are only read; no write lies outside
 * d_purity[0 .. n_query) and d_over[0 .. 2).
 * PYA_ERR_ARG, with nothing launched: more than 2^32 - 2 queries or survey spectra, parameters outside the conditions above,
 * element types that are neither PYA_F64 nor PYA_F32, float32 m/z beside float64 intensities, a NULL array, records that are
 * not 8-byte aligned.  n_query == 0 is a call that writes nothing; n_survey == 0 is allowed (the survey arrays may then be
 * NULL but for the offsets: every query is inactive or out of range). */
int pya_purity_spectra(pya_handle *h, const pya_typed_spectra *d_survey_spectra, const int64_t *d_survey_off, uint64_t n_survey,
                       uint64_t n_survey_peaks, const int64_t *d_survey, const double *d_prec_mz, const int32_t *d_prec_z,
                       const double *d_win_lo, const double *d_win_hi, uint64_t n_query, const pya_purity_params *params,
                       void *hip_stream, pya_purity *d_purity, uint32_t *d_over);
/* The same over HOST arrays: uploads the survey spectra and the queries once, runs on the handle's stream, downloads only the
 * records and over, and waits.  survey_off[0] must not be negative and the offsets must not descend (PYA_ERR_ARG);
 * n_survey_peaks is survey_off[n_survey]. */
int pya_purity_spectra_host(pya_handle *h, const pya_typed_spectra *survey_spectra, const int64_t *survey_off, uint64_t n_survey,
                            const int64_t *survey, const double *prec_mz, const int32_t *prec_z, const double *win_lo,
                            const double *win_hi, uint64_t n_query, const pya_purity_params *params, pya_purity *purity,
                            uint32_t *over);
/* THE GATE of the precursor purity over the records d_purity[n_rows] (device memory, as pya_purity_spectra wrote them):
 * d_select[n_rows] (uint8, or NULL) takes 1 for a passing row and 0 otherwise; with n_channels in 1 .. PYA_QUANT_MAX_CHANNELS
 * d_out[n_rows * n_channels] takes d_values[n_rows * n_channels] (doubles, 8-byte aligned) with the readings of a passing row
 * copied bit for bit and those of a failing row set to the NaN of pya_marker_values.  d_out == d_values, exactly in place, is
 * allowed; any other overlap is the caller's error.  n_channels == 0 asks for d_select alone (d_values and d_out are not
 * looked at).  One launch on hip_stream, stream-ordered, no host wait, no allocation; the records are only read and no write
 * lies outside d_out[0 .. n_rows * n_channels) and d_select[0 .. n_rows).  PYA_ERR_ARG, with nothing launched: n_channels
 * above PYA_QUANT_MAX_CHANNELS, more than 2^32 - 2 rows, a threshold that is NaN or outside [0, 1], keep_unknown neither 0
 * nor 1, nothing to write (n_channels == 0 and d_select NULL), a NULL array that is needed, records or matrices that are not
 * 8-byte aligned.  n_rows == 0 is a call that writes nothing. */
int pya_purity_gate(pya_handle *h, const pya_purity *d_purity, uint64_t n_rows, double threshold, uint32_t keep_unknown,
                    const double *d_values, uint32_t n_channels, double *d_out, uint8_t *d_select, void *hip_stream);
/* Whether each of n_survey survey spectra on the device ascends in m/z (scan_ok of THE RULE at pya_xic_params above;
 * csrc/xic.hip): d_scan_ok[n_survey] takes one byte per scan, 1 iff x[j] <= x[j + 1] for every adjacent pair of the scan's
 * m/z (the offsets clipped to n_survey_peaks).  Only the m/z array of d_survey_spectra is read.  Run once per survey set; it
 * serves every later pya_xic_spectra call.  One launch on hip_stream, one wavefront per scan, stream-ordered, no host wait, no
 * allocation; no write lies outside d_scan_ok[0 .. n_survey).  PYA_ERR_ARG, with nothing launched: more than 2^32 - 2 scans,
 * element types as pya_purity_spectra refuses them, a NULL array.  n_survey == 0 is a call that writes nothing. */
int pya_xic_survey_check(pya_handle *h, const pya_typed_spectra *d_survey_spectra, const int64_t *d_survey_off, uint64_t n_survey,
                         uint64_t n_survey_peaks, void *hip_stream, uint8_t *d_scan_ok);
/* The precursor XIC of n_query queries over n_survey survey spectra on the device (THE RULE at pya_xic_params above;
 * csrc/xic.hip).  The survey spectra, d_survey_off, n_survey and n_survey_peaks as pya_purity_spectra takes them; d_rt[n_survey]
 * (double), d_scan_ok[n_survey] (uint8, of pya_xic_survey_check over the same spectra: a byte that says 1 for a scan that does
 * not ascend makes that scan's trace undefined, nothing else); d_seed, d_scan_lo, d_scan_hi [n_query] (int64), d_prec_mz
 * [n_query] (double), d_prec_z[n_query] (int32); d_xic[n_query]: one pya_xic per query (8-byte aligned); d_over[2] (zeroed by
 * the caller) as pya_purity_spectra's.  One launch on hip_stream, one wavefront per query with lane j on survey scan
 * scan_lo + j, stream-ordered, no host wait, no allocation, no workspace.  The inputs are only read; no write lies outside
 * d_xic[0 .. n_query) and d_over[0 .. 2).
 * PYA_ERR_ARG, with nothing launched: more than 2^32 - 2 queries or survey spectra, parameters outside the conditions above,
 * element types as pya_purity_spectra refuses them, a NULL array, records that are not 8-byte aligned.  n_query == 0 is a
 * call that writes nothing; n_survey == 0 is allowed (the survey arrays, d_rt and d_scan_ok may then be NULL but for the
 * offsets: every query is silent or out of range). */
int pya_xic_spectra(pya_handle *h, const pya_typed_spectra *d_survey_spectra, const int64_t *d_survey_off, uint64_t n_survey,
                    uint64_t n_survey_peaks, const double *d_rt, const uint8_t *d_scan_ok, const int64_t *d_seed,
                    const int64_t *d_scan_lo, const int64_t *d_scan_hi, const double *d_prec_mz, const int32_t *d_prec_z,
                    uint64_t n_query, const pya_xic_params *params, void *hip_stream, pya_xic *d_xic, uint32_t *d_over);
/* The same over HOST arrays: uploads the survey spectra and the queries once, runs pya_xic_survey_check itself when scan_ok is
 * NULL (else uploads scan_ok[n_survey]), runs on the handle's stream, downloads only the records and over, and waits.
 * survey_off[0] must not be negative and the offsets must not descend (PYA_ERR_ARG). */
int pya_xic_spectra_host(pya_handle *h, const pya_typed_spectra *survey_spectra, const int64_t *survey_off, uint64_t n_survey,
                         const double *rt, const uint8_t *scan_ok, const int64_t *seed, const int64_t *scan_lo,
                         const int64_t *scan_hi, const double *prec_mz, const int32_t *prec_z, uint64_t n_query,
                         const pya_xic_params *params, pya_xic *xic, uint32_t *over);
/* One column of the records d_xic[n] (device memory, as pya_xic_spectra wrote them) as the one-channel matrix
 * pya_plan_site_quant and pya_plan_peptidoform_quant take: d_out[n] (doubles) takes the area (which PYA_XIC_AREA), the apex,
 * the seed or the sum intensity, or the NaN of pya_marker_values (0x7ff8000000000000) where the record is not SEEN or the
 * value is not > 0.  One launch on hip_stream, stream-ordered, no host wait, no allocation; no write lies outside
 * d_out[0 .. n).  PYA_ERR_ARG, with nothing launched: which above 3, more than 2^32 - 2 records, a NULL or not 8-byte aligned
 * array.  n == 0 is a call that writes nothing. */
int pya_xic_values(pya_handle *h, const pya_xic *d_xic, uint64_t n, uint32_t which, void *hip_stream, double *d_out);
/* Applies a correction to the channel matrix d_values[n_rows * n_channels] (APPLY of the channel correction above;
 * csrc/channel_correct.hip): d_matrix[n_channels * n_channels] (row-major) or NULL, d_factor[n_channels] or NULL, not both
 * NULL; d_out[n_rows * n_channels] takes the result (all device memory, doubles, 8-byte aligned).  d_out == d_values, exactly
 * in place, is allowed: a row is read whole by the lanes that write it before they write; any other overlap is the caller's
 * error.  One launch on hip_stream, stream-ordered, no host wait, no allocation and no workspace; 64-bit index arithmetic; the
 * inputs are only read and no write lies outside d_out[0 .. n_rows * n_channels).  PYA_ERR_ARG, with nothing launched:
 * n_channels outside 1 .. PYA_QUANT_MAX_CHANNELS, d_matrix and d_factor both NULL, more than 2^32 - 2 rows, a NULL or not
 * 8-byte aligned array.  n_rows == 0 is a call that writes nothing. */
int pya_channel_correct(pya_handle *h, const double *d_values, uint64_t n_rows, uint32_t n_channels, const double *d_matrix,
                        const double *d_factor, void *hip_stream, double *d_out);
/* Adds the column sums of d_values[n_rows * n_channels] into the table row d_cell[n_channels] (SUMS of the channel correction
 * above): d_select[n_rows], one byte per row (0: the row is left out), or NULL for all rows; scale_log2 as
 * pya_site_quant_params has it.  The caller clears d_cell (hipMemsetAsync to 0) before the first call.  One launch,
 * stream-ordered, no host wait, no allocation and no workspace; everything that reaches memory is a 64-bit integer atomic add
 * to d_cell[0 .. n_channels).  PYA_ERR_ARG, with nothing launched: n_channels outside 1 .. PYA_QUANT_MAX_CHANNELS, scale_log2
 * outside -64 .. 64, more than 2^32 - 2 rows, a NULL array that is needed, d_values or d_cell not 8-byte aligned.  n_rows == 0
 * is a call that writes nothing. */
int pya_channel_sums(pya_handle *h, const double *d_values, uint64_t n_rows, uint32_t n_channels, const uint8_t *d_select,
                     int32_t scale_log2, void *hip_stream, pya_site_quant *d_cell);
/* The loading factors d_factor[n_channels] of a table row d_cell[n_channels] (FACTORS of the channel correction above): one
 * wavefront on hip_stream, so that a resident chain -- sums, factors, apply -- has no host wait.  d_cell is only read.
 * PYA_ERR_ARG, with nothing launched: n_channels outside 1 .. PYA_QUANT_MAX_CHANNELS, a NULL or not 8-byte aligned array. */
int pya_channel_factors(pya_handle *h, const pya_site_quant *d_cell, uint32_t n_channels, void *hip_stream, double *d_factor);
/* The chain over HOST arrays: one upload (values, matrix and select where given), pya_channel_correct with the matrix if one is
 * given, pya_channel_sums over the result into a cleared row, and with PYA_CHANNEL_NORMALIZE in flags pya_channel_factors and
 * pya_channel_correct with the factor alone, in place; one download of out[n_rows * n_channels], cell[n_channels] (the sums
 * BEFORE the factor; may be NULL without PYA_CHANNEL_NORMALIZE) and, with PYA_CHANNEL_NORMALIZE, factor[n_channels]; waits.
 * With both steps the result is clamp(clamp(M u) f): two applications of the rule, not a third rule.  out == values is
 * allowed.  PYA_ERR_ARG: what the three calls refuse, matrix NULL without PYA_CHANNEL_NORMALIZE, unknown flag bits. */
int pya_channel_correct_host(pya_handle *h, const double *values, uint64_t n_rows, uint32_t n_channels, const double *matrix,
                             const uint8_t *select, int32_t scale_log2, uint32_t flags, double *out, pya_site_quant *cell,
                             double *factor);
/* The device bytes pya_centroid_spectra needs as its workspace for n_spectra spectra of n_peaks points together: what
 * pya_deisotope_workspace_bytes gives (one keep bit per point in 64-bit words that no two spectra share, and the tile sums of
 * the offset scan; 8 bytes at the least).  Centroids are recomputed by the last pass, not stored. */
uint64_t pya_centroid_workspace_bytes(uint64_t n_spectra, uint64_t n_peaks);
/* Centroids n_spectra spectra on the device (THE RULE at pya_centroid_params above; csrc/centroid.hip).  The arguments, the
 * contract and the refusals are those of pya_deisotope_spectra, one for one, with d_select beside them: one byte per spectrum
 * in device memory (0: the spectrum is copied unchanged), or NULL for all.  Three passes on hip_stream -- mark (the apexes of
 * every 64 points as one keep word; counts), an exclusive scan of the counts, place (every apex walks its footprint, computes
 * its centroid and writes the pair at its position) --, stream-ordered, no host wait and no allocation; the caller lends d_work
 * (8-byte aligned, work_bytes >= pya_centroid_workspace_bytes(n_spectra, d_peak_off[n_spectra])).  The peaks of spectrum s are
 * d_out[d_new_off[s] .. d_new_off[s + 1]).  A spectrum that is not ascending is copied unchanged and counted in d_over[0], the
 * smallest such spectrum in d_over[1] as 0xffffffff - spectrum.  No write lies outside out[0 .. d_new_off[n_spectra]),
 * d_new_off[0 .. n_spectra], d_over[0 .. 2) and d_work[0 .. work_bytes): the out elements from d_new_off[n_spectra] up to the
 * input's length stay as they were.  There is no limit on the points of a spectrum beyond int64 offsets: a profile spectrum of
 * 200 000 points may come out under the scorer's 65 535 peaks.  The point count is on the device, so the host can only check
 * the workspace against pya_centroid_workspace_bytes(n_spectra, 0); the kernels clip the offsets to the points the lent
 * workspace has bits for, and a spectrum that reaches beyond them is reported in d_over as well.
 * PYA_ERR_ARG, with nothing launched: everything pya_deisotope_spectra refuses about its arrays, its workspace and n_spectra,
 * parameters outside the conditions above.  n_spectra == 0 writes d_new_off[0] = 0 and nothing else. */
int pya_centroid_spectra(pya_handle *h, const pya_typed_spectra *d_in, const int64_t *d_peak_off, uint64_t n_spectra,
                         const uint8_t *d_select, const pya_centroid_params *params, void *hip_stream, void *d_work,
                         uint64_t work_bytes, const pya_typed_spectra *d_out, int64_t *d_new_off, uint32_t *d_over);
/* The same over HOST arrays, as pya_deisotope_spectra_host: uploads (select too, when it is not NULL), runs on the handle's
 * stream with a workspace of its own, downloads out[0 .. new_off[n_spectra]), new_off and over, and waits.  peak_off[0] must
 * not be negative and the offsets must not descend (PYA_ERR_ARG). */
int pya_centroid_spectra_host(pya_handle *h, const pya_typed_spectra *in, const int64_t *peak_off, uint64_t n_spectra,
                              const uint8_t *select, const pya_centroid_params *params, const pya_typed_spectra *out,
                              int64_t *new_off, uint32_t *over);
/* Diagnostic: which of the three passes pya_centroid_spectra launches from now on, in every handle (bit 0 mark, bit 1 scan,
 * bit 2 place; 7 is the default).  For scripts/centroid_probe.py, which times the passes apart; not thread-safe. */
void pya_debug_centroid_passes(uint32_t passes);
/* The device bytes pya_plan_peptidoforms / pya_peptidoform_reduce need as their workspace for n_entries entries (PSMs of the
 * plan + records of d_prev; records of d_a + d_b): keys double-buffered, the entries, the staged list, digit histograms, tile
 * totals, about 133 bytes per entry; 0 for no entries (and above 2^31 - 1, which the calls refuse). */
uint64_t pya_peptidoform_workspace_bytes(uint64_t n_entries);
/* The same pipeline as pya_plan_peptidoforms without a plan, over one or two DEVICE arrays of records (d_b may be NULL with
 * n_b == 0): the list over all of them.  The records may be in any order and may repeat keys; records with n_psm == 0 are
 * skipped; the incoming n_isomers is ignored and recomputed.  Merging the lists of two ranks or two files is this call.
 * d_out[cap] must not alias an input; d_n[2]: the true length of the list (when it is longer than cap the first cap records
 * in order are written) and an error word, 0 here.  Stream-ordered on hip_stream, no host synchronisation and no allocation
 * inside; the caller lends d_work (work_bytes >= pya_peptidoform_workspace_bytes(n_a + n_b); 16-byte aligned, as the record
 * arrays are).  The inputs are only read.  No write lies outside d_out[0 .. cap), d_n[0 .. 2) and d_work[0 ..
 * workspace_bytes).  No entries is valid and launches nothing (d_n is zeroed).  PYA_ERR_ARG, with nothing launched: more
 * than 2^31 - 1 entries, a workspace that is too small, NULL or misaligned where an array is needed. */
int pya_peptidoform_reduce(pya_handle *h, const pya_peptidoform *d_a, uint64_t n_a, const pya_peptidoform *d_b, uint64_t n_b, void *hip_stream,
                           void *d_work, uint64_t work_bytes, pya_peptidoform *d_out, uint64_t cap, uint32_t *d_n);
/* The same for HOST arrays: uploads, runs pya_peptidoform_reduce on the handle's stream with a workspace of its own and
 * downloads.  *n: the length of the list; the first min(*n, cap) records into out. */
int pya_peptidoform_reduce_host(pya_handle *h, const pya_peptidoform *a, uint64_t n_a, const pya_peptidoform *b, uint64_t n_b,
                                pya_peptidoform *out, uint64_t cap, uint64_t *n);
/* The device bytes pya_plan_peptidoform_quant / pya_peptidoform_quant_reduce need as their workspace: never less than
 * pya_peptidoform_workspace_bytes(n_entries) (today exactly that: the table stage keeps nothing in the workspace). */
uint64_t pya_peptidoform_quant_workspace_bytes(uint64_t n_entries, uint32_t n_channels);
/* The merge of two pairs (peptidoform quantification above) over DEVICE arrays: the list as pya_peptidoform_reduce gives it for
 * d_a[n_a] and d_b[n_b], and d_head[cap] / d_cell[cap * n_channels] row-aligned with it: per key the rows of d_a_head /
 * d_a_cell and d_b_head / d_b_cell of the records with that key, added field by field.  The head and cells of a side may both
 * be NULL: that side counts as having an all-zero table (exactly one of them NULL: PYA_ERR_ARG).  Records with n_psm == 0 are
 * skipped and their rows with them.  The call clears d_head[0 .. cap) and d_cell[0 .. cap * n_channels) itself; the outputs
 * must not alias an input.  Otherwise pya_peptidoform_reduce's contract: stream-ordered, no host synchronisation, no
 * allocation; work_bytes >= pya_peptidoform_quant_workspace_bytes(n_a + n_b, n_channels); cells 16-byte, heads 8-byte aligned.
 * No write lies outside d_out[0 .. cap), d_head[0 .. cap), d_cell[0 .. cap * n_channels), d_n[0 .. 2) and the workspace.
 * PYA_ERR_ARG, with nothing launched: pya_peptidoform_reduce's refusals, n_channels outside 1 .. 64. */
int pya_peptidoform_quant_reduce(pya_handle *h, const pya_peptidoform *d_a, const pya_site_quant_head *d_a_head, const pya_site_quant *d_a_cell,
                                 uint64_t n_a, const pya_peptidoform *d_b, const pya_site_quant_head *d_b_head, const pya_site_quant *d_b_cell,
                                 uint64_t n_b, uint32_t n_channels, void *hip_stream, void *d_work, uint64_t work_bytes, pya_peptidoform *d_out,
                                 pya_site_quant_head *d_head, pya_site_quant *d_cell, uint64_t cap, uint32_t *d_n);
/* The same for HOST arrays: uploads, runs pya_peptidoform_quant_reduce on the handle's stream with a workspace of its own and
 * downloads.  *n: the length of the list; the first min(*n, cap) rows into out, head and cell; the rows behind them up to
 * min(cap, n_a + n_b) are zeroed. */
int pya_peptidoform_quant_reduce_host(pya_handle *h, const pya_peptidoform *a, const pya_site_quant_head *a_head, const pya_site_quant *a_cell,
                                      uint64_t n_a, const pya_peptidoform *b, const pya_site_quant_head *b_head, const pya_site_quant *b_cell,
                                      uint64_t n_b, uint32_t n_channels, pya_peptidoform *out, pya_site_quant_head *head, pya_site_quant *cell,
                                      uint64_t cap, uint64_t *n);

/* device-resident path: plan once (host pre-pass, tables, workspace), run many times.
 * LIFETIME.  A plan belongs to the handle and to the SETTINGS it was made under: its routes, launch caps, LDS carves and its
 * score-table need are fixed then.  It stays valid while the handle makes other plans, scores other batches or single PSMs,
 * and while the handle's own device tables grow and move (a run asks for them anew).  After pya_add_neutral_loss on the
 * handle every call that would LAUNCH over the plan -- pya_plan_run, pya_plan_run_typed, pya_plan_evidence,
 * pya_plan_ions_count, pya_plan_ions, pya_plan_named, pya_plan_sites, pya_plan_probs, pya_plan_ranked, pya_plan_rollup,
 * pya_plan_site_quant, pya_plan_peptidoforms, pya_plan_peptidoform_quant, pya_plan_mz_profile, pya_plan_coverage, and
 * pya_calculate_ambiguity over a retained batch -- returns PYA_ERR_STATE ("settings changed since the plan was made") with
 * nothing enqueued; the library does not rebuild a plan behind its caller's back.  Make a new plan.  What only reads back
 * (pya_plan_check, pya_plan_timings*, pya_plan_workspace_bytes, pya_plan_site_offsets, pya_get_pep_scores*) and
 * pya_plan_destroy stay valid.  The debug switches of pyascore_debug.h and the sizes (workspace budget, ranked list length,
 * site cap) do not end a plan's life. */
int pya_plan_create(pya_handle *h, const pya_batch *batch, uint32_t flags, pya_plan **out);
/* the same for a batch whose PSMs share spectra (pya_score_batch_shared: batch->peak_off describes n_spectra spectra,
 * spec_of[i] names PSM i's; the reference's hit_depth loop, pyascore/__main__.py).  pya_plan_run and every other pya_plan_*
 * function take such a plan unchanged: d_mz / d_intensity are laid out by the spectra's peak_off, results and status are per
 * PSM.  pya_plan_workspace_bytes is smaller than the repeated-spectrum plan's by the retained tables saved. */
int pya_plan_create_shared(pya_handle *h, const pya_batch *batch, const uint32_t *spec_of, uint64_t n_spectra,
                           uint32_t flags, pya_plan **out);
int pya_plan_run(pya_plan *plan, const double *d_mz, const double *d_intensity,
                 void *hip_stream, const pya_results *d_out);
/* pya_plan_run with typed device arrays (pya_typed_spectra above: the same combinations, the same refusals).  A plan is not
 * tied to a type: pya_plan_create / pya_plan_create_shared know nothing of it, one plan may be run with float64 arrays and
 * then with float32 ones, and the type selects the binning kernels' instantiation at launch time.  The arrays need the
 * alignment of their element type only.  A typed run of a handful of PSMs takes the plan's launches (the one-launch kernel
 * for tiny batches reads float64).  No reference counterpart. */
int pya_plan_run_typed(pya_plan *plan, const pya_typed_spectra *d_spectra, void *hip_stream, const pya_results *d_out);
/* The evidence records (pya_evidence above; cpp/Ascore.cpp:157-210) of the results the last pya_plan_run* of this plan
 * wrote: d_res is that run's results structure (device pointers), d_out device memory for n_psm * d_res->max_k records.
 * Enqueues the evidence kernel (csrc/evidence.hip) on hip_stream, stream-ordered like pya_plan_run: it waits for that run
 * -- the plan's side stream included when the run forked -- also when hip_stream is not the run's stream.  It reads the
 * retained tables of the run, so it is valid until the plan is run again; it may be called more than once.  A run issues
 * the launches it issues without this call, and no kernel of a run knows of it.  PYA_ERR_STATE when the plan has not been
 * run.  PSMs the kernels rejected surface through pya_plan_check as they do for a run; their rows are all zero. */
int pya_plan_evidence(pya_plan *plan, const pya_results *d_res, void *hip_stream, pya_evidence *d_out);
/* The ion records (pya_ion above) of the results the last pya_plan_run* of this plan wrote, in two stream-ordered steps
 * without a host synchronisation inside (csrc/ions.hip); d_res as for pya_plan_evidence, and the same validity: until the
 * plan is run again; both wait for the run, its side stream included.  PYA_ERR_STATE before the first run.
 *   pya_plan_ions_count  the count kernel and an exclusive scan on the device: d_ion_off[n_psm + 1], d_ion_off[n_psm] = the
 *                        number of records.  The caller reads that number in its own time and allocates.
 *   pya_plan_ions        the fill: d_out[cap] records at the offsets of the count (the same d_ion_off; PYA_ERR_STATE when
 *                        the run has not been counted).  A PSM whose records would pass cap writes nothing -- no write
 *                        ever lies at or past d_out + cap -- and pya_plan_check reports it (PYA_ERR_LIMIT) until the fill
 *                        is repeated with room or the plan is run again.
 * PYA_ERR_LIMIT when a fragment list needs more LDS than a compute unit has, as for pya_plan_evidence. */
int pya_plan_ions_count(pya_plan *plan, const pya_results *d_res, void *hip_stream, int64_t *d_ion_off);
int pya_plan_ions(pya_plan *plan, const pya_results *d_res, void *hip_stream, const int64_t *d_ion_off, pya_ion *d_out, uint64_t cap);
/* The named-localisation records (pya_named above; cpp/Ascore.cpp:53-210) of the results the last pya_plan_run* of this plan
 * wrote, for the queries d_q_off[n_psm + 1] / d_q_bits (device memory): d_out[n_q] records, d_counts / d_scores NULL or
 * [n_q * n_top].  d_res as for pya_plan_evidence.  Enqueues the kernel (csrc/named.hip) on hip_stream, stream-ordered, no
 * host synchronisation inside; it waits for that run -- the side stream included -- also when hip_stream is not the run's
 * stream, is valid until the plan is run again, and may be called again with other queries.  n_q is the host-known size of
 * the output (d_q_off[n_psm] of a well-formed list): no write ever lies at or past d_out + n_q (rows of d_counts / d_scores
 * alike) whatever d_q_off holds -- a PSM whose range is not inside [0, n_q] writes nothing and pya_plan_check reports it
 * (PYA_ERR_LIMIT) until the call is repeated or the plan is run again.  PYA_ERR_STATE when the plan has not been run,
 * PYA_ERR_LIMIT when a fragment list needs more LDS than a compute unit has.  A plan of a handful of PSMs must have been
 * created with PYA_FLAG_NAMED (or PYA_FLAG_EVIDENCE / PYA_FLAG_IONS): the one-launch kernel leaves no retained tables. */
int pya_plan_named(pya_plan *plan, const pya_results *d_res, void *hip_stream, const int64_t *d_q_off, const uint64_t *d_q_bits,
                   uint64_t n_q, pya_named *d_out, int32_t *d_counts, float *d_scores);
/* The site records (pya_site above) of the results the last pya_plan_run* of this plan wrote.
 *   pya_plan_site_offsets  site_off[n_psm + 1] (host memory): where the records of every PSM lie; known from the plan's
 *                          pre-pass, so it may be called before a run, and no scan runs on the device.
 *   pya_plan_sites         d_out[site_off[n_psm]] records; d_res as for pya_plan_evidence; sig_cap: PSMs with more site
 *                          assignments get PYA_SITE_OVER records, 0 = no cap.  Enqueues the kernel (csrc/sites.hip) on
 *                          hip_stream, stream-ordered, no host synchronisation inside; it waits for that run -- the side
 *                          stream included -- also when hip_stream is not the run's stream, is valid until the plan is run
 *                          again, and may be called again.  PYA_ERR_STATE when the plan has not been run, PYA_ERR_LIMIT as
 *                          for pya_plan_evidence.  A plan of a handful of PSMs must have been created with PYA_FLAG_SITES
 *                          (or PYA_FLAG_EVIDENCE / _IONS / _NAMED): the one-launch kernel leaves no retained tables. */
int pya_plan_site_offsets(const pya_plan *plan, int64_t *site_off);
int pya_plan_sites(pya_plan *plan, const pya_results *d_res, void *hip_stream, uint32_t sig_cap, pya_site *d_out);
/* The site probabilities of the results the last pya_plan_run* of this plan wrote: d_sites[site_off[n_psm]] records at the
 * offsets of pya_plan_site_offsets, d_psms[n_psm] records, device memory.  Everything else as for pya_plan_sites:
 * stream-ordered (csrc/probs.hip), no host synchronisation inside, waits for the run, valid until the plan is run again, may
 * be called again; no write lies at or past d_sites + site_off[n_psm].  It reads best_score, best_sig and n_sig of d_res. */
int pya_plan_probs(pya_plan *plan, const pya_results *d_res, void *hip_stream, uint32_t sig_cap, pya_site_prob *d_sites,
                   pya_psm_prob *d_psms);
/* The ranked localisations of the results the last pya_plan_run* of this plan wrote: d_out[n_psm * top_k] records, device
 * memory, the rows of PSM i at d_out[i * top_k]; top_k 1 .. PYA_MAX_RANKED (anything else: PYA_ERR_ARG).  Everything else as
 * for pya_plan_probs: stream-ordered (csrc/ranked.hip), no host synchronisation inside, waits for the run, valid until the
 * plan is run again, may be called again (with another top_k too); no write lies at or past d_out + n_psm * top_k.  It reads
 * best_score, best_sig and n_sig of d_res.  A plan of a handful of PSMs is created with PYA_FLAG_RANKED (or another stage
 * flag): the one-launch kernel leaves no retained tables. */
int pya_plan_ranked(pya_plan *plan, const pya_results *d_res, void *hip_stream, uint32_t top_k, uint32_t sig_cap, pya_ranked *d_out);
/* Rolls the probability records of this plan's PSMs into d_table[n_slots] (pya_site_rollup above; device memory, brought to
 * the empty state once by pya_rollup_clear): the stage ACCUMULATES, so the same table may take the records of other plans,
 * other runs and other calls.  d_site_probs / d_psm_probs: probability records laid out at the plan's site offsets
 * (pya_plan_site_offsets) -- normally what pya_plan_probs wrote for the same run, on the same stream or one that waits for
 * it; d_slot[site_off[n_psm]]; d_psm_id[n_psm] device memory, or NULL: PSM i is known as psm_base + i.  It reads best_sig and
 * ascores (row stride max_k, which must not be below the plan's largest n_of_mod) of d_res.  Two launches of csrc/rollup.hip,
 * stream-ordered, no host synchronisation inside, waits for the run, valid until the plan is run again, may be called
 * again with other slots or another table.  No write ever lies at or past d_table + n_slots: a record whose slot is at or
 * above n_slots writes nothing, and pya_plan_check reports it (PYA_ERR_LIMIT) until the call is repeated or the plan is run
 * again.  n_slots above 2^31 - 1: PYA_ERR_ARG. */
int pya_plan_rollup(pya_plan *plan, const pya_results *d_res, void *hip_stream, const pya_site_prob *d_site_probs,
                    const pya_psm_prob *d_psm_probs, const int32_t *d_slot, uint64_t n_slots, double threshold, const uint32_t *d_psm_id,
                    uint32_t psm_base, pya_site_rollup *d_table);
/* Adds the channel intensities of this plan's contributing records to the table d_head[n_slots] / d_cell[n_slots *
 * params->n_channels] (pya_site_quant above; device memory, emptied once by a hipMemsetAsync to 0): the stage ACCUMULATES, so
 * the same table may take other plans, other runs and other calls.  d_site_probs / d_psm_probs and d_slot as for
 * pya_plan_rollup; d_values[n_rows * n_channels] device memory; d_row[n_psm] device memory, or NULL: PSM i has row
 * row_base + i.  It reads best_sig of d_res.  One launch of csrc/site_quant.hip, stream-ordered, no host synchronisation, no
 * allocation of the caller's and no workspace; waits for the run as pya_plan_rollup does, valid until the plan is run again,
 * may be called again.  No write ever lies outside d_head[0 .. n_slots) and d_cell[0 .. n_slots * n_channels): a record that
 * would contribute but whose slot is at or above n_slots or whose row is at or above n_rows writes nothing, and pya_plan_check
 * reports it (PYA_ERR_LIMIT) until the call is repeated or the plan is run again.  PYA_ERR_ARG, with nothing launched:
 * parameters outside the conditions of pya_set_site_quant, n_slots or n_rows above 2^31 - 1, NULL where an array is needed;
 * PYA_ERR_STATE before the plan's first run.  A plan of a handful of PSMs is created with PYA_FLAG_QUANT (or another stage
 * flag), as for pya_plan_rollup. */
int pya_plan_site_quant(pya_plan *plan, const pya_results *d_res, void *hip_stream, const pya_site_prob *d_site_probs,
                        const pya_psm_prob *d_psm_probs, const int32_t *d_slot, uint64_t n_slots, const double *d_values,
                        uint64_t n_rows, const int32_t *d_row, uint32_t row_base, const pya_site_quant_params *params,
                        pya_site_quant_head *d_head, pya_site_quant *d_cell);
/* The peptidoform list (pya_peptidoform above) over this plan's contributing PSMs and the n_prev records of an earlier list
 * d_prev (only read, must not alias d_out; NULL with n_prev == 0): bytewise what one call over all the PSMs behind both would
 * give.  d_site_probs / d_psm_probs as for pya_plan_rollup; d_group[n_psm] device memory; d_psm_id[n_psm] device memory, or
 * NULL: PSM i is known as psm_base + i.  It reads best_sig and ascores (row stride max_k, not below the plan's largest
 * n_of_mod) of d_res.  d_n[0]: the true number of peptidoforms -- when the list is longer than cap the first cap records in
 * order are written, and no write ever lies at or past d_out + cap; d_n[1]: an error word, 0 when all is well: the number of
 * PSMs whose best_sig names a residue record the PSM does not have or more residues than max_k (results that are not this
 * plan's; such a PSM is left out).  Stream-ordered (csrc/peptidoforms.hip), no host synchronisation and no allocation inside:
 * the caller lends d_work (work_bytes >= pya_peptidoform_workspace_bytes(n_psm + n_prev), 16-byte aligned as d_prev and d_out
 * are); waits for the run as pya_plan_rollup does, valid until the plan is run again, may be called again.  No write lies
 * outside d_out[0 .. cap), d_n[0 .. 2) and d_work[0 .. workspace_bytes).  PYA_ERR_ARG, with nothing launched: more than
 * 2^31 - 1 entries, a workspace that is too small, NULL or misaligned where an array is needed; PYA_ERR_STATE before the
 * plan's first run.  A plan of a handful of PSMs is created with PYA_FLAG_PEPTIDOFORMS (or another stage flag), as for
 * pya_plan_rollup. */
int pya_plan_peptidoforms(pya_plan *plan, const pya_results *d_res, void *hip_stream, const pya_site_prob *d_site_probs,
                          const pya_psm_prob *d_psm_probs, const int32_t *d_group, double threshold, const uint32_t *d_psm_id,
                          uint32_t psm_base, const pya_peptidoform *d_prev, uint64_t n_prev, void *d_work, uint64_t work_bytes,
                          pya_peptidoform *d_out, uint64_t cap, uint32_t *d_n);
/* The pair of the peptidoform quantification (above) over this plan's contributing PSMs and an earlier pair: pya_plan_peptidoforms'
 * contract, extended.  d_out[cap] / d_n and everything up to n_prev as in that call, with the same bytes as its result;
 * d_prev_head[n_prev] / d_prev_cell[n_prev * n_channels], the table of d_prev, may both be NULL: the earlier list then counts as
 * having an all-zero table (exactly one of them NULL: PYA_ERR_ARG).  d_values / n_rows / d_row / row_base / params as for
 * pya_plan_site_quant.  d_head[cap] / d_cell[cap * n_channels] take the table; the call clears both on the stream before it
 * adds to them.  The list by the launches of csrc/peptidoforms.hip, one launch of csrc/pform_quant.hip behind them on the same
 * stream, inside the caller's workspace (work_bytes >= pya_peptidoform_quant_workspace_bytes(n_psm + n_prev, n_channels)): no
 * host synchronisation, no allocation of the caller's.  No write lies outside d_out[0 .. cap), d_head[0 .. cap), d_cell[0 ..
 * cap * n_channels), d_n[0 .. 2) and the workspace.  A PSM that would contribute and whose row is at or above n_rows writes
 * nothing to the table, and pya_plan_check reports it (PYA_ERR_LIMIT) until the call is repeated or the plan is run again.
 * PYA_ERR_ARG, with nothing launched: what pya_plan_peptidoforms and pya_set_site_quant refuse; PYA_ERR_STATE before the plan's
 * first run. */
int pya_plan_peptidoform_quant(pya_plan *plan, const pya_results *d_res, void *hip_stream, const pya_site_prob *d_site_probs,
                               const pya_psm_prob *d_psm_probs, const int32_t *d_group, double threshold, const uint32_t *d_psm_id,
                               uint32_t psm_base, const pya_peptidoform *d_prev, const pya_site_quant_head *d_prev_head,
                               const pya_site_quant *d_prev_cell, uint64_t n_prev, const double *d_values, uint64_t n_rows, const int32_t *d_row,
                               uint32_t row_base, const pya_site_quant_params *params, void *d_work, uint64_t work_bytes, pya_peptidoform *d_out,
                               pya_site_quant_head *d_head, pya_site_quant *d_cell, uint64_t cap, uint32_t *d_n);
/* Adds the fragment mass errors of this plan's contributing PSMs to d_table[n_slots] (pya_mz_profile above; device memory,
 * emptied once by a hipMemsetAsync to 0): the stage ACCUMULATES, so the same table may take other plans, other runs and other
 * calls.  d_run[n_psm] device memory, or NULL: every PSM is of slot 0.  It reads best_sig and n_sig of d_res, the run's status
 * and its retained tables.  One or two launches of csrc/mz_profile.hip (the PSMs inside the fast limits, the general ones),
 * stream-ordered, no host synchronisation and no allocation of the caller's inside, waits for the run (its side stream
 * included) as pya_plan_evidence does, valid until the plan is run again, may be called again.  No write ever lies at or past
 * d_table + n_slots: a PSM whose slot is at or above n_slots writes nothing, and pya_plan_check reports it (PYA_ERR_LIMIT)
 * until the call is repeated or the plan is run again.  PYA_ERR_ARG, with nothing launched: max_rank >= 16, an inv_* that is not
 * finite and positive, n_slots above 2^31 - 1, NULL where an array is needed; PYA_ERR_STATE before the plan's first run;
 * PYA_ERR_LIMIT under the LDS condition of pya_plan_evidence.  A plan of a handful of PSMs is created with
 * PYA_FLAG_MZ_PROFILE (or another stage flag): the one-launch kernel leaves no retained tables. */
int pya_plan_mz_profile(pya_plan *plan, const pya_results *d_res, void *hip_stream, const int32_t *d_run, uint64_t n_slots,
                        const pya_mz_profile_params *params, pya_mz_profile *d_table);
/* Writes the coverage record (pya_coverage above) of every PSM of this plan to d_out[n_psm] (device memory; every byte of it
 * is written).  d_spectra: the device arrays the last run scored (pya_plan_run_typed's; the float64 pair of pya_plan_run as
 * PYA_F64 / PYA_F64) -- the stage reads the raw peaks again, beside best_sig and n_sig of d_res, the run's status and its
 * retained tables.  One or two launches of csrc/coverage.hip (the PSMs inside the fast limits, the general ones),
 * stream-ordered, no host synchronisation and no allocation of the caller's inside, waits for the run (its side stream
 * included) as pya_plan_evidence does, valid until the plan is run again, may be called again.  PYA_ERR_ARG, with nothing
 * launched: NULL where an array is needed, a type pair the run refuses; PYA_ERR_STATE before the plan's first run;
 * PYA_ERR_LIMIT under the LDS condition of pya_plan_evidence.  A plan of a handful of PSMs is created with PYA_FLAG_COVERAGE
 * (or another stage flag): the one-launch kernel leaves no retained tables. */
int pya_plan_coverage(pya_plan *plan, const pya_results *d_res, const pya_typed_spectra *d_spectra, void *hip_stream,
                      pya_coverage *d_out);
/* ms per kernel family of the last pya_plan_run (PYA_FLAG_TIMING): bin_spectra, score_signatures,
 * score_localize (the fused kernel, with the localize launch for what it hands over), localize;
 * synchronises.  A batch that has fused PSMs and others runs the fused family on a stream of its own beside
 * the scoring and localize kernels: ms[2] is then that stream's interval, it OVERLAPS ms[1] and ms[3], and the
 * four no longer sum to the step. */
int pya_plan_timings(pya_plan *plan, float ms[4]);
/* the same, summed over the runs since the last call of this function (the events live in a ring of 128 runs:
 * of more runs than that only the latest 128 count); *n_runs = how many; synchronises with the latest run only,
 * so a caller can enqueue run after run without waiting in between */
int pya_plan_timings_sum(pya_plan *plan, double ms[4], uint32_t *n_runs);
/* The multi-GPU path's gather record (north_star: "a single RCCL gather at the end"; no reference counterpart -- the
 * reference scores on one core and has no collective): packs the device results of `n_psm` PSMs into fixed-size
 * records of 4 + 3 k int32 words (best_score bits, n_sig, best_sig lo / hi, k Ascore bit patterns, k alternative-site
 * masks lo / hi; k >= d_res->max_k, the job-wide widest row, columns beyond the results' own are zero) at d_out --
 * e.g. a rank's slice of its send buffer -- with ONE kernel on `hip_stream`. */
int pya_pack_records(pya_handle *h, const pya_results *d_res, uint64_t n_psm, uint32_t k, int32_t *d_out, void *hip_stream);
/* waits for the stream of the last run and reports the first PSM the kernels rejected */
int pya_plan_check(pya_plan *plan);
uint64_t pya_plan_workspace_bytes(const pya_plan *plan);
uint64_t pya_plan_total_signatures(const pya_plan *plan);
void pya_plan_destroy(pya_plan *plan);

/* all localisations of PSM `psm` of the last pya_score_batch(..., PYA_FLAG_KEEP, ...), in the
 * reference's sorted order; arrays sized for `cap` records; returns the record count in *n */
int pya_get_pep_scores(pya_handle *h, uint64_t psm, uint64_t cap, uint64_t *n, uint64_t *sig_bits,
                       int32_t *counts /* cap x n_top */, float *scores /* cap x n_top */,
                       float *weighted_score, int32_t *total_fragments);
/* the same for PSMs [psm_begin, psm_end) in one call (three device copies for the whole range):
 * rec_off[psm_end - psm_begin + 1] receives the CSR offsets of the PSMs' records; with cap == 0 only
 * rec_off is filled (size query), otherwise the arrays must hold rec_off[last] records.
 * (pep_scores of a whole batch, Ascore.pyx:241-252 at scale) */
int pya_get_pep_scores_range(pya_handle *h, uint64_t psm_begin, uint64_t psm_end, uint64_t cap,
                             int64_t *rec_off, uint64_t *sig_bits, int32_t *counts /* cap x n_top */,
                             float *scores /* cap x n_top */, float *weighted_score,
                             int32_t *total_fragments);
/* PyAscore.calculate_ambiguity (Ascore.pyx:208-230 -> Ascore::calculateAmbiguity, cpp/Ascore.cpp:157-210) for PSM `psm`
 * of the retained batch: the caller's two score containers as (signature bits over the modifiable residues, n_top depth
 * scores, weighted score).  Any PSM the library scores: peptides of up to 64 residues with ten depths and a spectrum of
 * up to PYA_FAST_PEAKS peaks on the fast kernel, everything else (long peptides, n_top 11..16, big spectra) on the
 * general kernel's Ascore code. */
int pya_calculate_ambiguity(pya_handle *h, uint64_t psm, uint64_t ref_bits,
                            const float *ref_scores, float ref_weighted, uint64_t other_bits,
                            const float *other_scores, float other_weighted, float *out);

/* host-only helpers */
int pya_format_peptide(const pya_handle *h, const uint8_t *pep, uint64_t pep_len, int32_t n_of_mod,
                       const uint32_t *aux_pos, const float *aux_mass, uint64_t n_aux,
                       uint64_t sig_bits, int32_t sig_len, char *buf, uint64_t cap);
/* pya_format_peptide for many records in ONE call: record r is the localisation sig_bits[r] of PSM
 * rec_psm[r] of `batch` (rec_psm NULL: record r belongs to PSM r -- the best sequences of a scored
 * batch; with rec_psm -- the sequence column of a bulk pep_scores export).  rec_valid (optional): a
 * record with rec_valid[r] <= 0 (n_sig of a PSM without localisation, a set-aside PSM) gets the empty
 * string.  Strings come back as CSR bytes without terminators: str_off[n_rec + 1], buf[cap]; with
 * cap == 0 only str_off is filled (size query).  (ModifiedPeptide.cpp:199-253 at scale) */
int pya_format_peptides(const pya_handle *h, const pya_batch *batch, uint64_t n_rec, const int64_t *rec_psm,
                        const uint64_t *sig_bits, const int32_t *rec_valid, int64_t *str_off, char *buf,
                        uint64_t cap);
int pya_count_sites(const pya_handle *h, const uint8_t *pep, uint64_t pep_len, int32_t *n_sites,
                    uint16_t *site_pos /* >= PYA_MAX_PEPTIDE_LEN, 0-based residue of each site */);

/* test hook: runs the on-device emulation of the reference's std::sort (descending, keyed by
 * weighted score) on arbitrary keys and returns the permutation */
int pya_debug_sort(pya_handle *h, const float *keys, uint32_t n, uint32_t *perm);

const char *pya_version(void);

#ifdef __cplusplus
}
#endif
#endif /* PYASCORE_HIP_H */
