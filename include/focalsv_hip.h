/* focalsv_hip.h -- C ABI of libfocalsv_hip.so (MI355X / gfx950).
 *
 * This is the drop-in boundary for FocalSV's per-region local-assembly +
 * SV-calling hot path.  The reference has no plugin API: its boundary is
 * "spawn a CPU binary and read its files back" (SURVEY.md 8b):
 *
 *   hifiasm -o <prefix> -t T <reads.fa>        focalsv/3_assembly/run_assembly.py:15-26
 *       -> GFA 'S' lines -> HP1.fa/HP2.fa       focalsv/3_assembly/post_assembly.py:79-95, combine_fas.py:10-35
 *   minimap2 -a -x asm5 --cs -r2k ref asm.fa   focalsv/4_sv_calling/Dippav/DipPAV_variant_call.py:103-108
 *       -> BAM records read through pysam       focalsv/4_sv_calling/Dippav/extract_contig_signature_CCS.py:14-47,342-432
 *
 * The entry points below are what a binding at those two call sites would
 * bind instead (INTEGRATION.md shows the ctypes stubs).  Conventions:
 *   - plain C types, pointers + sizes, no ownership transfer: every buffer is
 *     allocated by the caller (sized through the *_bound() calls) ;
 *   - every function returns 0 or a negative FSV_E* code, never aborts; batch
 *     calls also fill a per-unit status array;
 *   - one fsv_ctx per GPU/stream; calls on different contexts are independent,
 *     the library keeps no global state;
 *   - "_dev" arguments are device pointers valid on the context's device
 *     (hipMalloc / torch tensor data_ptr()); everything else is host memory.
 *   - there is NO CPU fallback: without a usable gfx950 device
 *     fsv_ctx_create() fails with FSV_ENODEV.
 *
 * Read store layout (hifiasm K0, Process_Read.h:108-137, restated for HBM):
 * bases are 2-bit codes A=0 C=1 G=2 T=3, 16 per little-endian uint32 word,
 * base i of a read in bits [2*(i%16), 2*(i%16)+1] of word (word_off + i/16).
 * Every read starts on a word boundary.  In a READ 'N' is stored as A (hifiasm keeps an
 * N side list; the FocalSV read FASTAs come from BAM records and carry none); the aligner's
 * reference windows keep their N (fsv_align_batch).
 */
#ifndef FOCALSV_HIP_H
#define FOCALSV_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FSV_OK        0
#define FSV_ENODEV   -1  /* no gfx950 device / HIP runtime unusable */
#define FSV_EINVAL   -2  /* bad argument */
#define FSV_ENOMEM   -3  /* device or host allocation failed */
#define FSV_EHIP     -4  /* HIP runtime error (fsv_last_error gives the text) */
#define FSV_ECAP     -5  /* caller buffer too small */
#define FSV_EUNSUP   -6  /* input outside what this build supports */
#define FSV_EINTERNAL -7 /* an invariant of the library did not hold, or a C++ exception was caught at the boundary (fsv_last_error gives the text) */

#define FSV_WINDOW          375 /* hifiasm WINDOW, Hash_Table.h:9 */
#define FSV_K_FULL           15 /* hifiasm THRESHOLD, Hash_Table.h:13 */
#define FSV_K_MAX            31 /* hifiasm THRESHOLD_MAX_SIZE, Hash_Table.h:17 */
#define FSV_K_WIDE           95 /* widest threshold of the wide-band kernels (191 rows in six 32-bit limbs): ONT-profile reads */

typedef struct fsv_ctx fsv_ctx;

/* ---- context ----------------------------------------------------------- */
int  fsv_ctx_create(int device, fsv_ctx **out);
void fsv_ctx_destroy(fsv_ctx *ctx);
/* use an existing HIP stream (e.g. torch.cuda.current_stream().cuda_stream); 0 = the context's own */
int  fsv_ctx_set_stream(fsv_ctx *ctx, void *hip_stream);
int  fsv_ctx_sync(fsv_ctx *ctx);
const char *fsv_last_error(const fsv_ctx *ctx);
const char *fsv_strerror(int code);
int  fsv_version(void);
/* device properties the benchmarks print: CU count, clock (kHz), HBM bytes */
int  fsv_device_info(const fsv_ctx *ctx, int *n_cu, int *clock_khz, uint64_t *hbm_bytes, char *name, size_t name_cap);

/* raw device memory helpers for callers without torch */
int  fsv_dev_alloc(fsv_ctx *ctx, size_t bytes, void **dev_ptr);
int  fsv_dev_free(fsv_ctx *ctx, void *dev_ptr);
int  fsv_h2d(fsv_ctx *ctx, void *dev_dst, const void *host_src, size_t bytes);
int  fsv_d2h(fsv_ctx *ctx, void *host_dst, const void *dev_src, size_t bytes);

/* ---- K0: read store ------------------------------------------------------
 * Replaces hifiasm's FASTA ingest + ha_compress_base (Assembly.cpp:21-65).
 * Host-side packing of ASCII reads into the layout above.
 *   seqs      concatenated ASCII bases of all reads
 *   seq_off   n_reads+1 offsets into seqs
 *   words     out, capacity words_cap (>= fsv_pack_bound)
 *   word_off  out, n_reads+1 word offsets (read r occupies [word_off[r], word_off[r+1]))
 */
size_t fsv_pack_bound(const uint64_t *seq_off, uint32_t n_reads);
int    fsv_pack_reads(const char *seqs, const uint64_t *seq_off, uint32_t n_reads,
                      uint32_t *words, size_t words_cap, uint64_t *word_off);

/* ---- K5: batched banded bit-parallel edit distance -------------------------
 * Replaces Reserve_Banded_BPM / Reserve_Banded_BPM_4_SSE_only as driven by
 * verify_window (hifiasm-0.14 Levenshtein_distance.h:274-461, 893-1198;
 * Correct.cpp:203-250, 306-531).  One task = one (x window, overlapping read) pair.
 */
typedef struct fsv_wtask {
    uint32_t x_word;   /* word offset of read x in the store */
    uint32_t y_word;   /* word offset of read y */
    int32_t  x_start;  /* first base of the window in x (forward strand) */
    int32_t  y_start;  /* chain-predicted partner of x_start in y's strand coordinates (before the -k pad) */
    int32_t  y_len;    /* length of read y */
    uint16_t x_len;    /* 1..FSV_WINDOW */
    uint8_t  k;        /* error threshold, band = 2k+1, <= FSV_K_MAX (hifiasm) or <= FSV_K_WIDE (wide-band kernels) */
    uint8_t  y_rev;    /* 1: y is read on its reverse-complement strand */
    uint32_t ovl;      /* caller tag: overlap id */
    uint32_t win;      /* caller tag: window index inside the overlap */
} fsv_wtask;           /* 32 bytes */

typedef struct fsv_wres {
    int32_t end_site;    /* 0-based end offset inside the padded y window, -1 = no alignment within k */
    int32_t err;         /* edit distance, -1 = none */
    int32_t y_beg;       /* first y base covered by the padded window after clipping to the read (determine_overlap_region) */
    int16_t extra_begin; /* 'N' columns padded in front (window starts before the read) */
    int16_t extra_end;   /* 'N' columns padded behind */
} fsv_wres;              /* 16 bytes */

/* K6 result of one window task: the alignment path after generate_cigar's end trimming and gap left-shift
 * (Reserve_Banded_BPM_PATH + generate_cigar, Levenshtein_distance.h:511-888, Correct.cpp:1387-1536). */
typedef struct fsv_wpath {
    int32_t ry_start, ry_end;   /* aligned y interval in y's strand coordinates (inclusive) */
    int16_t path_len, err;      /* ops in the path; edit distance after trimming */
    uint8_t state;              /* 0 no alignment within k, 1 path present */
    uint8_t y_rev;
    uint16_t pad;
    uint32_t y_word;
    int32_t y_len;
    uint8_t ops[104];           /* 2 bits per op, start-to-end: 0 match 1 mismatch 2 y-only 3 x-only; at most 416 ops */
} fsv_wpath;                    /* 128 bytes */

/* K5 + K6 over host tasks (test / integration entry point; fsv_assemble_batch runs the same kernels on its own task list):
 * res[i] as fsv_bpm_windows, paths[i] for every task with res[i].err >= 0. */
int fsv_bpm_paths(fsv_ctx *ctx, const uint32_t *store, size_t store_words, const fsv_wtask *tasks,
                  uint32_t n_tasks, fsv_wres *res, fsv_wpath *paths);

int fsv_bpm_windows_dev(fsv_ctx *ctx, const uint32_t *store_dev, const fsv_wtask *tasks_dev,
                        uint32_t n_tasks, fsv_wres *res_dev);
/* host convenience wrapper (copies in, runs, copies out) */
int fsv_bpm_windows(fsv_ctx *ctx, const uint32_t *store, size_t store_words, const fsv_wtask *tasks,
                    uint32_t n_tasks, fsv_wres *res);

/* ---- assembler boundary -----------------------------------------------------
 * Replaces the process boundary `hifiasm -o <prefix> -t <T> <reads.fa>` and the GFA
 * read-back (focalsv/3_assembly/run_assembly.py:15-44, post_assembly.py:79-95).
 * One "read set" = one FASTA the reference would hand to one hifiasm process
 * (PS<ps>_hp1.fa, PS<ps>_hp2.fa of a region).  Many sets are assembled per call: a
 * single 50 kb region cannot fill 256 CUs.
 *
 * Stages (hifiasm-0.14 file:line in DESIGN.md): minimizer sketch -> per-read index ->
 * anchors + chaining -> 375-bp window verification (K5) -> rescue/accept -> window
 * paths (K6) -> per-column consensus (K8) -> re-pack + reverse-complement, n_rounds
 * times; then exact overlaps, layout, contig stitching.
 */
typedef struct fsv_asm_params {
    int32_t k, w, hpc;        /* minimizer scheme; hifiasm defaults 51, 51, 1 (CommandLines.cpp:109-166) */
    int32_t n_rounds;         /* correction rounds, 3 */
    int32_t min_ovlp;         /* shortest overlap kept in a correction round: 1 -- hifiasm keeps every (target, strand) group that shares a minimizer,
                               * however short (calculate_overlap_region_by_chaining, Hash_Table.cpp:684-745); the ONT / CLR profiles: 500 */
    int32_t min_anchors;      /* shortest chain kept: 1 (the same); the ONT / CLR profiles: 3 */
    int32_t lookback;         /* chain DP predecessors examined, 64 (= one wavefront) */
    int32_t bw_ec;            /* chain indel budget per mille in correction rounds, 20 (hifiasm 0.02) */
    int32_t bw_final;         /* ... in the final overlap pass, 0 = co-linear anchors only */
    int32_t min_contig_reads; /* chains of fewer reads are dropped, as hifiasm's asg_cut_tip(max_short_tip = 3) does (Overlaps.cpp:4666): 4 */
    /* error model: hifiasm's constants for HiFi reads; fsv_asm_ont_params() raises them for ONT-profile reads (10 % error), where the
     * reference runs Flye / Shasta instead (run_assembly.py:74-100) */
    int32_t win_rate_pm;      /* window threshold = x_len x this / 1000: 40 (max_ov_diff_ec 0.04: k = 15 = FSV_K_FULL for a full window) */
    int32_t k_cap;            /* largest threshold the rescue pass doubles to: 31 = FSV_K_MAX (THRESHOLD_MAX_SIZE); at most FSV_K_WIDE */
    int32_t accept_err_pm;    /* an overlap is used when its error rate is at most this / 1000: 30 (Correct.cpp:725) */
    int32_t bw_rechain;       /* indel budget per mille when the final pass re-chains a pair without an exact overlap: 1 (max_ov_diff_final 0.001) */
    int32_t w_later;          /* minimizer window from the second correction round on; 0 = w throughout (hifiasm) */
    int32_t partition;        /* 1: haplotype partition of every read's overlaps before the consensus, as hifiasm (partition_overlaps_advance,
                               * Correct.cpp:7127); 0: off (the ONT profile: at 10 % error coincident errors pass for alleles) */
    int32_t second_round;     /* 1 (default): hifiasm's second consensus pass over the window junctions (process_boundary, Correct.cpp:4453): K5 + K6 +
                               * consensus once more per junction.  0: a vote on the bases both window alignments skip at a junction stands in for
                               * it -- a quarter faster, same reads after three rounds on all but one of 7 800 golden reads (ONT profile: 0) */
    int32_t ins_dag;          /* 1 (default): inserted strings that disagree go through hifiasm's DAG of inserted strings (build_DAGCon, Correct.cpp:3893);
                               * 0: the most frequent string is inserted (ONT profile) */
    int32_t min_anchors_final;/* shortest chain of the final overlap pass: 1 -- hifiasm keeps every (target, strand) group that shares a minimizer
                               * (calculate_overlap_region_by_chaining, Hash_Table.cpp:684-745: no minimum); 0 = min_anchors */
    int32_t min_ovlp_final;   /* shortest final overlap: 1 (the graph drops what is below 50 bases, ma_hit_cut, Overlaps.cpp:1785); 0 = min_ovlp */
    int32_t graph_layout;     /* 1 (default): the layout as hifiasm-0.14 makes it -- chimeric-read detection, containment in read order, string graph with
                               * transitive reduction and tip cutting, unitig polishing (Overlaps.cpp:1698, 1031, 2152, 4531, 4666, 7759, 8480, 8893) --
                               * for every set that is not flagged FSV_SET_UNPHASED; 0: best-buddy chains (ONT profile, unphased sets) */
    int32_t junction_cigars;  /* 1 (default): the haplotype partition reads the ~50 columns on each side of a window junction off the re-aligned
                               * junction cigar, as hifiasm does (calculate_boundary_cigars, Correct.cpp:2310; markSNP_advance :5054); 0: window cigars */
    int32_t deep_sets;        /* 0 (default in all three profiles): a consensus window or junction holds 256 inserted-base events in LDS (2 048 with the
                               * wide-band profiles); a deeper one drops the rest and its read gets FSV_W_INS_EVENTS.  1: no vote is dropped and the bit
                               * is never raised -- such a window, and one with more than 255 overlaps (whose 8-bit "after an insertion" counters
                               * could wrap), is listed on the device and redone by k_consensus_deep / k_bnd_consensus_deep with its events in a slab
                               * of HBM and 16-bit counters; corrected reads and contigs are the oracle's at any depth.  Any other value is FSV_EINVAL.
                               * What the two kernels took: fsv_asm_last_deep_windows.  (In front of full_lists: the struct's tail is pinned, see there.) */
    int32_t full_lists;       /* 0 (default in all three profiles): a read's per-read index holds its first 4 096 minimizers (FSV_W_MZ_TRUNC beyond) and a
                               * pair's chain the anchors its LDS tile holds (FSV_W_ANCHOR_TRUNC beyond).  1: neither is cut and neither bit is raised --
                               * lists above 4 096 entries are sorted through HBM (k_uniq_long), pairs above the tile are chained in an HBM slab
                               * (k_chain_spill); the result is the oracle's at any read length.  Any other value is FSV_EINVAL.  A read's minimizer slot holds
                               * len + 64 entries and the index two per unique minimizer; with w <= 2 (or 0 < w_later <= 2) that can be more, so with
                               * the option such a call gets slots of 2 len + 64 (the default keeps its slots, and FSV_W_INTERNAL for such a list).
                               * What the two kernels took: fsv_asm_last_long_lists.  (In front of kmer_filter: the struct's tail is pinned, see there.) */
    int32_t kmer_filter;      /* 0 (default in all three profiles): off.  1 (needs kmer_table = 1, else FSV_EINVAL): hifiasm's high-count k-mer filter in
                               * every sketch of the assembly (ha_ft_isflt in ha_sketch, sketch.cpp:89; every round and the final pass take the one
                               * filter of the raw reads): a k-mer on its set's filter list keeps its slot in the window but is no candidate.  Sets
                               * flagged FSV_W_LOW_COV are left alone as with kmer_table alone.  The figures of hifiasm's first ha_pt_gen on the
                               * filtered sketch stay on the context: fsv_asm_last_kmer_index.  (In front of kmer_table: the struct ends with
                               * kmer_table, partial_charge, which tests/test_partial_charge_abi.py pins.) */
    int32_t kmer_table;       /* 0 (default in all three profiles): off.  1: hifiasm's k-mer count table per read set before round 0 (ha_ft_gen, htab.cpp:917;
                               * see fsv_kmer_table) at (w = 1, k, hpc) -- a set whose count histogram has no coverage peak is left as hifiasm leaves
                               * it: reads uncorrected, no contig, FSV_W_LOW_COV | FSV_W_NO_LAYOUT; every other set is assembled as with 0 */
    int32_t partial_charge;   /* 0 (default in all three profiles): an unmatched window costs an overlap its whole length.  1: hifiasm's non_trim_error_rate
                               * (Correct.cpp:725-845): the window is charged what two banded extension alignments -- from the left neighbour's exact end,
                               * from the right neighbour's exact start, doubled threshold -- leave uncovered, plus their errors, and every overlap's error
                               * sum counts the matched windows' distances after generate_cigar (see fsv_bpm_extensions, fsv_asm_last_charge).  Needs
                               * k_cap <= FSV_K_MAX: FSV_EINVAL with the wide-band profiles */
} fsv_asm_params;
void fsv_asm_default_params(fsv_asm_params *p);
/* ONT-profile reads (BASELINE configs[4]: ~10 % error): k = 15, w = 15 without homopolymer compression (a 30 kb read then has ~3 750 minimizers: below the 4 096 a list holds by default; full_lists = 1 lifts that cap), chain indel budget 0.15 / 0.05,
 * windows up to 25 % apart (k = 93: wide-band K5 / K6), overlaps up to 30 % error.  Parity unpinned: the reference has Flye here. */
void fsv_asm_ont_params(fsv_asm_params *p);
/* CLR reads (~12 % error, insertion-rich; the reference: flye --pacbio-raw, run_assembly.py:46-72): the ONT profile's values under a name of
 * their own.  Parity unpinned (no Flye in the tree or the image); planted truth in tests/test_gpu_ont.py.  Reads above ~32 kb lose the anchors
 * beyond their first 4 096 minimizers in either profile (set status bits 1 / 2 say so) unless full_lists = 1, which is off in both. */
void fsv_asm_clr_params(fsv_asm_params *p);

typedef struct fsv_mz {       /* ha_mz1_t, htab.h:8-13 */
    uint64_t hash;
    uint32_t pos;             /* index of the k-mer's last base */
    uint8_t  rev, span;
    uint16_t pad;
} fsv_mz;                     /* 16 bytes */

typedef struct fsv_ovl {      /* overlap_region / ma_hit_t, Hash_Table.h:67-101, Overlaps.h:56-64 */
    uint32_t q, t;            /* read indices inside the set */
    int32_t x_s, x_e;         /* inclusive range on q (forward strand) */
    int32_t y_s, y_e;         /* inclusive range on t, strand coordinates */
    int32_t score, n_chain;
    int32_t chain_off;        /* unused on the device */
    int32_t first_win, n_win; /* window tasks of this overlap */
    int32_t align_len, err_sum;
    uint8_t rev, is_match, exact, valid;
} fsv_ovl;                    /* 56 bytes */

typedef struct fsv_readsets {
    const uint32_t *store_dev;  /* device: 2-bit read store */
    const uint64_t *word_off;   /* host: n_reads+1 word offsets into the store */
    const int32_t  *read_len;   /* host: n_reads lengths in bases */
    const uint32_t *set_start;  /* host: n_sets+1 read indices; set s owns reads [set_start[s], set_start[s+1]) */
    uint32_t n_reads, n_sets;
    const uint8_t  *set_flags;  /* host: n_sets flags, or NULL; informational since round 2 (see FSV_SET_UNPHASED) */
} fsv_readsets;
#define FSV_SET_UNPHASED 1      /* unphased.fa (run_assembly.py:17-21).  The haplotype partition that keeps the other allele's overlaps out
                                 * of a read's consensus (partition_overlaps_advance, Correct.cpp:7127) runs for EVERY set, as in hifiasm,
                                 * so the flag no longer changes the result; callers may keep passing it */

typedef struct fsv_contigs {
    char     *seq;         /* host, capacity seq_cap: ASCII contig bases back to back */
    uint64_t  seq_cap;
    uint64_t *off;         /* host, capacity contig_cap+1 */
    uint32_t *set;         /* host, capacity contig_cap: owning set of each contig */
    uint32_t *n_reads;     /* host, capacity contig_cap: reads laid out in each contig */
    uint32_t  contig_cap;
    uint32_t  n_contigs;   /* out */
    int32_t  *set_status;  /* host, n_sets: 0 ok, >0 warning bits (FSV_W_*), <0 FSV_E* for that set only */
} fsv_contigs;

#define FSV_W_MZ_TRUNC     1  /* a read had more minimizers than the per-read cap; the rest were ignored */
#define FSV_W_ANCHOR_TRUNC 2  /* a read pair had more anchors than the chaining tile holds */
#define FSV_W_NO_LAYOUT    4  /* no chain of min_contig_reads reads: the set has no contig (hifiasm writes an empty GFA for it too) */
#define FSV_W_INS_EVENTS   8  /* a consensus window saw more inserted-base events than its buffer holds; the extra votes were dropped
                                 * (never with fsv_asm_params.deep_sets = 1) */
#define FSV_W_WINDOW_KEPT 16  /* a corrected window would have outgrown its slot; the read keeps that window uncorrected */
#define FSV_W_INTERNAL    32  /* a minimizer slot overflowed (cannot happen: one minimizer per base at most) */
#define FSV_W_SITES       64  /* haplotype partition: more than 255 candidate sites in a window, 1 024 in a read (512 once sites beside another site are
                                 * dropped), or the site pool ran out;
                                 * that window's sites / that read's partition were skipped */
#define FSV_W_LOW_COV    128  /* kmer_table = 1: the set's k-mer count histogram has no coverage peak (ha_analyze_count returns -1); hifiasm then
                                 * filters every k-mer, finds no overlap and writes no contig, and so does this set (comes with FSV_W_NO_LAYOUT) */

/* capacity needed for fsv_contigs.seq / contig count for these read sets */
int fsv_assemble_batch_bound(const fsv_readsets *sets, uint64_t *seq_cap, uint32_t *contig_cap);
int fsv_assemble_batch(fsv_ctx *ctx, const fsv_readsets *sets, const fsv_asm_params *params, fsv_contigs *out);

/* Optional per-stage counters of the last fsv_assemble_batch on this context (for the roofline accounting):
 * window tasks verified (K5), paths computed (K6), DP column steps, algorithmic bytes (SURVEY.md 8d model). */
#define FSV_MAX_KERNEL_STATS 24
typedef struct fsv_kernel_stat {
    char     name[24];
    double   ms;           /* summed HIP-event time of this kernel's launches on the context's stream */
    uint64_t launches;
    uint64_t algo_bytes;   /* compulsory bytes in + out of those launches (per-kernel table) */
} fsv_kernel_stat;

typedef struct fsv_asm_stats {
    uint64_t n_pairs, n_overlaps, n_windows, n_windows_matched, n_paths, n_path_dp;
    uint64_t dp_columns;       /* K5 + K6 column steps (windows x their x_len) */
    uint64_t algo_bytes;       /* packed operand + result bytes of all DP tasks + reads in + contigs out */
    uint64_t n_exact_overlaps;  /* overlaps handed to the layout (exact, or inexact ones the last correction round verified) */
    uint64_t n_inexact_candidates; /* pairs re-chained with the gapped bandwidth in the final pass */
    uint64_t n_path_fr;         /* of those, distance <= 3: walked without the DP matrix (k_path_fr) */
    uint64_t n_junction_cigars; /* junctions re-aligned for the haplotype partition (k_bcig_tasks) */
    uint64_t n_junction_used;   /* of those, cigars the partition reads (accepted, and showing something the window cigars do not) */
    double   ms_sketch, ms_chain, ms_verify, ms_path, ms_consensus, ms_final, ms_total;
    uint32_t n_kernels, pad;
    fsv_kernel_stat kernels[FSV_MAX_KERNEL_STATS];
} fsv_asm_stats;
int fsv_asm_last_stats(const fsv_ctx *ctx, fsv_asm_stats *out);
/* full_lists = 1, the last fsv_assemble_batch on this context, all rounds, the final pass and chunks: minimizer lists above 4 096 entries that
 * k_uniq_long indexed, and pairs beyond the chaining tile that k_chain_spill chained (their kernel times: the rows "k_uniq_long" and
 * "k_chain_spill" of fsv_asm_stats.kernels, outside the k_uniq / k_chain rows).  Both 0 after a call with full_lists = 0. */
int fsv_asm_last_long_lists(const fsv_ctx *ctx, uint64_t *n_reads, uint64_t *n_pairs);
/* deep_sets = 1, the last fsv_assemble_batch on this context, all rounds and chunks: windows that k_consensus_deep and junctions that
 * k_bnd_consensus_deep redid (list entries: a window that both k_consensus and the redo after the haplotype partition set aside counts
 * twice), and the largest number of inserted-base events one of them held (their kernel times: the rows "k_consensus_deep" and
 * "k_bnd_consensus_deep" of fsv_asm_stats.kernels).  All 0 after a call with deep_sets = 0. */
int fsv_asm_last_deep_windows(const fsv_ctx *ctx, uint64_t *n_windows, uint64_t *n_junctions, uint32_t *max_events);

/* Test hook: after fsv_assemble_batch(...) with n_rounds = r, the corrected reads of the last round
 * can be fetched as ASCII (same order as the input reads). */
int fsv_asm_fetch_reads(fsv_ctx *ctx, char *seq, uint64_t seq_cap, uint64_t *off, uint32_t n_reads);

/* Test hook: the overlap stage of ONE pass of fsv_assemble_batch on the caller's read sets, up to the end of chaining -- sketch, per-read
 * index, k_chain -- through the code the batch call runs (same launches, same tile choice), and the raw records it leaves.
 *   pass 0  a correction round: bw_ec, min_anchors, min_ovlp; window tasks are emitted
 *   pass 1  the final pass (as with n_rounds = 0): w_later, bw_final, min_anchors_final, min_ovlp_final; no tasks
 *   pass 2  pass 1, then the gapped re-chain (bw_rechain, either direction chained from its own side) of the n_rechain unordered
 *           pairs listed in `rechain`; the slots of the other pairs keep their pass-1 records
 * ovl       one record per ORDERED pair slot, ovl_cap >= sum over the sets of ns (ns - 1).  Set s owns slots [pair_base[s],
 *           pair_base[s + 1]); with q, t the read indices inside the set (ns reads), the slot of (q, t) is
 *           pair_base[s] + q (ns - 1) + (t < q ? t : t - 1).  A slot without an overlap has valid == 0.
 * pair_base n_sets + 1 entries (out).  The UNORDERED pair (q < t) of set s has index pair_base[s] / 2 + q (2 ns - q - 1) / 2 + (t - q - 1):
 *           the entries of `rechain`.
 * tasks     the window tasks in the order the kernel's atomics gave them (an overlap's tasks are [first_win, first_win + n_win));
 *           task_cap >= sum over the sets of (grid windows of the set) x (ns - 1) always suffices.  *n_tasks: how many.
 * overflow  1 when the library's own task array ran full (then the overlaps hit have valid == 0)
 * warn      n_reads words of FSV_W_* bits, per read */
int fsv_asm_overlaps(fsv_ctx *ctx, const fsv_readsets *sets, const fsv_asm_params *params, int32_t pass, const uint32_t *rechain,
                     uint32_t n_rechain, fsv_ovl *ovl, uint64_t ovl_cap, uint32_t *pair_base, fsv_wtask *tasks, uint64_t task_cap,
                     uint32_t *n_tasks, uint32_t *overflow, uint32_t *warn);

/* ---- the per-read index exposed (test hook): the sketch and the unique-minimizer index as the chain kernels see it, through the
 * launch code of fsv_assemble_batch's overlap stage.  Read r with m minimizers whose hash occurs once in the read gets 2m entries at
 * out_mz[out_off[r] .. out_off[r + 1]): [0, m) sorted by hash, [m, 2m) the same entries sorted by position; out_off has n_reads + 1 entries.
 * full_lists as in fsv_asm_params: 0 cuts a list at 4 096 raw entries (warn[r] gets FSV_W_MZ_TRUNC), 1 indexes every entry; another value
 * is FSV_EINVAL.  (w, k) as fsv_sketch_reads takes them with variant 0; the slots are the assembly's for the same (w, full_lists).
 * warn: n_reads words of FSV_W_* bits. */
int fsv_read_index(fsv_ctx *ctx, const fsv_readsets *sets, int32_t w, int32_t k, int32_t hpc, int32_t full_lists,
                   fsv_mz *out_mz, uint64_t out_cap, uint64_t *out_off, uint32_t *warn);

/* ---- K1 exposed: minimizer sketch of every read (ha_sketch, sketch.cpp:39-137) -------------------------
 * out_mz receives, per read, its minimizers in position order; out_off (n_reads+1) indexes them.
 * variant: 0 = library's choice (position-parallel kernel for odd k, deque replay otherwise), 1 = force the replay kernel.
 * 1 <= k <= 63; 1 <= w <= 255 where the position-parallel kernel runs (odd k, variant 0), w <= 64 where the replay kernel does
 * (even k, or variant 1): FSV_EINVAL otherwise, and fsv_last_error names the limit that applied. */
int fsv_sketch_reads(fsv_ctx *ctx, const fsv_readsets *sets, int32_t w, int32_t k, int32_t hpc, int32_t variant,
                     fsv_mz *out_mz, uint64_t out_cap, uint64_t *out_off);

/* The same through the sets' high-count k-mer filters (ha_sketch with hf != 0, sketch.cpp:89) -- the stage hook of kmer_filter = 1: the
 * filter sets are built from the caller's lists by the launch code fsv_assemble_batch runs, and every read of set s (sets->set_start, sets->n_sets)
 * is sketched against list s = flt_hash[flt_off[s] .. flt_off[s + 1]) (n_sets + 1 offsets from 0), as fsv_kmer_table hands them out.  A listed
 * k-mer keeps its slot in the window and is never reported; a window of listed k-mers reports nothing.  The lists need not be sorted and may
 * repeat a hash; UINT64_MAX in a list is FSV_EINVAL.  flt_hash == NULL, or lists that are all empty: the bytes of fsv_sketch_reads.  The
 * (w, k, variant) limits are those of fsv_sketch_reads. */
int fsv_sketch_reads_filtered(fsv_ctx *ctx, const fsv_readsets *sets, int32_t w, int32_t k, int32_t hpc, int32_t variant,
                              fsv_mz *out_mz, uint64_t out_cap, uint64_t *out_off, const uint64_t *flt_hash, const uint64_t *flt_off);

/* ---- k-mer count table of a read set (ha_ft_gen / ha_analyze_count, htab.cpp:917-950, hist.cpp:15-96) ----------
 * Keys: the 64-bit hash of every entry the sketch emits for (w, k, hpc) -- with w = 1 every k-mer ha_sketch accepts, both strands
 * counted together.  Count: occurrences over all reads of the set, saturating at 4095.  hist[c]: distinct keys with count c. */
typedef struct fsv_kmer_set {           /* one read set */
    int32_t  peak_hom, peak_het;        /* -1: none */
    int32_t  cutoff, low_i, max_i;      /* cutoff: (int)(peak_hom x 5.0), at most 4094, -5 without a peak; max_i -1 when there is no peak */
    int32_t  pad;
    uint64_t n_entries, n_distinct;     /* sketch entries counted; distinct keys */
    uint64_t n_filtered, n_indexed;     /* distinct keys with count >= cutoff (all of them without a peak); sum of c x hist[c], c = 2..4094 */
} fsv_kmer_set;                         /* 56 bytes */
/* pure host function, no GPU: ha_analyze_count over n_cnt bins (3 <= n_cnt, 0 <= start_cnt < n_cnt; hifiasm: 4096, 5).  Returns peak_hom, -1 when
 * the histogram has no peak, FSV_EINVAL on a bad argument */
int fsv_kmer_peaks(const int64_t *hist, int32_t n_cnt, int32_t start_cnt, int32_t *peak_het, int32_t *low_i, int32_t *max_i);
/* the stage alone, on the caller's read sets (per-set, unlike fsv_sketch_reads); (w, k) as fsv_sketch_reads takes them with variant 0.
 * out: n_sets records.
 * hist: n_sets x 4096 uint64 or NULL.
 * flt_hash / flt_off (n_sets + 1): every set's filtered hashes in ascending order, or both NULL; FSV_ECAP when flt_cap is too small. */
int fsv_kmer_table(fsv_ctx *ctx, const fsv_readsets *sets, int32_t w, int32_t k, int32_t hpc,
                   fsv_kmer_set *out, uint64_t *hist, uint64_t *flt_hash, uint64_t flt_cap, uint64_t *flt_off);
/* verdicts of the last fsv_assemble_batch with kmer_table = 1 on this context, all chunks, in set order (n_sets: that call's; FSV_EINVAL
 * otherwise, or when that call ran with kmer_table = 0); ms: the stage's summed kernel time */
int fsv_asm_last_kmer_table(const fsv_ctx *ctx, fsv_kmer_set *out, uint32_t n_sets, double *ms);

/* ---- the minimizer index figures of a read set (hifiasm's first ha_pt_gen, htab.cpp:952-998) ----------
 * The count table at (w = 1, k, hpc), its filter list, the sketch at (w, k, hpc) through that filter, and the count table's kernels on what
 * that sketch emits. */
typedef struct fsv_kmer_index_set {     /* one read set */
    uint64_t n_entries, n_distinct;     /* entries of the filtered sketch; distinct minimizers (hifiasm: "counted") */
    uint64_t n_indexed;                 /* sum of c x hist[c], c = 2..4094 (hifiasm: "indexed" positions) */
    int32_t  low_i, max_i;              /* the histogram's lowest point and highest peak (-1: none) */
    int32_t  peak_hom, peak_het;        /* peak_hom: hifiasm's hom_cov from round 0 on; -1: none */
} fsv_kmer_index_set;                   /* 40 bytes */
/* per-set on the caller's read sets; (w, k) as fsv_kmer_table takes them.  table / index: n_sets records each; hist: the index histograms,
 * n_sets x 4096 uint64, or NULL.  A set without a peak in its table has cutoff -5: every k-mer is filtered and its index is that of nothing
 * (counts 0, no peak), as hifiasm logs. */
int fsv_kmer_index(fsv_ctx *ctx, const fsv_readsets *sets, int32_t w, int32_t k, int32_t hpc,
                   fsv_kmer_set *table, fsv_kmer_index_set *index, uint64_t *hist);
/* the index figures of round 0 of the last fsv_assemble_batch with kmer_filter = 1 on this context, all chunks, in set order (n_sets: that
 * call's; FSV_EINVAL otherwise, or when that call ran with kmer_filter = 0); ms: the summed kernel time of the filter-set build and the index */
int fsv_asm_last_kmer_index(const fsv_ctx *ctx, fsv_kmer_index_set *out, uint32_t n_sets, double *ms);

/* ---- partial charge of unmatched windows (non_trim_error_rate, Correct.cpp:725-845; fsv_asm_params.partial_charge) ----------
 * The extension alignment (Reserve_Banded_BPM_Extension, Levenshtein_distance.h:14-205): K5's recurrence, and after every column the
 * best band cell within k; the extension ends at the last x column that has one. */
typedef struct fsv_wext {
    int32_t t_end;   /* last x column with a band cell within k, -1: none (or the window geometry was rejected) */
    int32_t err;     /* its distance, -1: none */
    int32_t p_end;   /* offset inside the padded y window it ends at, -1: none */
    int32_t pad;     /* 0 */
} fsv_wext;          /* 16 bytes */
/* The extension kernel alone, on host tasks, through the launch code fsv_assemble_batch runs with partial_charge = 1.  A task is read as
 * K5 reads it: y_start is the strand coordinate where the window's first x base is placed, k the (already doubled) threshold <= FSV_K_MAX,
 * the padded window columns y_start - k .. y_start + x_len + k - 1 ('N' outside the read); the geometry rule is K5's with k_cap.
 * dir[i] = 0: x against the padded window.  dir[i] = 1: both strings reversed; the results are in the reversed coordinates. */
int fsv_bpm_extensions(fsv_ctx *ctx, const uint32_t *store, size_t store_words, const fsv_wtask *tasks, const uint8_t *dir,
                       uint32_t n_tasks, int32_t k_cap, fsv_wext *out);

/* The charge itself (Correct.cpp:820-838): an unmatched window of n bases, al0 bases covered from the left with er0 errors, al1 from the
 * right with er1 (al = 0: no extension on that side), terr the overlap's running error total; returns the new total.  Where the two
 * extensions overlap the reference scales their errors in single precision, so the running total takes part.  Pure host function. */
int64_t fsv_partial_charge(int32_t n, int32_t al0, int32_t er0, int32_t al1, int32_t er1, int64_t terr);

typedef struct fsv_charge_stats {
    uint64_t n_overlaps;   /* overlaps that passed the 0.9 filter with at least one unmatched window */
    uint64_t n_windows;    /* unmatched windows charged */
    uint64_t n_ext;        /* extension alignments run (at most 2 per window) */
    uint64_t n_accepted;   /* of n_overlaps: accepted */
    uint64_t n_flipped;    /* of n_accepted: the full-length charge (same matched distances) would have rejected them */
    double   ms;           /* summed kernel time of the stage (k_charge_tasks, k_bpm_ext, k_charge_accept) */
} fsv_charge_stats;
/* counters of the last fsv_assemble_batch on this context, all rounds and chunks; FSV_EINVAL when that call ran with partial_charge = 0 */
int fsv_asm_last_charge(const fsv_ctx *ctx, fsv_charge_stats *out);

/* ---- aligner boundary ---------------------------------------------------------
 * Replaces `minimap2 -a -x asm5 --cs -r2k ref_chr.fa assemblies.fa | samtools sort` and the pysam read-back
 * (focalsv/4_sv_calling/Dippav/DipPAV_variant_call.py:103-112; fields consumed by
 * extract_contig_signature_CCS.py:14-47, 279-282, 347-356: reference_name, pos, reference_end, cigar with
 * ops {0 M, 1 I, 2 D, 4 S, 5 H}, qname, is_reverse, mapq).  Every contig is aligned against the reference
 * window of its own region (the caller adds the window's chromosome offset to ref_start/ref_end).
 * minimap2 itself is not part of the reference tree; scoring is its published asm5 preset and the DP
 * follows the in-tree ksw2 (software/hifiasm-0.14/ksw2_extz2_sse.c, ksw2.h:115-150).
 */
typedef struct fsv_aln_params {
    int32_t k, w;               /* seeds: 19, 19; w grows with the sequence length (len/3000 + 1) */
    int32_t min_anchors, lookback, max_gap;  /* 3, 64, 50000: one chain runs across any SV DipPAV calls (max_svlen, extract_contig_signature_CCS.py:411) */
    int32_t a, b, q, e, q2, e2; /* asm5: 1, 19, 39, 3, 81, 1 */
    int32_t pad;                /* identical bases added on each side of a DP event, 24 */
    int32_t max_mm_run;         /* equal-length inter-seed run with <= this many mismatches stays M, 4 */
    int32_t xdrop;              /* gap-free end extension, 100 */
    int32_t max_cells;          /* largest DP event, 2^26 cells; a larger one (both copies of a duplication between two unique seeds) is seeded
                                   again on its own, and what is still larger inside it is closed from its corners: never refused */
} fsv_aln_params;
void fsv_aln_default_params(fsv_aln_params *p);

typedef struct fsv_aln_rec {
    int32_t  ref_start, ref_end;  /* 0-based in the window, end exclusive (pysam pos / reference_end) */
    int32_t  q_start, q_end;      /* aligned part of the strand-oriented contig */
    uint32_t n_cigar;
    uint32_t n_chain;
    uint64_t cigar_off;           /* into fsv_alns.cigar */
    uint32_t contig;              /* index of the contig */
    uint8_t  rev, mapq, pad[2];
} fsv_aln_rec;                    /* 40 bytes */

typedef struct fsv_alns {
    fsv_aln_rec *rec;       /* host, capacity rec_cap: 5 x n_contigs holds every case (FSV_ALN_MAX_REC records per contig) */
    uint32_t  rec_cap, n_rec;
    uint32_t *cigar;        /* host, BAM encoding len << 4 | op */
    uint64_t  cigar_cap, n_cigar;
    int32_t  *contig_status; /* host, n_contigs: 0 aligned, 1 no chain (unaligned), <0 FSV_E* for that contig */
} fsv_alns;

#define FSV_ALN_MAX_REC 5
/* contig i is aligned to reference window contig_ref[i].  A contig yields its primary record and, when the primary chain leaves
 * part of the contig uncovered (an SV beyond max_gap), up to two supplementary records on the same strand -- consecutive in
 * `rec`, primary first, soft clips for the parts the record does not align -- from which DipPAV's split-alignment rules call the
 * SV (extract_contig_signature_CCS.py:251-327).  An inverted piece of the contig comes back as one record of the other strand
 * (rev differs), and the record it interrupts is cut in two around it: the split rule pairs records of one strand only (:286),
 * so an inversion yields no INS / DEL call, as with minimap2's reverse-strand supplementary alignment.
 * contig_seq == NULL (contig_off ignored): align the n_contigs contigs of the last fsv_assemble_batch on this context straight
 * from device memory, in their output order -- the device-resident hand-off between the two boundaries.
 * Reference windows may hold N (anything but ACGT / acgt): an N pairs with nothing, costs 1 in the alignment score (minimap2's sc_ambi)
 * and does not seed; the alignment runs through a short run of N as 'M'. */
int fsv_align_batch(fsv_ctx *ctx, const char *contig_seq, const uint64_t *contig_off, uint32_t n_contigs,
                    const uint32_t *contig_ref, const char *ref_seq, const uint64_t *ref_off, uint32_t n_refs,
                    const fsv_aln_params *params, fsv_alns *out);

typedef struct fsv_aln_stats {
    uint64_t n_pairs, n_events, dp_cells, algo_bytes;
    double ms_seed, ms_chain, ms_events, ms_dp, ms_total;
    uint64_t n_boxes;       /* events larger than max_cells that were seeded again */
} fsv_aln_stats;
int fsv_aln_last_stats(const fsv_ctx *ctx, fsv_aln_stats *out);

/* single global alignment (the DP of one event), exposed for known-answer tests against ksw2 */
int fsv_nw(fsv_ctx *ctx, const char *target, int32_t tl, const char *query, int32_t ql, const fsv_aln_params *params,
           int32_t *score, uint32_t *cigar, uint32_t cigar_cap, uint32_t *n_cigar);

/* ---- NM / cs tags of alignment records (what `--cs` adds to minimap2's output; opt-in, nothing runs unless this is called) ----
 * alns: records as fsv_align_batch returns them (contig, rev, ref_start / ref_end, cigar_off / n_cigar are read); they are the
 * caller's: any CIGAR of the ops M, I, D, S, H is taken, another op is FSV_EUNSUP for the call.  The sequences are given as in
 * fsv_align_batch, or contig_seq == NULL && ref_seq == NULL: the sequences the last fsv_align_batch on this context left packed on
 * the device (FSV_EINVAL when there are none, or when n_contigs / n_refs differ from that call's; fsv_nw and an fsv_aln_tags call
 * with sequences replace them).
 * Every record is checked on the host before anything is launched: its query-consuming ops, clips included, must sum to the
 * contig's length, ref_start plus its reference-consuming ops must equal ref_end, and ref_end must not exceed the window.  A
 * record that fails has rec_status FSV_EINVAL, nm -1 and an empty cs, and is not compared; the call still succeeds.
 * cs is the short form of minimap2's --cs as its manual page defines it: `:<n>` n identical columns, `*<ref><query>` a
 * substitution, `+<query bases>` an insertion, `-<ref bases>` a deletion; bases lower case (acgtn); clips are not represented; a
 * run of identical columns ends at the end of its M op.  Conventions of this library (pinned to that grammar, not to a minimap2
 * run): an N (anything but ACGT / acgt, on either side) pairs with nothing -- the column is written `*n<q>` (or `*<r>n`) and counts
 * in NM, as the aligner charges it; a record with rev = 1 is compared on the reverse complement of the contig, as SAM shows it.
 * Two passes on the device (count, scan, emit): a first call with cs == NULL only counts (nm, cs_off, cs_bytes are set); with
 * cs_cap < cs_bytes the call returns FSV_ECAP with cs_bytes set. */
struct fsv_aln_tags {     /* (no typedef: the call has the name, as stat() has beside struct stat) */
    int32_t  *nm;        /* host, n_rec: mismatched columns + inserted + deleted bases */
    uint64_t *cs_off;    /* host, n_rec + 1 offsets into cs */
    char     *cs;        /* host, capacity cs_cap: the records' cs strings back to back, no terminators; NULL: only count */
    uint64_t  cs_cap, cs_bytes;   /* cs_bytes out: bytes needed / written */
    int32_t  *rec_status;/* host, n_rec: 0, or FSV_EINVAL for a record whose CIGAR does not fit its sequences */
    double    ms;        /* out: summed kernel time */
};
int fsv_aln_tags(fsv_ctx *ctx, const char *contig_seq, const uint64_t *contig_off, uint32_t n_contigs, const uint32_t *contig_ref,
                 const char *ref_seq, const uint64_t *ref_off, uint32_t n_refs, const fsv_alns *alns, struct fsv_aln_tags *out);

/* ---- chromosome-level mapping quality of the contig records (opt-in, nothing runs or is allocated unless these are called) ----
 * fsv_align_batch aligns a contig to the window of its own region and stamps mapq 60.  The reference pipeline aligns to the whole
 * chromosome (minimap2 -x asm5) and drops records below mapq 50 (extract_contig_signature_CCS.py:679-680).  These calls give a record
 * the mapping quality of minimap2's published formula (Li 2018, Bioinformatics 34:3094, section 2.1.4) from this library's own chaining:
 * f1 the best chain score of the record's seeds at its own locus, f2 the best anywhere else on the chromosome, m the anchors of the
 * former.  Pinned to that formula and to tests/mapq_model.py, not to a minimap2 run; a paralog on another chromosome is not seen.
 *
 * The index (one per context; a new build replaces it, fsv_ref_index_drop or fsv_ctx_destroy frees it): the chromosome packed as one
 * sequence (an N holds a base hashed from its position, as in a window), cut into tiles that own FSV_REF_TILE k-mer end positions each
 * and are sketched with 64 bases of context on either side, HPC off; a minimizer is kept by the tile that owns its end, unless its k
 * bases cover an N.  The kept ones fill one open-addressed table by hash: a key's count, and for a count <= max_occ its occurrences
 * pos | rev << 31 in ascending position.  k odd, 1 <= k <= 31, 1 <= w <= 32, 1 <= max_occ <= 64, 0 < len < 2^31: FSV_EINVAL otherwise. */
#define FSV_REF_TILE 65536
typedef struct fsv_ref_stats {
    uint64_t tiles, owned, dropped_n;       /* minimizers whose end a tile owns; of those, dropped for an N */
    uint64_t keys, keys_above, stored;      /* distinct hashes; those with count > max_occ; occurrences stored */
    uint64_t slots, max_count;              /* of the table: a power of two, at least twice owned - dropped_n; the largest count */
    double ms;                              /* summed kernel time of the build */
} fsv_ref_stats;
int fsv_ref_index_build(fsv_ctx *ctx, const char *seq, uint64_t len, int32_t k, int32_t w, int32_t max_occ);
int fsv_ref_index_stats(const fsv_ctx *ctx, fsv_ref_stats *out);     /* FSV_EINVAL without an index */
int fsv_ref_index_drop(fsv_ctx *ctx);
/* stage hook: count_out[i] the count of hashes[i] (0: not a key), its occurrences at occ_out[off_out[i] .. off_out[i + 1]) -- none for a
 * count above max_occ.  off_out: n + 1.  FSV_ECAP when cap is too small (off_out[n] says how many are needed), FSV_EINVAL without an index. */
int fsv_ref_index_lookup(fsv_ctx *ctx, const uint64_t *hashes, uint32_t n, uint32_t *count_out, uint64_t *off_out, uint32_t *occ_out, uint64_t cap);

#define FSV_MQ_TRUNC 1      /* flags: the occurrence cutoff is below max_occ (a class of hits would not fit the chain's anchor array) */
struct fsv_contig_mapq {    /* all host, n_rec entries each */
    int32_t *f1, *f2, *m;   /* best chain score at the record's own locus, best elsewhere (0: no hit elsewhere), anchors of the former */
    int32_t *cutoff, *thin; /* c*: seeds with a higher count are ignored; t: every t-th seed by hash is used (1: all) */
    int32_t *flags;         /* FSV_MQ_* */
    int32_t *rec_status;    /* 0, or FSV_EINVAL for a record that does not fit its sequences (mapq 0, nothing else set) */
    double   ms;            /* out: summed kernel time */
};
/* 0 when f1 <= 0, m <= 0 or f2 >= f1; else (int)(40 (1 - f2 / f1) min(1, m / 10) ln f1) in double arithmetic, clamped to [0, 60].  Host only. */
int32_t fsv_mapq_of(int32_t f1, int32_t f2, int32_t m);
/* Writes alns->rec[i].mapq.  alns: records as fsv_align_batch returned them; ref_origin[r]: the chromosome position of window r's first
 * base.  Every record is checked on the host as fsv_aln_tags checks it, the chromosome taking the window's place: its query-consuming
 * ops must sum to the contig's length, ref_start plus its reference-consuming ops must equal ref_end, origin + ref_end must not exceed
 * the chromosome, and 0 <= q_start <= q_end <= the contig's length; a record that fails has rec_status FSV_EINVAL and mapq 0 and reaches
 * no kernel.  contig_seq == NULL: the contigs the last fsv_align_batch left on the device (FSV_EINVAL when there are none or n_contigs /
 * n_refs differ from that call's; contig_off and contig_ref are then not read).  Every contig is sketched once with the index's (w, k); one workgroup per record then takes the minimizers whose end
 * lies in the record's interval of the forward contig (every t-th by hash beyond 4 096), splits their hits into own locus (relative strand
 * = rev, position inside [origin + ref_start, origin + ref_end)), elsewhere forward and elsewhere reverse, finds the largest occurrence
 * count c* <= max_occ up to which every class has at most 8 192 hits, and chains each class (anchors sorted by chromosome, then contig
 * coordinate; params: k, max_gap, look-back 64; the chain DP of fsv_align_batch). */
int fsv_contig_mapq(fsv_ctx *ctx, const char *contig_seq, const uint64_t *contig_off, uint32_t n_contigs, const uint32_t *contig_ref,
                    const int64_t *ref_origin, uint32_t n_refs, fsv_alns *alns, const fsv_aln_params *params, struct fsv_contig_mapq *out);

/* ---- BAM output: a coordinate-sorted BAM and its .bai, host only (no GPU, like the rest of fsv_bam_*) -------------------------
 * Struct of arrays in the reader's style.  The writer sorts the records stably by (ref_id, pos), unmapped ones (ref_id -1, pos -1,
 * flag & 4, no CIGAR) last in input order; encodes them as SAM v1 section 4.2 (bin by reg2bin, qualities 0xff, mate fields
 * -1 / -1 / 0, aux in the order NM:i, cs:Z, SA:Z, each only when given); cuts the stream into BGZF blocks of at most 0xff00
 * payload bytes, deflated with zlib on n_threads host threads (clamped to 1 .. 16), and appends the EOF marker block; writes
 * path + ".bai" (bins with their chunks, the 16 kb linear index with empty windows carrying the previous offset forward, virtual
 * offsets at record starts).  Both files are written under temporary names in the same directory and renamed: a failed call leaves
 * neither.  FSV_EINVAL: a bad argument, ref_id >= n_refs, a mapped record without reference bases in its CIGAR, a name of more
 * than 254 bytes; FSV_EUNSUP: a CIGAR of more than 65535 ops; FSV_EINTERNAL: the files could not be written. */
typedef struct fsv_bam_out {
    uint32_t n_refs;
    const char *const *ref_name;  /* n_refs NUL-terminated names */
    const int32_t *ref_len;
    const char *header_text;      /* SAM header text (may be NULL: empty) */
    uint64_t n_rec;
    const int32_t  *ref_id, *pos; /* 0-based position; -1 / -1 unmapped */
    const uint16_t *flag;
    const uint8_t  *mapq;
    const uint64_t *qname_off;    /* NUL-terminated name of record r at qname + qname_off[r] */
    const char     *qname;
    const uint64_t *cigar_off;    /* record r owns cigar[cigar_off[r] .. + n_cigar_op[r]) */
    const uint32_t *n_cigar_op;
    const uint32_t *cigar;        /* BAM encoding len << 4 | op */
    const uint64_t *seq_off;      /* n_rec + 1: ASCII bases of record r are seq[seq_off[r] .. seq_off[r + 1]) */
    const char     *seq;
    const int32_t  *nm;           /* optional (NULL: no NM tags); FSV_BAM_NO_TAG: none for this record */
    const uint64_t *cs_off;       /* optional with cs (both or neither): n_rec + 1 offsets; an empty range: no cs tag for this record */
    const char     *cs;
    const uint64_t *sa_off;       /* optional with sa: NUL-terminated SA text of record r at sa + sa_off[r], "" for none */
    const char     *sa;
} fsv_bam_out;
int fsv_bam_write(const char *path, const fsv_bam_out *in, int n_threads);

/* ---- BAM input without pysam / samtools --------------------------------------------------------------
 * Replaces, at the reference's pysam boundary, `pysam.AlignmentFile(bam).fetch(chr)` with its per-record fields
 * (extract_reads_signature.py:68-105, 160-209: reference_name, pos, reference_end, cigar, qname, is_reverse, mapq, flag) and the
 * `samtools view bam chr:start-end` crop of 1_crop_bam.py:74.  BGZF blocks are inflated with zlib on the host; a .bai next to the
 * file (x.bam.bai or x.bai) gives the start of a region, without one the file is scanned from its first record.  No GPU needed
 * for fsv_bam_*; fsv_read_signatures runs the CIGAR scan (extract_sig_from_cigar, extract_reads_signature.py:11-44) as a kernel. */
typedef struct fsv_bam fsv_bam;
int  fsv_bam_open(const char *path, fsv_bam **out);
void fsv_bam_close(fsv_bam *bam);
int  fsv_bam_n_refs(const fsv_bam *bam);
const char *fsv_bam_ref_name(const fsv_bam *bam, int ref_id);
int64_t fsv_bam_ref_length(const fsv_bam *bam, int ref_id);   /* -1: no such reference sequence (pysam get_reference_length) */
int  fsv_bam_ref_id(const fsv_bam *bam, const char *name);   /* -1: no such reference sequence */
int  fsv_bam_has_index(const fsv_bam *bam);
void fsv_bam_set_threads(fsv_bam *bam, int n);   /* host threads inflating BGZF blocks (default: the machine's, at most 16) */

typedef struct fsv_bam_records {
    /* all host; caller-allocated with the capacities below (a first call with pos == NULL only counts) */
    int32_t  *pos, *ref_end;      /* 0-based start, exclusive end on the reference (pysam pos / reference_end) */
    uint16_t *flag;
    uint8_t  *mapq;
    uint64_t *cigar_off;          /* record r owns cigar[cigar_off[r] .. + n_cigar_op[r]) */
    uint32_t *n_cigar_op;
    uint64_t *qname_off;          /* NUL-terminated name of record r at qname + qname_off[r] */
    int32_t  *l_seq;
    uint32_t *cigar;              /* BAM encoding len << 4 | op */
    char     *qname;
    uint64_t *seq_word_off;       /* want_seq: bases of record r, 2 bits each as in the read store, from seq_words_buf[seq_word_off[r]] */
    uint32_t *seq_words_buf;
    char     *seq_ascii;          /* want_seq & 2: bases of record r as text (pysam read.seq), l_seq[r] bytes from seq_ascii + seq_ascii_off[r] */
    uint64_t *seq_ascii_off;
    int32_t  *ref_id;             /* optional: reference sequence of the record (-1 unmapped) */
    char     *sa;                 /* want_seq & 4: NUL-terminated text of the record's SA tag ("" when it has none) at sa + sa_off[r] */
    uint64_t *sa_off;
    int32_t  *ps, *hp;            /* optional (both or neither): integer PS / HP tags of the record, FSV_BAM_NO_TAG when absent (output_fas.py:31-33) */
    uint64_t rec_cap, cigar_cap, qname_cap, seq_cap, seq_ascii_cap, sa_cap;
    uint64_t n_rec, n_cigar, qname_bytes, seq_words, seq_ascii_bytes, sa_bytes;   /* out */
} fsv_bam_records;
#define FSV_BAM_NO_TAG (-2147483647 - 1)
/* mapped records of reference ref_id that overlap [beg, end) (end <= 0: to the end), in file order; ref_id -1: every record of the
 * file (pysam fetch(until_eof=True), output_fas.py:26).  want_seq: bit 0 the 2-bit words, bit 1 the text, bit 2 the SA tags (supplementary alignments, Reads_Based_Scan.py:527-531) */
int fsv_bam_fetch(fsv_bam *bam, int ref_id, int64_t beg, int64_t end, fsv_bam_records *out, int want_seq);

typedef struct fsv_read_sig {
    uint32_t rec;                 /* index into the fetched records */
    uint32_t type;                /* 0 DEL, 1 INS */
    int32_t  ref_pos, len;        /* 0-based reference position of the event, its length */
    int32_t  read_off;            /* offset in the read, hard clip at the head included (extract_reads_signature.py:19-24) */
    uint32_t pad;
} fsv_read_sig;                   /* 24 bytes */
/* DEL / INS of at least min_svlen in the CIGARs of records with mapq >= min_mapq; order of `out` is unspecified (sort by rec, read_off) */
int fsv_read_signatures(fsv_ctx *ctx, const fsv_bam_records *rec, int min_mapq, int min_svlen, fsv_read_sig *out, uint32_t cap, uint32_t *n_out);

#ifdef __cplusplus
}
#endif
#endif /* FOCALSV_HIP_H */
