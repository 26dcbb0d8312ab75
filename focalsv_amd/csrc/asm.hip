// asm.hip -- host orchestration of the batched per-read-set assembly (fsv_assemble_batch).
//
// Replaces the process boundary `hifiasm -o <prefix> -t T <reads.fa>` + GFA read-back
// (focalsv/3_assembly/run_assembly.py:15-44, post_assembly.py:79-95).  All base-level work runs in the
// kernels of asm_kernels.h and the stage files it includes; the host only sizes buffers between stages and walks the (tiny, <= a few
// hundred nodes per set) overlap graph, which is host code in hifiasm as well (Overlaps.cpp).
#include "asm_kernels.h"
#include "k_kmer.h"
#include "layout.h"
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <thread>
#include <atomic>

namespace {

enum { KN_SKETCH, KN_UNIQ, KN_CHAIN, KN_BPM, KN_RESCUE, KN_PATH_FAST, KN_PATH_DP, KN_CONSENSUS, KN_REPACK, KN_EXACT, KN_STITCH, KN_PARTITION, KN_BND, KN_BND_CONS,
       KN_UNIQ_LONG, KN_CHAIN_SPILL,   // full_lists = 1: timed on their own, outside the k_uniq / k_chain groups
       KN_CONS_DEEP, KN_BND_DEEP,      // deep_sets = 1: timed on their own, outside the k_partition / k_consensus / k_bnd_consensus rows
       KN_COUNT,
       ST_SKETCH = KN_COUNT, ST_CHAIN, ST_VERIFY, ST_PATH, ST_CONSENSUS, ST_FINAL };
const char *const kn_names[KN_COUNT] = {"k_sketch", "k_uniq", "k_chain", "k5_bpm", "k_rescue_accept", "k_path_fast", "k_path_dp", "k_consensus",
                                        "k_repack", "k_exact", "k_stitch", "k_partition", "k_bnd_tasks", "k_bnd_consensus", "k_uniq_long", "k_chain_spill",
                                        "k_consensus_deep", "k_bnd_consensus_deep"};
static_assert(KN_COUNT <= FSV_MAX_KERNEL_STATS, "fsv_asm_stats holds every kernel's row");
// the task lists of a round: its window tasks, the junction tasks of its second consensus pass, the junction cigars of its partition
// (PASS_NONE: a list outside a batch -- fsv_bpm_paths).  Pass p of round r keeps its device counters in row p (n_rounds + 1) + r.
enum { PASS_NONE = -1, PASS_WINDOWS, PASS_JUNCTIONS, PASS_BCIG, PASS_COUNT };

// HIP-event timing of kernels and of whole stages on the context's stream: recorded while the work is queued, resolved once
// at the end of the batch -- nothing here waits for the GPU (round 1's stage timers synchronised the stream twice each)
struct KTimes {
    struct Rec { int k; hipEvent_t a, b; uint64_t bytes; };
    std::vector<Rec> recs;
    std::vector<hipEvent_t> pool;
    size_t used = 0;
    // the records whose byte counts are only known when the batch ends: (pass, kernel) -> record index, one per round in order
    std::vector<size_t> by[PASS_COUNT][KN_COUNT];
    hipEvent_t get() { if (used == pool.size()) { hipEvent_t e; (void)hipEventCreate(&e); pool.push_back(e); } return pool[used++]; }
    size_t begin(fsv_ctx *ctx, int k, uint64_t bytes) { Rec r{k, get(), get(), bytes}; (void)hipEventRecord(r.a, ctx->stream); recs.push_back(r); return recs.size() - 1; }
    void begin(fsv_ctx *ctx, int pass, int k, uint64_t bytes) { const size_t i = begin(ctx, k, bytes); if (pass != PASS_NONE) by[pass][k].push_back(i); }
    void end(fsv_ctx *ctx) { (void)hipEventRecord(recs.back().b, ctx->stream); }
    void end(fsv_ctx *ctx, size_t idx) { (void)hipEventRecord(recs[idx].b, ctx->stream); }
    uint64_t *bytes_of(int pass, int k, size_t round) { const auto &v = by[pass][k]; return round < v.size() ? &recs[v[round]].bytes : nullptr; }
    void reset() { recs.clear(); used = 0; for (auto &p : by) for (auto &v : p) v.clear(); }
    ~KTimes() { for (auto e : pool) (void)hipEventDestroy(e); }
};

// a stage: from construction to stop(), in stream order
struct Span {
    fsv_ctx *ctx; KTimes &kt; size_t idx;
    Span(fsv_ctx *c, KTimes &k, int stage) : ctx(c), kt(k), idx(k.begin(c, stage, 0)) {}
    void stop() { kt.end(ctx, idx); }
};

// HIP-event time of a few spans on a stream: mark() where a span starts and where it ends, ms() once the stream has passed them all
// (the host reads counts back between the spans, or the chunk has ended).  It owns its events: clear(), or the destructor, destroys them.
struct EventClock {
    std::vector<hipEvent_t> ev;
    EventClock() = default;
    EventClock(const EventClock &) = delete;
    EventClock &operator=(const EventClock &) = delete;
    ~EventClock() { clear(); }
    int mark(fsv_ctx *ctx) { hipEvent_t e; FSV_HIP(ctx, hipEventCreate(&e)); ev.push_back(e); FSV_HIP(ctx, hipEventRecord(e, ctx->stream)); return FSV_OK; }
    double ms() const { double t = 0; for (size_t i = 0; i + 1 < ev.size(); i += 2) { float x = 0; if (hipEventElapsedTime(&x, ev[i], ev[i + 1]) == hipSuccess) t += x; } return t; }
    void clear() { for (auto e : ev) (void)hipEventDestroy(e); ev.clear(); }
};

// per-round block of device counters (one 64-byte slot per correction round + one for the final pass, zeroed once per batch and
// read back with the round's one synchronisation or at the end): u32 indices
enum { CT_TASKS = 0, CT_OVERFLOW = 1, CT_DP = 2, CT_INEXACT = 3, CT_COLS_LO = 4, CT_COLS_HI = 5, CT_DP_WIDE = 6, CT_DP_SB = 7, CT_DP_GEN = 8, CT_DP_XW = 9,
       CT_MZ_LO = 10, CT_MZ_HI = 11, CT_B_RETRY = 12, CT_B_LIST = 13, CT_DP_SB16 = 14, CT_WIDE = 15,
       CT_MZRAW_LO = 16, CT_MZRAW_HI = 17, CT_BASES_LO = 18, CT_BASES_HI = 19,   // k_uniq's other two sums: CT_MZ + 3 and + 4 as 64-bit words
       CT_DP_FR3 = 20,       // k_path_fr's lists by distance: CT_DP_SB16 (1), CT_DP (2), CT_DP_FR3 (3)
       CT_LEFT = 21,         // overlaps set aside for the left-extension rescue pass (k_left_rescue)
       CT_FIX = 22, CT_FIXED = 23,   // fix_boundary's candidates (k_path_fast) and the windows it moved
       CT_SPILL = 24,        // full_lists = 1: pairs set aside for k_chain_spill (more anchors than the tile in use)
       CT_SPILLED = 25,      // ... summed over the pass's launches (the re-chain starts the list again for either side)
       CT_UQ_LONG = 26,      // full_lists = 1: reads whose list k_uniq_long indexed
       CT_DEEP_W = 27,       // deep_sets = 1: windows listed for k_consensus_deep (k_consensus and k_consensus_redo: a window can be listed twice)
       CT_DEEP_B = 28,       // ... junctions listed for k_bnd_consensus_deep
       CT_DEEP_MAX = 29,     // ... the largest event count of a listed window or junction
       CT_SLOT = 32 };      // even: the 64-bit sums stay aligned in every slot

template <class... Ts> size_t cap_sum(const Ts &...b) { return (b.cap + ... + 0); }

// ---- the opt-in stages: each one's buffers and what the last fsv_assemble_batch left of it (reset() when a call begins; valid: set when it
// ---- ends, see AsmWs::mark_valid), with held() as the stage's share of AsmWs::held()
// kmer_table = 1, the k-mer count table stage (k_kmer.h): one open-addressed table per set back to back (keys, counts), the sets' histograms,
// the filter list of the last stage and -- for a batch of several chunks -- of all its chunks, in set order
struct KmerTableState {
    Dev<unsigned long long> keys, flt, flt_all; Dev<uint32_t> cnt, hist, cursor, err; Dev<uint64_t> tab_off, flt_off;
    Dev<int32_t> cutoff; Dev<KmerTile> tiles;
    // per set its verdict (peak_hom is hifiasm's hom_cov), and its segment [last_flt_off[s], last_flt_off[s + 1]) of the filter list on the
    // device (flt_all, unordered inside a set); ms: the stage's launches, all chunks
    std::vector<fsv_kmer_set> last; std::vector<uint64_t> last_flt_off{0}; double ms = 0; bool valid = false;
    size_t held() const { return cap_sum(keys, flt, flt_all, cnt, hist, cursor, err, tab_off, flt_off, cutoff, tiles); }
    void reset() { last.clear(); last_flt_off.assign(1, 0); ms = 0; valid = false; }
};
// kmer_filter = 1 (and the stage hooks fsv_sketch_reads_filtered / fsv_kmer_index): the sets' filter sets that the sketch kernels probe
// (k_flt_build: keys back to back, n_sets + 1 slot offsets), the set of every read, a caller's lists on the device; view: what a sketch
// launch takes -- nothing when no set has a slot
struct FilterState {
    Dev<unsigned long long> keys, list; Dev<uint64_t> off, list_off; Dev<uint32_t> read_set;
    SketchFilter view;
    // per set the figures of hifiasm's first ha_pt_gen (peak_hom: its hom_cov); ms: the filter-set builds and the index, all chunks
    std::vector<fsv_kmer_index_set> last; double ms = 0; bool valid = false;
    size_t held() const { return cap_sum(keys, list, off, list_off, read_set); }
    void reset() { view = SketchFilter{}; last.clear(); ms = 0; valid = false; }
};
// partial_charge = 1 (charge_stage): two extension tasks and results per window task at fixed slots, the slots in use, the overlaps waiting
// for their verdict, the two list lengths, the stage's counters (fsv_charge_stats' five, summed over the chunk's rounds)
struct ChargeState {
    Dev<fsv_wtask> ext_tasks; Dev<fsv_wext> ext_res; Dev<uint32_t> ext_list, list, n; Dev<unsigned long long> ct;
    EventClock clock;          // start / end of every charge_stage of the chunk, resolved when the chunk ends (charge_collect)
    fsv_charge_stats last{};   // all chunks
    bool valid = false;
    size_t held() const { return cap_sum(ext_tasks, ext_res, ext_list, list, n, ct); }
    void reset() { clock.clear(); last = fsv_charge_stats{}; valid = false; }   // (clock: marks of a call that failed half-way)
};

struct AsmWs {
    Dev<uint32_t> store[2], word_off, set_start, read_set, pair_base, upair_base, pair_read, mz_off, mz_cnt, counters, warn, set_cols, changed, read_dirty,
        dp_list, dp_list2, dp_list3, dp_list16, dp_list_e3, dp_wide, dp_xwide, left_list, fix_list, wide_list, inexact_list, cols_wide,
        gwin_off, gwin_read, lb, unpack_off, brel_off, src3, bnd_flag, bnd_list, site_cnt, site_off, redo, sk_ends, sk_low, sk_high;
    Dev<uint32_t> sr_store;      // the round's reads, then the first consensus pass's result as a second store behind them
    Dev<uint32_t> site_cursor;   // four counters: [0] vectors, [1] listed windows, [3] site records
    Dev<uint32_t> site_lists;    // two lists of n_gwin entries: windows with a site, windows to redo
    Dev<uint32_t> set_hits;      // hits per set, then (behind them) n_sets + 1 offsets
    Dev<int32_t> len, new_len, idx2, bc_idx;
    Dev<int32_t> bc_win;         // three words per grid window
    Dev<fsv_mz> mz; Dev<fsv_ovl> ovl, ovl_prev; Dev<fsv_hit> hits, hits_packed; Dev<fsv_piece> pieces; Dev<BndPatch> bnd_patch;
    Dev<fsv_wtask> tasks, tasks2, tasks3; Dev<fsv_wres> res, res2, res3; Dev<fsv_wpath> paths, paths2;
    Dev<uint4> cols_sb, ovl_c, upair_tab, upair_tab_sw, gwin_tab, bc_rec; Dev<uint2> site_rec; Dev<int8_t> site_vec;
    Dev<uint4> uq_ws, spill_list; Dev<uint8_t> spill_slab;   // full_lists = 1: k_uniq_long's merge buffers; the pairs set aside for k_chain_spill, its slabs
    Dev<uint2> deep_list, deep_blist; Dev<uint32_t> deep_slab;   // deep_sets = 1: the windows / junctions set aside for the two deep kernels, their event slabs
    Dev<uint64_t> cols;          // k_path_dp's column scratch: 64-bit columns, or 32-bit ones in the same bytes
    Dev<unsigned long long> tmp; // cycle stamps of the diagnostic runs
    Dev<uint8_t> cov3, bnd_bytes, exact_flag, cwin, thr_tab; Dev<uint16_t> cwin_len; Dev<char> contig_out, contig_all;
    KmerTableState km;   // kmer_table = 1
    FilterState fs;      // kmer_filter = 1
    ChargeState ch;      // partial_charge = 1
    std::vector<uint32_t> h_store;   // the corrected reads of the sets whose layout compares bases (kept between calls: no 96 MB zero-fill a step)
    int occ_sb = 0, occ_fr[3] = {0, 0, 0}, occ_wide = 0;   // blocks per CU of the persistent K6 kernels (hipOccupancyMaxActiveBlocksPerMultiprocessor: asked once)
    ChainArgs last_chain;   // arguments of the last k_chain launch (the final pass re-chains a few pairs with another bandwidth)
    // state of the last run (for fsv_asm_fetch_reads / stats)
    std::vector<uint32_t> h_word_off;
    std::vector<int32_t> h_len;
    const uint32_t *cur_store = nullptr;
    uint32_t n_reads = 0;
    fsv_asm_stats stats;
    uint64_t n_long_reads = 0, n_spilled_pairs = 0;   // full_lists = 1, last call, all rounds and chunks: lists k_uniq_long indexed, pairs k_chain_spill chained
    uint64_t n_deep_windows = 0, n_deep_junctions = 0; uint32_t deep_max_events = 0;   // deep_sets = 1, last call, all rounds and chunks: what the two deep kernels took
    KTimes kt;
    void *h_pin = nullptr; size_t h_pin_cap = 0; // pinned host staging (exact hits)
    uint32_t *ct_of(int row) { return counters.p + (size_t)row * CT_SLOT; }   // a row of the counter block (valid until counters grows)
    // bytes this context holds.  Only the chunking budget reads it: a buffer missing from the list is undercounted there, not leaked
    size_t held() const
    {
        return cap_sum(store[0], store[1], cols_sb, contig_all, word_off, len, set_start, read_set, pair_base, mz, mz_off, mz_cnt, ovl, tasks, res, paths,
                       counters, dp_list, dp_list2, dp_list3, dp_list16, dp_list_e3, dp_wide, dp_xwide, cols_wide, set_cols, site_cnt, site_rec, site_off, site_vec,
                       site_cursor, redo, site_lists, read_dirty, cov3, lb, sr_store, brel_off, tasks2, res2, paths2, idx2, bc_idx, bc_rec, bc_win, left_list, fix_list,
                       tasks3, res3, src3, bnd_flag, bnd_list, bnd_patch, bnd_bytes, changed, pair_read, wide_list, cols, tmp, gwin_off, gwin_read, sk_ends, sk_low, sk_high,
                       hits, hits_packed, set_hits, ovl_prev, exact_flag, inexact_list, upair_base, upair_tab, upair_tab_sw, ovl_c, gwin_tab, cwin, cwin_len, warn, thr_tab,
                       pieces, contig_out, new_len, unpack_off, uq_ws, spill_list, spill_slab, deep_list, deep_blist, deep_slab) + km.held() + fs.held() + ch.held();
    }
    // the opt-in stages' state between two calls of fsv_assemble_batch: forgotten when a call begins, valid when it ends well.  stages_ran:
    // false for a call that returned before its first chunk (no set, or no read and no kmer_table) -- the k-mer getters then go on refusing
    void reset_stages() { km.reset(); fs.reset(); ch.reset(); }
    void mark_valid(const fsv_asm_params &P, bool stages_ran) { km.valid = stages_ran && P.kmer_table; fs.valid = stages_ran && P.kmer_filter; ch.valid = P.partial_charge != 0; }
};

void ws_free(fsv_ctx *ctx)
{
    AsmWs *w = (AsmWs *)ctx->asm_ws;
    if (!w) return;
    if (w->h_pin) (void)hipHostFree(w->h_pin);
    delete w;
    ctx->asm_ws = nullptr;
}

AsmWs *ws_get(fsv_ctx *ctx)
{
    if (!ctx->asm_ws) { ctx->asm_ws = new AsmWs(); ctx->asm_ws_free = ws_free; memset(&((AsmWs *)ctx->asm_ws)->stats, 0, sizeof(fsv_asm_stats)); }
    return (AsmWs *)ctx->asm_ws;
}

uint8_t thr_for_len_host(int x_len, int rate_pm)
{
    // verify_window: threshold = x_len * max_ov_diff_ec (0.04 as a double, truncated), Adjust_Threshold (Correct.h:39)
    const double rate = rate_pm / 1000.0;       // 40 / 1000.0 is the double 0.04
    if (x_len == FSV_WINDOW) return rate_pm == 40 ? FSV_K_FULL : (uint8_t)(int)(FSV_WINDOW * rate);
    int t = (int)(x_len * rate);
    if (t == 0 && x_len >= 4) t = 1;
    return (uint8_t)t;
}

struct Batch {
    uint32_t n_reads = 0, n_sets = 0, n_pairs = 0, n_upairs = 0;
    std::vector<uint32_t> set_start, read_set, pair_base, upair_base;
};

// per-round geometry derived from the current read lengths
struct Geometry {
    std::vector<uint32_t> word_off, mz_off, gwin_off, gwin_read;
    uint64_t task_bound = 0;
    uint32_t max_words = 1;
};

// minimizer slots of a read: the worst case is one per base (inside a long homopolymer or a short-unit tandem repeat every
// k-mer ties with the window minimum and ha_sketch reports all of them); 16 B x bases is 2 % of HBM for 256 regions
// full_lists = 1 with w <= 2: the index holds every unique minimizer twice, and with such a window more than half the bases can be one, so the
// slot gets that room too (with larger windows 2m stays below len + 64, and the default path keeps the slots it had)
static inline uint64_t mz_slots(int64_t len, int w, bool full_lists = false) { return (uint64_t)len + 64 + (full_lists && w <= 2 ? (uint64_t)len : 0); }

int make_geometry(fsv_ctx *ctx, const Batch &B, const std::vector<int32_t> &len, Geometry &G, int mz_w = 51, const std::vector<uint32_t> *fixed_mz_off = nullptr,
                  bool full_lists = false)
{
    G.word_off.assign(B.n_reads + 1, 0); G.mz_off.assign(B.n_reads + 1, 0); G.gwin_off.assign(B.n_reads + 1, 0);
    G.max_words = 1;
    uint64_t w = 0, m = 0, g = 0;
    for (uint32_t r = 0; r < B.n_reads; r++) {
        G.word_off[r] = (uint32_t)w; G.mz_off[r] = (uint32_t)m; G.gwin_off[r] = (uint32_t)g;
        w += (uint64_t)(len[r] + 15) / 16;
        G.max_words = std::max<uint32_t>(G.max_words, (uint32_t)((len[r] + 15) / 16));
        m += mz_slots(len[r], mz_w, full_lists);
        g += (uint64_t)(len[r] + FSV_WINDOW - 1) / FSV_WINDOW;
    }
    if (w + 4 >= (1ull << 32) || m >= (1ull << 32) || g >= (1ull << 32)) return fsv_fail(ctx, FSV_EUNSUP, "batch too large for 32-bit offsets; split it");
    G.word_off[B.n_reads] = (uint32_t)w; G.mz_off[B.n_reads] = (uint32_t)m; G.gwin_off[B.n_reads] = (uint32_t)g;
    if (fixed_mz_off) G.mz_off = *fixed_mz_off;   // slots that do not move between rounds (sized for the longest a read can get)
    G.gwin_read.resize(g);
    for (uint32_t r = 0; r < B.n_reads; r++) for (uint32_t x = G.gwin_off[r]; x < G.gwin_off[r + 1]; x++) G.gwin_read[x] = r;
    G.task_bound = 0;
    for (uint32_t s = 0; s < B.n_sets; s++) {
        uint64_t nw = 0;
        uint32_t ns = B.set_start[s + 1] - B.set_start[s];
        for (uint32_t r = B.set_start[s]; r < B.set_start[s + 1]; r++) nw += G.gwin_off[r + 1] - G.gwin_off[r];
        if (ns > 1) G.task_bound += nw * (ns - 1);
    }
    return FSV_OK;
}

// a workgroup may use more than 64 KB of dynamic LDS only after opting in (the ONT profile's 4 096-anchor tile in the long layout is
// 96 KB: without this the launch was rejected and the whole batch came back FSV_EHIP -- ADVICE r02)
template <class F> int lds_opt_in(fsv_ctx *ctx, F f, size_t bytes)
{
    if (bytes > 48u * 1024u) FSV_HIP(ctx, hipFuncSetAttribute((const void *)f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return FSV_OK;
}

// What a correction round, and the final pass after the last one, carries from stage to stage
struct Round {
    const fsv_asm_params &P;
    Batch B;
    const uint8_t *set_flags = nullptr;
    // kmer_table = 1: the caller's sets whose k-mer histogram has no peak (empty: none).  Every read of such a set is a set of its own in B
    // -- no pair, so no overlap stage sees it and no consensus changes it -- and caller_set maps B's sets back to the caller's
    std::vector<uint8_t> low_cov;
    std::vector<uint32_t> caller_set;
    bool is_low(uint32_t s) const { return !low_cov.empty() && low_cov[caller_set[s]]; }
    const uint32_t *store = nullptr; std::vector<int32_t> len; Geometry G;   // the reads as they are now: the caller's in round 0, then the store the last round repacked
    std::vector<uint32_t> mz_fixed;  // minimizer slots: fixed for the whole call
    bool wide_bands = false;         // the error model allows thresholds above hifiasm's 31: wide-band K5 / K6 / rescue
    bool short_reads = true;         // every read below 65 536 bases: k_chain's compact LDS layout
    int round = 0; uint32_t task_cap = 0, n_gwin = 0;
    uint32_t *ct = nullptr;          // the round's (or the final pass's) row of device counters
    ConsArgs C;
    DeepSlabs deep{};                // deep_sets = 1: the event slabs of the round's deep kernels (deep_setup)
    uint32_t deep_grid = 0;
    std::vector<uint32_t> h_ct;      // the counter rows on the host, as on the device
    uint64_t reads_in_bytes = 0;
    const std::chrono::steady_clock::time_point t_enter = std::chrono::steady_clock::now();
    explicit Round(const fsv_asm_params &p) : P(p) {}
    int row(int pass) const { return pass * (P.n_rounds + 1) + round; }
};

// k_chain in its three forms: a block per chunk of pairs, a block per pair (or per entry of A.pair_list), persistent blocks
// walking A.wide_list with the large tile.  The one place that picks the LDS layout and opts in to its size.
enum ChainKind { CHAIN_CHUNKS, CHAIN_PAIRS, CHAIN_WIDE_LIST };
template <bool SHORT> int launch_chain_as(fsv_ctx *ctx, ChainKind kind, uint32_t grid, const ChainArgs &A, uint32_t n_upairs)
{
    const size_t lds = chain_lds_bytes(SHORT, A.amax);
    if (kind == CHAIN_CHUNKS) { TRY(lds_opt_in(ctx, k_chain_chunks<SHORT>, lds)); FSV_LAUNCH(ctx, ctx->stream, k_chain_chunks<SHORT>, dim3(grid), dim3(64), lds, A, n_upairs); }
    else if (kind == CHAIN_PAIRS) { TRY(lds_opt_in(ctx, k_chain<SHORT>, lds)); FSV_LAUNCH(ctx, ctx->stream, k_chain<SHORT>, dim3(grid), dim3(64), lds, A); }
    else { TRY(lds_opt_in(ctx, k_chain_wide_list<SHORT>, lds)); FSV_LAUNCH(ctx, ctx->stream, k_chain_wide_list<SHORT>, dim3(grid), dim3(64), lds, A); }
    return FSV_OK;
}
int launch_chain(fsv_ctx *ctx, ChainKind kind, bool short_reads, uint32_t grid, const ChainArgs &A, uint32_t n_upairs)
{
    return short_reads ? launch_chain_as<true>(ctx, kind, grid, A, n_upairs) : launch_chain_as<false>(ctx, kind, grid, A, n_upairs);
}
// the pairs a k_chain launch set aside (both lists beyond its tile: reads above ~25 kb), chained with the large tile
int chain_wide_pairs(fsv_ctx *ctx, const ChainArgs &A, bool short_reads, uint32_t n_upairs)
{
    ChainArgs AW = A;
    AW.amax = short_reads ? FSV_AMAX_WIDE : FSV_AMAX_WIDE_LONG; AW.stamps = nullptr; AW.pair_list = nullptr; AW.n_list_dev = nullptr;   // (the kernel walks AW.wide_list)
    return launch_chain(ctx, CHAIN_WIDE_LIST, short_reads, std::min<uint32_t>(n_upairs, 2u * (uint32_t)ctx->n_cu), AW, n_upairs);
}

// full_lists = 1: the pairs the launches above set aside because their anchors exceed the tile (A.spill_list), chained in HBM slabs and timed on
// their own (KN_CHAIN_SPILL).  max_slot: the batch's longest minimizer slot; an index takes at most half of it and a pair has at most min(nq, nt)
// anchors, so a slab holds max_slot / 2 + 64.  A small fixed grid: FSV_SPILL_GRID slabs of 32 B an anchor (1.8 MB each for a 100 kb read) stay in
// L2 and are under a thousandth of the workspace budget.  The list's length is on the device only, so the launch is unconditional: with an
// empty list every block reads the count and returns
int chain_spilled_pairs(fsv_ctx *ctx, AsmWs &W, const ChainArgs &A, uint32_t n_upairs, uint32_t max_slot, uint32_t *ct)
{
    if (!A.spill_list) return FSV_OK;
    const uint32_t grid = std::min<uint32_t>(std::max(1u, n_upairs), FSV_SPILL_GRID), slab_cap = max_slot / 2 + 64;
    TRY(ensure(ctx, W.spill_slab, (size_t)grid * slab_cap * FSV_SPILL_BYTES));
    const size_t it = W.kt.begin(ctx, KN_CHAIN_SPILL, 0);
    FSV_LAUNCH(ctx, ctx->stream, k_chain_spill, dim3(grid), dim3(64), 0, A, W.spill_slab.p, slab_cap, ct + CT_SPILLED);
    W.kt.end(ctx, it);
    return FSV_OK;
}
static uint32_t longest_slot(const Geometry &G, uint32_t n_reads)
{
    uint32_t m = 64;
    for (uint32_t r = 0; r < n_reads; r++) m = std::max(m, G.mz_off[r + 1] - G.mz_off[r]);
    return m;
}
static uint32_t reads_above(const std::vector<int32_t> &len, int32_t bases)
{
    uint32_t n = 0;
    for (int32_t l : len) n += l > bases;
    return n;
}

// sketch + per-read index + chaining on the current store; fills ws.ovl (and, in a correction round, ws.tasks).  Nothing here waits
// for the GPU: launches are sized from the read lengths the host already has, counts stay in the counter row R.ct.
int overlap_stage(fsv_ctx *ctx, AsmWs &W, const Round &R, bool final_pass)
{
    const fsv_asm_params &P = R.P; const Batch &B = R.B; const Geometry &G = R.G;
    uint32_t *ct = R.ct;
    // ONT-profile batches: dense seeds and 4 096-anchor tiles for the first round only (noisy reads share few minimizers, but nothing bounds
    // them); from the second round on the reads are accurate and the sparser seeds keep a pair below 1 024 anchors
    const int w = ((final_pass || R.round > 0) && P.w_later > 0) ? P.w_later : P.w;
    const bool wide_anchors = R.wide_bands && w == P.w;
    // hifiasm's final pass keeps every pair that shares a minimizer on a strand, however short the overlap (the graph sorts them out)
    const int min_anchors = final_pass && P.min_anchors_final > 0 ? P.min_anchors_final : P.min_anchors;
    const int min_ovlp = final_pass && P.min_ovlp_final > 0 ? P.min_ovlp_final : P.min_ovlp;
    // in the final pass the reads the last round left untouched keep that round's minimizer lists (the last round does not
    // reverse-complement) -- when that round sketched with the same window, and only with the position-parallel kernel (odd k):
    // the replay kernel always sketches every read
    const bool keep_lists = final_pass && P.n_rounds > 0 && (P.n_rounds > 1 || w == P.w) && (P.k & 1);
    const uint32_t *only_changed = keep_lists ? W.changed.p : nullptr;
    Span ts(ctx, W.kt, ST_SKETCH);
    TRY(ensure(ctx, W.mz, G.mz_off[B.n_reads]));
    TRY(ensure(ctx, W.mz_cnt, B.n_reads));
    TRY(ensure(ctx, W.ovl, std::max(1u, B.n_pairs)));
    TRY(ensure(ctx, W.ovl_c, std::max(1u, B.n_pairs)));
    W.kt.begin(ctx, PASS_WINDOWS, KN_SKETCH, 0);    // bytes: filled in from the round's counters (minimizers produced, bases sketched)
    TRY(launch_sketch(ctx, W, SketchJob{R.store, B.n_reads, G.word_off[B.n_reads], G.max_words, w, P.k, P.hpc, nullptr, w, false, only_changed,
                                     P.kmer_filter ? W.fs.view : SketchFilter{}}));   // (every round and the final pass: the one filter of the raw reads, as ha_flt_tab)
    W.kt.end(ctx);
    unsigned long long *mz_total = (unsigned long long *)(ct + CT_MZ_LO);
    const uint32_t max_slot = P.full_lists ? longest_slot(G, B.n_reads) : 0u;
    W.kt.begin(ctx, PASS_WINDOWS, KN_UNIQ, 0);
    size_t t_long = 0; bool long_timed = false;
    TRY(launch_uniq(ctx, W, UniqJob{B.n_reads, G.max_words, only_changed, mz_total, P.full_lists != 0, max_slot, P.full_lists ? reads_above(R.len, FSV_UQ_MAX) : 0u, ct + CT_UQ_LONG},
                    [&] { W.kt.end(ctx); t_long = W.kt.begin(ctx, KN_UNIQ_LONG, 0); long_timed = true; }));   // (the long class: timed on its own)
    if (long_timed) W.kt.end(ctx, t_long);
    else W.kt.end(ctx);
    ts.stop();
    if (B.n_pairs == 0) return FSV_OK;
    Span tc(ctx, W.kt, ST_CHAIN);
    ChainArgs A;
    A.store = R.store; A.word_off = W.word_off.p; A.read_len = W.len.p;
    A.set_start = W.set_start.p; A.pair_base = W.pair_base.p; A.upair_base = W.upair_base.p;
    A.mz = W.mz.p; A.mz_off = W.mz_off.p; A.mz_cnt = W.mz_cnt.p;
    A.ovl = W.ovl.p; A.tasks = W.tasks.p; A.task_counter = ct + CT_TASKS; A.task_cap = R.task_cap;
    A.overflow = ct + CT_OVERFLOW; A.warn = W.warn.p; A.set_cols = W.set_cols.p; A.thr_tab = W.thr_tab.p;
    A.n_sets = B.n_sets; A.k_score = P.k; A.min_anchors = min_anchors; A.min_ovlp = min_ovlp; A.bw = final_pass ? P.bw_final : P.bw_ec;
    A.emit_tasks = final_pass ? 0 : 1; A.primary_only = 0;
    // LDS per pair: the anchor arrays for FSV_AMAX entries -- 12 B each in the compact layout (every read of the batch below
    // 65 536 bases), so the tile no longer has to be cut to the batch's longest list to keep several pairs per CU
    A.upair_tab = W.upair_tab.p; A.pair_list = nullptr; A.n_list_dev = nullptr;
    A.amax = wide_anchors ? FSV_AMAX_WIDE : FSV_AMAX;
    // a pair whose lists both exceed the tile is set aside and chained with the large tile afterwards (reads above ~25 kb)
    A.wide_list = nullptr; A.n_wide = nullptr;
    if (!wide_anchors) {
        TRY(ensure(ctx, W.wide_list, (size_t)B.n_upairs + 4));
        A.wide_list = W.wide_list.p; A.n_wide = ct + CT_WIDE;
    }
    // full_lists = 1: a pair with more anchors than the tile in use is set aside, not cut (the counter is the round's own and zeroed with its row)
    A.spill_list = nullptr; A.n_spill = nullptr;
    if (P.full_lists) {
        TRY(ensure(ctx, W.spill_list, (size_t)B.n_upairs + 4));
        A.spill_list = W.spill_list.p; A.n_spill = ct + CT_SPILL;
    }
    A.stamps = nullptr;
    if (getenv("FSV_CHAIN_STAMPS")) {   // diagnostic: where a k_chain wave spends its cycles (never in a measured run)
        TRY(ensure(ctx, W.tmp, 16));
        TRY(zero(ctx, W.tmp, 16));
        A.stamps = W.tmp.p;
    }
    // algorithmic bytes of the launch are filled in when the batch ends (they need the counts this launch leaves on the device)
    W.kt.begin(ctx, PASS_WINDOWS, KN_CHAIN, 0);
    const uint32_t n_chunks = ((B.n_upairs + FSV_CHAIN_CH - 1) / FSV_CHAIN_CH + 7u) & ~7u;   // (xcd_block: a multiple of eight blocks)
    TRY(launch_chain(ctx, CHAIN_CHUNKS, R.short_reads, n_chunks, A, B.n_upairs));
    if (A.wide_list) TRY(chain_wide_pairs(ctx, A, R.short_reads, B.n_upairs));
    W.kt.end(ctx);
    TRY(chain_spilled_pairs(ctx, W, A, B.n_upairs, max_slot, ct));
    if (A.stamps) {
        unsigned long long h[16];
        TRY(download(ctx, h, W.tmp, 16));
        FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
        static const char *nm[7] = {"stage lists", "lookups", "exit: few anchors", "compaction", "chain DP", "best + walk", "tasks + records"};
        fprintf(stderr, "[fsv] k_chain (%u pairs, tasks %d):", B.n_upairs, A.emit_tasks);
        for (int i = 0; i < 7; i++) fprintf(stderr, " %s %.0f cyc x %llu;", nm[i], h[8 + i] ? (double)h[i] / h[8 + i] : 0.0, h[8 + i]);
        fprintf(stderr, "\n");
        A.stamps = nullptr;
    }
    W.last_chain = A;
    tc.stop();
    return FSV_OK;
}

// ---- layout (host): containment removal, longest mutual out-arcs, unitig walk ------------------------------
// Oriented node v = 2*read + strand.  A hit (q forward, t on strand rev) with x_e == len(q)-1 and y_s == 0 is the
// arc (q,+) -> (t,rev); its complement is (t,!rev) -> (q,-).  Mirrors ma_hit_contained / ma_hit2arc / asg_arc_del_trans
// on error-free linear data (Overlaps.cpp:1198, 2152, 4531; Overlaps.h:178-246) and ma_ug_seq for the sequence.
struct Piece { uint32_t read, rev, len; };
void layout_set(const int32_t *len, uint32_t n, const fsv_hit *hits, uint32_t n_hit, int min_reads,
                std::vector<std::vector<Piece>> &contigs, bool &fallback)
{
    std::vector<uint8_t> contained(n, 0), used(n, 0);
    std::vector<int32_t> succ(2 * n, -1), sovl(2 * n, 0), pred(2 * n, -1);
    fallback = false;
    // ma_hit2arc (Overlaps.h:178-246) from the query's side of every hit; the mirrored hit supplies the other side.
    // tl5 / tl3 = overhang of the target in front of / behind the overlap on the query's strand (y is strand-corrected).
    struct Geom { int ql, tl, qs, qe, tl5, tl3, ext5, ext3, tspan; bool internal; };
    auto geom = [&](const fsv_hit &h) {
        Geom g;
        g.ql = len[h.q]; g.tl = len[h.t]; g.qs = h.x_s; g.qe = h.x_e + 1; g.tl5 = h.y_s; g.tl3 = g.tl - (h.y_e + 1);
        g.ext5 = std::min(g.qs, g.tl5); g.ext3 = std::min(g.ql - g.qe, g.tl3); g.tspan = h.y_e + 1 - h.y_s;
        g.internal = g.ext5 > 1000 || g.ext3 > 1000 || (g.qe - g.qs) < (g.qe - g.qs + g.ext5 + g.ext3) * 0.8f || g.tspan < (g.tspan + g.ext5 + g.ext3) * 0.8f;
        return g;
    };
    for (uint32_t i = 0; i < n_hit; i++) {
        const fsv_hit &h = hits[i];
        const Geom g = geom(h);
        if (g.internal) continue;
        if (g.qs <= g.tl5 && g.ql - g.qe <= g.tl3) {                       // MA_HT_QCONT
            if (g.qs >= g.tl5 && g.ql - g.qe >= g.tl3) { if (h.q > h.t) contained[h.q] = 1; } // mutual: keep the lower index
            else contained[h.q] = 1;
        }
    }
    for (uint32_t v = 0; v < 2 * n; v++) sovl[v] = 0x7fffffff;
    for (uint32_t i = 0; i < n_hit; i++) {
        const fsv_hit &h = hits[i];
        const Geom g = geom(h);
        if (g.internal || contained[h.q] || contained[h.t]) continue;
        if ((g.qs <= g.tl5 && g.ql - g.qe <= g.tl3) || (g.qs >= g.tl5 && g.ql - g.qe >= g.tl3)) continue; // containments
        if (g.qe - g.qs + g.ext5 + g.ext3 < 50 || g.tspan + g.ext5 + g.ext3 < 50) continue;                 // MA_HT_SHORT_OVLP
        int from, to, l;
        if (g.qs > g.tl5) { from = 2 * (int)h.q; to = 2 * (int)h.t + (int)h.rev; l = g.qs - g.tl5; }          // (q,+) -> (t,rev)
        else { from = 2 * (int)h.q + 1; to = 2 * (int)h.t + (h.rev ? 0 : 1); l = (g.ql - g.qe) - g.tl3; }      // (q,-) -> (t,!rev)
        // every node keeps its nearest successor: the smallest node length = the longest overlap
        if (l < sovl[from] || (l == sovl[from] && succ[from] >= 0 && to < succ[from])) { succ[from] = to; sovl[from] = l; }
    }
    for (uint32_t v = 0; v < 2 * n; v++) { int w = succ[v]; if (w >= 0 && succ[w ^ 1] != (int)(v ^ 1)) succ[v] = -1; }
    for (uint32_t v = 0; v < 2 * n; v++) if (succ[v] >= 0) pred[succ[v]] = (int)v;
    // ma_ug_gen (Overlaps.cpp:7759): vertices in increasing order; the unitig through the first unvisited one is emitted in that
    // vertex's direction, from its start (found by walking the in-arcs back).  So the lowest-numbered read of a chain sits on its
    // forward strand -- the two directions spell reverse complements only while every overlap is exact.
    for (uint32_t v = 0; v < 2 * n; v++) {
        const uint32_t r = v >> 1;
        if (contained[r] || used[r]) continue;
        int start = (int)v, steps = 0;
        while (pred[start] >= 0 && !used[pred[start] >> 1] && steps < (int)(2 * n)) { start = pred[start]; steps++; if (start == (int)v) break; }
        int cnt = 0;
        for (int w = start; w >= 0 && !used[w >> 1] && cnt <= (int)(2 * n); w = succ[w]) { cnt++; if (succ[w] == start) break; }
        if (cnt < min_reads) continue;
        std::vector<Piece> c;
        for (int w = start; w >= 0 && !used[w >> 1]; w = succ[w]) {
            used[w >> 1] = 1;
            const bool more = succ[w] >= 0 && !used[succ[w] >> 1];
            c.push_back(Piece{(uint32_t)(w >> 1), (uint32_t)(w & 1), (uint32_t)(more ? sovl[w] : len[w >> 1])});
        }
        contigs.push_back(std::move(c));
    }
    // no fall-back to a single read: hifiasm's asg_cut_tip (Overlaps.cpp:4666-4709) removes dead-end chains of fewer than four
    // reads, a lone read included, and writes no contig for such a set
    fallback = contigs.empty();
}

} // namespace

extern "C" void fsv_asm_default_params(fsv_asm_params *p)
{
    if (!p) return;
    p->k = 51; p->w = 51; p->hpc = 1; p->n_rounds = 3; p->min_ovlp = 1; p->min_anchors = 1; p->lookback = 64;   // hifiasm keeps every (target, strand) group that shares a minimizer, whatever its length
    p->bw_ec = 20; p->bw_final = 0; p->min_contig_reads = 4;
    p->win_rate_pm = 40; p->k_cap = FSV_K_MAX; p->accept_err_pm = 30; p->bw_rechain = 1; p->w_later = 0; p->partition = 1; p->second_round = 1; p->ins_dag = 1;
    p->min_anchors_final = 1; p->min_ovlp_final = 1; p->graph_layout = 1; p->junction_cigars = 1;
    p->full_lists = 0;
    p->deep_sets = 0;
    p->kmer_filter = 0;
    p->kmer_table = 0;
    p->partial_charge = 0;
}

extern "C" void fsv_asm_ont_params(fsv_asm_params *p)
{
    if (!p) return;
    fsv_asm_default_params(p);
    p->min_ovlp = 500; p->min_anchors = 3;      // chains of noisy reads: three seeds and 500 bases make an overlap (hifiasm's HiFi rule -- one shared seed -- would chain noise)
    p->k = 15; p->w = 15; p->hpc = 0;           // 15-mers survive 10 % error often enough to seed (20 % of them per read); no HPC: indel errors dominate
    p->bw_ec = 150; p->bw_final = 50;           // chains of noisy reads drift by several per cent between anchors
    p->win_rate_pm = 250; p->k_cap = FSV_K_WIDE; p->accept_err_pm = 300;   // two 10 % reads differ by ~20 %: k = 93 for a full window
    p->bw_rechain = 50;                         // corrected reads keep a 1-base indel every few kb
    p->w_later = 63;                            // after one round the reads are ~99 % accurate: sparser seeds keep a pair's anchors below 1 024
    p->partition = 0;                           // coincident errors of 10 % reads would pass for alleles and split the set
    p->second_round = 0;                        // the junction vote: what the ONT outcome was validated with (and a third less work)
    p->ins_dag = 0;                             // at 10 % error nearly every column has inserted strings that disagree: the most frequent one, per lane
    p->min_contig_reads = 2;                    // reads of 10-30 kb tile a 50 kb window with three or four uncontained reads: hifiasm's tip rule (4) would drop them
    p->min_anchors_final = 0; p->min_ovlp_final = 0; p->graph_layout = 0;   // the layout this profile was validated with
}

// CLR reads (the reference: `flye --pacbio-raw`, run_assembly.py:46-72): ~12 % error, insertions before deletions before
// substitutions, reads of 10-25 kb.  Two such reads differ by about a quarter of a window, which the ONT profile's thresholds (k = 93 of
// 375 columns, overlaps up to 30 % error, 15-mer seeds without homopolymer compression) already hold: the same values, under a name of
// their own so that the two data types can part ways.  Planted truth on the synthetic CLR profile: tests/test_gpu_ont.py.
extern "C" void fsv_asm_clr_params(fsv_asm_params *p)
{
    fsv_asm_ont_params(p);
}

extern "C" int fsv_assemble_batch_bound(const fsv_readsets *sets, uint64_t *seq_cap, uint32_t *contig_cap)
{
    if (!sets || !sets->read_len) return FSV_EINVAL;
    uint64_t tot = 0;
    for (uint32_t r = 0; r < sets->n_reads; r++) tot += (uint64_t)sets->read_len[r];
    // a contig is a concatenation of prefixes of distinct (corrected) reads; consensus can lengthen a read slightly
    if (seq_cap) *seq_cap = tot + tot / 8 + 1024 * (uint64_t)sets->n_sets + 4096;
    if (contig_cap) *contig_cap = sets->n_reads + sets->n_sets + 1;
    return FSV_OK;
}

// A task list for K6, with its K5 results and the counter row its lists are counted in
struct PathJob {
    const uint32_t *store; fsv_wtask *tasks; fsv_wres *res; fsv_wpath *paths;
    uint32_t task_cap; const uint32_t *n_tasks_dev; uint32_t *ct;   // the bound the grids are sized for; the count on the device (null: task_cap)
    int pass, round;
    bool wide_bands; int k_cap;
    bool all_accepted;    // every task belongs to an accepted overlap (W.ovl then holds that one overlap)
};

// The two walk kernels nearly every window that needs a walk goes to: the sub-band kernel (distance 4 .. FSV_SB_MAXERR) and, a launch per
// distance, the walk without the matrix (distance <= 3: nine in ten).  persistent(per_cu): the grid of path_stage.
// STAMP (FSV_K6_STAMPS=1; diagnostic, never in a measured run): the kernels' stamp instantiations, each launch waited for and where its
// waves spent their cycles printed -- PhaseClock's layout: cycles of phase i in h[i], trips through the list that passed it in h[8 + i].
template <bool STAMP, class Grid>
static int path_walks(fsv_ctx *ctx, AsmWs &W, const PathJob &J, Grid persistent)
{
    const uint32_t *store = J.store; const fsv_wtask *tasks = J.tasks; const fsv_wres *res = J.res; fsv_wpath *paths = J.paths;
    uint32_t *ct = J.ct;
    unsigned long long h[16] = {0};
    uint32_t nl = 0;
    auto clear_stamps = [&]() -> int { TRY(ensure(ctx, W.tmp, 16)); return zero(ctx, W.tmp, 16); };
    auto read_stamps = [&](const uint32_t *cnt) -> int {   // waits for the launch: its stamps in h, its list's length in nl
        TRY(download(ctx, h, W.tmp, 16));
        if (cnt) FSV_HIP(ctx, hipMemcpyAsync(&nl, cnt, 4, hipMemcpyDeviceToHost, ctx->stream));
        FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return FSV_OK;
    };
    auto per_wave = [&](int i) { return h[8 + i] ? (double)h[i] / h[8 + i] : 0.0; };
    if (!W.occ_sb) FSV_HIP(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&W.occ_sb, k_path_sb<false>, 64, 0));
    const uint32_t grid = persistent(W.occ_sb);
    TRY(ensure(ctx, W.cols_sb, (size_t)grid * FSV_SB_QUADS * 64));
    if (STAMP) TRY(clear_stamps());
    FSV_LAUNCH(ctx, ctx->stream, k_path_sb<STAMP>, dim3(grid), dim3(64), 0, store, tasks, res, W.dp_list2.p, ct + CT_DP_SB, paths, W.cols_sb.p,
               STAMP ? W.tmp.p : nullptr);
    if (STAMP) {
        TRY(read_stamps(nullptr));
        fprintf(stderr, "[fsv] k_path_sb round %d: %llu waves, cycles per wave: forward %.0f, walk %.0f, finish %.0f (grid %u)\n", J.round, h[8], per_wave(0), per_wave(1),
                per_wave(2), grid);
    }
    auto fr = [&](auto kern, int e, const Dev<uint32_t> &list, uint32_t *cnt) -> int {
        int &pf = W.occ_fr[e - 1];
        if (!pf || STAMP) FSV_HIP(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&pf, kern, 64, 0));
        if (STAMP) TRY(clear_stamps());
        FSV_LAUNCH(ctx, ctx->stream, kern, dim3(persistent(pf)), dim3(64), 0, store, tasks, res, list.p, cnt, paths, STAMP ? W.tmp.p : nullptr);
        if (STAMP) {
            TRY(read_stamps(cnt));
            fprintf(stderr, "[fsv] k_path_fr<%d> round %d: %u windows, %llu waves (%d per CU), cycles per wave: table %.0f, walk %.0f, finish %.0f\n", e, J.round, nl, h[8], pf,
                    per_wave(0), per_wave(1), per_wave(2));
        }
        return FSV_OK;
    };
    TRY(fr(k_path_fr<1, STAMP>, 1, W.dp_list16, ct + CT_DP_SB16));
    TRY(fr(k_path_fr<2, STAMP>, 2, W.dp_list, ct + CT_DP));
    TRY(fr(k_path_fr<3, STAMP>, 3, W.dp_list_e3, ct + CT_DP_FR3));
    return FSV_OK;
}

// K6 for a task list: the fast paths, then the DP kernels on what is left (the lists and their counters live in the counter row J.ct).
// Used for the window tasks of a round, the junction tasks of its second consensus pass, the junction cigars of its partition,
// and for the caller's tasks of fsv_bpm_paths.
static int path_stage(fsv_ctx *ctx, AsmWs &W, const PathJob &J)
{
    const uint32_t *store = J.store; const fsv_wtask *tasks = J.tasks; const fsv_wres *res = J.res; fsv_wpath *paths = J.paths;
    uint32_t *ct = J.ct;
    const uint32_t task_cap = J.task_cap, n_cu = (uint32_t)ctx->n_cu;
    // a persistent grid: as many blocks as the device holds at once (per_cu each CU), never more than one wave per 64 tasks
    auto persistent = [&](int per_cu) { return std::min<uint32_t>(fsv_grid_for(task_cap, 64), (uint32_t)std::max(1, per_cu) * n_cu); };
    W.kt.begin(ctx, J.pass, KN_PATH_FAST, 0);
    const bool fix = J.pass == PASS_WINDOWS && !J.wide_bands;      // fix_boundary: the windows' final cigars only (not the junction alignments)
    if (fix) TRY(ensure(ctx, W.fix_list, task_cap));
    const PathLists lists{{W.dp_list16.p, W.dp_list.p, W.dp_list_e3.p, W.dp_list2.p, W.dp_list3.p, W.dp_wide.p, W.dp_xwide.p, fix ? W.fix_list.p : nullptr},
                          {ct + CT_DP_SB16, ct + CT_DP, ct + CT_DP_FR3, ct + CT_DP_SB, ct + CT_DP_GEN, ct + CT_DP_WIDE, ct + CT_DP_XW, fix ? ct + CT_FIX : nullptr}};
    FSV_LAUNCH(ctx, ctx->stream, k_path_fast, dim3((fsv_grid_for(task_cap, 256) + 7u) & ~7u), dim3(256), 0, store, W.ovl.p, tasks, res, task_cap, paths, lists,
               J.all_accepted, J.n_tasks_dev);
    W.kt.end(ctx);
    // what the fast paths left: distance <= 3 is walked without the DP matrix (k_path_fr), <= FSV_SB_MAXERR by the sub-band kernel,
    // the rest by the general one
    W.kt.begin(ctx, J.pass, KN_PATH_DP, 0);
    // persistent grids, each block striding through its list, so the column scratch is a fixed few hundred MB whatever the number of windows
    TRY(getenv("FSV_K6_STAMPS") ? path_walks<true>(ctx, W, J, persistent) : path_walks<false>(ctx, W, J, persistent));
    // the general kernel's lists are short (rescue windows, distances above 7): two blocks per CU are plenty
    const uint32_t gridg = persistent(2);
    TRY(ensure(ctx, W.cols, (size_t)gridg * 64 * (FSV_WINDOW + 2) * 3));
    FSV_LAUNCH(ctx, ctx->stream, k_path_dp<uint32_t>, dim3(gridg), dim3(64), 0, store, tasks, W.dp_list3.p, ct + CT_DP_GEN, paths,
               (uint32_t *)W.cols.p /* 32-bit columns in the same scratch */);
    FSV_LAUNCH(ctx, ctx->stream, k_path_dp<uint64_t>, dim3(gridg), dim3(64), 0, store, tasks, W.dp_wide.p, ct + CT_DP_WIDE, paths, W.cols.p);
    if (J.wide_bands) {
        // bands above 63 rows: every gapped window of an ONT-profile batch; 1.15 MB of column scratch per persistent block
        if (!W.occ_wide) FSV_HIP(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&W.occ_wide, k_path_wide, 64, 0));
        const uint32_t gridw = persistent(std::min(W.occ_wide, 12));
        TRY(ensure(ctx, W.cols_wide, (size_t)gridw * FSV_WINDOW * 2 * FSV_WL * 64));
        FSV_LAUNCH(ctx, ctx->stream, k_path_wide, dim3(gridw), dim3(64), 0, store, tasks, res, W.dp_xwide.p, ct + CT_DP_XW, paths, W.cols_wide.p, J.k_cap);
    }
    if (fix)
        // fix_boundary (Correct.cpp:1676): the few windows whose alignment may touch the edge of its band (k_path_fast listed them)
        FSV_LAUNCH(ctx, ctx->stream, k_fix_boundary, dim3(persistent(8)), dim3(64), 0, store, W.fix_list.p, ct + CT_FIX, J.tasks, J.res, paths, J.k_cap, ct + CT_FIXED);
    W.kt.end(ctx);
    return FSV_OK;
}

// The second consensus pass of a round (process_boundary, Correct.cpp:4453): see k_consensus.h "second consensus pass".
// Runs between the windows' consensus (cwin / cwin_len final for the first pass) and k_newlen; leaves cwin / cwin_len patched.
static int second_pass(fsv_ctx *ctx, AsmWs &W, const Round &R)
{
    const fsv_asm_params &P = R.P; const Batch &B = R.B; const Geometry &G = R.G;
    const uint32_t n_gwin = R.n_gwin, task_cap = R.task_cap;
    uint32_t *ct2 = W.ct_of(R.row(PASS_JUNCTIONS));
    // where window g starts in the first pass's result, and that result as a 2-bit store behind a copy of the round's reads
    TRY(ensure(ctx, W.lb, std::max(1u, n_gwin)));
    W.kt.begin(ctx, PASS_JUNCTIONS, KN_BND, 0);
    FSV_LAUNCH(ctx, ctx->stream, k_newlen, dim3(fsv_grid_for(B.n_reads, 256)), dim3(256), 0, W.gwin_off.p, W.cwin_len.p, B.n_reads, W.new_len.p, W.lb.p);
    const uint32_t a_words = G.word_off[B.n_reads];
    std::vector<uint32_t> brel(B.n_reads + 1, 0);
    for (uint32_t r = 0; r < B.n_reads; r++) {
        const uint64_t nx = (uint64_t)brel[r] + (uint64_t)(G.gwin_off[r + 1] - G.gwin_off[r]) * (FSV_CW_STRIDE / 16) + 2;
        if (nx + a_words >= (1ull << 32)) return fsv_fail(ctx, FSV_EUNSUP, "second consensus pass: store larger than 2^32 words; split the batch");
        brel[r + 1] = (uint32_t)nx;
    }
    const uint32_t b_words = brel[B.n_reads];
    TRY(ensure(ctx, W.sr_store, (size_t)a_words + b_words + 16));
    FSV_HIP(ctx, hipMemcpyAsync(W.sr_store.p, R.store, (size_t)a_words * 4, hipMemcpyDeviceToDevice, ctx->stream));
    TRY(upload(ctx, W.brel_off, brel));
    uint32_t *store2 = W.sr_store.p;
    FSV_LAUNCH(ctx, ctx->stream, k_repack, dim3(B.n_reads), dim3(256), 0, W.gwin_off.p, W.lb.p, W.cwin.p, W.brel_off.p, W.new_len.p, B.n_reads, 0, store2 + a_words,
               W.read_dirty.p);
    FSV_HIP(ctx, hipMemsetAsync(store2 + a_words + b_words, 0, 32, ctx->stream));
    // junction tasks
    TRY(ensure_each(ctx, task_cap, W.tasks2, W.res2, W.paths2, W.idx2, W.tasks3, W.res3, W.src3));
    TRY(ensure_each(ctx, (size_t)n_gwin + 2, W.bnd_flag, W.bnd_list, W.bnd_patch));
    TRY(ensure(ctx, W.bnd_bytes, (size_t)(n_gwin + 2) * FSV_CW_STRIDE));
    TRY(zero(ctx, W.bnd_flag, (size_t)n_gwin + 2));
    BndArgs A;
    A.tasks = W.tasks.p; A.paths = W.paths.p; A.n_tasks = R.ct + CT_TASKS;
    A.ovl_c = W.ovl_c.p; A.pair_base = W.pair_base.p; A.set_start = W.set_start.p; A.n_sets = B.n_sets; A.pair_read = W.pair_read.p;
    A.gwin_off = W.gwin_off.p; A.lb = W.lb.p; A.cwin_len = W.cwin_len.p;
    A.cov3 = W.cov3.p; A.read_dirty = W.read_dirty.p;
    A.brel_off = W.brel_off.p; A.b_base = a_words; A.thr_tab = W.thr_tab.p;
    A.tasks2 = W.tasks2.p; A.idx2 = W.idx2.p; A.n_tasks2 = ct2 + CT_TASKS;
    A.bnd_flag = W.bnd_flag.p; A.bnd_list = W.bnd_list.p; A.n_bnd = ct2 + CT_B_LIST; A.store2 = store2;
    A.deep_list = nullptr; A.deep_n = nullptr; A.deep_cap = 0;
    if (P.deep_sets) {      // a junction is listed at most once
        TRY(ensure(ctx, W.deep_blist, (size_t)n_gwin + 2));
        A.deep_list = W.deep_blist.p; A.deep_n = R.ct + CT_DEEP_B; A.deep_cap = n_gwin + 2;
    }
    FSV_LAUNCH(ctx, ctx->stream, k_bnd_tasks, dim3((fsv_grid_for(task_cap, 256) + 7u) & ~7u), dim3(256), 0, A);
    W.kt.end(ctx);
    W.kt.begin(ctx, PASS_JUNCTIONS, KN_BPM, 0);
    // K5, once more with the doubled threshold for the tasks without an alignment, K6
    TRY(fsv_bpm_windows_dev_n(ctx, store2, W.tasks2.p, task_cap, ct2 + CT_TASKS, W.res2.p, P.k_cap));
    FSV_LAUNCH(ctx, ctx->stream, k_bnd_retry, dim3(fsv_grid_for(task_cap, 256)), dim3(256), 0, W.tasks2.p, W.res2.p, ct2 + CT_TASKS, W.tasks3.p, W.src3.p,
               ct2 + CT_B_RETRY, P.k_cap);
    TRY(fsv_bpm_windows_dev_n(ctx, store2, W.tasks3.p, task_cap, ct2 + CT_B_RETRY, W.res3.p, P.k_cap));
    FSV_LAUNCH(ctx, ctx->stream, k_bnd_scatter, dim3(fsv_grid_for(task_cap, 256)), dim3(256), 0, W.res2.p, W.res3.p, W.src3.p, ct2 + CT_B_RETRY);
    W.kt.end(ctx);
    TRY(path_stage(ctx, W, PathJob{store2, W.tasks2.p, W.res2.p, W.paths2.p, task_cap, ct2 + CT_TASKS, ct2, PASS_JUNCTIONS, R.round, R.wide_bands, P.k_cap, false}));
    // the junctions' consensus, handed to the windows as patches
    const uint32_t grid_l = std::min<uint32_t>(std::max(1u, n_gwin), (uint32_t)ctx->n_cu * 16);
    W.kt.begin(ctx, PASS_JUNCTIONS, KN_BND_CONS, 0);
    if (P.deep_sets) {
        if (R.wide_bands) FSV_LAUNCH(ctx, ctx->stream, (k_bnd_consensus<FSV_EV_CAP_WIDE, true>), dim3(grid_l), dim3(64), 0, R.C, A, W.paths2.p, store2, W.bnd_patch.p, W.bnd_bytes.p);
        else FSV_LAUNCH(ctx, ctx->stream, (k_bnd_consensus<FSV_EV_CAP, true>), dim3(grid_l), dim3(64), 0, R.C, A, W.paths2.p, store2, W.bnd_patch.p, W.bnd_bytes.p);
    } else {
        if (R.wide_bands) FSV_LAUNCH(ctx, ctx->stream, (k_bnd_consensus<FSV_EV_CAP_WIDE, false>), dim3(grid_l), dim3(64), 0, R.C, A, W.paths2.p, store2, W.bnd_patch.p, W.bnd_bytes.p);
        else FSV_LAUNCH(ctx, ctx->stream, (k_bnd_consensus<FSV_EV_CAP, false>), dim3(grid_l), dim3(64), 0, R.C, A, W.paths2.p, store2, W.bnd_patch.p, W.bnd_bytes.p);
    }
    if (P.deep_sets) {      // the listed junctions once more, before their patches are applied (the list's length is on the device only)
        W.kt.end(ctx);
        W.kt.begin(ctx, KN_BND_DEEP, 0);
        FSV_LAUNCH(ctx, ctx->stream, k_bnd_consensus_deep, dim3(R.deep_grid), dim3(64), 0, R.C, A, W.paths2.p, store2, W.bnd_patch.p, W.bnd_bytes.p, R.deep);
        W.kt.end(ctx);
        W.kt.begin(ctx, KN_BND_CONS, 0);
    }
    FSV_LAUNCH(ctx, ctx->stream, k_bnd_apply, dim3(std::max(1u, n_gwin)), dim3(64), 0, W.gwin_read.p, W.gwin_off.p, W.bnd_patch.p, W.bnd_bytes.p, W.bnd_flag.p, n_gwin,
               W.cwin.p, W.cwin_len.p, W.changed.p, W.warn.p);
    W.kt.end(ctx);
    return FSV_OK;
}

// K5 + K6 on caller-supplied tasks: the launch code fsv_assemble_batch drives (path_stage, on this context's workspace), with every
// task treated as belonging to an accepted overlap and without fix_boundary.  Leaves the last assembly's reads and contigs alone
// (fsv_asm_fetch_reads / fsv_align_batch may follow): the store goes into a buffer of its own.
static int fsv_bpm_paths_impl(fsv_ctx *ctx, const uint32_t *store, size_t store_words, const fsv_wtask *tasks, uint32_t n_tasks,
                             fsv_wres *res, fsv_wpath *paths)
{
    if (!ctx || !store || (!tasks && n_tasks) || (!res && n_tasks) || (!paths && n_tasks)) return FSV_EINVAL;
    if (n_tasks == 0) return FSV_OK;
    int kmax = 0;
    for (uint32_t i = 0; i < n_tasks; i++) {
        if (tasks[i].k > FSV_K_WIDE || tasks[i].x_len == 0 || tasks[i].x_len > FSV_WINDOW) return fsv_fail(ctx, FSV_EINVAL, "task k/x_len out of range");
        kmax = std::max<int>(kmax, tasks[i].k);
    }
    const int k_cap = kmax > FSV_K_MAX ? kmax : FSV_K_MAX;     // a threshold above 31 anywhere: K5 of the whole list through the wide kernel
    FSV_HIP(ctx, hipSetDevice(ctx->device));
    AsmWs &W = *ws_get(ctx);
    W.kt.reset();       // (path_stage times its launches: no record of them is left for a later batch's statistics)
    std::vector<fsv_wtask> t(tasks, tasks + n_tasks);
    for (auto &x : t) x.ovl = 0;
    fsv_ovl o; memset(&o, 0, sizeof(o)); o.valid = 1; o.is_match = 1;
    Dev<uint32_t> d_store;
    TRY(ensure(ctx, d_store, store_words + 16));
    TRY(zero(ctx, d_store, store_words + 16));
    FSV_HIP(ctx, hipMemcpyAsync(d_store.p, store, store_words * 4, hipMemcpyHostToDevice, ctx->stream));
    TRY(upload(ctx, W.tasks, t));
    TRY(upload(ctx, W.ovl, std::vector<fsv_ovl>{o}));
    TRY(ensure_each(ctx, n_tasks, W.res, W.paths, W.dp_list, W.dp_list2, W.dp_list3, W.dp_list16, W.dp_list_e3, W.dp_wide, W.dp_xwide));
    TRY(ensure(ctx, W.counters, CT_SLOT));
    TRY(zero(ctx, W.counters, CT_SLOT));
    TRY(zero(ctx, W.paths, n_tasks));
    TRY(fsv_bpm_windows_dev_n(ctx, d_store.p, W.tasks.p, n_tasks, nullptr, W.res.p, k_cap));
    TRY(path_stage(ctx, W, PathJob{d_store.p, W.tasks.p, W.res.p, W.paths.p, n_tasks, nullptr, W.counters.p, PASS_NONE, 0, kmax > FSV_K_MAX, k_cap, true}));
    TRY(download(ctx, res, W.res, n_tasks));
    TRY(download(ctx, paths, W.paths, n_tasks));
    FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return FSV_OK;
}

// the extension kernel over a task list: the launch fsv_assemble_batch (charge_stage) and fsv_bpm_extensions share.  A persistent grid
// striding through the list; bound sizes it, *n_dev (when given) is the count.  list: the slots to run (null: slot i = task i).
static int launch_bpm_ext(fsv_ctx *ctx, const uint32_t *store, const fsv_wtask *tasks, const uint32_t *list, const uint32_t *n_dev, uint32_t bound, int k_cap,
                          fsv_wext *out, unsigned long long *n_run)
{
    if (!bound) return FSV_OK;
    const uint32_t grid = std::min<uint32_t>(fsv_grid_for(bound, 64), 8u * (uint32_t)std::max(1, ctx->n_cu));
    FSV_LAUNCH(ctx, ctx->stream, k_bpm_ext, dim3(grid), dim3(64), 0, store, tasks, list, n_dev, bound, k_cap, out, n_run);
    return FSV_OK;
}

// the extension kernel on caller-supplied tasks, through launch_bpm_ext as charge_stage drives it (here: every slot holds a task)
static int fsv_bpm_extensions_impl(fsv_ctx *ctx, const uint32_t *store, size_t store_words, const fsv_wtask *tasks, const uint8_t *dir, uint32_t n_tasks,
                                   int32_t k_cap, fsv_wext *out)
{
    if (!ctx || !store || (n_tasks && (!tasks || !dir || !out))) return FSV_EINVAL;
    if (k_cap < 1 || k_cap > FSV_K_WIDE) return fsv_fail(ctx, FSV_EINVAL, "k_cap must be in [1, 95]");
    if (n_tasks == 0) return FSV_OK;
    std::vector<fsv_wtask> t(tasks, tasks + n_tasks);
    for (uint32_t i = 0; i < n_tasks; i++) {
        fsv_wtask &x = t[i];
        if (x.k > FSV_K_MAX || x.x_len == 0 || x.x_len > FSV_WINDOW || dir[i] > 1) return fsv_fail(ctx, FSV_EINVAL, "extension task: k <= 31 (FSV_K_MAX), 1 <= x_len <= 375, dir 0 or 1");
        // every base the kernel may touch lies inside the caller's store
        if (x.x_start < 0 || x.y_len < 0 || (uint64_t)x.x_word + ((uint64_t)x.x_start + x.x_len + 15) / 16 > store_words ||
            (uint64_t)x.y_word + ((uint64_t)x.y_len + 15) / 16 > store_words)
            return fsv_fail(ctx, FSV_EINVAL, "extension task reaches outside the store");
        x.ovl = i; x.win = dir[i];
    }
    FSV_HIP(ctx, hipSetDevice(ctx->device));
    AsmWs &W = *ws_get(ctx);
    Dev<uint32_t> d_store;
    TRY(ensure(ctx, d_store, store_words + 16));
    TRY(zero(ctx, d_store, store_words + 16));
    FSV_HIP(ctx, hipMemcpyAsync(d_store.p, store, store_words * 4, hipMemcpyHostToDevice, ctx->stream));
    TRY(upload(ctx, W.ch.ext_tasks, t));
    TRY(ensure(ctx, W.ch.ext_res, n_tasks));
    TRY(launch_bpm_ext(ctx, d_store.p, W.ch.ext_tasks.p, nullptr, nullptr, n_tasks, k_cap, W.ch.ext_res.p, nullptr));
    TRY(download(ctx, out, W.ch.ext_res, n_tasks));
    FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return FSV_OK;
}

static int fsv_asm_last_charge_impl(const fsv_ctx *ctx, fsv_charge_stats *out)
{
    if (!ctx || !out || !ctx->asm_ws) return FSV_EINVAL;
    const AsmWs &W = *(const AsmWs *)ctx->asm_ws;
    if (!W.ch.valid) return FSV_EINVAL;
    *out = W.ch.last;
    return FSV_OK;
}

extern "C" int fsv_asm_last_stats(const fsv_ctx *ctx, fsv_asm_stats *out)
{
    if (!ctx || !out || !ctx->asm_ws) return FSV_EINVAL;
    *out = ((const AsmWs *)ctx->asm_ws)->stats;
    return FSV_OK;
}

// ---- one chunk of read sets through the whole assembly, stage by stage ---------------------------------------------------------
// Every launch of a round is sized from what the host knows when the round starts (read lengths, the window-task bound); counts the
// kernels produce stay in the round's counter row.  One synchronisation per round is left: the corrected reads' lengths, which the
// host turns into the next round's geometry -- the round's counters ride along with it (finish_round).

// the batch's tables on the device, the geometry of round 0, zeroed counters
static int prepare_batch(fsv_ctx *ctx, AsmWs &W, const fsv_readsets *sets, Round &R)
{
    // (set_start, the read lengths and the word offsets are in range: the entry points have checked -- check_readsets)
    const fsv_asm_params &P = R.P; Batch &B = R.B;
    B.n_reads = sets->n_reads;
    R.set_flags = sets->set_flags;   // (FSV_SET_UNPHASED only picks the layout: the haplotype partition runs for every read of every set, as in hifiasm)
    B.set_start.clear(); R.caller_set.clear();
    for (uint32_t s = 0; s < sets->n_sets; s++) {
        const bool low = !R.low_cov.empty() && R.low_cov[s];
        for (uint32_t r = sets->set_start[s]; r < sets->set_start[s + 1]; r++) if (low || r == sets->set_start[s]) { B.set_start.push_back(r); R.caller_set.push_back(s); }
        if (sets->set_start[s + 1] == sets->set_start[s]) { B.set_start.push_back(sets->set_start[s]); R.caller_set.push_back(s); }
    }
    B.n_sets = (uint32_t)R.caller_set.size();
    B.set_start.push_back(B.n_reads);
    B.read_set.resize(B.n_reads); B.pair_base.resize(B.n_sets + 1); B.upair_base.resize(B.n_sets + 1);
    uint64_t np = 0;
    for (uint32_t s = 0; s < B.n_sets; s++) {
        uint64_t ns = B.set_start[s + 1] - B.set_start[s];
        B.pair_base[s] = (uint32_t)np;
        B.upair_base[s] = (uint32_t)(np / 2);
        np += ns > 1 ? ns * (ns - 1) : 0;
        for (uint32_t r = B.set_start[s]; r < B.set_start[s + 1]; r++) B.read_set[r] = s;
    }
    if (np >= (1ull << 31)) return fsv_fail(ctx, FSV_EUNSUP, "too many read pairs in one batch; split it");
    B.pair_base[B.n_sets] = (uint32_t)np; B.n_pairs = (uint32_t)np;
    B.upair_base[B.n_sets] = (uint32_t)(np / 2); B.n_upairs = (uint32_t)(np / 2);
    std::vector<int32_t> &len = R.len;
    len.assign(sets->read_len, sets->read_len + B.n_reads);

    std::vector<uint8_t> thr(FSV_WINDOW + 1);
    for (int i = 0; i <= FSV_WINDOW; i++) thr[i] = thr_for_len_host(i, P.win_rate_pm);
    TRY(upload(ctx, W.thr_tab, thr));
    TRY(upload(ctx, W.set_start, B.set_start));
    TRY(upload(ctx, W.read_set, B.read_set));
    TRY(upload(ctx, W.pair_base, B.pair_base));
    TRY(upload(ctx, W.upair_base, B.upair_base));
    if (B.n_upairs) {
        TRY(ensure(ctx, W.upair_tab, B.n_upairs));
        TRY(ensure(ctx, W.pair_read, B.n_pairs));
        FSV_LAUNCH(ctx, ctx->stream, k_pair_tab, dim3((B.n_upairs + 255) / 256), dim3(256), 0, W.set_start.p, W.pair_base.p, W.upair_base.p, B.n_sets, B.n_upairs,
                   W.upair_tab.p, W.pair_read.p);
    }
    TRY(ensure(ctx, W.warn, B.n_reads));
    TRY(zero(ctx, W.warn, B.n_reads));

    // minimizer slots stay where they are for the whole call (a read grows by a few bases at most when it is corrected): the
    // final pass can then keep the lists of reads the last round did not change
    R.mz_fixed.assign(B.n_reads + 1, 0);
    {
        uint64_t m = 0;
        for (uint32_t r = 0; r < B.n_reads; r++) { R.mz_fixed[r] = (uint32_t)m; m += mz_slots((int64_t)len[r] + len[r] / 8 + 64, P.w_later > 0 ? std::min(P.w, P.w_later) : P.w, P.full_lists != 0); }
        if (m >= (1ull << 32)) return fsv_fail(ctx, FSV_EUNSUP, "batch too large for 32-bit offsets; split it");
        R.mz_fixed[B.n_reads] = (uint32_t)m;
    }
    TRY(make_geometry(ctx, B, len, R.G, P.w, &R.mz_fixed));
    // round 0 reads the caller's store through the caller's word offsets
    for (uint32_t r = 0; r <= B.n_reads; r++) R.G.word_off[r] = (uint32_t)sets->word_off[r];
    R.store = sets->store_dev;
    R.wide_bands = P.k_cap > FSV_K_MAX;
    for (uint32_t r = 0; r < B.n_reads; r++) { R.reads_in_bytes += (uint64_t)(len[r] + 3) / 4; if (len[r] >= 65536) R.short_reads = false; }
    // rows 0 .. n_rounds: the rounds and the final pass; rows n_rounds + 1 ..: the second consensus pass of every round; rows
    // 2 n_rounds + 2 ..: the junction cigars of every round's partition (Round::row)
    const size_t n_ct = (size_t)(3 * P.n_rounds + 2) * CT_SLOT;
    TRY(ensure(ctx, W.counters, n_ct));
    TRY(zero(ctx, W.counters, n_ct));
    R.h_ct.assign(n_ct, 0u);
    TRY(ensure(ctx, W.set_cols, B.n_reads));       // K5 columns per set, summed over the rounds (statistics)
    TRY(zero(ctx, W.set_cols, B.n_reads));
    return FSV_OK;
}

// the round's geometry on the device, room for its window tasks
static int begin_round(fsv_ctx *ctx, AsmWs &W, Round &R)
{
    R.ct = W.ct_of(R.row(PASS_WINDOWS));
    TRY(upload(ctx, W.word_off, R.G.word_off));
    TRY(upload(ctx, W.len, R.len));
    TRY(upload(ctx, W.mz_off, R.G.mz_off));
    TRY(upload(ctx, W.gwin_off, R.G.gwin_off));
    TRY(upload(ctx, W.gwin_read, R.G.gwin_read));
    if (R.G.task_bound >= (1ull << 31)) return fsv_fail(ctx, FSV_EUNSUP, "window task bound exceeds 2^31; split the batch");
    const uint32_t task_cap = R.task_cap = (uint32_t)std::max<uint64_t>(R.G.task_bound, 1);
    R.n_gwin = R.G.gwin_off[R.B.n_reads];
    TRY(ensure_each(ctx, task_cap, W.tasks, W.res, W.paths, W.dp_list, W.dp_list_e3, W.dp_list2, W.dp_list3, W.dp_list16, W.dp_wide));
    TRY(ensure(ctx, W.dp_xwide, R.wide_bands ? task_cap : 16));
    return FSV_OK;
}

// partial_charge = 1, after K6: the final verdict on every overlap the rescue kernels let through provisionally (k_verify.h,
// "partial charge").  Nothing here waits for the GPU; the counters are read when the chunk ends.
static int charge_stage(fsv_ctx *ctx, AsmWs &W, const Round &R)
{
    const fsv_asm_params &P = R.P; const Batch &B = R.B;
    const uint32_t ext_cap = 2u * R.task_cap;      // (task_cap < 2^31: begin_round)
    ChargeState &S = W.ch;
    TRY(ensure_each(ctx, ext_cap, S.ext_tasks, S.ext_res, S.ext_list));
    TRY(ensure(ctx, S.list, (size_t)B.n_pairs + 4));
    TRY(ensure(ctx, S.n, 2));
    TRY(zero(ctx, S.n, 2));
    ChargeArgs A;
    A.ovl = W.ovl.p; A.n_pairs = B.n_pairs; A.tasks = W.tasks.p; A.res = W.res.p; A.paths = W.paths.p; A.ovl_c = W.ovl_c.p;
    A.ext_tasks = S.ext_tasks.p; A.ext_res = S.ext_res.p; A.ext_list = S.ext_list.p; A.n_ext = S.n.p;
    A.ovl_list = S.list.p; A.n_ovl = S.n.p + 1; A.stats = S.ct.p;
    A.k_cap = P.k_cap; A.accept_err_pm = P.accept_err_pm;
    TRY(S.clock.mark(ctx));
    FSV_LAUNCH(ctx, ctx->stream, k_charge_tasks, dim3(fsv_grid_for(B.n_pairs, 64)), dim3(64), 0, A);
    TRY(launch_bpm_ext(ctx, R.store, S.ext_tasks.p, S.ext_list.p, S.n.p, ext_cap, P.k_cap, S.ext_res.p, S.ct.p + CH_EXT));
    FSV_LAUNCH(ctx, ctx->stream, k_charge_accept, dim3(fsv_grid_for(B.n_pairs, 64)), dim3(64), 0, A);
    TRY(S.clock.mark(ctx));
    return FSV_OK;
}

// K5 on the window tasks, the rescue of unmatched windows and the verdict on every overlap, then K6 on the same tasks
static int verify_stage(fsv_ctx *ctx, AsmWs &W, const Round &R)
{
    const fsv_asm_params &P = R.P; const Batch &B = R.B;
    uint32_t *ct = R.ct;
    unsigned long long *cols = (unsigned long long *)(ct + CT_COLS_LO);   // a 64-bit sum in two counter words
    Span tv(ctx, W.kt, ST_VERIFY);
    W.kt.begin(ctx, PASS_WINDOWS, KN_BPM, 0);
    TRY(fsv_bpm_windows_dev_n(ctx, R.store, W.tasks.p, R.task_cap, ct + CT_TASKS, W.res.p, P.k_cap));
    W.kt.end(ctx);
    W.kt.begin(ctx, PASS_WINDOWS, KN_RESCUE, (uint64_t)B.n_pairs * sizeof(fsv_ovl) * 2);
    if (R.wide_bands)
        FSV_LAUNCH(ctx, ctx->stream, k_rescue_accept<true>, dim3(fsv_grid_for(B.n_pairs, 64)), dim3(64), 0, R.store, W.ovl.p, B.n_pairs, W.tasks.p, W.res.p, cols,
                   W.ovl_c.p, P.k_cap, P.accept_err_pm, (uint32_t *)nullptr, (uint32_t *)nullptr);
    else {
        // the right-extension pass and the verdict in one kernel; an overlap with an unmatched window LEFT of a matched one is set
        // aside for the left-extension pass (k_left_rescue: it needs the matched window's path first), which then gives its verdict
        TRY(ensure(ctx, W.left_list, (size_t)B.n_pairs + 4));
        const uint32_t gridl = std::min<uint32_t>(std::max(1u, B.n_pairs), 8u * (uint32_t)ctx->n_cu);
        if (!P.partial_charge) {
            FSV_LAUNCH(ctx, ctx->stream, k_rescue_accept<false>, dim3(fsv_grid_for(B.n_pairs, 64)), dim3(64), 0, R.store, W.ovl.p, B.n_pairs, W.tasks.p, W.res.p, cols,
                       W.ovl_c.p, P.k_cap, P.accept_err_pm, W.left_list.p, ct + CT_LEFT);
            FSV_LAUNCH(ctx, ctx->stream, k_left_rescue<false>, dim3(gridl), dim3(64), 0, R.store, W.ovl.p, W.left_list.p, ct + CT_LEFT, W.tasks.p, W.res.p, W.paths.p,
                       W.ovl_c.p, P.k_cap, P.accept_err_pm);
        } else {
            // the same two kernels with the error-rate test deferred: charge_stage gives the verdict once K6 has run
            FSV_LAUNCH(ctx, ctx->stream, (k_rescue_accept<false, true>), dim3(fsv_grid_for(B.n_pairs, 64)), dim3(64), 0, R.store, W.ovl.p, B.n_pairs, W.tasks.p, W.res.p,
                       cols, W.ovl_c.p, P.k_cap, P.accept_err_pm, W.left_list.p, ct + CT_LEFT);
            FSV_LAUNCH(ctx, ctx->stream, k_left_rescue<true>, dim3(gridl), dim3(64), 0, R.store, W.ovl.p, W.left_list.p, ct + CT_LEFT, W.tasks.p, W.res.p, W.paths.p,
                       W.ovl_c.p, P.k_cap, P.accept_err_pm);
        }
    }
    W.kt.end(ctx);
    tv.stop();
    Span tp(ctx, W.kt, ST_PATH);
    TRY(path_stage(ctx, W, PathJob{R.store, W.tasks.p, W.res.p, W.paths.p, R.task_cap, R.ct + CT_TASKS, R.ct, PASS_WINDOWS, R.round, R.wide_bands, R.P.k_cap, false}));
    tp.stop();
    if (P.partial_charge) TRY(charge_stage(ctx, W, R));
    return FSV_OK;
}

// deep_sets = 1: the spill list of the round's windows and the event slabs of k_consensus_deep / k_bnd_consensus_deep, sized from what the
// host knows.  Events of one window or junction: an overlap votes with at most one path there (one window task per overlap and grid
// window, one junction task per overlap and junction).  A path holds at most FSV_PATH_CAP ops and an event is a maximal run of y-only
// ops, so two events of a path have an op of another kind between them: at most (FSV_PATH_CAP + 1) / 2 runs.  A window path can add one
// event in front of its first column (the junction vote).  So FSV_DEEP_EV_PER_OVL events per overlap, times the overlaps a read can have:
// the largest set's reads minus one.  Tally::add_event checks the bound all the same.  The grid is as many blocks as 256 MB of slabs
// allow, at most one per CU; the lists' lengths are on the device only, so the launches are unconditional.
#define FSV_DEEP_EV_PER_OVL ((FSV_PATH_CAP + 1) / 2 + 1)
static int deep_setup(fsv_ctx *ctx, AsmWs &W, Round &R)
{
    const Batch &B = R.B;
    uint32_t max_set = 1;
    for (uint32_t s = 0; s < B.n_sets; s++) max_set = std::max(max_set, B.set_start[s + 1] - B.set_start[s]);
    const uint64_t cap = (uint64_t)FSV_DEEP_EV_PER_OVL * (max_set - 1) + 64;
    if (cap >= EvSlab::NIL) return fsv_fail(ctx, FSV_EUNSUP, "deep_sets: a set too large for 31-bit event links");
    const uint64_t per_block = cap * 3 * sizeof(uint32_t);
    R.deep_grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>({(uint64_t)ctx->n_cu, (uint64_t)std::max(1u, R.n_gwin), (256ull << 20) / per_block}));
    TRY(ensure(ctx, W.deep_slab, (size_t)R.deep_grid * cap * 3));
    TRY(ensure(ctx, W.deep_list, (size_t)R.n_gwin * 2 + 2));      // k_consensus and k_consensus_redo list a window once each
    R.deep = DeepSlabs{W.deep_slab.p, (uint32_t)cap, R.ct + CT_DEEP_MAX};
    R.C.deep_list = W.deep_list.p; R.C.deep_n = R.ct + CT_DEEP_W; R.C.deep_cap = R.n_gwin * 2 + 2;
    return FSV_OK;
}

// room for the corrected windows, the per-window table, the consensus kernels' arguments (R.C), the reads whose overlaps changed
static int consensus_setup(fsv_ctx *ctx, AsmWs &W, Round &R)
{
    const fsv_asm_params &P = R.P; const Batch &B = R.B;
    const uint32_t n_gwin = R.n_gwin;
    TRY(ensure(ctx, W.cwin, (size_t)n_gwin * FSV_CW_STRIDE));
    TRY(ensure(ctx, W.cwin_len, n_gwin));
    TRY(ensure(ctx, W.new_len, B.n_reads));
    if (!B.n_pairs) TRY(zero(ctx, W.ovl_c, 1));
    TRY(ensure(ctx, W.gwin_tab, std::max(1u, n_gwin)));
    FSV_LAUNCH(ctx, ctx->stream, k_gwin_tab, dim3(fsv_grid_for(n_gwin, 256)), dim3(256), 0, W.gwin_read.p, W.gwin_off.p, W.read_set.p, W.set_start.p, W.pair_base.p, n_gwin,
               W.gwin_tab.p);
    ConsArgs &C = R.C;
    C.store = R.store; C.word_off = W.word_off.p; C.read_len = W.len.p;
    C.read_set = W.read_set.p; C.set_start = W.set_start.p; C.pair_base = W.pair_base.p;
    C.gwin_off = W.gwin_off.p; C.gwin_read = W.gwin_read.p; C.ovl_c = W.ovl_c.p;
    C.gwin_tab = W.gwin_tab.p; C.tasks = W.tasks.p;
    C.paths = W.paths.p; C.cwin = W.cwin.p; C.cwin_len = W.cwin_len.p; C.warn = W.warn.p;
    C.n_reads = B.n_reads;
    TRY(ensure(ctx, W.changed, B.n_reads));
    TRY(zero(ctx, W.changed, B.n_reads));
    C.changed = W.changed.p;
    C.read_dirty = nullptr;
    C.junction_vote = P.second_round ? 0 : 1;
    C.ins_dag = P.ins_dag ? 1 : 0;
    C.cov3 = nullptr;
    if (P.second_round && B.n_pairs) { TRY(ensure(ctx, W.cov3, std::max(1u, n_gwin))); C.cov3 = W.cov3.p; }
    if (B.n_pairs) {
        TRY(ensure(ctx, W.read_dirty, B.n_reads));
        FSV_LAUNCH(ctx, ctx->stream, k_read_dirty, dim3(B.n_reads), dim3(64), 0, W.ovl_c.p, W.paths.p, W.read_set.p, W.set_start.p, W.pair_base.p, B.n_reads, W.read_dirty.p);
        C.read_dirty = W.read_dirty.p;
    }
    C.deep_list = nullptr; C.deep_n = nullptr; C.deep_cap = 0;
    if (P.deep_sets && B.n_pairs) TRY(deep_setup(ctx, W, R));
    return FSV_OK;
}

// the haplotype partition's (K7) site records, vectors and window lists
static int partition_setup(fsv_ctx *ctx, AsmWs &W, const Round &R, SiteArgs &SA, SiteLists &SL)
{
    const Batch &B = R.B;
    const uint32_t n_gwin = R.n_gwin;
    const size_t vec_cap = (size_t)B.n_pairs * 64 + (1u << 20);
    TRY(ensure(ctx, W.site_cnt, std::max(1u, n_gwin)));
    const size_t rec_cap = (size_t)n_gwin * 4 + 65536;
    TRY(ensure(ctx, W.site_rec, rec_cap));
    TRY(ensure(ctx, W.site_off, std::max(1u, n_gwin)));
    TRY(ensure(ctx, W.site_vec, vec_cap));
    TRY(ensure(ctx, W.site_cursor, 4));
    TRY(ensure(ctx, W.redo, B.n_reads));
    TRY(ensure(ctx, W.site_lists, (size_t)std::max(1u, n_gwin) * 2));
    TRY(zero(ctx, W.site_cursor, 4));
    TRY(zero(ctx, W.redo, B.n_reads));
    SA.site_cnt = W.site_cnt.p; SA.site_rec = W.site_rec.p; SA.vec = W.site_vec.p;
    SA.site_off = W.site_off.p; SA.rec_cursor = W.site_cursor.p + 3; SA.rec_cap = (uint32_t)std::min<size_t>(rec_cap, 0xfffffff0u);
    SA.vec_cursor = W.site_cursor.p; SA.vec_cap = (uint32_t)std::min<size_t>(vec_cap, 0xfffffff0u);
    SA.read_sites = W.redo.p;
    SL.site_cnt = SA.site_cnt; SL.win_list = W.site_lists.p; SL.redo_list = SL.win_list + std::max(1u, n_gwin);
    SL.win_n = W.site_cursor.p + 1;
    return FSV_OK;
}

// calculate_boundary_cigars (Correct.cpp:2310): junction tasks -> K5 -> K6 -> which of the new cigars the partition uses
static int junction_cigars(fsv_ctx *ctx, AsmWs &W, const Round &R, SiteArgs &SA, SiteLists &SL)
{
    const fsv_asm_params &P = R.P;
    const uint32_t n_gwin = R.n_gwin, task_cap = R.task_cap;
    uint32_t *ct3 = W.ct_of(R.row(PASS_BCIG));
    TRY(ensure_each(ctx, task_cap, W.tasks2, W.res2, W.paths2, W.bc_idx, W.bc_rec));
    TRY(ensure(ctx, W.bc_win, (size_t)(n_gwin + 2) * 3));
    FSV_LAUNCH(ctx, ctx->stream, k_bcwin_init, dim3(fsv_grid_for(n_gwin + 2, 256)), dim3(256), 0, W.bc_win.p, n_gwin + 2);
    BcigArgs BA;
    BA.tasks = W.tasks.p; BA.paths = W.paths.p; BA.n_tasks = R.ct + CT_TASKS;
    BA.pair_read = W.pair_read.p; BA.read_dirty = W.read_dirty.p; BA.gwin_off = W.gwin_off.p;
    BA.thr_tab = W.thr_tab.p; BA.k_cap = P.k_cap;
    BA.tasks2 = W.tasks2.p; BA.bc_idx = W.bc_idx.p; BA.n_tasks2 = ct3 + CT_TASKS;
    BA.n_same = ct3 + CT_B_RETRY; BA.n_used = ct3 + CT_B_LIST;
    BA.res2 = W.res2.p; BA.paths2 = W.paths2.p; BA.bc_rec = W.bc_rec.p; BA.bc_win = W.bc_win.p;
    W.kt.begin(ctx, KN_PARTITION, 0);
    FSV_LAUNCH(ctx, ctx->stream, k_bcig_tasks, dim3((fsv_grid_for(task_cap, 256) + 7u) & ~7u), dim3(256), 0, BA);
    W.kt.end(ctx);
    W.kt.begin(ctx, PASS_BCIG, KN_BPM, 0);
    TRY(fsv_bpm_windows_dev_n(ctx, R.store, W.tasks2.p, task_cap, ct3 + CT_TASKS, W.res2.p, P.k_cap));
    W.kt.end(ctx);
    TRY(path_stage(ctx, W, PathJob{R.store, W.tasks2.p, W.res2.p, W.paths2.p, task_cap, ct3 + CT_TASKS, ct3, PASS_BCIG, R.round, R.wide_bands, P.k_cap, false}));
    W.kt.begin(ctx, KN_PARTITION, 0);
    FSV_LAUNCH(ctx, ctx->stream, k_bcig_accept, dim3(fsv_grid_for(task_cap, 256)), dim3(256), 0, BA);
    W.kt.end(ctx);
    SA.bc_idx = W.bc_idx.p; SA.bc_rec = W.bc_rec.p; SA.bc_paths = W.paths2.p;
    SL.bc_win = W.bc_win.p;
    return FSV_OK;
}

// consensus of every window; with the haplotype partition (K7) on, the windows that hold a candidate site are listed on the
// way, k_snp_sites / k_hap_partition take the overlaps with the other allele out (is_match 2 / 4: out of the consensus and,
// through that, out of what the final pass accepts as verified), and the reads that lost an overlap get their windows redone
static int consensus_stage(fsv_ctx *ctx, AsmWs &W, Round &R)
{
    const fsv_asm_params &P = R.P; const Batch &B = R.B;
    const uint32_t n_gwin = R.n_gwin;
    TRY(consensus_setup(ctx, W, R));
    const ConsArgs &C = R.C;
    const bool partition = B.n_pairs && P.partition;
    SiteArgs SA{};
    SiteLists SL{};
    if (partition) TRY(partition_setup(ctx, W, R, SA, SL));
    if (partition && P.junction_cigars) TRY(junction_cigars(ctx, W, R, SA, SL));
    const dim3 grid_w((n_gwin + 7u) & ~7u);
    W.kt.begin(ctx, PASS_WINDOWS, KN_CONSENSUS, (uint64_t)n_gwin * (96 + 448));
    if (R.wide_bands) {
        if (partition) FSV_LAUNCH(ctx, ctx->stream, (k_consensus<FSV_EV_CAP_WIDE, 1>), grid_w, dim3(64), 0, C, n_gwin, SL);
        else FSV_LAUNCH(ctx, ctx->stream, (k_consensus<FSV_EV_CAP_WIDE, 0>), grid_w, dim3(64), 0, C, n_gwin, SL);
    } else {
        if (partition) FSV_LAUNCH(ctx, ctx->stream, (k_consensus<FSV_EV_CAP, 1>), grid_w, dim3(64), 0, C, n_gwin, SL);
        else FSV_LAUNCH(ctx, ctx->stream, (k_consensus<FSV_EV_CAP, 0>), grid_w, dim3(64), 0, C, n_gwin, SL);
    }
    W.kt.end(ctx);
    if (partition) {
        const uint32_t grid_l = std::min<uint32_t>(std::max(1u, n_gwin), (uint32_t)ctx->n_cu * 16);
        W.kt.begin(ctx, KN_PARTITION, (uint64_t)B.n_reads * 4);
        FSV_LAUNCH(ctx, ctx->stream, k_snp_sites, dim3(grid_l), dim3(64), 0, C, SA, SL);
        FSV_LAUNCH(ctx, ctx->stream, k_hap_partition, dim3(B.n_reads), dim3(64), 0, C, SA, W.ovl.p, W.ovl_c.p, SL);
        if (R.wide_bands) FSV_LAUNCH(ctx, ctx->stream, k_consensus_redo<FSV_EV_CAP_WIDE>, dim3(grid_l), dim3(64), 0, C, SL);
        else FSV_LAUNCH(ctx, ctx->stream, k_consensus_redo<FSV_EV_CAP>, dim3(grid_l), dim3(64), 0, C, SL);
        W.kt.end(ctx);
    }
    if (C.deep_list) {      // the listed windows once more, from the partition's final accepted bits
        W.kt.begin(ctx, KN_CONS_DEEP, 0);
        FSV_LAUNCH(ctx, ctx->stream, k_consensus_deep, dim3(R.deep_grid), dim3(64), 0, C, SL, R.deep);
        W.kt.end(ctx);
    }
    return FSV_OK;
}

// new read lengths -> the round's one synchronisation (the round's counters ride along) -> the next geometry -> the corrected reads
// repacked into the other store
static int finish_round(fsv_ctx *ctx, AsmWs &W, Round &R)
{
    const fsv_asm_params &P = R.P; const Batch &B = R.B;
    const uint32_t n_gwin = R.n_gwin;
    TRY(ensure(ctx, W.lb, std::max(1u, n_gwin)));
    FSV_LAUNCH(ctx, ctx->stream, k_newlen, dim3(fsv_grid_for(B.n_reads, 256)), dim3(256), 0, W.gwin_off.p, W.cwin_len.p, B.n_reads, W.new_len.p, W.lb.p);
    std::vector<int32_t> nlen(B.n_reads);
    TRY(download(ctx, nlen.data(), W.new_len, B.n_reads));
    for (int pass = 0; pass < PASS_COUNT; pass++)
        FSV_HIP(ctx, hipMemcpyAsync(R.h_ct.data() + (size_t)R.row(pass) * CT_SLOT, W.ct_of(R.row(pass)), CT_SLOT * 4, hipMemcpyDeviceToHost, ctx->stream));
    FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (R.h_ct[(size_t)R.round * CT_SLOT + CT_OVERFLOW]) return fsv_fail(ctx, FSV_ECAP, "internal window task buffer overflow");
    Geometry G2;
    TRY(make_geometry(ctx, B, nlen, G2, P.w, &R.mz_fixed));
    Dev<uint32_t> &dst = W.store[R.round & 1];
    const uint32_t total_words = G2.word_off[B.n_reads];
    TRY(ensure(ctx, dst, (size_t)total_words + 8));
    // k_repack needs the new offsets while the old ones are still in use: they go up in a buffer of their own
    TRY(upload(ctx, W.unpack_off, G2.word_off));
    W.kt.begin(ctx, KN_REPACK, (uint64_t)n_gwin * 384 + (uint64_t)total_words * 4);
    FSV_LAUNCH(ctx, ctx->stream, k_repack, dim3(B.n_reads), dim3(256), 0, W.gwin_off.p, W.lb.p, W.cwin.p, W.unpack_off.p, W.new_len.p, B.n_reads,
               R.round + 1 < P.n_rounds ? 1 : 0, dst.p);
    W.kt.end(ctx);
    FSV_HIP(ctx, hipMemsetAsync(dst.p + total_words, 0, 32, ctx->stream));
    R.store = dst.p;
    R.len = nlen;
    for (int32_t l : R.len) if (l >= 65536) R.short_reads = false;
    R.G = G2;
    return FSV_OK;
}

// What the final pass hands from the hit gather to the layout, the contigs and the statistics
struct SetLayout { std::vector<std::vector<Piece>> contigs; bool fallback = false; };
struct Final {
    std::vector<uint32_t> hit_first, hwarn, h_setcols;   // hits of set s: [hit_first[s], hit_first[s + 1]); per-read warnings; K5 columns per set
    const fsv_hit *hraw = nullptr;                        // the hits, grouped by set (pinned host memory)
    bool any_inexact = false;                             // some set's layout compares bases: W.h_store holds its reads
    std::vector<SetLayout> lay;
    uint64_t used = 0;                                    // contig bases written
    Trace trace;                                          // FSV_TRACE: the final pass, step by step
};

// the final pass's geometry on the device; its counter row
static int begin_final(fsv_ctx *ctx, AsmWs &W, Round &R)
{
    R.ct = W.ct_of(R.P.n_rounds); R.task_cap = 0;      // (the final pass emits no window tasks)
    TRY(upload(ctx, W.word_off, R.G.word_off));
    TRY(upload(ctx, W.len, R.len));
    TRY(upload(ctx, W.mz_off, R.G.mz_off));
    TRY(ensure(ctx, W.tasks, 2));
    return FSV_OK;
}

// the gapped re-chain of the unordered pairs listed in W.inexact_list (*n_list_dev of them, a count on the device), after the final
// pass's overlap_stage: both slots of a listed pair are overwritten, the other slots stay
static int rechain_listed(fsv_ctx *ctx, AsmWs &W, const Round &R, const uint32_t *n_list_dev)
{
    const fsv_asm_params &P = R.P; const Batch &B = R.B;
    ChainArgs A2 = W.last_chain;
    A2.bw = P.bw_rechain; A2.emit_tasks = 0; A2.pair_list = W.inexact_list.p; A2.n_list_dev = n_list_dev;
    // Either direction of a listed pair is chained from its own side, as hifiasm does: with an indel budget the chain DP depends
    // on the end it starts from (the budget is a rate over the span chained so far; on the reverse strand the two sides start
    // from opposite ends), and the mirror image of one side's chain can be off by the bases of an indel near a read end.
    A2.primary_only = 1;
    TRY(ensure(ctx, W.upair_tab_sw, std::max(1u, B.n_upairs)));
    FSV_LAUNCH(ctx, ctx->stream, k_pair_tab_swap, dim3(fsv_grid_for(B.n_upairs, 256)), dim3(256), 0, W.upair_tab.p, B.n_upairs, W.upair_tab_sw.p);
    // timed like the other k_chain launches (a profiler counts it too)
    for (int side = 0; side < 2; side++) {
        const size_t tk = W.kt.begin(ctx, KN_CHAIN, 0);
        if (side == 1) A2.upair_tab = W.upair_tab_sw.p;
        if (A2.wide_list) FSV_HIP(ctx, hipMemsetAsync(A2.n_wide, 0, 4, ctx->stream));   // (the final pass's own wide pairs are done)
        if (A2.spill_list) FSV_HIP(ctx, hipMemsetAsync(A2.n_spill, 0, 4, ctx->stream)); // (and its spilled ones, and the other side's)
        TRY(launch_chain(ctx, CHAIN_PAIRS, R.short_reads, B.n_upairs, A2, B.n_upairs));
        if (A2.wide_list) TRY(chain_wide_pairs(ctx, A2, R.short_reads, B.n_upairs));
        W.kt.end(ctx, tk);
        TRY(chain_spilled_pairs(ctx, W, A2, B.n_upairs, longest_slot(R.G, B.n_reads), R.ct));
    }
    return FSV_OK;
}

// final overlaps on the corrected reads: the exact ones (k_exact), and the inexact ones the last correction round had verified
static int final_overlaps(fsv_ctx *ctx, AsmWs &W, Round &R, Final &F)
{
    const fsv_asm_params &P = R.P; const Batch &B = R.B;
    TRY(begin_final(ctx, W, R));
    // what the last correction round verified (coordinates on the reads as they were before that round) -- the final pass
    // accepts inexact overlaps against it; the slots are about to be overwritten
    const bool have_prev = P.n_rounds > 0 && B.n_pairs > 0;
    if (have_prev) {
        TRY(ensure(ctx, W.ovl_prev, B.n_pairs));
        FSV_HIP(ctx, hipMemcpyAsync(W.ovl_prev.p, W.ovl.p, (size_t)B.n_pairs * sizeof(fsv_ovl), hipMemcpyDeviceToDevice, ctx->stream));
    }
    TRY(overlap_stage(ctx, W, R, true));
    F.trace("overlaps");
    if (!B.n_pairs) return FSV_OK;
    TRY(ensure(ctx, W.hits, B.n_pairs));
    TRY(ensure(ctx, W.set_hits, (size_t)2 * B.n_sets + 2));
    TRY(zero(ctx, W.set_hits, B.n_sets));
    W.kt.begin(ctx, KN_EXACT, (uint64_t)B.n_pairs * sizeof(fsv_ovl));
    TRY(ensure(ctx, W.exact_flag, (size_t)B.n_upairs + 16));
    FSV_LAUNCH(ctx, ctx->stream, k_exact, dim3(B.n_upairs), dim3(64), 0, R.store, W.word_off.p, W.len.p, W.read_set.p, W.pair_base.p, W.upair_tab.p, W.ovl.p,
               W.hits.p, W.set_hits.p, W.exact_flag.p);
    W.kt.end(ctx);
    if (!have_prev) return FSV_OK;
    // pairs without an exact overlap that the last correction round had verified: gapped re-chain, accept per direction.
    // The list's length stays on the device: the re-chain is launched over every pair slot and the blocks beyond the list
    // return at once (a few hundred pairs are listed out of hundreds of thousands; the empty blocks cost ~40 us)
    TRY(ensure(ctx, W.inexact_list, (size_t)B.n_upairs + 4));
    uint32_t *n_list_dev = R.ct + CT_INEXACT;
    FSV_LAUNCH(ctx, ctx->stream, k_inexact_list, dim3(fsv_grid_for(B.n_upairs, 256)), dim3(256), 0, W.upair_tab.p, W.exact_flag.p, W.ovl_prev.p, B.n_upairs,
               W.inexact_list.p, n_list_dev);
    TRY(rechain_listed(ctx, W, R, n_list_dev));
    FSV_LAUNCH(ctx, ctx->stream, k_accept_inexact, dim3(fsv_grid_for(2ull * B.n_upairs, 256)), dim3(256), 0, W.upair_tab.p, W.inexact_list.p, 0u, W.ovl.p, W.ovl_prev.p,
               W.read_set.p, W.pair_base.p, W.hits.p, W.set_hits.p, n_list_dev);
    return FSV_OK;
}

// per-set counts -> offsets; the segments are packed on the device and come back in one copy, already grouped by set.
// The order inside a set depends on atomics and does not matter: the layout's containment marks and "longest arc,
// smallest target on ties" choices are order-independent.  The warnings and the batch's counters ride along.
static int gather_hits(fsv_ctx *ctx, AsmWs &W, Round &R, Final &F)
{
    const Batch &B = R.B;
    F.hit_first.assign(B.n_sets + 1, 0);
    F.hwarn.resize(B.n_reads); F.h_setcols.assign(B.n_reads, 0u);
    if (B.n_pairs) TRY(download(ctx, F.hit_first.data() + 1, W.set_hits, B.n_sets));
    TRY(download(ctx, F.hwarn.data(), W.warn, B.n_reads));
    TRY(download(ctx, F.h_setcols.data(), W.set_cols, B.n_reads));
    FSV_HIP(ctx, hipMemcpyAsync(R.h_ct.data() + (size_t)R.P.n_rounds * CT_SLOT, R.ct, CT_SLOT * 4, hipMemcpyDeviceToHost, ctx->stream));
    FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (B.n_pairs) {
        std::vector<uint32_t> &hit_first = F.hit_first;
        for (uint32_t s = 0; s < B.n_sets; s++) hit_first[s + 1] += hit_first[s];
        const uint32_t nh = hit_first[B.n_sets];
        if ((size_t)nh * sizeof(fsv_hit) > W.h_pin_cap) {
            if (W.h_pin) FSV_HIP(ctx, hipHostFree(W.h_pin));
            W.h_pin = nullptr; W.h_pin_cap = (size_t)nh * sizeof(fsv_hit) * 5 / 4 + 4096;
            FSV_HIP(ctx, hipHostMalloc(&W.h_pin, W.h_pin_cap, hipHostMallocDefault));
        }
        F.hraw = (const fsv_hit *)W.h_pin;
        if (nh) {
            uint32_t *first_dev = W.set_hits.p + B.n_sets;   // the offsets go behind the counts
            TRY(ensure(ctx, W.hits_packed, nh));
            FSV_HIP(ctx, hipMemcpyAsync(first_dev, hit_first.data(), (size_t)(B.n_sets + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
            FSV_LAUNCH(ctx, ctx->stream, k_hits_compact, dim3(B.n_sets), dim3(256), 0, W.hits.p, W.pair_base.p, first_dev, W.hits_packed.p);
            TRY(download(ctx, (fsv_hit *)W.h_pin, W.hits_packed, nh));
            FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
        }
        W.stats.n_exact_overlaps = nh;
    }
    F.trace("exact+gather");
    return FSV_OK;
}

// layout per set on the host.  The sets are independent: they are laid out on a few host threads
static int layout_sets(fsv_ctx *ctx, AsmWs &W, const Round &R, Final &F)
{
    const fsv_asm_params &P = R.P; const Batch &B = R.B; const Geometry &G = R.G;
    const std::vector<int32_t> &len = R.len;
    const std::vector<uint32_t> &hit_first = F.hit_first;
    const fsv_hit *hraw = F.hraw;
    // the unitig polishing compares reads base for base where they are joined by an inexact overlap (low coverage only): the
    // corrected reads then come to the host too, 2 bits a base (24 MB for 256 regions)
    // (only the reads of the sets that hold an inexact overlap: a handful of sets, ~200 KB each.  Since the correction rounds keep
    // overlaps of any length a 256-region batch nearly always has one somewhere, and the whole store -- 96 MB into a freshly
    // zero-filled vector -- cost 17 ms a step)
    std::vector<uint32_t> &h_store = W.h_store;
    bool any_inexact = false;
    if (P.graph_layout && hraw) {
        for (uint32_t s2 = 0; s2 < B.n_sets; s2++) {
            bool inexact = false;
            for (uint32_t i = hit_first[s2]; i < hit_first[s2 + 1] && !inexact; i++) inexact = !(hraw[i].slot >> 31);
            if (!inexact) continue;
            if (!any_inexact && h_store.size() < (size_t)G.word_off[B.n_reads] + 1) h_store.resize((size_t)G.word_off[B.n_reads] + 1);
            any_inexact = true;
            const uint32_t w0 = G.word_off[B.set_start[s2]], w1 = G.word_off[B.set_start[s2 + 1]];
            if (w1 > w0) FSV_HIP(ctx, hipMemcpyAsync(h_store.data() + w0, R.store + w0, (size_t)(w1 - w0) * 4, hipMemcpyDeviceToHost, ctx->stream));
        }
        if (any_inexact) FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    F.any_inexact = any_inexact;
    const uint8_t *set_flags = R.set_flags;
    std::vector<SetLayout> &lay = F.lay;
    lay.resize(B.n_sets);
    const uint32_t nthr = std::max(1u, std::min({8u, std::thread::hardware_concurrency(), B.n_sets / 16 + 1}));
    std::atomic<uint32_t> next{0};
    // a worker never lets an exception out (it would end the process): the first failure is kept and returned after the join
    std::atomic<int> rc_work{FSV_OK};
    auto work = [&]() {
        try {
        for (uint32_t s = next.fetch_add(1); s < B.n_sets && rc_work.load() == FSV_OK; s = next.fetch_add(1)) {
            const uint32_t r0 = B.set_start[s], ns = B.set_start[s + 1] - r0;
            if (ns == 0) continue;
            if (R.is_low(s)) { lay[s].fallback = true; continue; }   // no contig, whatever min_contig_reads is
            const uint32_t nh_s = hit_first[s + 1] - hit_first[s];
            const bool unphased = set_flags && (set_flags[R.caller_set[s]] & FSV_SET_UNPHASED);
            if (P.graph_layout && !unphased) {
                // the layout as hifiasm makes it (layout.h)
                fsv_layout::ReadBases rb; rb.words = any_inexact ? h_store.data() : nullptr; rb.word_off = G.word_off.data() + r0; rb.len = len.data() + r0;
                fsv_layout::Graph g(len.data() + r0, (int)ns, rb);
                std::vector<fsv_layout::Hit> hs(nh_s);
                for (uint32_t i = 0; i < nh_s; i++) {
                    const fsv_hit &h = hraw[hit_first[s] + i];
                    const int tl = len[r0 + h.t];
                    fsv_layout::Hit &x = hs[i];
                    x.qn = (int32_t)h.q; x.tn = (int32_t)h.t; x.qs = h.x_s; x.qe = h.x_e + 1; x.rev = (uint8_t)h.rev; x.el = (uint8_t)(h.slot >> 31); x.del = 0;
                    if (h.rev) { x.ts = tl - h.y_e - 1; x.te = tl - h.y_s; } else { x.ts = h.y_s; x.te = h.y_e + 1; }
                }
                g.set_hits(std::move(hs));
                g.build();
                std::vector<std::vector<fsv_layout::PieceOut>> cs;
                g.unitigs(P.min_contig_reads, cs);
                for (auto &c : cs) { std::vector<Piece> pc; for (auto &e : c) pc.push_back(Piece{e.read, e.rev, e.len}); lay[s].contigs.push_back(std::move(pc)); }
                lay[s].fallback = cs.empty();
                continue;
            }
            layout_set(len.data() + r0, ns, hraw + hit_first[s], nh_s, P.min_contig_reads, lay[s].contigs, lay[s].fallback);
        }
        } catch (const std::bad_alloc &) { int ok = FSV_OK; rc_work.compare_exchange_strong(ok, FSV_ENOMEM); }
        catch (...) { int ok = FSV_OK; rc_work.compare_exchange_strong(ok, FSV_EINTERNAL); }
    };
    // joined on every way out of this scope, an exception from emplace_back (a thread that cannot start) included: no joinable
    // std::thread is ever destroyed
    struct Joiner { std::vector<std::thread> thr; ~Joiner() { for (auto &t : thr) if (t.joinable()) t.join(); } };
    {
        Joiner j;
        j.thr.reserve(nthr);
        for (uint32_t t = 1; t < nthr; t++) j.thr.emplace_back(work);
        work();
    }
    if (rc_work.load() != FSV_OK) return fsv_fail(ctx, rc_work.load(), rc_work.load() == FSV_ENOMEM ? "out of host memory (layout)" : "exception in the layout of a read set");
    return FSV_OK;
}

// the contigs in set order: their pieces, stitched on the device (k_stitch) and copied back; the sets' status words
static int emit_contigs(fsv_ctx *ctx, AsmWs &W, const Round &R, Final &F, fsv_contigs *out)
{
    const Batch &B = R.B;
    std::vector<fsv_piece> pieces;
    uint64_t used = 0;
    uint32_t nc = 0;
    int rc_out = FSV_OK;
    for (uint32_t s = 0; s < B.n_sets && rc_out == FSV_OK; s++) {
        const uint32_t r0 = B.set_start[s], ns = B.set_start[s + 1] - r0;
        int32_t st = 0;
        for (uint32_t r = r0; r < r0 + ns; r++) st |= (int32_t)(F.hwarn[r] & (FSV_W_MZ_TRUNC | FSV_W_ANCHOR_TRUNC | FSV_W_INS_EVENTS | FSV_W_WINDOW_KEPT | FSV_W_INTERNAL | FSV_W_SITES));
        const uint32_t cs = R.caller_set[s];      // (the status words were zeroed when the chunk began)
        if (ns == 0) { out->set_status[cs] |= st; continue; }
        if (F.lay[s].fallback) st |= FSV_W_NO_LAYOUT;
        for (auto &c : F.lay[s].contigs) {
            uint64_t clen = 0;
            for (auto &pc : c) clen += pc.len;
            if (nc >= out->contig_cap || used + clen > out->seq_cap) { rc_out = fsv_fail(ctx, FSV_ECAP, "contig output buffers too small (use fsv_assemble_batch_bound)"); break; }
            for (auto &pc : c) { pieces.push_back(fsv_piece{r0 + pc.read, pc.rev, pc.len, 0u, used}); used += pc.len; }
            out->set[nc] = cs; out->n_reads[nc] = (uint32_t)c.size();
            out->off[++nc] = used;
        }
        out->set_status[cs] |= st;
    }
    F.trace("layout");
    if (rc_out != FSV_OK) return rc_out;
    out->n_contigs = nc;
    ctx->last_contigs_dev = nullptr;
    ctx->last_contig_off.assign(out->off, out->off + nc + 1);
    if (!pieces.empty()) {
        TRY(upload(ctx, W.pieces, pieces));
        TRY(ensure(ctx, W.contig_out, used + 16));
        W.kt.begin(ctx, KN_STITCH, used + used / 4);    // 2-bit bases in, ASCII out
        FSV_LAUNCH(ctx, ctx->stream, k_stitch, dim3((uint32_t)pieces.size()), dim3(256), 0, R.store, W.word_off.p, W.len.p, W.pieces.p, W.contig_out.p);
        W.kt.end(ctx);
        ctx->last_contigs_dev = W.contig_out.p;
        TRY(download(ctx, out->seq, W.contig_out, used));
        FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    F.trace("stitch+d2h");
    F.used = used;
    return FSV_OK;
}

// statistics out of the counter rows (Round::row), and the byte counts of the launches that had to wait for them
static void fill_stats(AsmWs &W, const Round &R, const Final &F)
{
    const fsv_asm_params &P = R.P; const Batch &B = R.B;
    const std::vector<uint32_t> &h_ct = R.h_ct;
    KTimes &kt = W.kt;
    auto set = [&](int pass, int k, size_t round, uint64_t bytes) { if (uint64_t *b = kt.bytes_of(pass, k, round)) *b = bytes; };
    auto add = [&](int pass, int k, size_t round, uint64_t bytes) { if (uint64_t *b = kt.bytes_of(pass, k, round)) *b += bytes; };
    auto n_dp_of = [](const uint32_t *c) { return (uint64_t)c[CT_DP_SB] + c[CT_DP_SB16] + c[CT_DP] + c[CT_DP_FR3] + c[CT_DP_GEN] + c[CT_DP_WIDE] + c[CT_DP_XW]; };
    uint64_t mz_total[17] = {0}, n_windows2 = 0;
    for (int sl = 0; sl <= P.n_rounds; sl++) {
        const uint32_t *c = h_ct.data() + (size_t)sl * CT_SLOT;
        mz_total[sl] = (uint64_t)c[CT_MZ_LO] | (uint64_t)c[CT_MZ_HI] << 32;
        W.n_long_reads += c[CT_UQ_LONG]; W.n_spilled_pairs += c[CT_SPILLED];
        W.n_deep_windows += c[CT_DEEP_W]; W.n_deep_junctions += c[CT_DEEP_B]; W.deep_max_events = std::max(W.deep_max_events, c[CT_DEEP_MAX]);
        if (sl == P.n_rounds) { W.stats.n_inexact_candidates = c[CT_INEXACT]; break; }
        W.stats.n_windows += c[CT_TASKS];
        W.stats.dp_columns += (uint64_t)c[CT_COLS_LO] | (uint64_t)c[CT_COLS_HI] << 32;      // rescue re-runs (k_rescue_accept)
        W.stats.n_path_dp += n_dp_of(c);
        W.stats.n_path_fr += (uint64_t)c[CT_DP_SB16] + c[CT_DP] + c[CT_DP_FR3];
        // algorithmic bytes of the round's launches, now that the counts are known: a window task is
        // 94 + 102 B of 2-bit operands + 16 B of result; a K6 window leaves a 128 B path record instead;
        // k_chain reads every unique-minimizer list once (two sorted copies, 16 B entries) and writes the overlap slots and
        // the 32 B task records; the consensus reads the path records and writes its corrected windows
        const uint64_t nt = c[CT_TASKS], n_dp = n_dp_of(c);
        set(PASS_WINDOWS, KN_BPM, sl, nt * 212ull);
        add(PASS_WINDOWS, KN_RESCUE, sl, nt * 16ull);
        set(PASS_WINDOWS, KN_PATH_FAST, sl, nt * (16ull + 196ull) + (nt - n_dp) * 128ull);
        set(PASS_WINDOWS, KN_PATH_DP, sl, n_dp * (196ull + 128ull));
        add(PASS_WINDOWS, KN_CONSENSUS, sl, nt * 128ull);
        if (kt.bytes_of(PASS_BCIG, KN_BPM, sl)) {      // the junction cigars of the round's partition: window tasks like the others
            const uint32_t *c3 = h_ct.data() + (size_t)(PASS_BCIG * (P.n_rounds + 1) + sl) * CT_SLOT;
            const uint64_t n3 = c3[CT_TASKS], n_dp3 = n_dp_of(c3);
            n_windows2 += n3;
            W.stats.n_junction_cigars += n3;
            W.stats.n_junction_used += c3[CT_B_LIST];
            if (getenv("FSV_BCIG_DEBUG")) fprintf(stderr, "[fsv] round %d: %u overlaps set aside for the left-extension pass; fix_boundary: %u candidates, %u windows moved\n", sl, c[CT_LEFT], c[CT_FIX], c[CT_FIXED]);
            if (getenv("FSV_BCIG_DEBUG")) fprintf(stderr, "[fsv] round %d: %llu junction cigars, %u accepted but showing what the window cigars show, %u used\n", sl, (unsigned long long)n3, c3[CT_B_RETRY], c3[CT_B_LIST]);
            set(PASS_BCIG, KN_BPM, sl, n3 * 212ull);
            set(PASS_BCIG, KN_PATH_FAST, sl, n3 * (16ull + 196ull) + (n3 - n_dp3) * 128ull);
            set(PASS_BCIG, KN_PATH_DP, sl, n_dp3 * (196ull + 128ull));
        }
        // the round's second consensus pass: the junction tasks are window tasks like the first pass's; k_bnd_tasks reads every
        // first-pass task and path record and writes the junction tasks; the junctions' consensus reads their path records and
        // writes a patch per junction
        if (kt.bytes_of(PASS_JUNCTIONS, KN_BND, sl)) {
            const uint32_t *c2 = h_ct.data() + (size_t)(PASS_JUNCTIONS * (P.n_rounds + 1) + sl) * CT_SLOT;
            const uint64_t n2 = c2[CT_TASKS], n3 = c2[CT_B_RETRY], n_dp2 = n_dp_of(c2);
            n_windows2 += n2 + n3;
            set(PASS_JUNCTIONS, KN_BND, sl, nt * (sizeof(fsv_wtask) + 128ull) + n2 * sizeof(fsv_wtask));
            set(PASS_JUNCTIONS, KN_BPM, sl, (n2 + n3) * 212ull);
            set(PASS_JUNCTIONS, KN_PATH_FAST, sl, n2 * (16ull + 196ull) + (n2 - n_dp2) * 128ull);
            set(PASS_JUNCTIONS, KN_PATH_DP, sl, n_dp2 * (196ull + 128ull));
            set(PASS_JUNCTIONS, KN_BND_CONS, sl, n2 * 128ull + (uint64_t)c2[CT_B_LIST] * (sizeof(BndPatch) + 2ull * FSV_BND_HALF));
        }
    }
    // the sketch reads the packed bases of the reads it sketches and writes 16 B per minimizer it produces ("len/4
    // in + 16 B / minimizer out"); k_uniq reads those and writes the unique ones twice (sorted by hash, sorted by position).
    // Round 2 charged 16 B per slot of CAPACITY (one per base) -- seven times what the counters saw.
    // (overlap_stage runs once per round and once more for the final pass: its record i belongs to counter row i)
    for (size_t i = 0; i <= (size_t)P.n_rounds; i++) {
        const uint32_t *c = h_ct.data() + i * CT_SLOT;
        const uint64_t raw = (uint64_t)c[CT_MZRAW_LO] | (uint64_t)c[CT_MZRAW_HI] << 32, bases = (uint64_t)c[CT_BASES_LO] | (uint64_t)c[CT_BASES_HI] << 32;
        set(PASS_WINDOWS, KN_SKETCH, i, bases / 4 + raw * sizeof(fsv_mz));
        set(PASS_WINDOWS, KN_UNIQ, i, raw * sizeof(fsv_mz) + mz_total[i] * 2 * sizeof(fsv_mz));
        set(PASS_WINDOWS, KN_CHAIN, i, mz_total[i] * 32ull + (uint64_t)B.n_pairs * sizeof(fsv_ovl) + (i < (size_t)P.n_rounds ? (uint64_t)c[CT_TASKS] * sizeof(fsv_wtask) : 0ull));
    }
    for (uint32_t s2 = 0; s2 < B.n_sets; s2++) if (B.set_start[s2] < B.n_reads && B.set_start[s2 + 1] > B.set_start[s2]) W.stats.dp_columns += F.h_setcols[B.set_start[s2]];   // K5 windows
    // algorithmic bytes: 2-bit operands + result of every DP task, reads in once per pass, contigs out
    W.stats.algo_bytes = (W.stats.n_windows + n_windows2) * 212ull + R.reads_in_bytes * (uint64_t)(P.n_rounds + 1) + F.used;
    W.stats.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - R.t_enter).count();
    // resolve the per-kernel event timings
    W.stats.n_kernels = KN_COUNT;
    for (int k = 0; k < KN_COUNT; k++) { memset(&W.stats.kernels[k], 0, sizeof(fsv_kernel_stat)); strncpy(W.stats.kernels[k].name, kn_names[k], 23); }
    for (auto &r : kt.recs) {
        float ms = 0;
        const bool ok = hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess;
        if (r.k >= KN_COUNT) {   // a stage
            double *dst = r.k == ST_SKETCH ? &W.stats.ms_sketch : r.k == ST_CHAIN ? &W.stats.ms_chain : r.k == ST_VERIFY ? &W.stats.ms_verify
                        : r.k == ST_PATH ? &W.stats.ms_path : r.k == ST_CONSENSUS ? &W.stats.ms_consensus : &W.stats.ms_final;
            if (ok) *dst += ms;
            continue;
        }
        if (ok) W.stats.kernels[r.k].ms += ms;
        W.stats.kernels[r.k].launches++;
        W.stats.kernels[r.k].algo_bytes += r.bytes;
    }
}

// a chunk's statistics join those of the chunks before it (the junction-cigar counts of fsv_asm_stats are a single chunk's: never summed)
static void add_stats(fsv_asm_stats &total, const fsv_asm_stats &st)
{
    total.n_pairs += st.n_pairs; total.n_overlaps += st.n_overlaps; total.n_windows += st.n_windows; total.n_windows_matched += st.n_windows_matched;
    total.n_paths += st.n_paths; total.n_path_dp += st.n_path_dp; total.dp_columns += st.dp_columns; total.algo_bytes += st.algo_bytes;
    total.n_exact_overlaps += st.n_exact_overlaps; total.n_inexact_candidates += st.n_inexact_candidates; total.n_path_fr += st.n_path_fr;
    total.ms_sketch += st.ms_sketch; total.ms_chain += st.ms_chain; total.ms_verify += st.ms_verify; total.ms_path += st.ms_path;
    total.ms_consensus += st.ms_consensus; total.ms_final += st.ms_final; total.ms_total += st.ms_total;
    total.n_kernels = st.n_kernels;
    for (uint32_t k = 0; k < st.n_kernels; k++) {
        memcpy(total.kernels[k].name, st.kernels[k].name, sizeof(st.kernels[k].name));
        total.kernels[k].ms += st.kernels[k].ms; total.kernels[k].launches += st.kernels[k].launches; total.kernels[k].algo_bytes += st.kernels[k].algo_bytes;
    }
}

// ---- the caller's read sets: checked once per entry point, staged once for a sketch-only job ------------------------------------------
// the pointers an entry needs (without them it returns FSV_EINVAL and no message)
static bool readsets_present(const fsv_readsets *sets, bool with_sets)
{
    return sets && sets->store_dev && sets->word_off && sets->read_len && (!with_sets || sets->set_start);
}

// The values of the caller's read sets, before anything is launched.  RS_SETS: set_start spans [0, n_reads] and is monotone; RS_LEN: every
// read length in [1, 2^24); RS_WORD_OFF: every word offset below 2^32 (the kernels take 32-bit ones).  What runs behind an entry point
// (prepare_batch, kmer_stage, stage_sketch_reads) assumes all three.
enum { RS_SETS = 1, RS_LEN = 2, RS_WORD_OFF = 4, RS_ALL = RS_SETS | RS_LEN | RS_WORD_OFF };
static int check_readsets(fsv_ctx *ctx, const fsv_readsets *sets, unsigned what)
{
    const uint32_t n_reads = sets->n_reads, n_sets = sets->n_sets;
    if (what & RS_SETS) {
        if (n_sets == 0 ? n_reads != 0 : (sets->set_start[0] != 0 || sets->set_start[n_sets] != n_reads)) return fsv_fail(ctx, FSV_EINVAL, "set_start must span [0, n_reads]");
        for (uint32_t s = 0; s < n_sets; s++) if (sets->set_start[s + 1] < sets->set_start[s]) return fsv_fail(ctx, FSV_EINVAL, "set_start not monotone");
    }
    if (what & RS_LEN)
        for (uint32_t r = 0; r < n_reads; r++) if (sets->read_len[r] < 1 || sets->read_len[r] >= (1 << 24)) return fsv_fail(ctx, FSV_EUNSUP, "read length must be in [1, 2^24)");
    if ((what & RS_WORD_OFF) && n_reads)
        for (uint32_t r = 0; r <= n_reads; r++) if (sets->word_off[r] >= (1ull << 32)) return fsv_fail(ctx, FSV_EUNSUP, "store larger than 2^32 words; split the batch");
    return FSV_OK;
}

// the set of every read of the caller's sets
static std::vector<uint32_t> read_set_of(const fsv_readsets *sets)
{
    std::vector<uint32_t> read_set(sets->n_reads);
    for (uint32_t s = 0; s < sets->n_sets; s++) for (uint32_t r = sets->set_start[s]; r < sets->set_start[s + 1]; r++) read_set[r] = s;
    return read_set;
}

// The reads of a sketch-only job (fsv_sketch_reads, the k-mer stages) on the device: all of them as one set with its geometry at window w
// (G), read through the caller's word offsets; word_off, len, mz_off -- and read_set, when given -- uploaded, warn zeroed, room for mz and
// mz_cnt.  (lengths and word offsets in range: check_readsets)
static int stage_sketch_reads(fsv_ctx *ctx, AsmWs &W, const fsv_readsets *sets, int w, const std::vector<uint32_t> *read_set, Geometry &G, bool full_lists = false)
{
    const uint32_t n_reads = sets->n_reads;
    Batch B;
    B.n_reads = n_reads; B.n_sets = 1; B.set_start = {0u, n_reads};
    const std::vector<int32_t> len(sets->read_len, sets->read_len + n_reads);
    TRY(make_geometry(ctx, B, len, G, w, nullptr, full_lists));
    for (uint32_t r = 0; r <= n_reads; r++) G.word_off[r] = (uint32_t)sets->word_off[r];
    TRY(upload(ctx, W.word_off, G.word_off));
    TRY(upload(ctx, W.len, len));
    TRY(upload(ctx, W.mz_off, G.mz_off));
    if (read_set) TRY(upload(ctx, W.read_set, *read_set));
    TRY(ensure(ctx, W.warn, n_reads));
    TRY(zero(ctx, W.warn, n_reads));
    TRY(ensure(ctx, W.mz, G.mz_off[n_reads]));
    TRY(ensure(ctx, W.mz_cnt, n_reads));
    return FSV_OK;
}

// n elements of src (device) behind the `have` elements b holds, on the context's stream.  A buffer too small for them (and `slack` more)
// is replaced by one of twice what it must hold, min_elems at least, that keeps the contents: one synchronisation when it grows, none otherwise
template <class T> int append_on_device(fsv_ctx *ctx, Dev<T> &b, size_t have, const T *src, size_t n, size_t slack = 0, size_t min_elems = 0)
{
    if (!n) return FSV_OK;
    if (b.cap < (have + n + slack) * sizeof(T)) {
        Dev<T> bigger;
        TRY(ensure(ctx, bigger, std::max((have + n) * 2, min_elems)));
        if (have) FSV_HIP(ctx, hipMemcpyAsync(bigger.p, b.p, have * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream));
        FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
        b.swap(bigger);      // (the old allocation goes with `bigger`)
    }
    FSV_HIP(ctx, hipMemcpyAsync(b.p + have, src, n * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream));
    return FSV_OK;
}

// ---- the k-mer count table stage (k_kmer.h) --------------------------------------------------------------------------------------
// The stage on the caller's read sets: sketch at (w, k, hpc) into W.mz, count per set, histogram, verdict (host: the histograms are 16 KB
// a set), filter list.
struct KmerJob {
    const fsv_readsets *sets; int w, k, hpc;
    const SketchFilter *sketch_flt;   // (the index of hifiasm's ha_pt_gen) the sketch takes these filter sets, and no filter list is made of what it counts; or null
    double *ms;                       // the launches' HIP-event time is added here; or null
};
struct KmerResult {
    std::vector<fsv_kmer_set> sets;   // the verdicts
    std::vector<uint32_t> hist;       // n_sets x FSV_KMER_BINS
    std::vector<uint64_t> flt_off;    // set s's keys: [flt_off[s], flt_off[s + 1]) of the filter list the stage leaves in W.km.flt (unordered)
};
// what the stage's pieces hand on; the clock's spans lie between the host's read-backs
struct KmerRun {
    const KmerJob &J; KmerResult &R; EventClock clock;
    std::vector<uint64_t> entries, tab_off; std::vector<KmerTile> tiles; std::vector<int32_t> cutoff;
};

// the sketch, and the tables sized from what it emitted
static int kmer_sketch(fsv_ctx *ctx, AsmWs &W, KmerRun &K)
{
    const KmerJob &J = K.J; const fsv_readsets *sets = J.sets;
    const uint32_t n_reads = sets->n_reads, n_sets = sets->n_sets;
    K.entries.assign(n_sets, 0); K.tab_off.assign((size_t)n_sets + 1, 0);
    if (!n_reads) return FSV_OK;
    const std::vector<uint32_t> read_set = read_set_of(sets);
    Geometry G;
    TRY(stage_sketch_reads(ctx, W, sets, J.w, &read_set, G));
    TRY(K.clock.mark(ctx));
    TRY(launch_sketch(ctx, W, SketchJob{sets->store_dev, n_reads, G.word_off[n_reads], G.max_words, J.w, J.k, J.hpc, nullptr, J.w, false, nullptr,
                                     J.sketch_flt ? *J.sketch_flt : SketchFilter{}}));
    TRY(K.clock.mark(ctx));
    std::vector<uint32_t> cnt(n_reads);
    TRY(download(ctx, cnt.data(), W.mz_cnt, n_reads));
    FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (uint32_t r = 0; r < n_reads; r++) K.entries[read_set[r]] += std::min<uint32_t>(cnt[r], G.mz_off[r + 1] - G.mz_off[r]);
    for (uint32_t s = 0; s < n_sets; s++) {
        const uint64_t slots = kmer_table_slots(K.entries[s]), tile = std::min<uint64_t>(slots, FSV_KMER_TILE);
        K.tab_off[s + 1] = K.tab_off[s] + slots;
        for (uint64_t f = 0; f < slots; f += tile) K.tiles.push_back(KmerTile{s, (uint32_t)tile, f});
    }
    if (K.tiles.size() >= (1ull << 31)) return fsv_fail(ctx, FSV_EUNSUP, "k-mer tables too large for one pass; split the batch");
    return FSV_OK;
}

// the sets' tables filled, their histograms on the host
static int kmer_count(fsv_ctx *ctx, AsmWs &W, KmerRun &K)
{
    KmerTableState &S = W.km;
    const uint32_t n_reads = K.J.sets->n_reads, n_sets = K.J.sets->n_sets;
    const uint64_t total_slots = K.tab_off[n_sets];
    std::vector<uint32_t> &h_hist = K.R.hist;
    h_hist.assign((size_t)n_sets * FSV_KMER_BINS, 0u);
    TRY(ensure(ctx, S.err, 1));
    TRY(zero(ctx, S.err, 1));
    TRY(ensure(ctx, S.cursor, std::max(1u, n_sets)));
    TRY(zero(ctx, S.cursor, std::max(1u, n_sets)));
    TRY(upload(ctx, S.tab_off, K.tab_off));
    if (!total_slots) return FSV_OK;
    TRY(ensure(ctx, S.keys, total_slots));
    TRY(ensure(ctx, S.cnt, total_slots));
    TRY(ensure(ctx, S.hist, h_hist.size()));
    TRY(upload(ctx, S.tiles, K.tiles));
    TRY(K.clock.mark(ctx));
    FSV_HIP(ctx, hipMemsetAsync(S.keys.p, 0xff, total_slots * sizeof(unsigned long long), ctx->stream));   // every slot FSV_KMER_EMPTY
    TRY(zero(ctx, S.cnt, total_slots));
    TRY(zero(ctx, S.hist, h_hist.size()));
    FSV_LAUNCH(ctx, ctx->stream, k_kmer_insert, dim3(n_reads), dim3(256), 0, W.mz.p, W.mz_off.p, W.mz_cnt.p, W.read_set.p, S.tab_off.p, S.keys.p, S.cnt.p, n_reads, S.err.p);
    FSV_LAUNCH(ctx, ctx->stream, k_kmer_hist, dim3((uint32_t)K.tiles.size()), dim3(256), 0, S.tiles.p, S.tab_off.p, S.keys.p, S.cnt.p, S.hist.p);
    TRY(K.clock.mark(ctx));
    uint32_t err = 0;
    TRY(download(ctx, h_hist.data(), S.hist, h_hist.size()));
    TRY(download(ctx, &err, S.err, 1));
    FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (err) return fsv_fail(ctx, FSV_EINTERNAL, "k-mer count table: a set's table ran full");
    return FSV_OK;
}

// the verdict per set, and the filter segments the histogram promises
static void kmer_verdicts(KmerRun &K)
{
    const uint32_t n_sets = K.J.sets->n_sets;
    K.R.sets.resize(n_sets); K.cutoff.resize(n_sets); K.R.flt_off.assign((size_t)n_sets + 1, 0);
    std::vector<int64_t> h64(FSV_KMER_BINS);
    for (uint32_t s = 0; s < n_sets; s++) {
        const uint32_t *h = K.R.hist.data() + (size_t)s * FSV_KMER_BINS;
        fsv_kmer_set &o = K.R.sets[s];
        memset(&o, 0, sizeof(o));
        for (int c = 0; c < FSV_KMER_BINS; c++) { h64[c] = h[c]; o.n_distinct += h[c]; }
        o.peak_hom = fsv_kmer_peaks_hd(h64.data(), FSV_KMER_BINS, FSV_KMER_START, &o.peak_het, &o.low_i, &o.max_i);
        o.cutoff = K.cutoff[s] = fsv_kmer_cutoff(o.peak_hom);
        o.n_entries = K.entries[s];
        for (int c = 1; c < FSV_KMER_BINS; c++) if (c >= o.cutoff) o.n_filtered += h[c];
        for (int c = 2; c <= FSV_KMER_BINS - 2; c++) o.n_indexed += (uint64_t)c * h[c];
        K.R.flt_off[s + 1] = K.R.flt_off[s] + (K.J.sketch_flt ? 0 : o.n_filtered);
    }
}

// the filter list: every set's keys at or above its cutoff into its segment of W.km.flt; the stage's last wait for the stream either way
static int kmer_filter_list(fsv_ctx *ctx, AsmWs &W, KmerRun &K)
{
    KmerTableState &S = W.km;
    const uint32_t n_sets = K.J.sets->n_sets;
    const uint64_t n_flt = K.R.flt_off[n_sets];
    if (!n_flt) { FSV_HIP(ctx, hipStreamSynchronize(ctx->stream)); return FSV_OK; }
    std::vector<uint32_t> cursor(n_sets);
    TRY(ensure(ctx, S.flt, n_flt));
    TRY(upload(ctx, S.cutoff, K.cutoff));
    TRY(upload(ctx, S.flt_off, K.R.flt_off));
    TRY(K.clock.mark(ctx));
    FSV_LAUNCH(ctx, ctx->stream, k_kmer_filter, dim3((uint32_t)K.tiles.size()), dim3(256), 0, S.tiles.p, S.tab_off.p, S.keys.p, S.cnt.p, S.cutoff.p, S.flt_off.p, S.cursor.p,
               S.flt.p, S.err.p);
    TRY(K.clock.mark(ctx));
    uint32_t err = 0;
    TRY(download(ctx, cursor.data(), S.cursor, n_sets));
    TRY(download(ctx, &err, S.err, 1));
    FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (uint32_t s = 0; s < n_sets; s++) if (cursor[s] != K.R.sets[s].n_filtered) err |= FSV_KMER_E_FLT;
    if (err) return fsv_fail(ctx, FSV_EINTERNAL, "k-mer count table: the filter pass and the histogram disagree");
    return FSV_OK;
}

// (the caller's sets have been checked: check_readsets)
static int kmer_stage(fsv_ctx *ctx, AsmWs &W, const KmerJob &J, KmerResult &R)
{
    KmerRun K{J, R};
    TRY(kmer_sketch(ctx, W, K));
    TRY(kmer_count(ctx, W, K));
    kmer_verdicts(K);
    TRY(kmer_filter_list(ctx, W, K));
    if (J.ms) *J.ms += K.clock.ms();
    return FSV_OK;
}

// a result's histograms as the callers of fsv_kmer_table / fsv_kmer_index take them: n_sets x FSV_KMER_BINS 64-bit counts
static void widen_hist(const KmerResult &R, uint64_t *hist) { for (size_t i = 0; i < R.hist.size(); i++) hist[i] = R.hist[i]; }

// The sets' filter sets for the sketch kernels (k_sketch.h), from filter lists on the device: set s's keys are list[list_off[s] ..
// list_off[s + 1]), any order, duplicates allowed.  skip (or null / empty): sets with a non-zero entry get no slots -- their reads are
// sketched unfiltered.  Leaves the view in W.fs.view -- nothing when no set has a slot: every launch then runs the kernels without the
// filter -- and adds the build's time to *ms.
static int build_filter_sets(fsv_ctx *ctx, AsmWs &W, const fsv_readsets *sets, const unsigned long long *list, const std::vector<uint64_t> &list_off,
                             const std::vector<uint8_t> *skip, double *ms)
{
    const uint32_t n_sets = sets->n_sets, n_reads = sets->n_reads;
    FilterState &S = W.fs;
    S.view = SketchFilter{};
    std::vector<uint64_t> set_off((size_t)n_sets + 1, 0);
    for (uint32_t s = 0; s < n_sets; s++)
        set_off[s + 1] = set_off[s] + ((skip && !skip->empty() && (*skip)[s]) ? 0 : flt_set_slots(list_off[s + 1] - list_off[s]));
    const uint64_t total = set_off[n_sets], n_keys = list_off[n_sets];
    if (!total || !n_reads) return FSV_OK;
    if (n_keys >= (1ull << 39)) return fsv_fail(ctx, FSV_EUNSUP, "filter lists too long for one pass; split the batch");
    TRY(ensure(ctx, S.keys, total));
    TRY(upload(ctx, S.off, set_off));
    TRY(upload(ctx, S.list_off, list_off));
    TRY(upload(ctx, S.read_set, read_set_of(sets)));
    TRY(ensure(ctx, W.km.err, 1));
    TRY(zero(ctx, W.km.err, 1));
    EventClock clock;
    TRY(clock.mark(ctx));
    FSV_HIP(ctx, hipMemsetAsync(S.keys.p, 0xff, total * sizeof(unsigned long long), ctx->stream));   // every slot FSV_KMER_EMPTY
    FSV_LAUNCH(ctx, ctx->stream, k_flt_build, dim3((uint32_t)((n_keys + 255) / 256)), dim3(256), 0, list, S.list_off.p, S.off.p, n_sets, S.keys.p, W.km.err.p);
    TRY(clock.mark(ctx));
    uint32_t err = 0;
    TRY(download(ctx, &err, W.km.err, 1));
    FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (err) return fsv_fail(ctx, FSV_EINTERNAL, "k-mer filter: a filter set ran full");
    if (ms) *ms += clock.ms();
    S.view = SketchFilter{S.keys.p, S.off.p, S.read_set.p};
    return FSV_OK;
}

// hifiasm's first ha_pt_gen (htab.cpp:952-998) on the caller's sets: the sketch at (w, k, hpc) through the filter sets in W.fs.view, counted
// with the count table's own kernels.  out: n_sets records; hist: n_sets x 4096 or null.  A skipped set (see build_filter_sets) is one
// hifiasm filters every k-mer of: the index of nothing.
static int index_stage(fsv_ctx *ctx, AsmWs &W, const fsv_readsets *sets, int w, int k, int hpc, const std::vector<uint8_t> *skip, fsv_kmer_index_set *out,
                       uint64_t *hist, double *ms)
{
    const SketchFilter flt = W.fs.view;
    KmerResult R;
    TRY(kmer_stage(ctx, W, KmerJob{sets, w, k, hpc, &flt, ms}, R));
    if (hist) widen_hist(R, hist);
    const std::vector<fsv_kmer_set> &v = R.sets;
    std::vector<int64_t> none(FSV_KMER_BINS, 0);
    for (uint32_t s = 0; s < sets->n_sets; s++) {
        fsv_kmer_index_set &o = out[s];
        memset(&o, 0, sizeof(o));
        if (skip && !skip->empty() && (*skip)[s]) {
            o.peak_hom = fsv_kmer_peaks_hd(none.data(), FSV_KMER_BINS, FSV_KMER_START, &o.peak_het, &o.low_i, &o.max_i);
            if (hist) memset(hist + (size_t)s * FSV_KMER_BINS, 0, FSV_KMER_BINS * sizeof(uint64_t));
            continue;
        }
        o.n_entries = v[s].n_entries; o.n_distinct = v[s].n_distinct; o.n_indexed = v[s].n_indexed;
        o.low_i = v[s].low_i; o.max_i = v[s].max_i; o.peak_hom = v[s].peak_hom; o.peak_het = v[s].peak_het;
    }
    return FSV_OK;
}

// the (w, k) a sketch launch takes: fsv_sketch_reads with variant 0, fsv_kmer_table
static int check_sketch_scheme(fsv_ctx *ctx, int w, int k)
{
    if (k < 1 || k > 63 || w < 1) return fsv_fail(ctx, FSV_EINVAL, "1 <= k <= 63, 1 <= w");
    if (k & 1) { if (w > 255) return fsv_fail(ctx, FSV_EINVAL, "w <= 255 (position-parallel kernel: odd k)"); }
    else if (w > 64) return fsv_fail(ctx, FSV_EINVAL, "w <= 64 (replay kernel: even k)");
    return FSV_OK;
}

static int fsv_kmer_table_impl(fsv_ctx *ctx, const fsv_readsets *sets, int32_t w, int32_t k, int32_t hpc, fsv_kmer_set *out, uint64_t *hist,
                               uint64_t *flt_hash, uint64_t flt_cap, uint64_t *flt_off)
{
    if (!ctx || !readsets_present(sets, true) || !out) return FSV_EINVAL;
    if ((flt_hash == nullptr) != (flt_off == nullptr)) return fsv_fail(ctx, FSV_EINVAL, "fsv_kmer_table: flt_hash and flt_off go together");
    TRY(check_sketch_scheme(ctx, w, k));
    TRY(check_readsets(ctx, sets, RS_ALL));
    FSV_HIP(ctx, hipSetDevice(ctx->device));
    AsmWs &W = *ws_get(ctx);
    W.n_reads = 0; W.cur_store = nullptr;     // (the workspace's read tables are this call's now: nothing for fsv_asm_fetch_reads)
    const uint32_t n_sets = sets->n_sets;
    KmerResult R;
    TRY(kmer_stage(ctx, W, KmerJob{sets, w, k, hpc ? 1 : 0, nullptr, nullptr}, R));
    if (n_sets) memcpy(out, R.sets.data(), (size_t)n_sets * sizeof(fsv_kmer_set));
    if (hist) widen_hist(R, hist);
    if (!flt_off) return FSV_OK;
    // the caller's copy of the filter list: every set's segment in ascending order
    const uint64_t n_flt = R.flt_off[n_sets];
    memcpy(flt_off, R.flt_off.data(), ((size_t)n_sets + 1) * sizeof(uint64_t));
    if (n_flt > flt_cap) return fsv_fail(ctx, FSV_ECAP, "fsv_kmer_table: flt_hash too small");
    if (n_flt) {
        FSV_HIP(ctx, hipMemcpyAsync(flt_hash, W.km.flt.p, n_flt * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
        FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    for (uint32_t s = 0; s < n_sets; s++) std::sort(flt_hash + flt_off[s], flt_hash + flt_off[s + 1]);
    return FSV_OK;
}

static int fsv_kmer_index_impl(fsv_ctx *ctx, const fsv_readsets *sets, int32_t w, int32_t k, int32_t hpc, fsv_kmer_set *table, fsv_kmer_index_set *index,
                               uint64_t *hist)
{
    if (!ctx || !readsets_present(sets, true) || !table || !index) return FSV_EINVAL;
    TRY(check_sketch_scheme(ctx, w, k));
    TRY(check_readsets(ctx, sets, RS_ALL));
    FSV_HIP(ctx, hipSetDevice(ctx->device));
    AsmWs &W = *ws_get(ctx);
    W.n_reads = 0; W.cur_store = nullptr;     // (the workspace's read tables are this call's now: nothing for fsv_asm_fetch_reads)
    KmerResult R;
    TRY(kmer_stage(ctx, W, KmerJob{sets, 1, k, hpc ? 1 : 0, nullptr, nullptr}, R));
    if (sets->n_sets) memcpy(table, R.sets.data(), (size_t)sets->n_sets * sizeof(fsv_kmer_set));
    // (a set without a peak has cutoff -5: its list holds every k-mer, its sketch comes out empty)
    TRY(build_filter_sets(ctx, W, sets, W.km.flt.p, R.flt_off, nullptr, nullptr));
    const int rc = index_stage(ctx, W, sets, w, k, hpc ? 1 : 0, nullptr, index, hist, nullptr);
    W.fs.view = SketchFilter{};
    return rc;
}

static int fsv_asm_last_kmer_index_impl(const fsv_ctx *ctx, fsv_kmer_index_set *out, uint32_t n_sets, double *ms)
{
    if (!ctx || !ctx->asm_ws || (!out && n_sets)) return FSV_EINVAL;
    const AsmWs &W = *(const AsmWs *)ctx->asm_ws;
    if (!W.fs.valid || W.fs.last.size() != n_sets) return FSV_EINVAL;
    if (n_sets) memcpy(out, W.fs.last.data(), (size_t)n_sets * sizeof(fsv_kmer_index_set));
    if (ms) *ms = W.fs.ms;
    return FSV_OK;
}

static int fsv_asm_last_kmer_table_impl(const fsv_ctx *ctx, fsv_kmer_set *out, uint32_t n_sets, double *ms)
{
    if (!ctx || !ctx->asm_ws || (!out && n_sets)) return FSV_EINVAL;
    const AsmWs &W = *(const AsmWs *)ctx->asm_ws;
    if (!W.km.valid || W.km.last.size() != n_sets) return FSV_EINVAL;
    if (n_sets) memcpy(out, W.km.last.data(), (size_t)n_sets * sizeof(fsv_kmer_set));
    if (ms) *ms = W.km.ms;
    return FSV_OK;
}

// kmer_table = 1: the stage on a chunk's raw reads at (w = 1, k, hpc) before round 0.  The verdicts and the filter list join what the
// chunks before left on the context (fsv_assemble_batch_impl cleared it); low[s] = 1 for the sets without a peak.
static int kmer_stage_of_chunk(fsv_ctx *ctx, AsmWs &W, const fsv_readsets *sets, const fsv_asm_params &P, std::vector<uint8_t> &low)
{
    KmerTableState &S = W.km;
    KmerResult R;
    TRY(kmer_stage(ctx, W, KmerJob{sets, 1, P.k, P.hpc ? 1 : 0, nullptr, &S.ms}, R));
    const std::vector<fsv_kmer_set> &v = R.sets;
    const std::vector<uint64_t> &off = R.flt_off;
    low.assign(sets->n_sets, 0);
    bool any = false;
    for (uint32_t s = 0; s < sets->n_sets; s++) if (v[s].peak_hom < 0) { low[s] = 1; any = true; }
    if (!any) low.clear();
    // the filter list of the chunks so far, back to back on the device
    const uint64_t have = S.last_flt_off.back();
    TRY(append_on_device(ctx, S.flt_all, have, S.flt.p, off.back()));
    for (uint32_t s = 0; s < sets->n_sets; s++) S.last_flt_off.push_back(have + off[s + 1]);
    S.last.insert(S.last.end(), v.begin(), v.end());
    if (P.kmer_filter) {
        // the chunk's filter sets, which every sketch of its rounds and of its final pass takes; sets without a peak stay as they are
        // (kmer_table leaves them alone).  Then hifiasm's first ha_pt_gen: the filtered sketch at w, counted
        TRY(build_filter_sets(ctx, W, sets, S.flt.p, off, &low, &W.fs.ms));
        std::vector<fsv_kmer_index_set> idx(sets->n_sets);
        TRY(index_stage(ctx, W, sets, P.w, P.k, P.hpc ? 1 : 0, &low, idx.data(), nullptr, &W.fs.ms));
        W.fs.last.insert(W.fs.last.end(), idx.begin(), idx.end());
    }
    return FSV_OK;
}

// the chunk's charge counters and stage time join the call's (W.ch.last)
static int charge_collect(fsv_ctx *ctx, AsmWs &W)
{
    unsigned long long h[8] = {0};
    TRY(download(ctx, h, W.ch.ct, 8));
    FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    fsv_charge_stats &c = W.ch.last;
    c.n_overlaps += h[CH_OVERLAPS]; c.n_windows += h[CH_WINDOWS]; c.n_ext += h[CH_EXT]; c.n_accepted += h[CH_ACCEPTED]; c.n_flipped += h[CH_FLIPPED];
    c.ms += W.ch.clock.ms();
    W.ch.clock.clear();
    return FSV_OK;
}

static int assemble_chunk(fsv_ctx *ctx, const fsv_readsets *sets, const fsv_asm_params &P, fsv_contigs *out)
{
    AsmWs &W = *ws_get(ctx);
    memset(&W.stats, 0, sizeof(W.stats));
    W.kt.reset();
    Round R(P);
    out->n_contigs = 0;
    out->off[0] = 0;
    for (uint32_t s = 0; s < sets->n_sets; s++) out->set_status[s] = 0;
    if (sets->n_sets == 0) return FSV_OK;
    // (the second level fsv_assemble_batch calls check_readsets from -- here, not at the entry: a chunk's offsets count from its first read, and
    // a store beyond 2^32 words that is cut so that every chunk stays below is served)
    TRY(check_readsets(ctx, sets, RS_WORD_OFF));
    if (P.kmer_table) {
        TRY(kmer_stage_of_chunk(ctx, W, sets, P, R.low_cov));
        for (uint32_t s = 0; s < sets->n_sets; s++) if (!R.low_cov.empty() && R.low_cov[s]) out->set_status[s] = FSV_W_LOW_COV | FSV_W_NO_LAYOUT;
    }
    if (sets->n_reads == 0) return FSV_OK;
    TRY(prepare_batch(ctx, W, sets, R));
    if (P.partial_charge) { TRY(ensure(ctx, W.ch.ct, 8)); TRY(zero(ctx, W.ch.ct, 8)); }
    for (R.round = 0; R.round < P.n_rounds; R.round++) {
        TRY(begin_round(ctx, W, R));
        TRY(overlap_stage(ctx, W, R, false));
        W.stats.n_pairs += R.B.n_pairs;
        if (R.B.n_pairs) TRY(verify_stage(ctx, W, R));
        // consensus -> corrected windows -> new read store
        Span tcs(ctx, W.kt, ST_CONSENSUS);
        TRY(consensus_stage(ctx, W, R));
        if (P.second_round && R.B.n_pairs) TRY(second_pass(ctx, W, R));
        TRY(finish_round(ctx, W, R));
        tcs.stop();
    }
    Span tf(ctx, W.kt, ST_FINAL);
    Final F;
    F.trace = Trace{ctx, "final"};
    TRY(final_overlaps(ctx, W, R, F));
    TRY(gather_hits(ctx, W, R, F));
    TRY(layout_sets(ctx, W, R, F));
    TRY(emit_contigs(ctx, W, R, F, out));
    tf.stop();
    W.h_word_off = R.G.word_off; W.h_len = R.len; W.cur_store = R.store; W.n_reads = R.B.n_reads;
    fill_stats(W, R, F);
    if (P.partial_charge) TRY(charge_collect(ctx, W));
    return FSV_OK;
}

// Work a set brings: its window-task bound (every read's windows against every other read) and its ordered pairs.
// kmer_bytes: what the k-mer count table stage would hold for the set -- a table slot (12 B) for at least twice its bases, the filter
// list when every k-mer is filtered (8 B a base), its histogram.  flt_bytes: the set's filter set with kmer_filter = 1 -- 8 B a slot for at
// least twice its filtered keys; a filtered key occurs 5 x peak_hom times or more and no peak lies below FSV_KMER_START + 1, so a thirtieth
// of the bases bounds them (a set without a peak gets no filter set)
static void set_cost(const fsv_readsets *sets, uint32_t s, uint64_t &tasks, uint64_t &pairs, uint64_t &bases, uint64_t &kmer_bytes, uint64_t &flt_bytes)
{
    const uint64_t ns = sets->set_start[s + 1] - sets->set_start[s];
    uint64_t nw = 0; bases = 0;
    for (uint32_t r = sets->set_start[s]; r < sets->set_start[s + 1]; r++) { nw += ((uint64_t)sets->read_len[r] + FSV_WINDOW - 1) / FSV_WINDOW; bases += (uint64_t)sets->read_len[r]; }
    tasks = ns > 1 ? nw * (ns - 1) : 0;
    pairs = ns > 1 ? ns * (ns - 1) : 0;
    kmer_bytes = kmer_table_slots(bases) * 12ull + bases * 8ull + FSV_KMER_BINS * 4ull;
    flt_bytes = flt_set_slots(bases / 30 + 1) * 8ull;
}

static int check_asm_params(fsv_ctx *ctx, const fsv_asm_params &P)
{
    if (P.k < 1 || P.k > 63 || P.w < 1 || P.w > 64 || P.lookback != 64 || P.n_rounds < 0 || P.n_rounds > 16 || P.min_anchors < 1)
        return fsv_fail(ctx, FSV_EINVAL, "fsv_asm_params out of range (k<=63, w<=64, lookback==64)");
    if (P.k_cap < 1 || P.k_cap > FSV_K_WIDE || P.win_rate_pm < 1 || (int)(FSV_WINDOW * (P.win_rate_pm / 1000.0)) > P.k_cap || P.accept_err_pm < 0 || P.accept_err_pm > 1000 ||
        P.w_later < 0 || P.w_later > 64)
        return fsv_fail(ctx, FSV_EINVAL, "fsv_asm_params error model out of range (k_cap <= 95, 375 x win_rate_pm / 1000 <= k_cap)");
    if (P.full_lists != 0 && P.full_lists != 1) return fsv_fail(ctx, FSV_EINVAL, "full_lists is 0 or 1");
    if (P.deep_sets != 0 && P.deep_sets != 1) return fsv_fail(ctx, FSV_EINVAL, "deep_sets is 0 or 1");
    if (P.kmer_filter && !P.kmer_table)
        return fsv_fail(ctx, FSV_EINVAL, "kmer_filter = 1 needs kmer_table = 1: the filter is the list the k-mer count table stage leaves");
    if (P.partial_charge && P.k_cap > FSV_K_MAX)
        return fsv_fail(ctx, FSV_EINVAL, "partial_charge needs k_cap <= 31 (FSV_K_MAX): the charge is not restated for the wide-band profiles");
    return FSV_OK;
}

static int fsv_assemble_batch_impl(fsv_ctx *ctx, const fsv_readsets *sets, const fsv_asm_params *params, fsv_contigs *out)
{
    if (!ctx || !readsets_present(sets, true) || !out) return FSV_EINVAL;
    if (!out->seq || !out->off || !out->set || !out->n_reads || !out->set_status) return FSV_EINVAL;
    fsv_asm_params P;
    if (params) P = *params; else fsv_asm_default_params(&P);
    TRY(check_asm_params(ctx, P));
    FSV_HIP(ctx, hipSetDevice(ctx->device));
    AsmWs &W = *ws_get(ctx);
    out->n_contigs = 0; out->off[0] = 0;
    // what the opt-in stages leave on the context belongs to this call from here on (its chunks add to it)
    W.reset_stages();
    W.n_long_reads = W.n_spilled_pairs = 0;
    W.n_deep_windows = W.n_deep_junctions = 0; W.deep_max_events = 0;
    // (without reads a kmer_table call still goes on: every set gets its verdict -- no k-mer, no peak)
    if (sets->n_sets == 0 || (sets->n_reads == 0 && !P.kmer_table)) { for (uint32_t s = 0; s < sets->n_sets; s++) out->set_status[s] = 0; memset(&W.stats, 0, sizeof(W.stats)); W.mark_valid(P, false); return FSV_OK; }
    TRY(check_readsets(ctx, sets, RS_SETS | RS_LEN));   // (the word offsets: per chunk, assemble_chunk)
    // Read sets are independent, so a batch that is too large for one pass -- 32-bit pair / task / offset indices, or a workspace
    // beyond the budget (FSV_ASM_BUDGET_GB, default 40 % of the device's memory: ~200 B per window task (400 with the second consensus pass), ~200 B per read pair,
    // ~48 B per base) -- is cut into runs of consecutive sets that go through one after the other; the caller sees one call.
    // (Round 1 returned FSV_EUNSUP and left the splitting to the caller.)
    // The default budget: 40 % of the device's memory, but never more than what this context can still get -- its own workspace plus
    // its share of the FREE bytes (divided among the contexts alive on the device; the budgets of all of them then add up to at
    // most 90 % of what is free plus what they hold).  Three lanes of one process used to be allowed 120 % of the device between them,
    // and a chromosome-sized batch failed in hipMalloc instead of being split.
    const char *env = getenv("FSV_ASM_BUDGET_GB");
    double budget = 0.4 * (double)ctx->hbm_bytes;
    {
        size_t free_b = 0, total_b = 0;
        const size_t own = W.held();
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess)
            budget = std::min(budget, 0.9 * ((double)free_b / (double)std::max(1, fsv_live_contexts(ctx->device)) + (double)own));
    }
    if (env && atof(env) > 0) budget = atof(env) * 1e9;
    std::vector<uint32_t> cut{0};
    {
        uint64_t tk = 0, pr = 0, bs = 0, km = 0;
        for (uint32_t s = 0; s < sets->n_sets; s++) {
            uint64_t t1, p1, b1, k1, f1;
            set_cost(sets, s, t1, p1, b1, k1, f1);
            if (!P.kmer_table) k1 = 0;
            if (P.kmer_filter) k1 += f1;
            if (t1 >= (1ull << 31) || p1 >= (1ull << 31) || b1 + b1 / 4 >= (1ull << 32)) return fsv_fail(ctx, FSV_EUNSUP, "a single read set exceeds the 2^31 window-task / pair bound");
            const bool over = tk + t1 >= (1ull << 31) || pr + p1 >= (1ull << 31) || (bs + b1) + (bs + b1) / 4 >= (1ull << 32) ||     /* minimizer slots: one per base + slack, 32-bit offsets */
                              (double)(tk + t1) * (P.second_round ? 400.0 : 200.0) + (double)(pr + p1) * 200.0 + (double)(bs + b1) * (P.second_round ? 52.0 : 48.0) +
                              (double)(km + k1) + (P.partial_charge ? (double)(tk + t1) * 104.0 : 0.0) > budget;   /* second pass: the junction tasks' records, the patch slots; kmer_table: the sets' tables */
            if (over && s > cut.back()) { cut.push_back(s); tk = pr = bs = km = 0; }
            tk += t1; pr += p1; bs += b1; km += k1;
        }
        cut.push_back(sets->n_sets);
    }
    if (cut.size() == 2) { TRY(assemble_chunk(ctx, sets, P, out)); W.mark_valid(P, true); return FSV_OK; }
    fsv_asm_stats total; memset(&total, 0, sizeof(total));
    uint64_t used = 0; uint32_t nc = 0;
    std::vector<uint64_t> all_off{0};
    for (size_t c = 0; c + 1 < cut.size(); c++) {
        const uint32_t s0 = cut[c], s1 = cut[c + 1], r0 = sets->set_start[s0], r1 = sets->set_start[s1];
        std::vector<uint32_t> sub_start(s1 - s0 + 1);
        for (uint32_t s = s0; s <= s1; s++) sub_start[s - s0] = sets->set_start[s] - r0;
        fsv_readsets sub = *sets;
        // the chunk sees a store of its own: offsets relative to its first read (with the caller's absolute offsets a late chunk's
        // second pass copied the whole store prefix in front of it, and offsets beyond 2^32 words made it fail -- ADVICE r02)
        std::vector<uint64_t> sub_woff((size_t)(r1 - r0) + 1);
        for (uint32_t r = r0; r <= r1; r++) sub_woff[r - r0] = sets->word_off[r] - sets->word_off[r0];
        sub.store_dev = sets->store_dev + sets->word_off[r0];
        sub.word_off = sub_woff.data(); sub.read_len = sets->read_len + r0; sub.set_start = sub_start.data();
        sub.n_reads = r1 - r0; sub.n_sets = s1 - s0; sub.set_flags = sets->set_flags ? sets->set_flags + s0 : nullptr;
        fsv_contigs part = *out;
        part.seq = out->seq + used; part.seq_cap = out->seq_cap - used; part.off = out->off + nc; part.set = out->set + nc; part.n_reads = out->n_reads + nc;
        part.contig_cap = out->contig_cap - nc; part.set_status = out->set_status + s0; part.n_contigs = 0;
        const uint64_t keep = out->off[nc];          // part.off[0] is this slot: the chunk writes 0 there
        TRY(assemble_chunk(ctx, &sub, P, &part));
        out->off[nc] = keep;
        for (uint32_t i = 0; i < part.n_contigs; i++) { out->set[nc + i] += s0; out->off[nc + i + 1] += used; }
        // the contigs stay on the device for the aligner (fsv_align_batch(contig_seq = NULL)): gather the chunks' contigs in one buffer
        const uint64_t bytes = part.n_contigs ? out->off[nc + part.n_contigs] - used : 0;
        TRY(append_on_device(ctx, W.contig_all, used, W.contig_out.p, bytes, 16, 1u << 20));
        used += bytes; nc += part.n_contigs;
        add_stats(total, W.stats);
    }
    FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    out->n_contigs = nc;
    W.stats = total;
    W.mark_valid(P, true);
    W.n_reads = 0; W.cur_store = nullptr;        // fsv_asm_fetch_reads serves single-pass batches only
    ctx->last_contigs_dev = nc ? W.contig_all.p : nullptr;
    ctx->last_contig_off.assign(out->off, out->off + nc + 1);
    return FSV_OK;
}

static int fsv_asm_fetch_reads_impl(fsv_ctx *ctx, char *seq, uint64_t seq_cap, uint64_t *off, uint32_t n_reads)
{
    if (!ctx || !ctx->asm_ws || !seq || !off) return FSV_EINVAL;
    AsmWs &W = *(AsmWs *)ctx->asm_ws;
    if (n_reads != W.n_reads || !W.cur_store) return fsv_fail(ctx, FSV_EINVAL, "no assembled batch with that many reads on this context");
    FSV_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<uint64_t> o(n_reads + 1, 0);
    for (uint32_t r = 0; r < n_reads; r++) o[r + 1] = o[r] + (uint64_t)W.h_len[r];
    if (o[n_reads] > seq_cap) return FSV_ECAP;
    memcpy(off, o.data(), (n_reads + 1) * sizeof(uint64_t));
    Dev<uint64_t> d_off;
    Dev<char> d_out;
    TRY(upload(ctx, d_off, o));
    TRY(ensure(ctx, d_out, o[n_reads] + 16));
    FSV_LAUNCH(ctx, ctx->stream, k_unpack_reads, dim3(n_reads), dim3(256), 0, W.cur_store, W.word_off.p, W.len.p, d_off.p, d_out.p);
    return fsv_d2h(ctx, seq, d_out.p, o[n_reads]);
}

// flt_hash / flt_off: fsv_sketch_reads_filtered's per-set lists, or null (fsv_sketch_reads, or a caller without lists)
static int fsv_sketch_reads_impl(fsv_ctx *ctx, const fsv_readsets *sets, int32_t w, int32_t k, int32_t hpc, int32_t variant, fsv_mz *out_mz,
                                uint64_t out_cap, uint64_t *out_off, const uint64_t *flt_hash = nullptr, const uint64_t *flt_off = nullptr)
{
    if (!ctx || !readsets_present(sets, false) || !out_mz || !out_off) return FSV_EINVAL;
    if (flt_hash) {
        if (!flt_off || !sets->set_start) return fsv_fail(ctx, FSV_EINVAL, "fsv_sketch_reads_filtered: flt_hash goes with flt_off and set_start");
        TRY(check_readsets(ctx, sets, RS_SETS));
        if (flt_off[0] != 0) return fsv_fail(ctx, FSV_EINVAL, "fsv_sketch_reads_filtered: flt_off starts at 0");
        for (uint32_t s = 0; s < sets->n_sets; s++) if (flt_off[s + 1] < flt_off[s]) return fsv_fail(ctx, FSV_EINVAL, "fsv_sketch_reads_filtered: flt_off not monotone");
        for (uint64_t i = 0; i < flt_off[sets->n_sets]; i++)
            if (flt_hash[i] == FSV_KMER_EMPTY) return fsv_fail(ctx, FSV_EINVAL, "fsv_sketch_reads_filtered: UINT64_MAX is the dummy hash, not a k-mer");
    }
    if (k < 1 || k > 63 || w < 1) return fsv_fail(ctx, FSV_EINVAL, "1 <= k <= 63, 1 <= w");
    // the position-parallel kernel's LDS tile holds w <= 255 (as the aligner uses it); the replay kernel keeps w deque slots per lane
    if ((k & 1) && variant != 1) { if (w > 255) return fsv_fail(ctx, FSV_EINVAL, "w <= 255 (position-parallel kernel: odd k, variant 0)"); }
    else if (w > 64) return fsv_fail(ctx, FSV_EINVAL, "w <= 64 (replay kernel: even k, or variant 1)");
    FSV_HIP(ctx, hipSetDevice(ctx->device));
    AsmWs &W = *ws_get(ctx);
    W.kt.reset();
    const uint32_t n_reads = sets->n_reads;
    out_off[0] = 0;
    if (n_reads == 0) return FSV_OK;
    TRY(check_readsets(ctx, sets, RS_LEN | RS_WORD_OFF));
    Geometry G;
    TRY(stage_sketch_reads(ctx, W, sets, w, nullptr, G));
    W.fs.view = SketchFilter{};
    if (flt_hash && flt_off[sets->n_sets]) {    // the caller's lists -> the filter sets, as kmer_stage_of_chunk builds them from the stage's list
        const std::vector<uint64_t> list_off(flt_off, flt_off + sets->n_sets + 1);
        TRY(ensure(ctx, W.fs.list, list_off.back()));
        FSV_HIP(ctx, hipMemcpyAsync(W.fs.list.p, flt_hash, list_off.back() * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
        TRY(build_filter_sets(ctx, W, sets, W.fs.list.p, list_off, nullptr, nullptr));
    }
    const SketchFilter flt = W.fs.view;
    W.fs.view = SketchFilter{};
    // variant 1: the replay kernel for an odd k as well (by itself the launch picks the kernel by the parity of k)
    TRY(launch_sketch(ctx, W, SketchJob{sets->store_dev, n_reads, G.word_off[n_reads], G.max_words, w, k, hpc, nullptr, w, variant == 1, nullptr, flt}));
    std::vector<uint32_t> cnt(n_reads);
    TRY(download(ctx, cnt.data(), W.mz_cnt, n_reads));
    FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    uint64_t tot = 0;
    for (uint32_t r = 0; r < n_reads; r++) {
        const uint32_t c = std::min<uint32_t>(cnt[r], G.mz_off[r + 1] - G.mz_off[r]);
        if (tot + c > out_cap) return fsv_fail(ctx, FSV_ECAP, "out_mz too small");
        FSV_HIP(ctx, hipMemcpyAsync(out_mz + tot, W.mz.p + G.mz_off[r], (size_t)c * sizeof(fsv_mz), hipMemcpyDeviceToHost, ctx->stream));
        tot += c;
        out_off[r + 1] = tot;
    }
    FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (uint32_t r = 0; r < n_reads; r++)
        std::sort(out_mz + out_off[r], out_mz + out_off[r + 1], [](const fsv_mz &a, const fsv_mz &b) { return a.pos < b.pos; });
    return FSV_OK;
}

// The per-read index alone (test hook): launch_sketch and launch_uniq as overlap_stage runs them, all reads as one set.
static int fsv_read_index_impl(fsv_ctx *ctx, const fsv_readsets *sets, int32_t w, int32_t k, int32_t hpc, int32_t full_lists, fsv_mz *out_mz,
                               uint64_t out_cap, uint64_t *out_off, uint32_t *warn)
{
    if (!ctx || !readsets_present(sets, false) || !out_mz || !out_off || !warn) return FSV_EINVAL;
    if (full_lists != 0 && full_lists != 1) return fsv_fail(ctx, FSV_EINVAL, "full_lists is 0 or 1");
    if (k < 1 || k > 63 || w < 1 || w > ((k & 1) ? 255 : 64)) return fsv_fail(ctx, FSV_EINVAL, "1 <= k <= 63, 1 <= w <= 255 (odd k) or 64 (even k)");
    FSV_HIP(ctx, hipSetDevice(ctx->device));
    AsmWs &W = *ws_get(ctx);
    W.kt.reset();
    const uint32_t n_reads = sets->n_reads;
    out_off[0] = 0;
    if (n_reads == 0) return FSV_OK;
    TRY(check_readsets(ctx, sets, RS_LEN | RS_WORD_OFF));
    Geometry G;
    TRY(stage_sketch_reads(ctx, W, sets, w, nullptr, G, full_lists != 0));   // (the slots of the assembly with these settings: mz_slots)
    const std::vector<int32_t> len(sets->read_len, sets->read_len + n_reads);
    TRY(launch_sketch(ctx, W, SketchJob{sets->store_dev, n_reads, G.word_off[n_reads], G.max_words, w, k, hpc, nullptr, w, false, nullptr, SketchFilter{}}));
    TRY(launch_uniq(ctx, W, UniqJob{n_reads, G.max_words, nullptr, nullptr, full_lists != 0, longest_slot(G, n_reads), reads_above(len, FSV_UQ_MAX), nullptr}, [] {}));
    std::vector<uint32_t> cnt(n_reads);
    TRY(download(ctx, cnt.data(), W.mz_cnt, n_reads));
    TRY(download(ctx, warn, W.warn, n_reads));
    FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    uint64_t tot = 0;
    for (uint32_t r = 0; r < n_reads; r++) {
        const uint64_t c = std::min<uint64_t>(2ull * cnt[r], G.mz_off[r + 1] - G.mz_off[r]);
        if (tot + c > out_cap) return fsv_fail(ctx, FSV_ECAP, "out_mz too small");
        if (c) FSV_HIP(ctx, hipMemcpyAsync(out_mz + tot, W.mz.p + G.mz_off[r], (size_t)c * sizeof(fsv_mz), hipMemcpyDeviceToHost, ctx->stream));
        tot += c;
        out_off[r + 1] = tot;
    }
    FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return FSV_OK;
}

// The overlap stage of one pass, alone (test hook): prepare_batch -> begin_round / begin_final -> overlap_stage, and for pass 2
// rechain_listed on the caller's pairs -- the functions assemble_chunk runs, on one pass's worth of them -- then the raw records.
static int fsv_asm_overlaps_impl(fsv_ctx *ctx, const fsv_readsets *sets, const fsv_asm_params *params, int32_t pass, const uint32_t *rechain,
                                 uint32_t n_rechain, fsv_ovl *ovl, uint64_t ovl_cap, uint32_t *pair_base, fsv_wtask *tasks, uint64_t task_cap,
                                 uint32_t *n_tasks, uint32_t *overflow, uint32_t *warn)
{
    if (!ctx || !readsets_present(sets, true) || !pair_base || !n_tasks || !overflow || !warn) return FSV_EINVAL;
    if (pass < 0 || pass > 2 || (n_rechain && (pass != 2 || !rechain)) || (ovl_cap && !ovl) || (task_cap && !tasks)) return fsv_fail(ctx, FSV_EINVAL, "fsv_asm_overlaps: pass is 0, 1 or 2; a pair list goes with pass 2");
    fsv_asm_params P;
    if (params) P = *params; else fsv_asm_default_params(&P);
    TRY(check_asm_params(ctx, P));
    if (pass > 0) P.n_rounds = 0;     // a final pass with no round before it: every read is sketched, no verdict of an earlier round
    if (sets->n_reads == 0 || sets->n_sets == 0) return fsv_fail(ctx, FSV_EINVAL, "fsv_asm_overlaps: no reads");
    TRY(check_readsets(ctx, sets, RS_ALL));
    FSV_HIP(ctx, hipSetDevice(ctx->device));
    AsmWs &W = *ws_get(ctx);
    memset(&W.stats, 0, sizeof(W.stats));
    W.kt.reset();
    W.n_reads = 0; W.cur_store = nullptr;     // (nothing here for fsv_asm_fetch_reads)
    W.fs.view = SketchFilter{};               // (the hook runs no k-mer count table stage: kmer_filter finds nothing to take)
    Round R(P);
    TRY(prepare_batch(ctx, W, sets, R));
    const Batch &B = R.B;
    if (B.n_pairs > ovl_cap) return fsv_fail(ctx, FSV_ECAP, "fsv_asm_overlaps: ovl holds fewer than one record per ordered pair");
    if (n_rechain > B.n_upairs) return fsv_fail(ctx, FSV_EINVAL, "fsv_asm_overlaps: more listed pairs than the batch has");
    for (uint32_t i = 0; i < n_rechain; i++) if (rechain[i] >= B.n_upairs) return fsv_fail(ctx, FSV_EINVAL, "fsv_asm_overlaps: no such unordered pair");
    if (pass == 0) { TRY(begin_round(ctx, W, R)); TRY(overlap_stage(ctx, W, R, false)); }
    else { TRY(begin_final(ctx, W, R)); TRY(overlap_stage(ctx, W, R, true)); }
    if (pass == 2 && B.n_pairs) {
        TRY(ensure(ctx, W.inexact_list, (size_t)B.n_upairs + 4));
        if (n_rechain) FSV_HIP(ctx, hipMemcpyAsync(W.inexact_list.p, rechain, (size_t)n_rechain * 4, hipMemcpyHostToDevice, ctx->stream));
        FSV_HIP(ctx, hipMemcpyAsync(R.ct + CT_INEXACT, &n_rechain, 4, hipMemcpyHostToDevice, ctx->stream));
        TRY(rechain_listed(ctx, W, R, R.ct + CT_INEXACT));
    }
    uint32_t h_ct[CT_SLOT];
    FSV_HIP(ctx, hipMemcpyAsync(h_ct, R.ct, sizeof(h_ct), hipMemcpyDeviceToHost, ctx->stream));
    TRY(download(ctx, warn, W.warn, B.n_reads));
    if (B.n_pairs) TRY(download(ctx, ovl, W.ovl, B.n_pairs));
    FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(pair_base, B.pair_base.data(), (size_t)(B.n_sets + 1) * 4);
    *overflow = h_ct[CT_OVERFLOW];
    *n_tasks = std::min(h_ct[CT_TASKS], R.task_cap);    // (after an overflow the counter has run past the array)
    if (*n_tasks > task_cap) return fsv_fail(ctx, FSV_ECAP, "fsv_asm_overlaps: tasks too small");
    if (*n_tasks) {
        TRY(download(ctx, tasks, W.tasks, *n_tasks));
        FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return FSV_OK;
}

// ---- the guarded C entry points (FSV_GUARD: no C++ exception crosses the boundary)
extern "C" int fsv_assemble_batch(fsv_ctx *ctx, const fsv_readsets *sets, const fsv_asm_params *params, fsv_contigs *out)
{
    FSV_GUARD(ctx, fsv_assemble_batch_impl(ctx, sets, params, out));
}

extern "C" int fsv_bpm_paths(fsv_ctx *ctx, const uint32_t *store, size_t store_words, const fsv_wtask *tasks, uint32_t n_tasks,
                             fsv_wres *res, fsv_wpath *paths)
{
    FSV_GUARD(ctx, fsv_bpm_paths_impl(ctx, store, store_words, tasks, n_tasks, res, paths));
}

extern "C" int fsv_asm_fetch_reads(fsv_ctx *ctx, char *seq, uint64_t seq_cap, uint64_t *off, uint32_t n_reads)
{
    FSV_GUARD(ctx, fsv_asm_fetch_reads_impl(ctx, seq, seq_cap, off, n_reads));
}

extern "C" int fsv_sketch_reads(fsv_ctx *ctx, const fsv_readsets *sets, int32_t w, int32_t k, int32_t hpc, int32_t variant, fsv_mz *out_mz,
                                uint64_t out_cap, uint64_t *out_off)
{
    FSV_GUARD(ctx, fsv_sketch_reads_impl(ctx, sets, w, k, hpc, variant, out_mz, out_cap, out_off));
}

extern "C" int fsv_asm_last_long_lists(const fsv_ctx *ctx, uint64_t *n_reads, uint64_t *n_pairs)
{
    if (!ctx || !ctx->asm_ws || !n_reads || !n_pairs) return FSV_EINVAL;
    const AsmWs &W = *(const AsmWs *)ctx->asm_ws;
    *n_reads = W.n_long_reads; *n_pairs = W.n_spilled_pairs;
    return FSV_OK;
}

extern "C" int fsv_asm_last_deep_windows(const fsv_ctx *ctx, uint64_t *n_windows, uint64_t *n_junctions, uint32_t *max_events)
{
    if (!ctx || !ctx->asm_ws || !n_windows || !n_junctions || !max_events) return FSV_EINVAL;
    const AsmWs &W = *(const AsmWs *)ctx->asm_ws;
    *n_windows = W.n_deep_windows; *n_junctions = W.n_deep_junctions; *max_events = W.deep_max_events;
    return FSV_OK;
}

extern "C" int fsv_read_index(fsv_ctx *ctx, const fsv_readsets *sets, int32_t w, int32_t k, int32_t hpc, int32_t full_lists, fsv_mz *out_mz,
                              uint64_t out_cap, uint64_t *out_off, uint32_t *warn)
{
    FSV_GUARD(ctx, fsv_read_index_impl(ctx, sets, w, k, hpc, full_lists, out_mz, out_cap, out_off, warn));
}

extern "C" int fsv_sketch_reads_filtered(fsv_ctx *ctx, const fsv_readsets *sets, int32_t w, int32_t k, int32_t hpc, int32_t variant, fsv_mz *out_mz,
                                        uint64_t out_cap, uint64_t *out_off, const uint64_t *flt_hash, const uint64_t *flt_off)
{
    FSV_GUARD(ctx, fsv_sketch_reads_impl(ctx, sets, w, k, hpc, variant, out_mz, out_cap, out_off, flt_hash, flt_off));
}

extern "C" int fsv_kmer_index(fsv_ctx *ctx, const fsv_readsets *sets, int32_t w, int32_t k, int32_t hpc, fsv_kmer_set *table, fsv_kmer_index_set *index,
                              uint64_t *hist)
{
    FSV_GUARD(ctx, fsv_kmer_index_impl(ctx, sets, w, k, hpc, table, index, hist));
}

extern "C" int fsv_asm_last_kmer_index(const fsv_ctx *ctx, fsv_kmer_index_set *out, uint32_t n_sets, double *ms)
{
    FSV_GUARD((fsv_ctx *)nullptr, fsv_asm_last_kmer_index_impl(ctx, out, n_sets, ms));
}

extern "C" int fsv_kmer_peaks(const int64_t *hist, int32_t n_cnt, int32_t start_cnt, int32_t *peak_het, int32_t *low_i, int32_t *max_i)
{
    if (!hist || !peak_het || !low_i || !max_i || n_cnt < 3 || start_cnt < 0 || start_cnt >= n_cnt) return FSV_EINVAL;
    return fsv_kmer_peaks_hd(hist, n_cnt, start_cnt, peak_het, low_i, max_i);
}

extern "C" int fsv_kmer_table(fsv_ctx *ctx, const fsv_readsets *sets, int32_t w, int32_t k, int32_t hpc, fsv_kmer_set *out, uint64_t *hist,
                              uint64_t *flt_hash, uint64_t flt_cap, uint64_t *flt_off)
{
    FSV_GUARD(ctx, fsv_kmer_table_impl(ctx, sets, w, k, hpc, out, hist, flt_hash, flt_cap, flt_off));
}

extern "C" int fsv_asm_last_kmer_table(const fsv_ctx *ctx, fsv_kmer_set *out, uint32_t n_sets, double *ms)
{
    FSV_GUARD((fsv_ctx *)nullptr, fsv_asm_last_kmer_table_impl(ctx, out, n_sets, ms));
}

extern "C" int fsv_asm_overlaps(fsv_ctx *ctx, const fsv_readsets *sets, const fsv_asm_params *params, int32_t pass, const uint32_t *rechain,
                                uint32_t n_rechain, fsv_ovl *ovl, uint64_t ovl_cap, uint32_t *pair_base, fsv_wtask *tasks, uint64_t task_cap,
                                uint32_t *n_tasks, uint32_t *overflow, uint32_t *warn)
{
    FSV_GUARD(ctx, fsv_asm_overlaps_impl(ctx, sets, params, pass, rechain, n_rechain, ovl, ovl_cap, pair_base, tasks, task_cap, n_tasks, overflow, warn));
}

extern "C" int fsv_bpm_extensions(fsv_ctx *ctx, const uint32_t *store, size_t store_words, const fsv_wtask *tasks, const uint8_t *dir,
                                  uint32_t n_tasks, int32_t k_cap, fsv_wext *out)
{
    FSV_GUARD(ctx, fsv_bpm_extensions_impl(ctx, store, store_words, tasks, dir, n_tasks, k_cap, out));
}

extern "C" int64_t fsv_partial_charge(int32_t n, int32_t al0, int32_t er0, int32_t al1, int32_t er1, int64_t terr)
{
    return (int64_t)fsv_partial_charge_hd(n, al0, er0, al1, er1, (long long)terr);
}

extern "C" int fsv_asm_last_charge(const fsv_ctx *ctx, fsv_charge_stats *out)
{
    FSV_GUARD((fsv_ctx *)nullptr, fsv_asm_last_charge_impl(ctx, out));
}
