// asm.hip -- host orchestration of the batched per-read-set assembly (fsv_assemble_batch).
//
// Replaces the process boundary `hifiasm -o <prefix> -t T <reads.fa>` + GFA read-back
// (focalsv/3_assembly/run_assembly.py:15-44, post_assembly.py:79-95).  All base-level work runs in the
// kernels of asm_kernels.h and k_sketch.h; the host only sizes buffers between stages and walks the (tiny, <= a few
// hundred nodes per set) overlap graph, which is host code in hifiasm as well (Overlaps.cpp).
#include "asm_kernels.h"
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

// HIP-event timing of kernels and of whole stages on the context's stream: recorded while the work is queued, resolved once
// at the end of the batch -- nothing here waits for the GPU (round 1's stage timers synchronised the stream twice each)
struct KTimes {
    struct Rec { int k; hipEvent_t a, b; uint64_t bytes; };
    std::vector<Rec> recs;
    std::vector<hipEvent_t> pool;
    size_t used = 0;
    hipEvent_t get() { if (used == pool.size()) { hipEvent_t e; (void)hipEventCreate(&e); pool.push_back(e); } return pool[used++]; }
    size_t begin(fsv_ctx *ctx, int k, uint64_t bytes) { Rec r{k, get(), get(), bytes}; (void)hipEventRecord(r.a, ctx->stream); recs.push_back(r); return recs.size() - 1; }
    void end(fsv_ctx *ctx) { (void)hipEventRecord(recs.back().b, ctx->stream); }
    void end(fsv_ctx *ctx, size_t idx) { (void)hipEventRecord(recs[idx].b, ctx->stream); }
    void reset() { recs.clear(); used = 0; }
    ~KTimes() { for (auto e : pool) (void)hipEventDestroy(e); }
};
enum { KN_SKETCH, KN_UNIQ, KN_CHAIN, KN_BPM, KN_RESCUE, KN_PATH_FAST, KN_PATH_DP, KN_CONSENSUS, KN_REPACK, KN_EXACT, KN_STITCH, KN_PARTITION, KN_BND, KN_BND_CONS, KN_COUNT,
       ST_SKETCH = KN_COUNT, ST_CHAIN, ST_VERIFY, ST_PATH, ST_CONSENSUS, ST_FINAL };
const char *const kn_names[KN_COUNT] = {"k_sketch", "k_uniq", "k_chain", "k5_bpm", "k_rescue_accept", "k_path_fast", "k_path_dp", "k_consensus",
                                        "k_repack", "k_exact", "k_stitch", "k_partition", "k_bnd_tasks", "k_bnd_consensus"};

// a stage: from construction to stop(), in stream order
struct Span {
    fsv_ctx *ctx; KTimes &kt; size_t idx;
    Span(fsv_ctx *c, KTimes &k, int stage) : ctx(c), kt(k), idx(k.begin(c, stage, 0)) {}
    void stop() { kt.end(ctx, idx); }
};

// per-round block of device counters (one 64-byte slot per correction round + one for the final pass, zeroed once per batch and
// read back with the round's one synchronisation or at the end): u32 indices
enum { CT_TASKS = 0, CT_OVERFLOW = 1, CT_DP = 2, CT_INEXACT = 3, CT_COLS_LO = 4, CT_COLS_HI = 5, CT_DP_WIDE = 6, CT_DP_SB = 7, CT_DP_GEN = 8, CT_DP_XW = 9,
       CT_MZ_LO = 10, CT_MZ_HI = 11, CT_B_RETRY = 12, CT_B_LIST = 13, CT_DP_SB16 = 14, CT_WIDE = 15,
       CT_MZRAW_LO = 16, CT_MZRAW_HI = 17, CT_BASES_LO = 18, CT_BASES_HI = 19,   // k_uniq's other two sums: CT_MZ + 3 and + 4 as 64-bit words
       CT_DP_FR3 = 20,       // k_path_fr's lists by distance: CT_DP_SB16 (1), CT_DP (2), CT_DP_FR3 (3)
       CT_LEFT = 21,         // overlaps set aside for the left-extension rescue pass (k_left_rescue)
       CT_FIX = 22, CT_FIXED = 23,   // fix_boundary's candidates (k_path_fast) and the windows it moved
       CT_SLOT = 24 };      // even: the 64-bit sums stay aligned in every slot

struct AsmWs {
    DevBuf store[2], cols_sb, contig_all, word_off, len, set_start, read_set, pair_base, mz, mz_off, mz_cnt, ovl, tasks, res, paths, counters, dp_list, dp_list2, dp_list3, dp_list16, dp_list_e3, dp_wide, dp_xwide, cols_wide, set_cols, site_cnt, site_rec, site_off, site_vec, site_cursor, redo, site_lists, read_dirty, cov3, lb, sr_store, brel_off, tasks2, res2, paths2, idx2, bc_idx, bc_rec, bc_win, left_list, fix_list, tasks3, res3, src3, bnd_flag, bnd_list, bnd_patch, bnd_bytes, changed, pair_read, wide_list,
        cols, tmp, gwin_off, gwin_read, sk_ends, sk_low, sk_high, hits, hits_packed, set_hits, ovl_prev, exact_flag, inexact_list, upair_base, upair_tab, upair_tab_sw, ovl_c, gwin_tab, cwin, cwin_len, warn, thr_tab, pieces, contig_out, new_len, unpack_off;
    std::vector<uint32_t> h_store;   // the corrected reads of the sets whose layout compares bases (kept between calls: no 96 MB zero-fill a step)
    int occ_sb = 0, occ_fr[3] = {0, 0, 0}, occ_wide = 0;   // blocks per CU of the persistent K6 kernels (hipOccupancyMaxActiveBlocksPerMultiprocessor: asked once)
    ChainArgs last_chain;   // arguments of the last k_chain launch (the final pass re-chains a few pairs with another bandwidth)
    std::vector<size_t> sk_rec, uq_rec, chain_rec, bpm_rec, rescue_rec, fast_rec, dp_rec, cons_rec, bnd_rec, bpm2_rec, fast2_rec, dp2_rec, bndc_rec, bc_bpm_rec, bc_fast_rec, bc_dp_rec;   // KTimes records of the k_chain launches of this batch (their byte counts are filled in at the end)
    // state of the last run (for fsv_asm_fetch_reads / stats)
    std::vector<uint32_t> h_word_off;
    std::vector<int32_t> h_len;
    const uint32_t *cur_store = nullptr;
    uint32_t n_reads = 0;
    fsv_asm_stats stats;
    KTimes kt;
    void *h_pin = nullptr; size_t h_pin_cap = 0; // pinned host staging (exact hits)
    // only the chunking budget reads this list (what this context already holds): a buffer missing from it is undercounted there, not leaked
    std::vector<const DevBuf *> all() const
    {
        return {&store[0], &store[1], &cols_sb, &contig_all, &word_off, &len, &set_start, &read_set, &pair_base, &mz, &mz_off, &mz_cnt, &ovl, &tasks, &res, &paths,
                &counters, &dp_list, &dp_list2, &dp_list3, &dp_list16, &dp_list_e3, &dp_wide, &dp_xwide, &cols_wide, &set_cols, &site_cnt, &site_rec, &site_off, &site_vec, &site_cursor, &redo, &site_lists, &read_dirty, &cov3, &lb, &sr_store, &brel_off, &tasks2, &res2, &paths2, &idx2, &bc_idx, &bc_rec, &bc_win, &left_list, &fix_list, &tasks3, &res3, &src3, &bnd_flag, &bnd_list, &bnd_patch, &bnd_bytes, &changed, &pair_read, &wide_list, &cols, &tmp, &gwin_off, &gwin_read, &sk_ends, &sk_low, &sk_high, &hits, &hits_packed, &set_hits, &ovl_prev, &exact_flag, &inexact_list, &upair_base, &upair_tab, &upair_tab_sw, &ovl_c, &gwin_tab, &cwin, &cwin_len, &warn, &thr_tab, &pieces, &contig_out, &new_len, &unpack_off};
    }
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
static inline uint64_t mz_slots(int64_t len, int) { return (uint64_t)len + 64; }

int make_geometry(fsv_ctx *ctx, const Batch &B, const std::vector<int32_t> &len, Geometry &G, int mz_w = 51, const std::vector<uint32_t> *fixed_mz_off = nullptr)
{
    G.word_off.assign(B.n_reads + 1, 0); G.mz_off.assign(B.n_reads + 1, 0); G.gwin_off.assign(B.n_reads + 1, 0);
    G.max_words = 1;
    uint64_t w = 0, m = 0, g = 0;
    for (uint32_t r = 0; r < B.n_reads; r++) {
        G.word_off[r] = (uint32_t)w; G.mz_off[r] = (uint32_t)m; G.gwin_off[r] = (uint32_t)g;
        w += (uint64_t)(len[r] + 15) / 16;
        G.max_words = std::max<uint32_t>(G.max_words, (uint32_t)((len[r] + 15) / 16));
        m += mz_slots(len[r], mz_w);
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

// sketch + per-read index + chaining on the current store; fills ws.ovl (and ws.tasks when emit_tasks).  Nothing here waits
// for the GPU: launches are sized from the read lengths the host already has, counts stay in the round's counter slot `ct`.
int overlap_stage(fsv_ctx *ctx, AsmWs &W, const Batch &B, const Geometry &G, const uint32_t *store, const fsv_asm_params &P, int bw,
                  bool emit_tasks, uint32_t task_cap, uint32_t *ct, bool short_reads, bool wide_anchors, int w, const uint32_t *only_changed = nullptr)
{
    Span ts(ctx, W.kt, ST_SKETCH);
    TRY(ensure(ctx, W.mz, (size_t)G.mz_off[B.n_reads] * sizeof(fsv_mz)));
    TRY(ensure(ctx, W.mz_cnt, (size_t)B.n_reads * 4));
    TRY(ensure(ctx, W.ovl, (size_t)std::max(1u, B.n_pairs) * sizeof(fsv_ovl)));
    TRY(ensure(ctx, W.ovl_c, (size_t)std::max(1u, B.n_pairs) * sizeof(uint4)));
    W.sk_rec.push_back(W.kt.begin(ctx, KN_SKETCH, 0));    // bytes: filled in from the round's counters (minimizers produced, bases sketched)
    if (!(only_changed && (P.k & 1))) FSV_HIP(ctx, hipMemsetAsync(W.mz_cnt.p, 0, (size_t)B.n_reads * 4, ctx->stream));
    // (with only_changed the unchanged reads keep their count; the kernel zeroes the others itself)
    if (!(P.k & 1)) only_changed = nullptr; // the replay kernel (even k) always sketches every read
    if (P.k & 1) {
        // position-parallel sketch (odd k): per-read scratch for run ends (4 B / base) and two bit planes, planes zeroed per launch
        const size_t total_words = G.word_off[B.n_reads];
        TRY(ensure(ctx, W.sk_ends, (total_words * 16 + 64) * 4));
        TRY(ensure(ctx, W.sk_low, (total_words + B.n_reads + 8) * 4));
        TRY(ensure(ctx, W.sk_high, (total_words + B.n_reads + 8) * 4));
        FSV_HIP(ctx, hipMemsetAsync(W.sk_low.p, 0, (total_words + B.n_reads + 8) * 4, ctx->stream));
        FSV_HIP(ctx, hipMemsetAsync(W.sk_high.p, 0, (total_words + B.n_reads + 8) * 4, ctx->stream));
        hipLaunchKernelGGL(k_sketch_fast, dim3(B.n_reads), dim3(256), 0, ctx->stream, store, (const uint32_t *)W.word_off.p,
                           (const int32_t *)W.len.p, (const uint32_t *)W.mz_off.p, (fsv_mz *)W.mz.p, (uint32_t *)W.mz_cnt.p, B.n_reads, w, P.k,
                           P.hpc, (uint32_t *)W.warn.p, (const uint8_t *)nullptr, (uint32_t *)W.sk_ends.p, (uint32_t *)W.sk_low.p, (uint32_t *)W.sk_high.p,
                           only_changed);
        FSV_HIP(ctx, hipGetLastError());
    } else {
        const uint32_t lds_words = std::min<uint32_t>(G.max_words, 8192u);
        FSV_HIP(ctx, hipFuncSetAttribute((const void *)k_sketch, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sketch_lds_bytes(w, lds_words)));
        hipLaunchKernelGGL(k_sketch, dim3(B.n_reads), dim3(64), sketch_lds_bytes(w, lds_words), ctx->stream, store, (const uint32_t *)W.word_off.p,
                           (const int32_t *)W.len.p, (const uint32_t *)W.mz_off.p, (fsv_mz *)W.mz.p, (uint32_t *)W.mz_cnt.p, B.n_reads, w, P.k,
                           P.hpc, (uint32_t *)W.warn.p, (const uint8_t *)nullptr, w, lds_words);
        FSV_HIP(ctx, hipGetLastError());
    }
    W.kt.end(ctx);
    // the sort in k_uniq holds a read's minimizers in LDS (16 B per entry): one instantiation for lists up to 1 024 entries (many
    // reads per CU), one for longer ones; each launch skips the reads of the other size class, so the host need not know the
    // longest list of the batch (round 1 read the counts back to choose)
    unsigned long long *mz_total = (unsigned long long *)(ct + CT_MZ_LO);
    W.uq_rec.push_back(W.kt.begin(ctx, KN_UNIQ, 0));
    hipLaunchKernelGGL(k_uniq<1024>, dim3(B.n_reads), dim3(256), 0, ctx->stream, (fsv_mz *)W.mz.p, (const uint32_t *)W.mz_off.p,
                       (uint32_t *)W.mz_cnt.p, (uint32_t *)W.warn.p, only_changed, 0u, 1024u, mz_total);
    FSV_HIP(ctx, hipGetLastError());
    if (G.max_words * 16u > 1024u) {   // at most one minimizer per base: shorter reads cannot have a longer list
        hipLaunchKernelGGL(k_uniq_walk<FSV_UQ_MAX>, dim3(std::min<uint32_t>(B.n_reads, 2u * (uint32_t)ctx->n_cu)), dim3(256), 0, ctx->stream, (fsv_mz *)W.mz.p, (const uint32_t *)W.mz_off.p,
                           (uint32_t *)W.mz_cnt.p, (uint32_t *)W.warn.p, only_changed, 1024u, 0xffffffffu, mz_total, B.n_reads);
        FSV_HIP(ctx, hipGetLastError());
    }
    W.kt.end(ctx);
    ts.stop();
    if (B.n_pairs == 0) return FSV_OK;
    Span tc(ctx, W.kt, ST_CHAIN);
    ChainArgs A;
    A.store = store; A.word_off = (const uint32_t *)W.word_off.p; A.read_len = (const int32_t *)W.len.p;
    A.set_start = (const uint32_t *)W.set_start.p; A.pair_base = (const uint32_t *)W.pair_base.p; A.upair_base = (const uint32_t *)W.upair_base.p;
    A.mz = (const fsv_mz *)W.mz.p; A.mz_off = (const uint32_t *)W.mz_off.p; A.mz_cnt = (const uint32_t *)W.mz_cnt.p;
    A.ovl = (fsv_ovl *)W.ovl.p; A.tasks = (fsv_wtask *)W.tasks.p; A.task_counter = ct + CT_TASKS; A.task_cap = task_cap;
    A.overflow = ct + CT_OVERFLOW; A.warn = (uint32_t *)W.warn.p; A.set_cols = (uint32_t *)W.set_cols.p; A.thr_tab = (const uint8_t *)W.thr_tab.p;
    A.n_sets = B.n_sets; A.k_score = P.k; A.min_anchors = P.min_anchors; A.min_ovlp = P.min_ovlp; A.bw = bw; A.emit_tasks = emit_tasks ? 1 : 0; A.primary_only = 0;
    // LDS per pair: the anchor arrays for FSV_AMAX entries -- 12 B each in the compact layout (every read of the batch below
    // 65 536 bases), so the tile no longer has to be cut to the batch's longest list to keep several pairs per CU
    A.upair_tab = (const uint4 *)W.upair_tab.p; A.pair_list = nullptr; A.n_list_dev = nullptr;
    A.amax = wide_anchors ? FSV_AMAX_WIDE : FSV_AMAX;
    // a pair whose lists both exceed the tile is set aside and chained with the large tile afterwards (reads above ~25 kb)
    A.wide_list = nullptr; A.n_wide = nullptr;
    if (!wide_anchors) {
        TRY(ensure(ctx, W.wide_list, (size_t)B.n_upairs * 4 + 16));
        A.wide_list = (uint32_t *)W.wide_list.p; A.n_wide = ct + CT_WIDE;
    }
    A.stamps = nullptr;
    if (getenv("FSV_CHAIN_STAMPS")) {   // diagnostic: where a k_chain wave spends its cycles (never in a measured run)
        TRY(ensure(ctx, W.tmp, 128));
        FSV_HIP(ctx, hipMemsetAsync(W.tmp.p, 0, 128, ctx->stream));
        A.stamps = (unsigned long long *)W.tmp.p;
    }
    // algorithmic bytes of the launch are filled in when the batch ends (they need the counts this launch leaves on the device)
    W.chain_rec.push_back(W.kt.begin(ctx, KN_CHAIN, 0));
    const uint32_t n_chunks = ((B.n_upairs + FSV_CHAIN_CH - 1) / FSV_CHAIN_CH + 7u) & ~7u;   // (xcd_block: a multiple of eight blocks)
    if (short_reads) { TRY(lds_opt_in(ctx, k_chain_chunks<true>, chain_lds_bytes(true, A.amax))); hipLaunchKernelGGL(k_chain_chunks<true>, dim3(n_chunks), dim3(64), chain_lds_bytes(true, A.amax), ctx->stream, A, B.n_upairs); }
    else { TRY(lds_opt_in(ctx, k_chain_chunks<false>, chain_lds_bytes(false, A.amax))); hipLaunchKernelGGL(k_chain_chunks<false>, dim3(n_chunks), dim3(64), chain_lds_bytes(false, A.amax), ctx->stream, A, B.n_upairs); }
    FSV_HIP(ctx, hipGetLastError());
    if (A.wide_list) {
        ChainArgs AW = A;
        AW.amax = short_reads ? FSV_AMAX_WIDE : FSV_AMAX_WIDE_LONG; AW.stamps = nullptr;   // (the kernel walks AW.wide_list)
        const uint32_t gridw = std::min<uint32_t>(B.n_upairs, 2u * (uint32_t)ctx->n_cu);
        if (short_reads) { TRY(lds_opt_in(ctx, k_chain_wide_list<true>, chain_lds_bytes(true, AW.amax))); hipLaunchKernelGGL(k_chain_wide_list<true>, dim3(gridw), dim3(64), chain_lds_bytes(true, AW.amax), ctx->stream, AW); }
        else { TRY(lds_opt_in(ctx, k_chain_wide_list<false>, chain_lds_bytes(false, AW.amax))); hipLaunchKernelGGL(k_chain_wide_list<false>, dim3(gridw), dim3(64), chain_lds_bytes(false, AW.amax), ctx->stream, AW); }
        FSV_HIP(ctx, hipGetLastError());
    }
    W.kt.end(ctx);
    if (A.stamps) {
        unsigned long long h[16];
        FSV_HIP(ctx, hipMemcpyAsync(h, W.tmp.p, 128, hipMemcpyDeviceToHost, ctx->stream));
        FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
        static const char *nm[7] = {"stage lists", "lookups", "exit: few anchors", "compaction", "chain DP", "best + walk", "tasks + records"};
        fprintf(stderr, "[fsv] k_chain (%u pairs, tasks %d):", B.n_upairs, emit_tasks ? 1 : 0);
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

// K5 + K6 on caller-supplied tasks: the same kernels fsv_assemble_batch drives, with every task treated as belonging to an
// accepted overlap
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
    DevBuf d_store, d_tasks, d_res, d_paths, d_ovl, d_list, d_list2, d_list3, d_list16, d_list_e3, d_wide, d_xwide, d_cnt, d_cols, d_cols_sb, d_cols_wide;
    {
        std::vector<fsv_wtask> t(tasks, tasks + n_tasks);
        for (auto &x : t) x.ovl = 0;
        fsv_ovl o; memset(&o, 0, sizeof(o)); o.valid = 1; o.is_match = 1;
        TRY(ensure(ctx, d_store, store_words * 4 + 64));
        FSV_HIP(ctx, hipMemsetAsync(d_store.p, 0, store_words * 4 + 64, ctx->stream));
        FSV_HIP(ctx, hipMemcpyAsync(d_store.p, store, store_words * 4, hipMemcpyHostToDevice, ctx->stream));
        TRY(upload(ctx, d_tasks, t));
        TRY(upload(ctx, d_ovl, std::vector<fsv_ovl>{o}));
        TRY(ensure(ctx, d_res, (size_t)n_tasks * sizeof(fsv_wres)));
        TRY(ensure(ctx, d_paths, (size_t)n_tasks * sizeof(fsv_wpath)));
        for (DevBuf *b : {&d_list, &d_list2, &d_list3, &d_list16, &d_list_e3, &d_wide, &d_xwide}) TRY(ensure(ctx, *b, (size_t)n_tasks * 4));
        TRY(ensure(ctx, d_cnt, CT_SLOT * 4));
        uint32_t *ct = (uint32_t *)d_cnt.p;
        FSV_HIP(ctx, hipMemsetAsync(d_cnt.p, 0, CT_SLOT * 4, ctx->stream));
        FSV_HIP(ctx, hipMemsetAsync(d_paths.p, 0, (size_t)n_tasks * sizeof(fsv_wpath), ctx->stream));
        // the same launches as a correction round of fsv_assemble_batch (device-side list lengths, no host round trip in between)
        TRY(fsv_bpm_windows_dev_n(ctx, (const uint32_t *)d_store.p, (const fsv_wtask *)d_tasks.p, n_tasks, nullptr, (fsv_wres *)d_res.p, k_cap));
        const PathLists lists{{(uint32_t *)d_list16.p, (uint32_t *)d_list.p, (uint32_t *)d_list_e3.p, (uint32_t *)d_list2.p, (uint32_t *)d_list3.p, (uint32_t *)d_wide.p, (uint32_t *)d_xwide.p},
                              {ct + CT_DP_SB16, ct + CT_DP, ct + CT_DP_FR3, ct + CT_DP_SB, ct + CT_DP_GEN, ct + CT_DP_WIDE, ct + CT_DP_XW}};
        hipLaunchKernelGGL(k_path_fast, dim3((fsv_grid_for(n_tasks, 256) + 7u) & ~7u), dim3(256), 0, ctx->stream, (const uint32_t *)d_store.p, (const fsv_ovl *)d_ovl.p,
                           (const fsv_wtask *)d_tasks.p, (const fsv_wres *)d_res.p, n_tasks, (fsv_wpath *)d_paths.p, lists, true, (const uint32_t *)nullptr);
        FSV_HIP(ctx, hipGetLastError());
        const uint32_t grid = std::min<uint32_t>(fsv_grid_for(n_tasks, 64), 8u * (uint32_t)ctx->n_cu);
        TRY(ensure(ctx, d_cols_sb, (size_t)grid * FSV_SB_QUADS * 64 * sizeof(uint4)));
        hipLaunchKernelGGL(k_path_sb<false>, dim3(grid), dim3(64), 0, ctx->stream, (const uint32_t *)d_store.p, (const fsv_wtask *)d_tasks.p, (const fsv_wres *)d_res.p,
                           (const uint32_t *)d_list2.p, (const uint32_t *)(ct + CT_DP_SB), (fsv_wpath *)d_paths.p, (uint4 *)d_cols_sb.p, (unsigned long long *)nullptr);
        FSV_HIP(ctx, hipGetLastError());
        hipLaunchKernelGGL(k_path_fr<1>, dim3(grid), dim3(64), 0, ctx->stream, (const uint32_t *)d_store.p, (const fsv_wtask *)d_tasks.p, (const fsv_wres *)d_res.p,
                           (const uint32_t *)d_list16.p, (const uint32_t *)(ct + CT_DP_SB16), (fsv_wpath *)d_paths.p);
        hipLaunchKernelGGL(k_path_fr<2>, dim3(grid), dim3(64), 0, ctx->stream, (const uint32_t *)d_store.p, (const fsv_wtask *)d_tasks.p, (const fsv_wres *)d_res.p,
                           (const uint32_t *)d_list.p, (const uint32_t *)(ct + CT_DP), (fsv_wpath *)d_paths.p);
        hipLaunchKernelGGL(k_path_fr<3>, dim3(grid), dim3(64), 0, ctx->stream, (const uint32_t *)d_store.p, (const fsv_wtask *)d_tasks.p, (const fsv_wres *)d_res.p,
                           (const uint32_t *)d_list_e3.p, (const uint32_t *)(ct + CT_DP_FR3), (fsv_wpath *)d_paths.p);
        FSV_HIP(ctx, hipGetLastError());
        const uint32_t gridg = std::min<uint32_t>(fsv_grid_for(n_tasks, 64), 2u * (uint32_t)ctx->n_cu);
        TRY(ensure(ctx, d_cols, (size_t)gridg * 64 * (FSV_WINDOW + 2) * 3 * 8));
        hipLaunchKernelGGL(k_path_dp<uint32_t>, dim3(gridg), dim3(64), 0, ctx->stream, (const uint32_t *)d_store.p, (const fsv_wtask *)d_tasks.p,
                           (const uint32_t *)d_list3.p, 0u, 0u, (fsv_wpath *)d_paths.p, (uint32_t *)d_cols.p, gridg * 64, (const uint32_t *)(ct + CT_DP_GEN));
        FSV_HIP(ctx, hipGetLastError());
        hipLaunchKernelGGL(k_path_dp<uint64_t>, dim3(gridg), dim3(64), 0, ctx->stream, (const uint32_t *)d_store.p, (const fsv_wtask *)d_tasks.p,
                           (const uint32_t *)d_wide.p, 0u, 0u, (fsv_wpath *)d_paths.p, (uint64_t *)d_cols.p, gridg * 64, (const uint32_t *)(ct + CT_DP_WIDE));
        FSV_HIP(ctx, hipGetLastError());
        if (kmax > FSV_K_MAX) {
            const uint32_t gridw = std::min<uint32_t>(fsv_grid_for(n_tasks, 64), 4u * (uint32_t)ctx->n_cu);
            TRY(ensure(ctx, d_cols_wide, (size_t)gridw * FSV_WINDOW * 2 * FSV_WL * 64 * 4));
            hipLaunchKernelGGL(k_path_wide, dim3(gridw), dim3(64), 0, ctx->stream, (const uint32_t *)d_store.p, (const fsv_wtask *)d_tasks.p, (const fsv_wres *)d_res.p,
                               (const uint32_t *)d_xwide.p, (const uint32_t *)(ct + CT_DP_XW), (fsv_wpath *)d_paths.p, (uint32_t *)d_cols_wide.p, k_cap);
            FSV_HIP(ctx, hipGetLastError());
        }
        FSV_HIP(ctx, hipMemcpyAsync(res, d_res.p, (size_t)n_tasks * sizeof(fsv_wres), hipMemcpyDeviceToHost, ctx->stream));
        FSV_HIP(ctx, hipMemcpyAsync(paths, d_paths.p, (size_t)n_tasks * sizeof(fsv_wpath), hipMemcpyDeviceToHost, ctx->stream));
        FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return FSV_OK;
}

extern "C" int fsv_asm_last_stats(const fsv_ctx *ctx, fsv_asm_stats *out)
{
    if (!ctx || !out || !ctx->asm_ws) return FSV_EINVAL;
    *out = ((const AsmWs *)ctx->asm_ws)->stats;
    return FSV_OK;
}

// one chunk of read sets through the whole assembly (what fsv_assemble_batch was before it learnt to split a batch)
// K6 for a task list: the fast paths, then the DP kernels on what is left (the lists and their counters live in the counter row ct).
// Used for the window tasks of a round and, with second_round, for the junction tasks of its second consensus pass.
static int path_stage(fsv_ctx *ctx, AsmWs &W, const uint32_t *store, const fsv_wtask *tasks, const fsv_wres *res, fsv_wpath *paths, uint32_t task_cap,
                      const uint32_t *n_tasks_dev, uint32_t *ct, int round, bool wide_bands, const fsv_asm_params &P, int pass_kind)
{
    // pass_kind 0: the round's window tasks, 1: the junction tasks of its second consensus pass, 2: the junction cigars of the partition
    { const size_t rec_ = W.kt.begin(ctx, KN_PATH_FAST, 0); (pass_kind == 0 ? W.fast_rec : pass_kind == 1 ? W.fast2_rec : W.bc_fast_rec).push_back(rec_); }
    const bool fix = pass_kind == 0 && !wide_bands;      // fix_boundary: the windows' final cigars only (not the junction alignments)
    if (fix) TRY(ensure(ctx, W.fix_list, (size_t)task_cap * 4));
    const PathLists lists{{(uint32_t *)W.dp_list16.p, (uint32_t *)W.dp_list.p, (uint32_t *)W.dp_list_e3.p, (uint32_t *)W.dp_list2.p, (uint32_t *)W.dp_list3.p, (uint32_t *)W.dp_wide.p, (uint32_t *)W.dp_xwide.p,
                           fix ? (uint32_t *)W.fix_list.p : (uint32_t *)nullptr},
                          {ct + CT_DP_SB16, ct + CT_DP, ct + CT_DP_FR3, ct + CT_DP_SB, ct + CT_DP_GEN, ct + CT_DP_WIDE, ct + CT_DP_XW, fix ? ct + CT_FIX : (uint32_t *)nullptr}};
    hipLaunchKernelGGL(k_path_fast, dim3((fsv_grid_for(task_cap, 256) + 7u) & ~7u), dim3(256), 0, ctx->stream, store, (const fsv_ovl *)W.ovl.p,
                       tasks, res, task_cap, paths, lists, false, n_tasks_dev);
    FSV_HIP(ctx, hipGetLastError());
    W.kt.end(ctx);
    // what the fast paths left: distance <= 3 is walked without the DP matrix (k_path_fr), <= FSV_SB_MAXERR by the sub-band kernel,
    // the rest by the general one
    { const size_t rec_ = W.kt.begin(ctx, KN_PATH_DP, 0); (pass_kind == 0 ? W.dp_rec : pass_kind == 1 ? W.dp2_rec : W.bc_dp_rec).push_back(rec_); }
    // persistent grids: as many blocks as the device holds at once, each striding through its list, so the column scratch
    // is a fixed few hundred MB whatever the number of windows
    {
        if (!W.occ_sb) FSV_HIP(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&W.occ_sb, k_path_sb<false>, 64, 0));
        const int per_cu = W.occ_sb;
        const uint32_t grid = std::min<uint32_t>(fsv_grid_for(task_cap, 64), (uint32_t)std::max(1, per_cu) * (uint32_t)ctx->n_cu);
        TRY(ensure(ctx, W.cols_sb, (size_t)grid * FSV_SB_QUADS * 64 * sizeof(uint4)));
        if (getenv("FSV_K6_STAMPS")) {   // diagnostic: where a k_path_sb wave spends its cycles (never in a measured run)
            DevBuf &sb = W.tmp;
            TRY(ensure(ctx, sb, 64));
            FSV_HIP(ctx, hipMemsetAsync(sb.p, 0, 64, ctx->stream));
            hipLaunchKernelGGL(k_path_sb<true>, dim3(grid), dim3(64), 0, ctx->stream, store, tasks, res,
                               (const uint32_t *)W.dp_list2.p, (const uint32_t *)(ct + CT_DP_SB), paths, (uint4 *)W.cols_sb.p, (unsigned long long *)sb.p);
            unsigned long long h[4] = {0, 0, 0, 0};
            FSV_HIP(ctx, hipMemcpyAsync(h, sb.p, 32, hipMemcpyDeviceToHost, ctx->stream));
            FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
            fprintf(stderr, "[fsv] k_path_sb round %d: %llu waves, cycles per wave: forward %.0f, walk %.0f, finish %.0f (grid %u)\n", round, h[3],
                    h[3] ? (double)h[0] / h[3] : 0.0, h[3] ? (double)h[1] / h[3] : 0.0, h[3] ? (double)h[2] / h[3] : 0.0, grid);
        } else
        hipLaunchKernelGGL(k_path_sb<false>, dim3(grid), dim3(64), 0, ctx->stream, store, tasks, res,
                           (const uint32_t *)W.dp_list2.p, (const uint32_t *)(ct + CT_DP_SB), paths, (uint4 *)W.cols_sb.p, (unsigned long long *)nullptr);
        FSV_HIP(ctx, hipGetLastError());
        // distance <= 3 (nine in ten): walked without the matrix, a launch per distance
        {
            const bool stamps = getenv("FSV_K6_STAMPS") != nullptr;    // diagnostic, never in a measured run
            auto fr = [&](auto kern, int e, const DevBuf &list, uint32_t *cnt) -> int {
                int &pf = W.occ_fr[e - 1];
                if (!pf || stamps) FSV_HIP(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&pf, kern, 64, 0));
                const uint32_t gridf = std::min<uint32_t>(fsv_grid_for(task_cap, 64), (uint32_t)std::max(1, pf) * (uint32_t)ctx->n_cu);
                if (stamps) { TRY(ensure(ctx, W.tmp, 64)); FSV_HIP(ctx, hipMemsetAsync(W.tmp.p, 0, 64, ctx->stream)); }
                hipLaunchKernelGGL(kern, dim3(gridf), dim3(64), 0, ctx->stream, store, tasks, res, (const uint32_t *)list.p, (const uint32_t *)cnt, paths,
                                   (unsigned long long *)(stamps ? W.tmp.p : nullptr));
                FSV_HIP(ctx, hipGetLastError());
                if (stamps) {
                    unsigned long long h[4] = {0, 0, 0, 0};
                    uint32_t nl = 0;
                    FSV_HIP(ctx, hipMemcpyAsync(h, W.tmp.p, 32, hipMemcpyDeviceToHost, ctx->stream));
                    FSV_HIP(ctx, hipMemcpyAsync(&nl, cnt, 4, hipMemcpyDeviceToHost, ctx->stream));
                    FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
                    fprintf(stderr, "[fsv] k_path_fr<%d> round %d: %u windows, %llu waves (%d per CU), cycles per wave: table %.0f, walk %.0f, finish %.0f\n", e, round, nl, h[3], pf,
                            h[3] ? (double)h[0] / h[3] : 0.0, h[3] ? (double)h[1] / h[3] : 0.0, h[3] ? (double)h[2] / h[3] : 0.0);
                }
                return FSV_OK;
            };
            if (stamps) {
                TRY(fr(k_path_fr<1, true>, 1, W.dp_list16, ct + CT_DP_SB16));
                TRY(fr(k_path_fr<2, true>, 2, W.dp_list, ct + CT_DP));
                TRY(fr(k_path_fr<3, true>, 3, W.dp_list_e3, ct + CT_DP_FR3));
            } else {
                TRY(fr(k_path_fr<1>, 1, W.dp_list16, ct + CT_DP_SB16));
                TRY(fr(k_path_fr<2>, 2, W.dp_list, ct + CT_DP));
                TRY(fr(k_path_fr<3>, 3, W.dp_list_e3, ct + CT_DP_FR3));
            }
        }
        // the general kernel's lists are short (rescue windows, distances above 7): two blocks per CU are plenty
        const uint32_t gridg = std::min<uint32_t>(fsv_grid_for(task_cap, 64), 2u * (uint32_t)ctx->n_cu), stride = gridg * 64;
        TRY(ensure(ctx, W.cols, (size_t)stride * (FSV_WINDOW + 2) * 3 * sizeof(uint64_t)));
        hipLaunchKernelGGL(k_path_dp<uint32_t>, dim3(gridg), dim3(64), 0, ctx->stream, store, tasks,
                           (const uint32_t *)W.dp_list3.p, 0u, 0u, paths, (uint32_t *)W.cols.p, stride, (const uint32_t *)(ct + CT_DP_GEN));
        FSV_HIP(ctx, hipGetLastError());
        hipLaunchKernelGGL(k_path_dp<uint64_t>, dim3(gridg), dim3(64), 0, ctx->stream, store, tasks,
                           (const uint32_t *)W.dp_wide.p, 0u, 0u, paths, (uint64_t *)W.cols.p, stride, (const uint32_t *)(ct + CT_DP_WIDE));
        FSV_HIP(ctx, hipGetLastError());
        if (wide_bands) {
            // bands above 63 rows: every gapped window of an ONT-profile batch; 1.15 MB of column scratch per persistent block
            if (!W.occ_wide) FSV_HIP(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&W.occ_wide, k_path_wide, 64, 0));
            const int pc = W.occ_wide;
            const uint32_t gridw = std::min<uint32_t>(fsv_grid_for(task_cap, 64), (uint32_t)std::max(1, std::min(pc, 12)) * (uint32_t)ctx->n_cu);
            TRY(ensure(ctx, W.cols_wide, (size_t)gridw * FSV_WINDOW * 2 * FSV_WL * 64 * 4));
            hipLaunchKernelGGL(k_path_wide, dim3(gridw), dim3(64), 0, ctx->stream, store, tasks, res,
                               (const uint32_t *)W.dp_xwide.p, (const uint32_t *)(ct + CT_DP_XW), paths, (uint32_t *)W.cols_wide.p, P.k_cap);
            FSV_HIP(ctx, hipGetLastError());
        }
    }
    if (fix) {
        // fix_boundary (Correct.cpp:1676): the few windows whose alignment may touch the edge of its band (k_path_fast listed them)
        const uint32_t gridf = std::min<uint32_t>(fsv_grid_for(task_cap, 64), 8u * (uint32_t)ctx->n_cu);
        hipLaunchKernelGGL(k_fix_boundary, dim3(gridf), dim3(64), 0, ctx->stream, store, (const uint32_t *)W.fix_list.p, (const uint32_t *)(ct + CT_FIX),
                           const_cast<fsv_wtask *>(tasks), const_cast<fsv_wres *>(res), paths, P.k_cap, ct + CT_FIXED);
        FSV_HIP(ctx, hipGetLastError());
    }
    W.kt.end(ctx);
    return FSV_OK;
}

// The second consensus pass of a round (process_boundary, Correct.cpp:4453): see asm_kernels.h "second consensus pass".
// Runs between the windows' consensus (cwin / cwin_len final for the first pass) and k_newlen; leaves cwin / cwin_len patched.
static int second_pass(fsv_ctx *ctx, AsmWs &W, const Batch &B, const Geometry &G, const uint32_t *store, const fsv_asm_params &P, const ConsArgs &C,
                       uint32_t n_gwin, uint32_t task_cap, const uint32_t *n_tasks_dev, uint32_t *ct2, int round, bool wide_bands)
{
    // where window g starts in the first pass's result, and that result as a 2-bit store behind a copy of the round's reads
    TRY(ensure(ctx, W.lb, (size_t)std::max(1u, n_gwin) * 4));
    W.bnd_rec.push_back(W.kt.begin(ctx, KN_BND, 0));
    hipLaunchKernelGGL(k_newlen, dim3(fsv_grid_for(B.n_reads, 256)), dim3(256), 0, ctx->stream, (const uint32_t *)W.gwin_off.p,
                       (const uint16_t *)W.cwin_len.p, B.n_reads, (int32_t *)W.new_len.p, (uint32_t *)W.lb.p);
    FSV_HIP(ctx, hipGetLastError());
    const uint32_t a_words = G.word_off[B.n_reads];
    std::vector<uint32_t> brel(B.n_reads + 1, 0);
    for (uint32_t r = 0; r < B.n_reads; r++) {
        const uint64_t nx = (uint64_t)brel[r] + (uint64_t)(G.gwin_off[r + 1] - G.gwin_off[r]) * (FSV_CW_STRIDE / 16) + 2;
        if (nx + a_words >= (1ull << 32)) return fsv_fail(ctx, FSV_EUNSUP, "second consensus pass: store larger than 2^32 words; split the batch");
        brel[r + 1] = (uint32_t)nx;
    }
    const uint32_t b_words = brel[B.n_reads];
    TRY(ensure(ctx, W.sr_store, ((size_t)a_words + b_words + 16) * 4));
    FSV_HIP(ctx, hipMemcpyAsync(W.sr_store.p, store, (size_t)a_words * 4, hipMemcpyDeviceToDevice, ctx->stream));
    TRY(upload(ctx, W.brel_off, brel));
    uint32_t *store2 = (uint32_t *)W.sr_store.p;
    hipLaunchKernelGGL(k_repack, dim3(B.n_reads), dim3(256), 0, ctx->stream, (const uint32_t *)W.gwin_off.p, (const uint32_t *)W.lb.p,
                       (const uint8_t *)W.cwin.p, (const uint32_t *)W.brel_off.p, (const int32_t *)W.new_len.p, B.n_reads, 0, store2 + a_words,
                       (const uint32_t *)W.read_dirty.p);
    FSV_HIP(ctx, hipGetLastError());
    FSV_HIP(ctx, hipMemsetAsync(store2 + a_words + b_words, 0, 32, ctx->stream));
    // junction tasks
    TRY(ensure(ctx, W.tasks2, (size_t)task_cap * sizeof(fsv_wtask)));
    TRY(ensure(ctx, W.res2, (size_t)task_cap * sizeof(fsv_wres)));
    TRY(ensure(ctx, W.paths2, (size_t)task_cap * sizeof(fsv_wpath)));
    TRY(ensure(ctx, W.idx2, (size_t)task_cap * 4));
    TRY(ensure(ctx, W.tasks3, (size_t)task_cap * sizeof(fsv_wtask)));
    TRY(ensure(ctx, W.res3, (size_t)task_cap * sizeof(fsv_wres)));
    TRY(ensure(ctx, W.src3, (size_t)task_cap * 4));
    TRY(ensure(ctx, W.bnd_flag, (size_t)(n_gwin + 2) * 4));
    TRY(ensure(ctx, W.bnd_list, (size_t)(n_gwin + 2) * 4));
    TRY(ensure(ctx, W.bnd_patch, (size_t)(n_gwin + 2) * sizeof(BndPatch)));
    TRY(ensure(ctx, W.bnd_bytes, (size_t)(n_gwin + 2) * FSV_CW_STRIDE));
    FSV_HIP(ctx, hipMemsetAsync(W.bnd_flag.p, 0, (size_t)(n_gwin + 2) * 4, ctx->stream));
    BndArgs A;
    A.tasks = (const fsv_wtask *)W.tasks.p; A.paths = (const fsv_wpath *)W.paths.p; A.n_tasks = n_tasks_dev;
    A.ovl_c = (const uint4 *)W.ovl_c.p; A.pair_base = (const uint32_t *)W.pair_base.p; A.set_start = (const uint32_t *)W.set_start.p; A.n_sets = B.n_sets; A.pair_read = (const uint32_t *)W.pair_read.p;
    A.gwin_off = (const uint32_t *)W.gwin_off.p; A.lb = (const uint32_t *)W.lb.p; A.cwin_len = (const uint16_t *)W.cwin_len.p;
    A.cov3 = (const uint8_t *)W.cov3.p; A.read_dirty = (const uint32_t *)W.read_dirty.p;
    A.brel_off = (const uint32_t *)W.brel_off.p; A.b_base = a_words; A.thr_tab = (const uint8_t *)W.thr_tab.p;
    A.tasks2 = (fsv_wtask *)W.tasks2.p; A.idx2 = (int32_t *)W.idx2.p; A.n_tasks2 = ct2 + CT_TASKS;
    A.bnd_flag = (uint32_t *)W.bnd_flag.p; A.bnd_list = (uint32_t *)W.bnd_list.p; A.n_bnd = ct2 + CT_B_LIST; A.store2 = store2;
    hipLaunchKernelGGL(k_bnd_tasks, dim3((fsv_grid_for(task_cap, 256) + 7u) & ~7u), dim3(256), 0, ctx->stream, A);
    FSV_HIP(ctx, hipGetLastError());
    W.kt.end(ctx);
    W.bpm2_rec.push_back(W.kt.begin(ctx, KN_BPM, 0));
    // K5, once more with the doubled threshold for the tasks without an alignment, K6
    TRY(fsv_bpm_windows_dev_n(ctx, store2, (const fsv_wtask *)W.tasks2.p, task_cap, ct2 + CT_TASKS, (fsv_wres *)W.res2.p, P.k_cap));
    hipLaunchKernelGGL(k_bnd_retry, dim3(fsv_grid_for(task_cap, 256)), dim3(256), 0, ctx->stream, (fsv_wtask *)W.tasks2.p, (const fsv_wres *)W.res2.p,
                       (const uint32_t *)(ct2 + CT_TASKS), (fsv_wtask *)W.tasks3.p, (uint32_t *)W.src3.p, ct2 + CT_B_RETRY, P.k_cap);
    FSV_HIP(ctx, hipGetLastError());
    TRY(fsv_bpm_windows_dev_n(ctx, store2, (const fsv_wtask *)W.tasks3.p, task_cap, ct2 + CT_B_RETRY, (fsv_wres *)W.res3.p, P.k_cap));
    hipLaunchKernelGGL(k_bnd_scatter, dim3(fsv_grid_for(task_cap, 256)), dim3(256), 0, ctx->stream, (fsv_wres *)W.res2.p, (const fsv_wres *)W.res3.p,
                       (const uint32_t *)W.src3.p, (const uint32_t *)(ct2 + CT_B_RETRY));
    FSV_HIP(ctx, hipGetLastError());
    W.kt.end(ctx);
    TRY(path_stage(ctx, W, store2, (const fsv_wtask *)W.tasks2.p, (const fsv_wres *)W.res2.p, (fsv_wpath *)W.paths2.p, task_cap, (const uint32_t *)(ct2 + CT_TASKS), ct2,
                   round, wide_bands, P, 1));
    // the junctions' consensus, handed to the windows as patches
    const uint32_t grid_l = std::min<uint32_t>(std::max(1u, n_gwin), (uint32_t)ctx->n_cu * 16);
    W.bndc_rec.push_back(W.kt.begin(ctx, KN_BND_CONS, 0));
    if (wide_bands) hipLaunchKernelGGL(k_bnd_consensus<FSV_EV_CAP_WIDE>, dim3(grid_l), dim3(64), 0, ctx->stream, C, A, (const fsv_wpath *)W.paths2.p, (const uint32_t *)store2,
                                       (BndPatch *)W.bnd_patch.p, (uint8_t *)W.bnd_bytes.p);
    else hipLaunchKernelGGL(k_bnd_consensus<FSV_EV_CAP>, dim3(grid_l), dim3(64), 0, ctx->stream, C, A, (const fsv_wpath *)W.paths2.p, (const uint32_t *)store2,
                            (BndPatch *)W.bnd_patch.p, (uint8_t *)W.bnd_bytes.p);
    FSV_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_bnd_apply, dim3(std::max(1u, n_gwin)), dim3(64), 0, ctx->stream, (const uint32_t *)W.gwin_read.p, (const uint32_t *)W.gwin_off.p,
                       (const BndPatch *)W.bnd_patch.p, (const uint8_t *)W.bnd_bytes.p, (const uint32_t *)W.bnd_flag.p, n_gwin, (uint8_t *)W.cwin.p,
                       (uint16_t *)W.cwin_len.p, (uint32_t *)W.changed.p, (uint32_t *)W.warn.p);
    FSV_HIP(ctx, hipGetLastError());
    W.kt.end(ctx);
    return FSV_OK;
}

static int assemble_chunk(fsv_ctx *ctx, const fsv_readsets *sets, const fsv_asm_params &P, fsv_contigs *out)
{
    AsmWs &W = *ws_get(ctx);
    memset(&W.stats, 0, sizeof(W.stats));
    W.kt.reset();
    W.sk_rec.clear(); W.uq_rec.clear(); W.chain_rec.clear(); W.bpm_rec.clear(); W.rescue_rec.clear(); W.fast_rec.clear(); W.dp_rec.clear(); W.cons_rec.clear();
    W.bnd_rec.clear(); W.bpm2_rec.clear(); W.fast2_rec.clear(); W.dp2_rec.clear(); W.bndc_rec.clear(); W.bc_bpm_rec.clear(); W.bc_fast_rec.clear(); W.bc_dp_rec.clear();
    const auto t_enter = std::chrono::steady_clock::now();

    Batch B;
    B.n_reads = sets->n_reads; B.n_sets = sets->n_sets;
    out->n_contigs = 0;
    out->off[0] = 0;
    for (uint32_t s = 0; s < B.n_sets; s++) out->set_status[s] = 0;
    if (B.n_reads == 0 || B.n_sets == 0) return FSV_OK;
    B.set_start.assign(sets->set_start, sets->set_start + B.n_sets + 1);
    if (B.set_start[0] != 0 || B.set_start[B.n_sets] != B.n_reads) return fsv_fail(ctx, FSV_EINVAL, "set_start must span [0, n_reads]");
    B.read_set.resize(B.n_reads); B.pair_base.resize(B.n_sets + 1); B.upair_base.resize(B.n_sets + 1);
    uint64_t np = 0;
    for (uint32_t s = 0; s < B.n_sets; s++) {
        if (B.set_start[s + 1] < B.set_start[s]) return fsv_fail(ctx, FSV_EINVAL, "set_start not monotone");
        uint64_t ns = B.set_start[s + 1] - B.set_start[s];
        B.pair_base[s] = (uint32_t)np;
        B.upair_base[s] = (uint32_t)(np / 2);
        np += ns > 1 ? ns * (ns - 1) : 0;
        for (uint32_t r = B.set_start[s]; r < B.set_start[s + 1]; r++) B.read_set[r] = s;
    }
    if (np >= (1ull << 31)) return fsv_fail(ctx, FSV_EUNSUP, "too many read pairs in one batch; split it");
    B.pair_base[B.n_sets] = (uint32_t)np; B.n_pairs = (uint32_t)np;
    B.upair_base[B.n_sets] = (uint32_t)(np / 2); B.n_upairs = (uint32_t)(np / 2);
    std::vector<int32_t> len(sets->read_len, sets->read_len + B.n_reads);
    for (uint32_t r = 0; r < B.n_reads; r++) if (len[r] < 1 || len[r] >= (1 << 24)) return fsv_fail(ctx, FSV_EUNSUP, "read length must be in [1, 2^24)");

    std::vector<uint8_t> thr(FSV_WINDOW + 1);
    for (int i = 0; i <= FSV_WINDOW; i++) thr[i] = thr_for_len_host(i, P.win_rate_pm);
    TRY(upload(ctx, W.thr_tab, thr));
    TRY(upload(ctx, W.set_start, B.set_start));
    TRY(upload(ctx, W.read_set, B.read_set));
    TRY(upload(ctx, W.pair_base, B.pair_base));
    TRY(upload(ctx, W.upair_base, B.upair_base));
    if (B.n_upairs) {
        TRY(ensure(ctx, W.upair_tab, (size_t)B.n_upairs * sizeof(uint4)));
        TRY(ensure(ctx, W.pair_read, (size_t)B.n_pairs * 4));
        hipLaunchKernelGGL(k_pair_tab, dim3((B.n_upairs + 255) / 256), dim3(256), 0, ctx->stream, (const uint32_t *)W.set_start.p,
                           (const uint32_t *)W.pair_base.p, (const uint32_t *)W.upair_base.p, B.n_sets, B.n_upairs, (uint4 *)W.upair_tab.p, (uint32_t *)W.pair_read.p);
        FSV_HIP(ctx, hipGetLastError());
    }
    TRY(ensure(ctx, W.warn, (size_t)B.n_reads * 4));
    FSV_HIP(ctx, hipMemsetAsync(W.warn.p, 0, (size_t)B.n_reads * 4, ctx->stream));
    // set_flags (FSV_SET_UNPHASED) no longer changes anything here: the haplotype partition runs for every read of every set, as in hifiasm

    // minimizer slots stay where they are for the whole call (a read grows by a few bases at most when it is corrected): the
    // final pass can then keep the lists of reads the last round did not change
    std::vector<uint32_t> mz_fixed(B.n_reads + 1, 0);
    {
        uint64_t m = 0;
        for (uint32_t r = 0; r < B.n_reads; r++) { mz_fixed[r] = (uint32_t)m; m += mz_slots((int64_t)len[r] + len[r] / 8 + 64, P.w); }
        if (m >= (1ull << 32)) return fsv_fail(ctx, FSV_EUNSUP, "batch too large for 32-bit offsets; split it");
        mz_fixed[B.n_reads] = (uint32_t)m;
    }
    Geometry G;
    TRY(make_geometry(ctx, B, len, G, P.w, &mz_fixed));
    // round 0 reads the caller's store through the caller's word offsets
    std::vector<uint32_t> woff0(B.n_reads + 1);
    for (uint32_t r = 0; r <= B.n_reads; r++) {
        if (sets->word_off[r] >= (1ull << 32)) return fsv_fail(ctx, FSV_EUNSUP, "store larger than 2^32 words; split the batch");
        woff0[r] = (uint32_t)sets->word_off[r];
    }
    G.word_off = woff0;
    const uint32_t *store = sets->store_dev;
    uint64_t reads_in_bytes = 0;
    const bool wide_bands = P.k_cap > FSV_K_MAX;   // the error model allows thresholds above hifiasm's 31: wide-band K5 / K6 / rescue
    bool short_reads = true;     // every read below 65 536 bases: k_chain's compact LDS layout
    for (uint32_t r = 0; r < B.n_reads; r++) { reads_in_bytes += (uint64_t)(len[r] + 3) / 4; if (len[r] >= 65536) short_reads = false; }
    // rows 0 .. n_rounds: the rounds and the final pass; rows n_rounds + 1 ..: the second consensus pass of every round; rows
    // 2 n_rounds + 2 ..: the junction cigars of every round's partition
    TRY(ensure(ctx, W.counters, (size_t)(3 * P.n_rounds + 2) * CT_SLOT * 4));
    FSV_HIP(ctx, hipMemsetAsync(W.counters.p, 0, (size_t)(3 * P.n_rounds + 2) * CT_SLOT * 4, ctx->stream));
    TRY(ensure(ctx, W.set_cols, (size_t)B.n_reads * 4));       // K5 columns per set, summed over the rounds (statistics)
    FSV_HIP(ctx, hipMemsetAsync(W.set_cols.p, 0, (size_t)B.n_reads * 4, ctx->stream));

    // every launch of a round is sized from what the host knows when the round starts (read lengths, the window-task bound);
    // counts the kernels produce stay in the round's counter slot.  One synchronisation per round is left: the corrected reads'
    // lengths, which the host turns into the next round's geometry -- the round's counters ride along with it.
    auto ct_of = [&](int slot) { return (uint32_t *)W.counters.p + (size_t)slot * CT_SLOT; };
    std::vector<uint32_t> h_ct((size_t)(3 * P.n_rounds + 2) * CT_SLOT, 0u);   // rows as on the device: rounds, final pass, the rounds' second passes
    for (int round = 0; round < P.n_rounds; round++) {
        uint32_t *ct = ct_of(round);
        TRY(upload(ctx, W.word_off, G.word_off));
        TRY(upload(ctx, W.len, len));
        TRY(upload(ctx, W.mz_off, G.mz_off));
        TRY(upload(ctx, W.gwin_off, G.gwin_off));
        TRY(upload(ctx, W.gwin_read, G.gwin_read));
        if (G.task_bound >= (1ull << 31)) return fsv_fail(ctx, FSV_EUNSUP, "window task bound exceeds 2^31; split the batch");
        const uint32_t task_cap = (uint32_t)std::max<uint64_t>(G.task_bound, 1);
        TRY(ensure(ctx, W.tasks, (size_t)task_cap * sizeof(fsv_wtask)));
        TRY(ensure(ctx, W.res, (size_t)task_cap * sizeof(fsv_wres)));
        TRY(ensure(ctx, W.paths, (size_t)task_cap * sizeof(fsv_wpath)));
        TRY(ensure(ctx, W.dp_list, (size_t)task_cap * 4));
        TRY(ensure(ctx, W.dp_list_e3, (size_t)task_cap * 4));
        TRY(ensure(ctx, W.dp_list2, (size_t)task_cap * 4));
        TRY(ensure(ctx, W.dp_list3, (size_t)task_cap * 4));
        TRY(ensure(ctx, W.dp_list16, (size_t)task_cap * 4));
        TRY(ensure(ctx, W.dp_wide, (size_t)task_cap * 4));
        TRY(ensure(ctx, W.dp_xwide, wide_bands ? (size_t)task_cap * 4 : 64));
        // ONT-profile batches: dense seeds and 4 096-anchor tiles for the first round only (noisy reads share few minimizers, but nothing bounds
        // them); from the second round on the reads are accurate and the sparser seeds keep a pair below 1 024 anchors
        const int w_round = (round > 0 && P.w_later > 0) ? P.w_later : P.w;
        TRY(overlap_stage(ctx, W, B, G, store, P, P.bw_ec, true, task_cap, ct, short_reads, wide_bands && w_round == P.w, w_round));
        W.stats.n_pairs += B.n_pairs;
        if (B.n_pairs) {
            Span tv(ctx, W.kt, ST_VERIFY);
            W.bpm_rec.push_back(W.kt.begin(ctx, KN_BPM, 0));
            TRY(fsv_bpm_windows_dev_n(ctx, store, (const fsv_wtask *)W.tasks.p, task_cap, ct + CT_TASKS, (fsv_wres *)W.res.p, P.k_cap));
            W.kt.end(ctx);
            W.rescue_rec.push_back(W.kt.begin(ctx, KN_RESCUE, (uint64_t)B.n_pairs * sizeof(fsv_ovl) * 2));
            if (wide_bands)
                hipLaunchKernelGGL(k_rescue_accept<true>, dim3(fsv_grid_for(B.n_pairs, 64)), dim3(64), 0, ctx->stream, store, (fsv_ovl *)W.ovl.p,
                                   B.n_pairs, (fsv_wtask *)W.tasks.p, (fsv_wres *)W.res.p, (unsigned long long *)(ct + CT_COLS_LO),
                                   (uint4 *)W.ovl_c.p, P.k_cap, P.accept_err_pm, (uint32_t *)nullptr, (uint32_t *)nullptr);
            else {
                // the right-extension pass and the verdict in one kernel; an overlap with an unmatched window LEFT of a matched one is set
                // aside for the left-extension pass (k_left_rescue: it needs the matched window's path first), which then gives its verdict
                TRY(ensure(ctx, W.left_list, (size_t)B.n_pairs * 4 + 16));
                hipLaunchKernelGGL(k_rescue_accept<false>, dim3(fsv_grid_for(B.n_pairs, 64)), dim3(64), 0, ctx->stream, store, (fsv_ovl *)W.ovl.p,
                                   B.n_pairs, (fsv_wtask *)W.tasks.p, (fsv_wres *)W.res.p, (unsigned long long *)(ct + CT_COLS_LO),
                                   (uint4 *)W.ovl_c.p, P.k_cap, P.accept_err_pm, (uint32_t *)W.left_list.p, ct + CT_LEFT);
                FSV_HIP(ctx, hipGetLastError());
                const uint32_t gridl = std::min<uint32_t>(std::max(1u, B.n_pairs), 8u * (uint32_t)ctx->n_cu);
                hipLaunchKernelGGL(k_left_rescue, dim3(gridl), dim3(64), 0, ctx->stream, store, (fsv_ovl *)W.ovl.p, (const uint32_t *)W.left_list.p,
                                   (const uint32_t *)(ct + CT_LEFT), (fsv_wtask *)W.tasks.p, (fsv_wres *)W.res.p, (fsv_wpath *)W.paths.p, (uint64_t *)nullptr,
                                   (uint4 *)W.ovl_c.p, P.k_cap, P.accept_err_pm);
            }
            FSV_HIP(ctx, hipGetLastError());
            W.kt.end(ctx);
            tv.stop();
            Span tp(ctx, W.kt, ST_PATH);
            TRY(path_stage(ctx, W, store, (const fsv_wtask *)W.tasks.p, (const fsv_wres *)W.res.p, (fsv_wpath *)W.paths.p, task_cap, (const uint32_t *)(ct + CT_TASKS), ct, round, wide_bands, P, 0));
            tp.stop();
        }
        // consensus -> corrected windows -> new read store
        Span tcs(ctx, W.kt, ST_CONSENSUS);
        const uint32_t n_gwin = G.gwin_off[B.n_reads];
        TRY(ensure(ctx, W.cwin, (size_t)n_gwin * FSV_CW_STRIDE));
        TRY(ensure(ctx, W.cwin_len, (size_t)n_gwin * 2));
        TRY(ensure(ctx, W.new_len, (size_t)B.n_reads * 4));
        if (!B.n_pairs) FSV_HIP(ctx, hipMemsetAsync(W.ovl_c.p, 0, sizeof(uint4), ctx->stream));
        TRY(ensure(ctx, W.gwin_tab, (size_t)std::max(1u, n_gwin) * sizeof(uint4)));
        hipLaunchKernelGGL(k_gwin_tab, dim3(fsv_grid_for(n_gwin, 256)), dim3(256), 0, ctx->stream, (const uint32_t *)W.gwin_read.p, (const uint32_t *)W.gwin_off.p,
                           (const uint32_t *)W.read_set.p, (const uint32_t *)W.set_start.p, (const uint32_t *)W.pair_base.p, n_gwin, (uint4 *)W.gwin_tab.p);
        FSV_HIP(ctx, hipGetLastError());
        ConsArgs C;
        C.store = store; C.word_off = (const uint32_t *)W.word_off.p; C.read_len = (const int32_t *)W.len.p;
        C.read_set = (const uint32_t *)W.read_set.p; C.set_start = (const uint32_t *)W.set_start.p; C.pair_base = (const uint32_t *)W.pair_base.p;
        C.gwin_off = (const uint32_t *)W.gwin_off.p; C.gwin_read = (const uint32_t *)W.gwin_read.p; C.ovl_c = (const uint4 *)W.ovl_c.p;
        C.gwin_tab = (const uint4 *)W.gwin_tab.p; C.tasks = (const fsv_wtask *)W.tasks.p;
        C.paths = (const fsv_wpath *)W.paths.p; C.cwin = (uint8_t *)W.cwin.p; C.cwin_len = (uint16_t *)W.cwin_len.p; C.warn = (uint32_t *)W.warn.p;
        C.n_reads = B.n_reads;
        TRY(ensure(ctx, W.changed, (size_t)B.n_reads * 4));
        FSV_HIP(ctx, hipMemsetAsync(W.changed.p, 0, (size_t)B.n_reads * 4, ctx->stream));
        C.changed = (uint32_t *)W.changed.p;
        C.read_dirty = nullptr;
        C.junction_vote = P.second_round ? 0 : 1;
        C.ins_dag = P.ins_dag ? 1 : 0;
        C.cov3 = nullptr;
        if (P.second_round && B.n_pairs) { TRY(ensure(ctx, W.cov3, (size_t)std::max(1u, n_gwin))); C.cov3 = (uint8_t *)W.cov3.p; }
        if (B.n_pairs) {
            TRY(ensure(ctx, W.read_dirty, (size_t)B.n_reads * 4));
            hipLaunchKernelGGL(k_read_dirty, dim3(B.n_reads), dim3(64), 0, ctx->stream, (const uint4 *)W.ovl_c.p, (const fsv_wpath *)W.paths.p,
                               (const uint32_t *)W.read_set.p, (const uint32_t *)W.set_start.p, (const uint32_t *)W.pair_base.p, B.n_reads, (uint32_t *)W.read_dirty.p);
            FSV_HIP(ctx, hipGetLastError());
            C.read_dirty = (const uint32_t *)W.read_dirty.p;
        }
        const bool partition = B.n_pairs && P.partition;
        SiteArgs SA{};
        SiteLists SL{};
        if (partition) {
            const size_t vec_cap = (size_t)B.n_pairs * 64 + (1u << 20);
            TRY(ensure(ctx, W.site_cnt, (size_t)std::max(1u, n_gwin) * 4));
            const size_t rec_cap = (size_t)n_gwin * 4 + 65536;
            TRY(ensure(ctx, W.site_rec, rec_cap * sizeof(uint2)));
            TRY(ensure(ctx, W.site_off, (size_t)std::max(1u, n_gwin) * 4));
            TRY(ensure(ctx, W.site_vec, vec_cap));
            TRY(ensure(ctx, W.site_cursor, 16));
            TRY(ensure(ctx, W.redo, (size_t)B.n_reads * 4));
            TRY(ensure(ctx, W.site_lists, (size_t)std::max(1u, n_gwin) * 8));
            FSV_HIP(ctx, hipMemsetAsync(W.site_cursor.p, 0, 16, ctx->stream));
            FSV_HIP(ctx, hipMemsetAsync(W.redo.p, 0, (size_t)B.n_reads * 4, ctx->stream));
            SA.site_cnt = (uint32_t *)W.site_cnt.p; SA.site_rec = (uint2 *)W.site_rec.p; SA.vec = (int8_t *)W.site_vec.p;
            SA.site_off = (uint32_t *)W.site_off.p; SA.rec_cursor = (uint32_t *)W.site_cursor.p + 3; SA.rec_cap = (uint32_t)std::min<size_t>(rec_cap, 0xfffffff0u);
            SA.vec_cursor = (uint32_t *)W.site_cursor.p; SA.vec_cap = (uint32_t)std::min<size_t>(vec_cap, 0xfffffff0u);
            SA.read_sites = (uint32_t *)W.redo.p;
            SL.site_cnt = SA.site_cnt; SL.win_list = (uint32_t *)W.site_lists.p; SL.redo_list = SL.win_list + std::max(1u, n_gwin);
            SL.win_n = (uint32_t *)W.site_cursor.p + 1;
        }
        if (partition && P.junction_cigars) {
            // calculate_boundary_cigars (Correct.cpp:2310): junction tasks -> K5 -> K6 -> which of the new cigars the partition uses
            uint32_t *ct3 = ct_of(2 * P.n_rounds + 2 + round);
            TRY(ensure(ctx, W.tasks2, (size_t)task_cap * sizeof(fsv_wtask)));
            TRY(ensure(ctx, W.res2, (size_t)task_cap * sizeof(fsv_wres)));
            TRY(ensure(ctx, W.paths2, (size_t)task_cap * sizeof(fsv_wpath)));
            TRY(ensure(ctx, W.bc_idx, (size_t)task_cap * 4));
            TRY(ensure(ctx, W.bc_rec, (size_t)task_cap * sizeof(uint4)));
            TRY(ensure(ctx, W.bc_win, (size_t)(n_gwin + 2) * 12));
            hipLaunchKernelGGL(k_bcwin_init, dim3(fsv_grid_for(n_gwin + 2, 256)), dim3(256), 0, ctx->stream, (int32_t *)W.bc_win.p, n_gwin + 2);
            FSV_HIP(ctx, hipGetLastError());
            BcigArgs BA;
            BA.tasks = (const fsv_wtask *)W.tasks.p; BA.paths = (const fsv_wpath *)W.paths.p; BA.n_tasks = ct + CT_TASKS;
            BA.pair_read = (const uint32_t *)W.pair_read.p; BA.read_dirty = (const uint32_t *)W.read_dirty.p; BA.gwin_off = (const uint32_t *)W.gwin_off.p;
            BA.thr_tab = (const uint8_t *)W.thr_tab.p; BA.k_cap = P.k_cap;
            BA.tasks2 = (fsv_wtask *)W.tasks2.p; BA.bc_idx = (int32_t *)W.bc_idx.p; BA.n_tasks2 = ct3 + CT_TASKS;
            BA.n_same = ct3 + CT_B_RETRY; BA.n_used = ct3 + CT_B_LIST;
            BA.res2 = (const fsv_wres *)W.res2.p; BA.paths2 = (const fsv_wpath *)W.paths2.p; BA.bc_rec = (uint4 *)W.bc_rec.p; BA.bc_win = (int32_t *)W.bc_win.p;
            W.kt.begin(ctx, KN_PARTITION, 0);
            hipLaunchKernelGGL(k_bcig_tasks, dim3((fsv_grid_for(task_cap, 256) + 7u) & ~7u), dim3(256), 0, ctx->stream, BA);
            FSV_HIP(ctx, hipGetLastError());
            W.kt.end(ctx);
            W.bc_bpm_rec.push_back(W.kt.begin(ctx, KN_BPM, 0));
            TRY(fsv_bpm_windows_dev_n(ctx, store, (const fsv_wtask *)W.tasks2.p, task_cap, ct3 + CT_TASKS, (fsv_wres *)W.res2.p, P.k_cap));
            W.kt.end(ctx);
            TRY(path_stage(ctx, W, store, (const fsv_wtask *)W.tasks2.p, (const fsv_wres *)W.res2.p, (fsv_wpath *)W.paths2.p, task_cap, (const uint32_t *)(ct3 + CT_TASKS), ct3,
                           round, wide_bands, P, 2));
            W.kt.begin(ctx, KN_PARTITION, 0);
            hipLaunchKernelGGL(k_bcig_accept, dim3(fsv_grid_for(task_cap, 256)), dim3(256), 0, ctx->stream, BA);
            FSV_HIP(ctx, hipGetLastError());
            W.kt.end(ctx);
            SA.bc_idx = (const int32_t *)W.bc_idx.p; SA.bc_rec = (const uint4 *)W.bc_rec.p; SA.bc_paths = (const fsv_wpath *)W.paths2.p;
            SL.bc_win = (const int32_t *)W.bc_win.p;
        }
        // consensus of every window; with the haplotype partition (K7) on, the windows that hold a candidate site are listed on the
        // way, k_snp_sites / k_hap_partition take the overlaps with the other allele out (is_match 2 / 4: out of the consensus and,
        // through that, out of what the final pass accepts as verified), and the reads that lost an overlap get their windows redone
        W.cons_rec.push_back(W.kt.begin(ctx, KN_CONSENSUS, (uint64_t)n_gwin * (96 + 448)));
        if (wide_bands) {
            if (partition) hipLaunchKernelGGL((k_consensus<FSV_EV_CAP_WIDE, 1>), dim3((n_gwin + 7u) & ~7u), dim3(64), 0, ctx->stream, C, n_gwin, SL);
            else hipLaunchKernelGGL((k_consensus<FSV_EV_CAP_WIDE, 0>), dim3((n_gwin + 7u) & ~7u), dim3(64), 0, ctx->stream, C, n_gwin, SL);
        } else {
            if (partition) hipLaunchKernelGGL((k_consensus<FSV_EV_CAP, 1>), dim3((n_gwin + 7u) & ~7u), dim3(64), 0, ctx->stream, C, n_gwin, SL);
            else hipLaunchKernelGGL((k_consensus<FSV_EV_CAP, 0>), dim3((n_gwin + 7u) & ~7u), dim3(64), 0, ctx->stream, C, n_gwin, SL);
        }
        FSV_HIP(ctx, hipGetLastError());
        W.kt.end(ctx);
        if (partition) {
            const uint32_t grid_l = std::min<uint32_t>(std::max(1u, n_gwin), (uint32_t)ctx->n_cu * 16);
            W.kt.begin(ctx, KN_PARTITION, (uint64_t)B.n_reads * 4);
            hipLaunchKernelGGL(k_snp_sites, dim3(grid_l), dim3(64), 0, ctx->stream, C, SA, SL);
            FSV_HIP(ctx, hipGetLastError());
            hipLaunchKernelGGL(k_hap_partition, dim3(B.n_reads), dim3(64), 0, ctx->stream, C, SA, (fsv_ovl *)W.ovl.p, (uint4 *)W.ovl_c.p, SL);
            FSV_HIP(ctx, hipGetLastError());
            if (wide_bands) hipLaunchKernelGGL(k_consensus_redo<FSV_EV_CAP_WIDE>, dim3(grid_l), dim3(64), 0, ctx->stream, C, SL);
            else hipLaunchKernelGGL(k_consensus_redo<FSV_EV_CAP>, dim3(grid_l), dim3(64), 0, ctx->stream, C, SL);
            FSV_HIP(ctx, hipGetLastError());
            W.kt.end(ctx);
        }
        if (P.second_round && B.n_pairs)
            TRY(second_pass(ctx, W, B, G, store, P, C, n_gwin, task_cap, (const uint32_t *)(ct + CT_TASKS), ct_of(P.n_rounds + 1 + round), round, wide_bands));
        TRY(ensure(ctx, W.lb, (size_t)std::max(1u, n_gwin) * 4));
        hipLaunchKernelGGL(k_newlen, dim3(fsv_grid_for(B.n_reads, 256)), dim3(256), 0, ctx->stream, (const uint32_t *)W.gwin_off.p,
                           (const uint16_t *)W.cwin_len.p, B.n_reads, (int32_t *)W.new_len.p, (uint32_t *)W.lb.p);
        FSV_HIP(ctx, hipGetLastError());
        // the round's one synchronisation: new read lengths (+ this round's counters)
        std::vector<int32_t> nlen(B.n_reads);
        FSV_HIP(ctx, hipMemcpyAsync(nlen.data(), W.new_len.p, (size_t)B.n_reads * 4, hipMemcpyDeviceToHost, ctx->stream));
        FSV_HIP(ctx, hipMemcpyAsync(h_ct.data() + (size_t)round * CT_SLOT, ct, CT_SLOT * 4, hipMemcpyDeviceToHost, ctx->stream));
        FSV_HIP(ctx, hipMemcpyAsync(h_ct.data() + (size_t)(P.n_rounds + 1 + round) * CT_SLOT, ct_of(P.n_rounds + 1 + round), CT_SLOT * 4, hipMemcpyDeviceToHost, ctx->stream));
        FSV_HIP(ctx, hipMemcpyAsync(h_ct.data() + (size_t)(2 * P.n_rounds + 2 + round) * CT_SLOT, ct_of(2 * P.n_rounds + 2 + round), CT_SLOT * 4, hipMemcpyDeviceToHost, ctx->stream));
        FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (h_ct[(size_t)round * CT_SLOT + CT_OVERFLOW]) return fsv_fail(ctx, FSV_ECAP, "internal window task buffer overflow");
        Geometry G2;
        TRY(make_geometry(ctx, B, nlen, G2, P.w, &mz_fixed));
        DevBuf &dst = W.store[round & 1];
        const uint32_t total_words = G2.word_off[B.n_reads];
        TRY(ensure(ctx, dst, ((size_t)total_words + 8) * 4));
        // k_repack needs the new offsets/lengths while the old ones are still in use by nothing else: stage them in mz_cnt/new_len
        TRY(upload(ctx, W.unpack_off, G2.word_off));
        W.kt.begin(ctx, KN_REPACK, (uint64_t)n_gwin * 384 + (uint64_t)total_words * 4);
        hipLaunchKernelGGL(k_repack, dim3(B.n_reads), dim3(256), 0, ctx->stream, (const uint32_t *)W.gwin_off.p,
                           (const uint32_t *)W.lb.p, (const uint8_t *)W.cwin.p, (const uint32_t *)W.unpack_off.p,
                           (const int32_t *)W.new_len.p, B.n_reads, round + 1 < P.n_rounds ? 1 : 0, (uint32_t *)dst.p);
        FSV_HIP(ctx, hipGetLastError());
        W.kt.end(ctx);
        FSV_HIP(ctx, hipMemsetAsync((uint8_t *)dst.p + (size_t)total_words * 4, 0, 32, ctx->stream));
        tcs.stop();
        store = (const uint32_t *)dst.p;
        len = nlen;
        for (int32_t l : len) if (l >= 65536) short_reads = false;
        G = G2;
    }

    // final overlaps on the corrected reads
    Span tf(ctx, W.kt, ST_FINAL);
    uint32_t *ctf = ct_of(P.n_rounds);
    auto tr0 = std::chrono::steady_clock::now();
    auto trace = [&](const char *what) { if (getenv("FSV_TRACE")) { (void)hipStreamSynchronize(ctx->stream); auto t = std::chrono::steady_clock::now(); fprintf(stderr, "[fsv] final %-14s %.2f ms\n", what, std::chrono::duration<double, std::milli>(t - tr0).count()); tr0 = t; } };
    TRY(upload(ctx, W.word_off, G.word_off));
    TRY(upload(ctx, W.len, len));
    TRY(upload(ctx, W.mz_off, G.mz_off));
    TRY(ensure(ctx, W.tasks, 64));
    // what the last correction round verified (coordinates on the reads as they were before that round) -- the final pass
    // accepts inexact overlaps against it; the slots are about to be overwritten
    const bool have_prev = P.n_rounds > 0 && B.n_pairs > 0;
    if (have_prev) {
        TRY(ensure(ctx, W.ovl_prev, (size_t)B.n_pairs * sizeof(fsv_ovl)));
        FSV_HIP(ctx, hipMemcpyAsync(W.ovl_prev.p, W.ovl.p, (size_t)B.n_pairs * sizeof(fsv_ovl), hipMemcpyDeviceToDevice, ctx->stream));
    }
    // reads the last round left untouched keep that round's minimizer lists (the last round does not reverse-complement)
    const int w_final = P.w_later > 0 ? P.w_later : P.w;
    // (the final pass keeps the lists of unchanged reads only when the last round sketched with the same window)
    const bool keep_lists = P.n_rounds > 0 && (P.n_rounds > 1 || w_final == P.w);
    // hifiasm's final pass keeps every pair that shares a minimizer on a strand, however short the overlap (the graph sorts them out)
    fsv_asm_params Pf = P;
    if (P.min_anchors_final > 0) Pf.min_anchors = P.min_anchors_final;
    if (P.min_ovlp_final > 0) Pf.min_ovlp = P.min_ovlp_final;
    TRY(overlap_stage(ctx, W, B, G, store, Pf, P.bw_final, false, 0, ctf, short_reads, wide_bands && w_final == P.w, w_final, keep_lists ? (const uint32_t *)W.changed.p : nullptr));
    trace("overlaps");
    const fsv_hit *hraw = nullptr;
    std::vector<uint32_t> hit_first(B.n_sets + 1, 0);
    std::vector<uint32_t> hwarn(B.n_reads), h_setcols(B.n_reads, 0u);
    if (B.n_pairs) {
        TRY(ensure(ctx, W.hits, (size_t)B.n_pairs * sizeof(fsv_hit)));
        TRY(ensure(ctx, W.set_hits, (size_t)(2 * B.n_sets + 2) * 4));
        FSV_HIP(ctx, hipMemsetAsync(W.set_hits.p, 0, (size_t)B.n_sets * 4, ctx->stream));
        W.kt.begin(ctx, KN_EXACT, (uint64_t)B.n_pairs * sizeof(fsv_ovl) + W.stats.n_pairs * 0);
        TRY(ensure(ctx, W.exact_flag, (size_t)B.n_upairs + 16));
        hipLaunchKernelGGL(k_exact, dim3(B.n_upairs), dim3(64), 0, ctx->stream, store, (const uint32_t *)W.word_off.p, (const int32_t *)W.len.p,
                           (const uint32_t *)W.read_set.p, (const uint32_t *)W.pair_base.p, (const uint4 *)W.upair_tab.p, (const fsv_ovl *)W.ovl.p,
                           (fsv_hit *)W.hits.p, (uint32_t *)W.set_hits.p, (uint8_t *)W.exact_flag.p);
        FSV_HIP(ctx, hipGetLastError());
        W.kt.end(ctx);
        if (have_prev) {
            // pairs without an exact overlap that the last correction round had verified: gapped re-chain, accept per direction.
            // The list's length stays on the device: the re-chain is launched over every pair slot and the blocks beyond the list
            // return at once (a few hundred pairs are listed out of hundreds of thousands; the empty blocks cost ~40 us)
            TRY(ensure(ctx, W.inexact_list, (size_t)B.n_upairs * 4 + 16));
            uint32_t *n_list_dev = ctf + CT_INEXACT;
            hipLaunchKernelGGL(k_inexact_list, dim3(fsv_grid_for(B.n_upairs, 256)), dim3(256), 0, ctx->stream, (const uint4 *)W.upair_tab.p,
                               (const uint8_t *)W.exact_flag.p, (const fsv_ovl *)W.ovl_prev.p, B.n_upairs, (uint32_t *)W.inexact_list.p, n_list_dev);
            FSV_HIP(ctx, hipGetLastError());
            ChainArgs A2 = W.last_chain;
            A2.bw = P.bw_rechain; A2.emit_tasks = 0; A2.pair_list = (const uint32_t *)W.inexact_list.p; A2.n_list_dev = n_list_dev;
            // Either direction of a listed pair is chained from its own side, as hifiasm does: with an indel budget the chain DP depends
            // on the end it starts from (the budget is a rate over the span chained so far; on the reverse strand the two sides start
            // from opposite ends), and the mirror image of one side's chain can be off by the bases of an indel near a read end.
            A2.primary_only = 1;
            TRY(ensure(ctx, W.upair_tab_sw, (size_t)std::max(1u, B.n_upairs) * sizeof(uint4)));
            hipLaunchKernelGGL(k_pair_tab_swap, dim3(fsv_grid_for(B.n_upairs, 256)), dim3(256), 0, ctx->stream, (const uint4 *)W.upair_tab.p, B.n_upairs, (uint4 *)W.upair_tab_sw.p);
            FSV_HIP(ctx, hipGetLastError());
            // timed like the other k_chain launches (a profiler counts it too)
            W.kt.begin(ctx, KN_CHAIN, 0);
            for (int side = 0; side < 2; side++) {
                if (side == 1) A2.upair_tab = (const uint4 *)W.upair_tab_sw.p;
                if (A2.wide_list) FSV_HIP(ctx, hipMemsetAsync(A2.n_wide, 0, 4, ctx->stream));   // (the final pass's own wide pairs are done)
                if (short_reads) { TRY(lds_opt_in(ctx, k_chain<true>, chain_lds_bytes(true, A2.amax))); hipLaunchKernelGGL(k_chain<true>, dim3(B.n_upairs), dim3(64), chain_lds_bytes(true, A2.amax), ctx->stream, A2); }
                else { TRY(lds_opt_in(ctx, k_chain<false>, chain_lds_bytes(false, A2.amax))); hipLaunchKernelGGL(k_chain<false>, dim3(B.n_upairs), dim3(64), chain_lds_bytes(false, A2.amax), ctx->stream, A2); }
                FSV_HIP(ctx, hipGetLastError());
                if (A2.wide_list) {
                    ChainArgs AW = A2;
                    AW.amax = short_reads ? FSV_AMAX_WIDE : FSV_AMAX_WIDE_LONG; AW.pair_list = nullptr; AW.n_list_dev = nullptr;
                    const uint32_t gridw = std::min<uint32_t>(B.n_upairs, 2u * (uint32_t)ctx->n_cu);
                    if (short_reads) { TRY(lds_opt_in(ctx, k_chain_wide_list<true>, chain_lds_bytes(true, AW.amax))); hipLaunchKernelGGL(k_chain_wide_list<true>, dim3(gridw), dim3(64), chain_lds_bytes(true, AW.amax), ctx->stream, AW); }
                    else { TRY(lds_opt_in(ctx, k_chain_wide_list<false>, chain_lds_bytes(false, AW.amax))); hipLaunchKernelGGL(k_chain_wide_list<false>, dim3(gridw), dim3(64), chain_lds_bytes(false, AW.amax), ctx->stream, AW); }
                    FSV_HIP(ctx, hipGetLastError());
                }
            }
            W.kt.end(ctx);
            hipLaunchKernelGGL(k_accept_inexact, dim3(fsv_grid_for(2ull * B.n_upairs, 256)), dim3(256), 0, ctx->stream, (const uint4 *)W.upair_tab.p,
                               (const uint32_t *)W.inexact_list.p, 0u, (const fsv_ovl *)W.ovl.p, (const fsv_ovl *)W.ovl_prev.p,
                               (const uint32_t *)W.read_set.p, (const uint32_t *)W.pair_base.p, (fsv_hit *)W.hits.p, (uint32_t *)W.set_hits.p,
                               (const uint32_t *)n_list_dev);
            FSV_HIP(ctx, hipGetLastError());
        }
        // per-set counts -> offsets; the segments are packed on the device and come back in one copy, already grouped by set.
        // The order inside a set depends on atomics and does not matter: the layout's containment marks and "longest arc,
        // smallest target on ties" choices are order-independent.  The warnings and the batch's counters ride along.
        FSV_HIP(ctx, hipMemcpyAsync(hit_first.data() + 1, W.set_hits.p, (size_t)B.n_sets * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    FSV_HIP(ctx, hipMemcpyAsync(hwarn.data(), W.warn.p, (size_t)B.n_reads * 4, hipMemcpyDeviceToHost, ctx->stream));
    FSV_HIP(ctx, hipMemcpyAsync(h_setcols.data(), W.set_cols.p, (size_t)B.n_reads * 4, hipMemcpyDeviceToHost, ctx->stream));
    FSV_HIP(ctx, hipMemcpyAsync(h_ct.data() + (size_t)P.n_rounds * CT_SLOT, ctf, CT_SLOT * 4, hipMemcpyDeviceToHost, ctx->stream));
    FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (B.n_pairs) {
        for (uint32_t s2 = 0; s2 < B.n_sets; s2++) hit_first[s2 + 1] += hit_first[s2];
        const uint32_t nh = hit_first[B.n_sets];
        if ((size_t)nh * sizeof(fsv_hit) > W.h_pin_cap) {
            if (W.h_pin) FSV_HIP(ctx, hipHostFree(W.h_pin));
            W.h_pin = nullptr; W.h_pin_cap = (size_t)nh * sizeof(fsv_hit) * 5 / 4 + 4096;
            FSV_HIP(ctx, hipHostMalloc(&W.h_pin, W.h_pin_cap, hipHostMallocDefault));
        }
        hraw = (const fsv_hit *)W.h_pin;
        if (nh) {
            uint32_t *first_dev = (uint32_t *)W.set_hits.p + B.n_sets;
            TRY(ensure(ctx, W.hits_packed, (size_t)nh * sizeof(fsv_hit)));
            FSV_HIP(ctx, hipMemcpyAsync(first_dev, hit_first.data(), (size_t)(B.n_sets + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
            hipLaunchKernelGGL(k_hits_compact, dim3(B.n_sets), dim3(256), 0, ctx->stream, (const fsv_hit *)W.hits.p, (const uint32_t *)W.pair_base.p,
                               (const uint32_t *)first_dev, (fsv_hit *)W.hits_packed.p);
            FSV_HIP(ctx, hipGetLastError());
            FSV_HIP(ctx, hipMemcpyAsync(W.h_pin, W.hits_packed.p, (size_t)nh * sizeof(fsv_hit), hipMemcpyDeviceToHost, ctx->stream));
            FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
        }
        W.stats.n_exact_overlaps = nh;
    }
    trace("exact+gather");

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
            if (w1 > w0) FSV_HIP(ctx, hipMemcpyAsync(h_store.data() + w0, store + w0, (size_t)(w1 - w0) * 4, hipMemcpyDeviceToHost, ctx->stream));
        }
        if (any_inexact) FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    const uint8_t *set_flags = sets->set_flags;
    // layout per set (host), then stitch on the device
    std::vector<fsv_piece> pieces;
    uint64_t used = 0;
    uint32_t nc = 0;
    int rc_out = FSV_OK;
    // the sets are independent: lay them out on a few host threads, then emit the contigs in set order
    struct SetLayout { std::vector<std::vector<Piece>> contigs; bool fallback = false; };
    std::vector<SetLayout> lay(B.n_sets);
    {
        const uint32_t nthr = std::max(1u, std::min({8u, std::thread::hardware_concurrency(), B.n_sets / 16 + 1}));
        std::atomic<uint32_t> next{0};
        // a worker never lets an exception out (it would end the process): the first failure is kept and returned after the join
        std::atomic<int> rc_work{FSV_OK};
        auto work = [&]() {
            try {
            for (uint32_t s = next.fetch_add(1); s < B.n_sets && rc_work.load() == FSV_OK; s = next.fetch_add(1)) {
                const uint32_t r0 = B.set_start[s], ns = B.set_start[s + 1] - r0;
                if (ns == 0) continue;
                const uint32_t nh_s = hit_first[s + 1] - hit_first[s];
                const bool unphased = set_flags && (set_flags[s] & FSV_SET_UNPHASED);
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
    }
    for (uint32_t s = 0; s < B.n_sets && rc_out == FSV_OK; s++) {
        const uint32_t r0 = B.set_start[s], ns = B.set_start[s + 1] - r0;
        int32_t st = 0;
        for (uint32_t r = r0; r < r0 + ns; r++) st |= (int32_t)(hwarn[r] & (FSV_W_MZ_TRUNC | FSV_W_ANCHOR_TRUNC | FSV_W_INS_EVENTS | FSV_W_WINDOW_KEPT | FSV_W_INTERNAL | FSV_W_SITES));
        if (ns == 0) { out->set_status[s] = st; continue; }
        if (lay[s].fallback) st |= FSV_W_NO_LAYOUT;
        for (auto &c : lay[s].contigs) {
            uint64_t clen = 0;
            for (auto &pc : c) clen += pc.len;
            if (nc >= out->contig_cap || used + clen > out->seq_cap) { rc_out = fsv_fail(ctx, FSV_ECAP, "contig output buffers too small (use fsv_assemble_batch_bound)"); break; }
            for (auto &pc : c) { pieces.push_back(fsv_piece{r0 + pc.read, pc.rev, pc.len, 0u, used}); used += pc.len; }
            out->set[nc] = s; out->n_reads[nc] = (uint32_t)c.size();
            out->off[++nc] = used;
        }
        out->set_status[s] = st;
    }
    trace("layout");
    if (rc_out != FSV_OK) return rc_out;
    out->n_contigs = nc;
    ctx->last_contigs_dev = nullptr;
    ctx->last_contig_off.assign(out->off, out->off + nc + 1);
    if (!pieces.empty()) {
        TRY(upload(ctx, W.pieces, pieces));
        TRY(ensure(ctx, W.contig_out, used + 16));
        W.kt.begin(ctx, KN_STITCH, used + used / 4);    // 2-bit bases in, ASCII out
        hipLaunchKernelGGL(k_stitch, dim3((uint32_t)pieces.size()), dim3(256), 0, ctx->stream, store, (const uint32_t *)W.word_off.p,
                           (const int32_t *)W.len.p, (const fsv_piece *)W.pieces.p, (char *)W.contig_out.p);
        FSV_HIP(ctx, hipGetLastError());
        W.kt.end(ctx);
        ctx->last_contigs_dev = (const char *)W.contig_out.p;
        FSV_HIP(ctx, hipMemcpyAsync(out->seq, W.contig_out.p, used, hipMemcpyDeviceToHost, ctx->stream));
        FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    trace("stitch+d2h");
    tf.stop();
    W.h_word_off = G.word_off; W.h_len = len; W.cur_store = store; W.n_reads = B.n_reads;
    // statistics out of the counter slots (one per correction round, one for the final pass)
    uint64_t mz_total[17] = {0}, n_windows2 = 0;
    for (int sl = 0; sl <= P.n_rounds; sl++) {
        const uint32_t *c = h_ct.data() + (size_t)sl * CT_SLOT;
        mz_total[sl] = (uint64_t)c[CT_MZ_LO] | (uint64_t)c[CT_MZ_HI] << 32;
        if (sl == P.n_rounds) { W.stats.n_inexact_candidates = c[CT_INEXACT]; break; }
        W.stats.n_windows += c[CT_TASKS];
        W.stats.dp_columns += (uint64_t)c[CT_COLS_LO] | (uint64_t)c[CT_COLS_HI] << 32;      // rescue re-runs (k_rescue_accept)
        W.stats.n_path_dp += (uint64_t)c[CT_DP_SB] + c[CT_DP_SB16] + c[CT_DP] + c[CT_DP_FR3] + c[CT_DP_GEN] + c[CT_DP_WIDE] + c[CT_DP_XW];
        W.stats.n_path_fr += (uint64_t)c[CT_DP_SB16] + c[CT_DP] + c[CT_DP_FR3];
        // algorithmic bytes of the round's launches, now that the counts are known: a window task is
        // 94 + 102 B of 2-bit operands + 16 B of result; a K6 window leaves a 128 B path record instead;
        // k_chain reads every unique-minimizer list once (two sorted copies, 16 B entries) and writes the overlap slots and
        // the 32 B task records; the consensus reads the path records and writes its corrected windows
        const uint64_t nt = c[CT_TASKS], n_dp = (uint64_t)c[CT_DP_SB] + c[CT_DP_SB16] + c[CT_DP] + c[CT_DP_FR3] + c[CT_DP_GEN] + c[CT_DP_WIDE] + c[CT_DP_XW];
        if ((size_t)sl < W.bpm_rec.size()) W.kt.recs[W.bpm_rec[sl]].bytes = nt * 212ull;
        if ((size_t)sl < W.rescue_rec.size()) W.kt.recs[W.rescue_rec[sl]].bytes += nt * 16ull;
        if ((size_t)sl < W.fast_rec.size()) W.kt.recs[W.fast_rec[sl]].bytes = nt * (16ull + 196ull) + (nt - n_dp) * 128ull;
        if ((size_t)sl < W.dp_rec.size()) W.kt.recs[W.dp_rec[sl]].bytes = n_dp * (196ull + 128ull);
        if ((size_t)sl < W.cons_rec.size()) W.kt.recs[W.cons_rec[sl]].bytes += nt * 128ull;
        // the round's second consensus pass (its counters sit n_rounds + 1 rows further): the junction tasks are window tasks like
        // the first pass's; k_bnd_tasks reads every first-pass task and path record and writes the junction tasks; the junctions'
        // consensus reads their path records and writes a patch per junction
        if ((size_t)sl < W.bc_bpm_rec.size()) {      // the junction cigars of the round's partition: window tasks like the others
            const uint32_t *c3 = h_ct.data() + (size_t)(2 * P.n_rounds + 2 + sl) * CT_SLOT;
            const uint64_t n3 = c3[CT_TASKS], n_dp3 = (uint64_t)c3[CT_DP_SB] + c3[CT_DP_SB16] + c3[CT_DP] + c3[CT_DP_FR3] + c3[CT_DP_GEN] + c3[CT_DP_WIDE] + c3[CT_DP_XW];
            n_windows2 += n3;
            W.stats.n_junction_cigars += n3;
            W.stats.n_junction_used += c3[CT_B_LIST];
            if (getenv("FSV_BCIG_DEBUG")) fprintf(stderr, "[fsv] round %d: %u overlaps set aside for the left-extension pass; fix_boundary: %u candidates, %u windows moved\n", sl, c[CT_LEFT], c[CT_FIX], c[CT_FIXED]);
            if (getenv("FSV_BCIG_DEBUG")) fprintf(stderr, "[fsv] round %d: %llu junction cigars, %u accepted but showing what the window cigars show, %u used\n", sl, (unsigned long long)n3, c3[CT_B_RETRY], c3[CT_B_LIST]);
            W.kt.recs[W.bc_bpm_rec[sl]].bytes = n3 * 212ull;
            if ((size_t)sl < W.bc_fast_rec.size()) W.kt.recs[W.bc_fast_rec[sl]].bytes = n3 * (16ull + 196ull) + (n3 - n_dp3) * 128ull;
            if ((size_t)sl < W.bc_dp_rec.size()) W.kt.recs[W.bc_dp_rec[sl]].bytes = n_dp3 * (196ull + 128ull);
        }
        if ((size_t)sl < W.bnd_rec.size()) {
            const uint32_t *c2 = h_ct.data() + (size_t)(P.n_rounds + 1 + sl) * CT_SLOT;
            const uint64_t n2 = c2[CT_TASKS], n3 = c2[CT_B_RETRY], n_dp2 = (uint64_t)c2[CT_DP_SB] + c2[CT_DP_SB16] + c2[CT_DP] + c2[CT_DP_FR3] + c2[CT_DP_GEN] + c2[CT_DP_WIDE] + c2[CT_DP_XW];
            n_windows2 += n2 + n3;
            W.kt.recs[W.bnd_rec[sl]].bytes = nt * (sizeof(fsv_wtask) + 128ull) + n2 * sizeof(fsv_wtask);
            if ((size_t)sl < W.bpm2_rec.size()) W.kt.recs[W.bpm2_rec[sl]].bytes = (n2 + n3) * 212ull;
            if ((size_t)sl < W.fast2_rec.size()) W.kt.recs[W.fast2_rec[sl]].bytes = n2 * (16ull + 196ull) + (n2 - n_dp2) * 128ull;
            if ((size_t)sl < W.dp2_rec.size()) W.kt.recs[W.dp2_rec[sl]].bytes = n_dp2 * (196ull + 128ull);
            if ((size_t)sl < W.bndc_rec.size()) W.kt.recs[W.bndc_rec[sl]].bytes = n2 * 128ull + (uint64_t)c2[CT_B_LIST] * (sizeof(BndPatch) + 2ull * FSV_BND_HALF);
        }
    }
    // the sketch reads the packed bases of the reads it sketches and writes 16 B per minimizer it produces ("len/4
    // in + 16 B / minimizer out"); k_uniq reads those and writes the unique ones twice (sorted by hash, sorted by position).
    // Round 2 charged 16 B per slot of CAPACITY (one per base) -- seven times what the counters saw.
    for (size_t i = 0; i < W.sk_rec.size() && i <= (size_t)P.n_rounds; i++) {
        const uint32_t *c = h_ct.data() + i * CT_SLOT;
        const uint64_t raw = (uint64_t)c[CT_MZRAW_LO] | (uint64_t)c[CT_MZRAW_HI] << 32, bases = (uint64_t)c[CT_BASES_LO] | (uint64_t)c[CT_BASES_HI] << 32;
        W.kt.recs[W.sk_rec[i]].bytes = bases / 4 + raw * sizeof(fsv_mz);
        if (i < W.uq_rec.size()) W.kt.recs[W.uq_rec[i]].bytes = raw * sizeof(fsv_mz) + mz_total[i] * 2 * sizeof(fsv_mz);
    }
    for (size_t i = 0; i < W.chain_rec.size(); i++) {
        const uint32_t *c = h_ct.data() + i * CT_SLOT;
        W.kt.recs[W.chain_rec[i]].bytes = mz_total[i] * 32ull + (uint64_t)B.n_pairs * sizeof(fsv_ovl) + (i < (size_t)P.n_rounds ? (uint64_t)c[CT_TASKS] * sizeof(fsv_wtask) : 0ull);
    }
    for (uint32_t s2 = 0; s2 < B.n_sets; s2++) if (B.set_start[s2] < B.n_reads && B.set_start[s2 + 1] > B.set_start[s2]) W.stats.dp_columns += h_setcols[B.set_start[s2]];   // K5 windows
    // algorithmic bytes: 2-bit operands + result of every DP task, reads in once per pass, contigs out
    W.stats.algo_bytes = (W.stats.n_windows + n_windows2) * 212ull + reads_in_bytes * (uint64_t)(P.n_rounds + 1) + used;
    W.stats.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_enter).count();
    // resolve the per-kernel event timings
    W.stats.n_kernels = KN_COUNT;
    for (int k = 0; k < KN_COUNT; k++) { memset(&W.stats.kernels[k], 0, sizeof(fsv_kernel_stat)); strncpy(W.stats.kernels[k].name, kn_names[k], 23); }
    for (auto &r : W.kt.recs) {
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
    return FSV_OK;
}

// Work a set brings: its window-task bound (every read's windows against every other read) and its ordered pairs.
static void set_cost(const fsv_readsets *sets, uint32_t s, uint64_t &tasks, uint64_t &pairs, uint64_t &bases)
{
    const uint64_t ns = sets->set_start[s + 1] - sets->set_start[s];
    uint64_t nw = 0; bases = 0;
    for (uint32_t r = sets->set_start[s]; r < sets->set_start[s + 1]; r++) { nw += ((uint64_t)sets->read_len[r] + FSV_WINDOW - 1) / FSV_WINDOW; bases += (uint64_t)sets->read_len[r]; }
    tasks = ns > 1 ? nw * (ns - 1) : 0;
    pairs = ns > 1 ? ns * (ns - 1) : 0;
}

static int fsv_assemble_batch_impl(fsv_ctx *ctx, const fsv_readsets *sets, const fsv_asm_params *params, fsv_contigs *out)
{
    if (!ctx || !sets || !out || !sets->store_dev || !sets->word_off || !sets->read_len || !sets->set_start) return FSV_EINVAL;
    if (!out->seq || !out->off || !out->set || !out->n_reads || !out->set_status) return FSV_EINVAL;
    fsv_asm_params P;
    if (params) P = *params; else fsv_asm_default_params(&P);
    if (P.k < 1 || P.k > 63 || P.w < 1 || P.w > 64 || P.lookback != 64 || P.n_rounds < 0 || P.n_rounds > 16 || P.min_anchors < 1)
        return fsv_fail(ctx, FSV_EINVAL, "fsv_asm_params out of range (k<=63, w<=64, lookback==64)");
    if (P.k_cap < 1 || P.k_cap > FSV_K_WIDE || P.win_rate_pm < 1 || (int)(FSV_WINDOW * (P.win_rate_pm / 1000.0)) > P.k_cap || P.accept_err_pm < 0 || P.accept_err_pm > 1000 ||
        P.w_later < 0 || P.w_later > 64)
        return fsv_fail(ctx, FSV_EINVAL, "fsv_asm_params error model out of range (k_cap <= 95, 375 x win_rate_pm / 1000 <= k_cap)");
    FSV_HIP(ctx, hipSetDevice(ctx->device));
    AsmWs &W = *ws_get(ctx);
    out->n_contigs = 0; out->off[0] = 0;
    if (sets->n_reads == 0 || sets->n_sets == 0) { for (uint32_t s = 0; s < sets->n_sets; s++) out->set_status[s] = 0; memset(&W.stats, 0, sizeof(W.stats)); return FSV_OK; }
    if (sets->set_start[0] != 0 || sets->set_start[sets->n_sets] != sets->n_reads) return fsv_fail(ctx, FSV_EINVAL, "set_start must span [0, n_reads]");
    for (uint32_t s = 0; s < sets->n_sets; s++) if (sets->set_start[s + 1] < sets->set_start[s]) return fsv_fail(ctx, FSV_EINVAL, "set_start not monotone");
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
        size_t free_b = 0, total_b = 0, own = 0;
        for (const DevBuf *b : W.all()) own += b->cap;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess)
            budget = std::min(budget, 0.9 * ((double)free_b / (double)std::max(1, fsv_live_contexts(ctx->device)) + (double)own));
    }
    if (env && atof(env) > 0) budget = atof(env) * 1e9;
    std::vector<uint32_t> cut{0};
    {
        uint64_t tk = 0, pr = 0, bs = 0;
        for (uint32_t s = 0; s < sets->n_sets; s++) {
            uint64_t t1, p1, b1;
            set_cost(sets, s, t1, p1, b1);
            if (t1 >= (1ull << 31) || p1 >= (1ull << 31) || b1 + b1 / 4 >= (1ull << 32)) return fsv_fail(ctx, FSV_EUNSUP, "a single read set exceeds the 2^31 window-task / pair bound");
            const bool over = tk + t1 >= (1ull << 31) || pr + p1 >= (1ull << 31) || (bs + b1) + (bs + b1) / 4 >= (1ull << 32) ||     /* minimizer slots: one per base + slack, 32-bit offsets */
                              (double)(tk + t1) * (P.second_round ? 400.0 : 200.0) + (double)(pr + p1) * 200.0 + (double)(bs + b1) * (P.second_round ? 52.0 : 48.0) > budget;   /* second pass: the junction tasks' records, the patch slots */
            if (over && s > cut.back()) { cut.push_back(s); tk = pr = bs = 0; }
            tk += t1; pr += p1; bs += b1;
        }
        cut.push_back(sets->n_sets);
    }
    if (cut.size() == 2) return assemble_chunk(ctx, sets, P, out);
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
        if (bytes) {
            if (W.contig_all.cap < used + bytes + 16) {
                DevBuf bigger;
                TRY(ensure(ctx, bigger, std::max<uint64_t>((used + bytes) * 2, 1u << 20)));
                if (used) FSV_HIP(ctx, hipMemcpyAsync(bigger.p, W.contig_all.p, used, hipMemcpyDeviceToDevice, ctx->stream));
                FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
                W.contig_all.swap(bigger);      // (the old allocation goes with `bigger`)
            }
            FSV_HIP(ctx, hipMemcpyAsync((char *)W.contig_all.p + used, W.contig_out.p, bytes, hipMemcpyDeviceToDevice, ctx->stream));
        }
        used += bytes; nc += part.n_contigs;
        // statistics: sums over the chunks
        const fsv_asm_stats &st = W.stats;
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
    FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    out->n_contigs = nc;
    W.stats = total;
    W.n_reads = 0; W.cur_store = nullptr;        // fsv_asm_fetch_reads serves single-pass batches only
    ctx->last_contigs_dev = nc ? (const char *)W.contig_all.p : nullptr;
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
    DevBuf d_off, d_out;
    int rc = upload(ctx, d_off, o);
    if (rc == FSV_OK) rc = ensure(ctx, d_out, o[n_reads] + 16);
    if (rc == FSV_OK) {
        hipLaunchKernelGGL(k_unpack_reads, dim3(n_reads), dim3(256), 0, ctx->stream, W.cur_store, (const uint32_t *)W.word_off.p,
                           (const int32_t *)W.len.p, (const uint64_t *)d_off.p, (char *)d_out.p);
        if (hipGetLastError() != hipSuccess) rc = FSV_EHIP;
    }
    if (rc == FSV_OK) rc = fsv_d2h(ctx, seq, d_out.p, o[n_reads]);
    memcpy(off, o.data(), (n_reads + 1) * sizeof(uint64_t));
    return rc;
}

static int fsv_sketch_reads_impl(fsv_ctx *ctx, const fsv_readsets *sets, int32_t w, int32_t k, int32_t hpc, int32_t variant, fsv_mz *out_mz,
                                uint64_t out_cap, uint64_t *out_off)
{
    if (!ctx || !sets || !sets->store_dev || !sets->word_off || !sets->read_len || !out_mz || !out_off) return FSV_EINVAL;
    if (k < 1 || k > 63 || w < 1 || w > 64) return fsv_fail(ctx, FSV_EINVAL, "k <= 63, w <= 64");
    FSV_HIP(ctx, hipSetDevice(ctx->device));
    AsmWs &W = *ws_get(ctx);
    W.kt.reset();
    Batch B;
    B.n_reads = sets->n_reads; B.n_sets = 1; B.n_pairs = 0;
    B.set_start = {0u, B.n_reads};
    out_off[0] = 0;
    if (B.n_reads == 0) return FSV_OK;
    std::vector<int32_t> len(sets->read_len, sets->read_len + B.n_reads);
    for (uint32_t r = 0; r < B.n_reads; r++) if (len[r] < 1 || len[r] >= (1 << 24)) return fsv_fail(ctx, FSV_EUNSUP, "read length must be in [1, 2^24)");
    Geometry G;
    TRY(make_geometry(ctx, B, len, G, w));
    for (uint32_t r = 0; r <= B.n_reads; r++) G.word_off[r] = (uint32_t)sets->word_off[r];
    TRY(upload(ctx, W.word_off, G.word_off));
    TRY(upload(ctx, W.len, len));
    TRY(upload(ctx, W.mz_off, G.mz_off));
    TRY(ensure(ctx, W.warn, (size_t)B.n_reads * 4));
    FSV_HIP(ctx, hipMemsetAsync(W.warn.p, 0, (size_t)B.n_reads * 4, ctx->stream));
    fsv_asm_params P;
    fsv_asm_default_params(&P);
    P.w = w; P.k = (variant == 1) ? (k | 0) : k; P.hpc = hpc;
    // overlap_stage picks the kernel by the parity of k; to force the replay kernel for an odd k, run its launch here
    TRY(ensure(ctx, W.mz, (size_t)G.mz_off[B.n_reads] * sizeof(fsv_mz)));
    TRY(ensure(ctx, W.mz_cnt, (size_t)B.n_reads * 4));
    FSV_HIP(ctx, hipMemsetAsync(W.mz_cnt.p, 0, (size_t)B.n_reads * 4, ctx->stream));
    if ((k & 1) && variant != 1) {
        const size_t total_words = G.word_off[B.n_reads];
        TRY(ensure(ctx, W.sk_ends, (total_words * 16 + 64) * 4));
        TRY(ensure(ctx, W.sk_low, (total_words + B.n_reads + 8) * 4));
        TRY(ensure(ctx, W.sk_high, (total_words + B.n_reads + 8) * 4));
        FSV_HIP(ctx, hipMemsetAsync(W.sk_low.p, 0, (total_words + B.n_reads + 8) * 4, ctx->stream));
        FSV_HIP(ctx, hipMemsetAsync(W.sk_high.p, 0, (total_words + B.n_reads + 8) * 4, ctx->stream));
        hipLaunchKernelGGL(k_sketch_fast, dim3(B.n_reads), dim3(256), 0, ctx->stream, sets->store_dev, (const uint32_t *)W.word_off.p,
                           (const int32_t *)W.len.p, (const uint32_t *)W.mz_off.p, (fsv_mz *)W.mz.p, (uint32_t *)W.mz_cnt.p, B.n_reads, w, k, hpc,
                           (uint32_t *)W.warn.p, (const uint8_t *)nullptr, (uint32_t *)W.sk_ends.p, (uint32_t *)W.sk_low.p, (uint32_t *)W.sk_high.p,
                           (const uint32_t *)nullptr);
    } else {
        const uint32_t lds_words = std::min<uint32_t>(G.max_words, 8192u);
        FSV_HIP(ctx, hipFuncSetAttribute((const void *)k_sketch, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sketch_lds_bytes(w, lds_words)));
        hipLaunchKernelGGL(k_sketch, dim3(B.n_reads), dim3(64), sketch_lds_bytes(w, lds_words), ctx->stream, sets->store_dev,
                           (const uint32_t *)W.word_off.p, (const int32_t *)W.len.p, (const uint32_t *)W.mz_off.p, (fsv_mz *)W.mz.p,
                           (uint32_t *)W.mz_cnt.p, B.n_reads, w, k, hpc, (uint32_t *)W.warn.p, (const uint8_t *)nullptr, w, lds_words);
    }
    FSV_HIP(ctx, hipGetLastError());
    std::vector<uint32_t> cnt(B.n_reads);
    FSV_HIP(ctx, hipMemcpyAsync(cnt.data(), W.mz_cnt.p, (size_t)B.n_reads * 4, hipMemcpyDeviceToHost, ctx->stream));
    FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    uint64_t tot = 0;
    for (uint32_t r = 0; r < B.n_reads; r++) {
        const uint32_t c = std::min<uint32_t>(cnt[r], G.mz_off[r + 1] - G.mz_off[r]);
        if (tot + c > out_cap) return fsv_fail(ctx, FSV_ECAP, "out_mz too small");
        FSV_HIP(ctx, hipMemcpyAsync(out_mz + tot, (const fsv_mz *)W.mz.p + G.mz_off[r], (size_t)c * sizeof(fsv_mz), hipMemcpyDeviceToHost, ctx->stream));
        tot += c;
        out_off[r + 1] = tot;
    }
    FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (uint32_t r = 0; r < B.n_reads; r++)
        std::sort(out_mz + out_off[r], out_mz + out_off[r + 1], [](const fsv_mz &a, const fsv_mz &b) { return a.pos < b.pos; });
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
