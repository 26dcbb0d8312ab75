// aln.hip -- contig-vs-reference-window alignment (fsv_align_batch) for gfx950.
//
// Replaces `minimap2 -a -x asm5 --cs -r2k` + pysam read-back (focalsv/4_sv_calling/Dippav/DipPAV_variant_call.py:103-112;
// extract_contig_signature_CCS.py:14-47, 342-432).  Restated in oracle/aln.c, which this file must match bit for bit.
//   k_sketch / k_uniq   seeds (ha_sketch without HPC, k = 19)           sketch.cpp:39-137
//   k_chain_aln         co-linear chains, one wavefront per pair, all state in LDS; the inverted piece as a record of the other strand
//   k_aln_events        gap-free runs vs DP events, padding, X-drop end extension
//   k_extract_boxes     an event of more than max_cells cells becomes a pair of its own, seeded / chained / walked again end to end
//   k_corner            what is still too large inside such a box: gap-free X-drop from its corners, the rest one I + one D
//   k_gap_shift         every gap of the stitched CIGAR to its leftmost position (minimap2's mm_fix_cigar rule)
//   k_nw                dual-affine global DP of one event on anti-diagonals (one workgroup per event), the
//                       recurrence / tie rules / backtrack of the in-tree ksw2 (ksw2_extz2_sse.c:171-196, ksw2.h:115-150)
//   k_aln_tags          fsv_aln_tags: NM and the cs difference string of finished records (what minimap2's --cs adds), count / scan / emit
//   k_ref_* / k_place   fsv_ref_index_* / fsv_contig_mapq: a chromosome-wide minimizer index and the records' mapping quality from it (opt-in)
// The kernels are in k_aln.h and k_place.h; this file is the host path, with aln_mapq.h (included at the end) for the last line above.
#include "k_aln.h"
#include "k_place.h"
#include <algorithm>
#include <memory>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

// ------------------------------------------------------------------------------------------------ host side
// The side streams of the event DP with their fork / join events: the size classes run side by side (a class is a handful of
// long-running blocks, never a full chip).  Made on first use, destroyed with the workspace.
struct NwLanes {
    hipStream_t side[3] = {nullptr, nullptr, nullptr};
    hipEvent_t fork = nullptr, join[3] = {nullptr, nullptr, nullptr};
    NwLanes() = default;
    NwLanes(const NwLanes &) = delete;
    NwLanes &operator=(const NwLanes &) = delete;
    ~NwLanes()
    {
        for (int i = 0; i < 3; i++) { if (side[i]) (void)hipStreamDestroy(side[i]); if (join[i]) (void)hipEventDestroy(join[i]); }
        if (fork) (void)hipEventDestroy(fork);
    }
    int ready(fsv_ctx *ctx)
    {
        if (fork) return FSV_OK;
        FSV_HIP(ctx, hipEventCreateWithFlags(&fork, hipEventDisableTiming));
        for (int i = 0; i < 3; i++) {
            FSV_HIP(ctx, hipStreamCreateWithFlags(&side[i], hipStreamNonBlocking));
            FSV_HIP(ctx, hipEventCreateWithFlags(&join[i], hipEventDisableTiming));
        }
        return FSV_OK;
    }
};

// Everything frees itself; members go in reverse order: the boxes' workspace, the lanes, the buffers.
struct AlnWs {
    Dev<uint32_t> store, word_off, pair_q, pair_t, sk_ends, sk_low, sk_high, mz_off, mz_cnt, warn, ev_count, cg, cg_n;
    Dev<uint32_t> nmask;      // FSV_NM_LEAD lead words (the first: "some window has an N"), then a mask word per store word
    Dev<int32_t> len, rows, scores, gap_shift;
    Dev<char> ascii;
    Dev<uint64_t> asc_off, chain;
    Dev<uint8_t> wper, bt;
    Dev<uint16_t> thin;
    Dev<fsv_mz> mz;
    Dev<AlnHeader> hdr;
    Dev<AlnEvent> events, ev_packed;
    Dev<NwTask> tasks;
    Dev<GapQuery> gaps;
    Dev<BoxSrc> box_src;
    Dev<CornerTask> corner;
    Dev<int2> corner_out;
    // fsv_aln_tags: per task its (contig, window), the caller's CIGARs, byte counts / offsets / NM, the cs bytes
    Dev<uint32_t> tag_q, tag_t, tag_cg;
    Dev<TagTask> tag_tasks;
    Dev<uint64_t> tag_cnt, tag_off;
    Dev<int32_t> tag_nm;
    Dev<char> tag_cs;
    // what the last fsv_align_batch left packed in store (n_refs windows, then n_contigs contigs); n_contigs 0: nothing
    struct Resident { uint32_t n_refs = 0, n_contigs = 0; std::vector<int32_t> len; std::vector<uint32_t> pair_t; } resident;
    fsv_aln_stats stats = {};
    NwLanes lanes;
    std::unique_ptr<AlnWs> sub;   // the workspace of the boxes of oversize events (a second, smaller alignment pass), made by the first box
    const uint32_t *nm() const { return nmask.p + FSV_NM_LEAD; }     // the N mask of the store (the kernels drop it when the batch has no N: nm_active)
};

void aln_ws_free(fsv_ctx *ctx)
{
    delete (AlnWs *)ctx->aln_ws;
    ctx->aln_ws = nullptr;
}

AlnWs *aln_ws_get(fsv_ctx *ctx)
{
    if (!ctx->aln_ws) { ctx->aln_ws = new AlnWs(); ctx->aln_ws_free = aln_ws_free; }
    return (AlnWs *)ctx->aln_ws;
}

// What every kernel that reads bases starts from: the store and its N mask, the word offsets and lengths and the slots'
// (query, target), as the one kernel argument PairSeqs; a block makes its PairView from it.
PairSeqs pair_seqs(const AlnWs &W) { return PairSeqs{W.store.p, W.nm(), W.word_off.p, W.len.p, W.pair_q.p, W.pair_t.p}; }
// the two kernels with a form per pass, each named once: SUB = false contigs against their windows, true the boxes (depth 1)
template <bool SUB> int launch_chain_aln(fsv_ctx *ctx, const AlnWs &W, uint32_t np, uint32_t R, const fsv_aln_params &P)
{
    FSV_LAUNCH(ctx, ctx->stream, k_chain_aln<SUB>, dim3(np), dim3(64), 0, W.len.p, W.mz.p, W.mz_off.p, W.mz_cnt.p, W.pair_q.p, W.pair_t.p, W.chain.p, W.hdr.p, R, P);
    return FSV_OK;
}
template <bool SUB> int launch_events(fsv_ctx *ctx, const AlnWs &W, uint32_t ns, const fsv_aln_params &P)
{
    FSV_LAUNCH(ctx, ctx->stream, k_aln_events<SUB>, dim3(ns), dim3(256), 0, pair_seqs(W), W.chain.p, W.hdr.p, W.events.p, W.ev_packed.p, W.ev_count.p, P);
    return FSV_OK;
}

// Sequences laid end to end, unit(length) elements each: off[r] the first element of sequence r, off[n] the total, which with
// `slack` elements behind it must stay below 2^32 (the kernels' offsets are 32-bit).  The store's words and the minimizer slots.
template <class L, class F> int lay_out(fsv_ctx *ctx, const std::vector<L> &len, F unit, uint64_t slack, std::vector<uint32_t> &off)
{
    const size_t n = len.size();
    off.assign(n + 1, 0);
    uint64_t t = 0;
    for (size_t r = 0; r < n; r++) { off[r] = (uint32_t)t; t += unit((uint64_t)len[r]); }
    if (t + slack >= (1ull << 32)) return fsv_fail(ctx, FSV_EUNSUP, "alignment batch too large; split it");
    off[n] = (uint32_t)t;
    return FSV_OK;
}
inline uint64_t store_words(uint64_t len) { return (len + 15) / 16; }
constexpr uint64_t STORE_SLACK = 8;   // words of room behind a store, zeroed (wide fetches run past the last base)

// room for a store of w words and its N mask, the slack behind both zeroed.  clear_lead: the "some window has an N" word as
// well, for k_pack_ascii to set (the host never looks at the text); k_extract_boxes copies that word from its source
int store_room(fsv_ctx *ctx, AlnWs &W, uint64_t w, bool clear_lead)
{
    TRY(ensure(ctx, W.store, w + STORE_SLACK));
    FSV_HIP(ctx, hipMemsetAsync(W.store.p + w, 0, 32, ctx->stream));
    TRY(ensure(ctx, W.nmask, w + STORE_SLACK + FSV_NM_LEAD));
    if (clear_lead) TRY(zero(ctx, W.nmask, FSV_NM_LEAD));
    FSV_HIP(ctx, hipMemsetAsync(W.nmask.p + FSV_NM_LEAD + w, 0, 32, ctx->stream));
    return FSV_OK;
}

// packs pairs (query, target) into a store; returns lens / offsets
// sequences (already concatenated by the caller in two buffers: reference windows, contigs) -> device 2-bit store
int pack_pairs(fsv_ctx *ctx, AlnWs &W, const std::vector<const char *> &seq, const std::vector<uint64_t> &slen, std::vector<uint32_t> &word_off,
               std::vector<int32_t> &len, const char *dev_src = nullptr, uint32_t dev_first = 0)
{
    const uint32_t n = (uint32_t)seq.size();
    TRY(lay_out(ctx, slen, store_words, STORE_SLACK, word_off));
    const uint64_t w = word_off[n];
    len.resize(n);
    std::vector<uint64_t> asc_off(n + 1, 0);
    for (uint32_t r = 0; r < n; r++) { len[r] = (int32_t)slen[r]; asc_off[r + 1] = asc_off[r] + slen[r]; }
    TRY(ensure(ctx, W.ascii, asc_off[n] + 64));
    // consecutive sequences that are adjacent in host memory go up in one copy (the callers pass two contiguous buffers)
    // sequences dev_first.. are already on the device, back to back at dev_src (contigs of the last assembly): one D2D copy
    const uint32_t n_host = dev_src ? dev_first : n;
    if (dev_src && n > dev_first)
        FSV_HIP(ctx, hipMemcpyAsync(W.ascii.p + asc_off[dev_first], dev_src, asc_off[n] - asc_off[dev_first], hipMemcpyDeviceToDevice, ctx->stream));
    for (uint32_t r = 0; r < n_host;) {
        uint32_t e = r + 1;
        while (e < n_host && seq[e] == seq[e - 1] + slen[e - 1]) e++;
        FSV_HIP(ctx, hipMemcpyAsync(W.ascii.p + asc_off[r], seq[r], asc_off[e] - asc_off[r], hipMemcpyHostToDevice, ctx->stream));
        r = e;
    }
    TRY(upload(ctx, W.asc_off, asc_off));
    TRY(upload(ctx, W.word_off, word_off));
    TRY(upload(ctx, W.len, len));
    TRY(store_room(ctx, W, w, true));
    FSV_LAUNCH(ctx, ctx->stream, k_pack_ascii, dim3(fsv_grid_for(w, 256)), dim3(256), 0, W.ascii.p, W.asc_off.p, W.word_off.p, W.len.p, n, (uint32_t)w, W.store.p, W.nmask.p + FSV_NM_LEAD);
    return FSV_OK;
}

// the event DP's size classes: 0 a short query, 3 a short target side under a long query (insertions: the row-owning
// single-wave kernel), 1 queries whose rolling rows fit in LDS, 2 the rest
inline int nw_class(int ql, int tl) { return ql <= 256 ? 0 : tl <= 256 ? 3 : ql <= NW_LDS_Q ? 1 : 2; }
inline uint64_t nw_bt_bytes(int ql, int tl) { return (uint64_t)(ql + tl) * (uint64_t)(nw_class(ql, tl) == 3 ? tl : ql); }   // diagonal-major traceback bytes

int run_nw(fsv_ctx *ctx, AlnWs &W, const std::vector<NwTask> &tasks, uint64_t bt_bytes, uint64_t row_words, const fsv_aln_params &P)
{
    // size classes, each a contiguous range of the (stably) reordered task array; outputs keep their task index
    const size_t n = tasks.size();
    std::vector<uint32_t> order;
    order.reserve(n);
    size_t cls_end[4];
    for (int c = 0; c < 4; c++) {
        for (size_t i = 0; i < n; i++)
            if (nw_class(tasks[i].ql, tasks[i].tl) == c) order.push_back((uint32_t)i);
        cls_end[c] = order.size();
    }
    std::vector<NwTask> sorted(n);
    for (size_t i = 0; i < n; i++) { sorted[i] = tasks[order[i]]; sorted[i].cg_off = order[i] * (uint32_t)ALN_CG_CAP; sorted[i].out_idx = order[i]; }
    TRY(upload(ctx, W.tasks, sorted));
    TRY(ensure(ctx, W.bt, bt_bytes + 16));
    TRY(ensure(ctx, W.rows, row_words + 4));
    TRY(ensure(ctx, W.cg, n * (size_t)ALN_CG_CAP));
    TRY(ensure(ctx, W.cg_n, n));
    TRY(ensure(ctx, W.scores, n));
    NwLanes &L = W.lanes;
    TRY(L.ready(ctx));
    // class c runs on its own stream between a fork and a join on the context's stream (class 0 stays on it)
    FSV_HIP(ctx, hipEventRecord(L.fork, ctx->stream));
    auto lane = [&](int c) -> hipStream_t { return c == 0 ? ctx->stream : L.side[c - 1]; };
    auto first = [&](int c) -> const NwTask * { return W.tasks.p + (c ? cls_end[c - 1] : 0); };
    auto count = [&](int c) -> size_t { return cls_end[c] - (c ? cls_end[c - 1] : 0); };
    for (int c = 1; c < 4; c++)
        if (count(c)) FSV_HIP(ctx, hipStreamWaitEvent(L.side[c - 1], L.fork, 0));
    const PairSeqs S = pair_seqs(W);
    const NwOut O{W.cg.p, W.cg_n.p, W.scores.p};
    if (count(0)) FSV_LAUNCH(ctx, lane(0), (k_nw<256, 64>), dim3((uint32_t)count(0)), dim3(64), 0, S, W.hdr.p, first(0), W.bt.p, O, P);
    if (count(1)) FSV_LAUNCH(ctx, lane(1), (k_nw<NW_LDS_Q, 1024>), dim3((uint32_t)count(1)), dim3(1024), 0, S, W.hdr.p, first(1), W.bt.p, O, P);
    if (count(2)) FSV_LAUNCH(ctx, lane(2), k_nw_any, dim3((uint32_t)count(2)), dim3(256), 0, S, W.hdr.p, first(2), W.bt.p, W.rows.p, O, P);
    if (count(3)) FSV_LAUNCH(ctx, lane(3), (k_nw_rows<256, 64>), dim3((uint32_t)count(3)), dim3(64), 0, S, W.hdr.p, first(3), W.bt.p, O, P);
    for (int c = 1; c < 4; c++)
        if (count(c)) { FSV_HIP(ctx, hipEventRecord(L.join[c - 1], L.side[c - 1])); FSV_HIP(ctx, hipStreamWaitEvent(ctx->stream, L.join[c - 1], 0)); }
    return FSV_OK;
}

void push_cg(std::vector<uint32_t> &cg, uint32_t op, uint32_t len)
{
    if (!len) return;
    if (!cg.empty() && (cg.back() & 0xf) == op) cg.back() += len << 4;
    else cg.push_back(len << 4 | op);
}
void push_all(std::vector<uint32_t> &cg, const uint32_t *runs, size_t n) { for (size_t i = 0; i < n; i++) push_cg(cg, runs[i] & 0xf, runs[i] >> 4); }

// What one pass aligns: n_refs targets then n_pairs queries, already packed in W.store (word_off / len uploaded), pair p =
// (query n_refs + p, target pair_t[p]).
struct PassIn {
    uint32_t n_refs = 0, n_pairs = 0;
    std::vector<uint32_t> word_off; std::vector<int32_t> len;
    std::vector<uint8_t> wper; std::vector<uint16_t> thin;   // minimizer window / thinning factor per sequence
    std::vector<uint32_t> pair_t;
    std::vector<int32_t> pre_status;                           // per pair: != 0 -> not aligned, reported as is
};
// per record slot (n_pairs x R): header, status, and the ops between the record's first and last aligned base (no clips)
struct PassOut { uint32_t R = 1; std::vector<AlnHeader> hdr; std::vector<int32_t> status; std::vector<std::vector<uint32_t>> body; };

// seed window of a pair whose longer side has L bases (oracle/aln.c:seed_window): w = max(w0, L / per + 1); beyond 255 (the
// sketch kernels' limit) w stays 255 and every thin-th minimizer by hash survives, on both sides alike
inline void seed_window(int w0, uint64_t L, uint64_t per, uint8_t &w_out, uint16_t &thin_out)
{
    uint64_t w = std::max<uint64_t>((uint64_t)w0, L / per + 1);
    thin_out = 1;
    if (w > 255) { thin_out = (uint16_t)std::min<uint64_t>((w + 254) / 255, 65535); w = 255; }
    w_out = (uint8_t)w;
}

// What a pass carries from stage to stage.  depth 0: contigs against their windows (ALN_MAX_REC record slots per contig, X-drop
// ends); depth 1: the boxes of the first pass's oversize events, end to end (one slot each, no statistics).
struct Big { uint32_t slot; int32_t qs, qe, ts, te; };   // an oversize event: a box for the second pass (depth 0), a corner task (inside a box)
struct EvRef { bool big; uint32_t at; };                 // an event of a slot: tasks[at], or bigs[at]
constexpr uint32_t CG_HEAD = 8;                          // CIGAR runs of a DP event that come back with the batch's one strided copy
struct Pass {
    fsv_ctx *ctx; const PassIn &S; const fsv_aln_params &P; const int depth; PassOut &O; fsv_aln_stats *stats;   // stats: null at depth 1
    const uint32_t np, nr, R, ns;                        // pairs, sequences, record slots per pair and in all
    Trace trace;
    std::vector<AlnEvent> events;                        // of all slots, packed (hdr[p].ev_off)
    std::vector<NwTask> tasks; uint64_t bt = 0, rows = 0;       // the DP tasks with their traceback bytes and HBM row words
    std::vector<Big> bigs;
    std::vector<std::vector<EvRef>> slot_ev;             // per slot, its events in order
    std::vector<uint32_t> cg_n, cg_head;                 // per task: number of runs (0xffffffff: beyond ALN_CG_CAP), its first CG_HEAD runs
    std::vector<std::vector<uint32_t>> cg_long, big_cg;  // per task with more runs: all of them; per oversize event: its ops
    Pass(fsv_ctx *c, const PassIn &s, const fsv_aln_params &p, int d, PassOut &o, fsv_aln_stats *st)
        : ctx(c), S(s), P(p), depth(d), O(o), stats(st), np(s.n_pairs), nr(s.n_refs + s.n_pairs), R(d == 0 ? ALN_MAX_REC : 1), ns(np * R) { O.R = R; }
    int32_t slot_status(uint32_t p) const { return S.pre_status[p / R] != 0 ? S.pre_status[p / R] : O.hdr[p].status; }
    const uint32_t *runs_of(size_t t) const { return cg_n[t] > CG_HEAD ? cg_long[t].data() : cg_head.data() + t * CG_HEAD; }
};

int align_pass(fsv_ctx *ctx, AlnWs &W, const PassIn &S, const fsv_aln_params &P, int depth, PassOut &O, fsv_aln_stats *stats);

// minimizers of every sequence, thinned where the window is capped, those that occur too often in their sequence dropped
int seed_stage(Pass &A, AlnWs &W)
{
    fsv_ctx *ctx = A.ctx; const PassIn &S = A.S; const uint32_t nr = A.nr;
    Timer t(ctx);
    A.trace = Trace{ctx, A.depth ? "align (boxes)" : "align"};
    TRY(upload(ctx, W.wper, S.wper));
    // kernels index pairs by record slot
    {
        std::vector<uint32_t> sq(A.ns), st(A.ns);
        for (uint32_t p = 0; p < A.np; p++) for (uint32_t r = 0; r < A.R; r++) { sq[p * A.R + r] = S.n_refs + p; st[p * A.R + r] = S.pair_t[p]; }
        TRY(upload(ctx, W.pair_q, sq));
        TRY(upload(ctx, W.pair_t, st));
    }
    std::vector<uint32_t> mz_off;
    TRY(lay_out(ctx, S.len, [](uint64_t len) { return len + 64; }, 0, mz_off));     // worst case one minimizer per base
    TRY(upload(ctx, W.mz_off, mz_off));
    TRY(ensure(ctx, W.mz, mz_off[nr]));
    TRY(ensure(ctx, W.mz_cnt, nr));
    TRY(ensure(ctx, W.warn, nr));
    TRY(zero(ctx, W.warn, nr));
    uint32_t max_words = 1; int w_max = 1;      // (the replay kernel's LDS tile: even k only)
    if (!(A.P.k & 1))
        for (uint32_t r = 0; r < nr; r++) { max_words = std::max<uint32_t>(max_words, (uint32_t)((S.len[r] + 15) / 16)); w_max = std::max<int>(w_max, S.wper[r]); }
    TRY(launch_sketch(ctx, W, SketchJob{W.store.p, nr, S.word_off[nr], max_words, A.P.w, A.P.k, 0, W.wper.p, w_max, false, nullptr}));
    bool any_thin = false;
    for (uint32_t r = 0; r < nr; r++) any_thin |= S.thin[r] > 1;
    if (any_thin) {
        TRY(upload(ctx, W.thin, S.thin));
        FSV_LAUNCH(ctx, ctx->stream, k_thin_seeds, dim3(nr), dim3(256), 0, W.mz.p, W.mz_off.p, W.mz_cnt.p, W.thin.p);
    }
    // first pass: seeds unique in their sequence; boxes: seeds that occur at most twice in their side
    FSV_LAUNCH(ctx, ctx->stream, k_uniq<ALN_AMAX>, dim3(nr), dim3(256), 0, W.mz.p, W.mz_off.p, W.mz_cnt.p, W.warn.p, (const uint32_t *)nullptr, 0u, 0xffffffffu, (unsigned long long *)nullptr, A.depth == 0 ? 1u : (uint32_t)ALN_SUB_OCC);
    A.trace("sketch+uniq");
    if (A.stats) A.stats->ms_seed = t.stop();
    return FSV_OK;
}

int chain_stage(Pass &A, AlnWs &W)
{
    fsv_ctx *ctx = A.ctx;
    Timer t(ctx);
    TRY(ensure(ctx, W.chain, (size_t)A.ns * ALN_CHAIN_STRIDE));
    TRY(ensure(ctx, W.hdr, A.ns));
    TRY(ensure(ctx, W.events, (size_t)A.ns * ALN_EV_CAP));
    TRY(A.depth == 0 ? launch_chain_aln<false>(ctx, W, A.np, A.R, A.P) : launch_chain_aln<true>(ctx, W, A.np, A.R, A.P));
    A.trace("chain");
    if (A.stats) A.stats->ms_chain = t.stop();
    return FSV_OK;
}

// the walk along every chain: headers and the packed events, down to the host
int event_stage(Pass &A, AlnWs &W)
{
    fsv_ctx *ctx = A.ctx;
    Timer t(ctx);
    TRY(ensure(ctx, W.ev_packed, (size_t)A.ns * ALN_EV_CAP));
    TRY(ensure(ctx, W.ev_count, 4));
    TRY(zero(ctx, W.ev_count, 1));
    TRY(A.depth == 0 ? launch_events<false>(ctx, W, A.ns, A.P) : launch_events<true>(ctx, W, A.ns, A.P));
    A.O.hdr.assign(A.ns, AlnHeader());
    uint32_t n_ev = 0;
    TRY(download(ctx, A.O.hdr.data(), W.hdr, A.ns));
    TRY(download(ctx, &n_ev, W.ev_count, 1));
    FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    A.events.resize(n_ev);
    if (n_ev) {
        TRY(download(ctx, A.events.data(), W.ev_packed, n_ev));
        FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    A.trace("events");
    if (A.stats) A.stats->ms_events = t.stop();
    return FSV_OK;
}

// host only: every event of every live slot becomes a DP task or, listed with qs < 0 (more than max_cells cells), an oversize event
void plan_dp(Pass &A)
{
    A.slot_ev.assign(A.ns, std::vector<EvRef>());
    for (uint32_t p = 0; p < A.ns; p++) {   // p: record slot; pair = p / R
        if (A.slot_status(p) != 0) continue;
        const AlnHeader &h = A.O.hdr[p];
        for (int e = 0; e < h.n_events; e++) {
            const AlnEvent &ev = A.events[(size_t)h.ev_off + e];
            if (ev.qs < 0) {
                A.slot_ev[p].push_back(EvRef{true, (uint32_t)A.bigs.size()});
                A.bigs.push_back(Big{p, -1 - ev.qs, ev.qe, ev.ts, ev.te});
                continue;
            }
            NwTask t;
            t.out_idx = 0; t.pad = 0;
            t.pair = p; t.qs = ev.qs; t.ql = ev.qe - ev.qs + 1; t.ts = ev.ts; t.tl = ev.te - ev.ts + 1;
            t.cg_off = (uint32_t)(A.tasks.size() * ALN_CG_CAP); t.bt_off = A.bt; t.row_off = A.rows;
            A.bt += nw_bt_bytes(t.ql, t.tl);
            if (nw_class(t.ql, t.tl) == 2) A.rows += 11ull * t.ql;
            if (A.stats) { A.stats->dp_cells += (uint64_t)t.ql * t.tl; A.stats->algo_bytes += (uint64_t)(t.ql + t.tl + 3) / 4; }
            A.slot_ev[p].push_back(EvRef{false, (uint32_t)A.tasks.size()});
            A.tasks.push_back(t);
        }
    }
}

// the DP of all tasks and their CIGAR runs: nearly all have a handful; the first CG_HEAD runs of every task come back in one
// strided copy, longer ones are fetched individually
int dp_stage(Pass &A, AlnWs &W)
{
    fsv_ctx *ctx = A.ctx; const size_t n = A.tasks.size();
    A.cg_n.assign(n, 0); A.cg_head.assign(n * (size_t)CG_HEAD, 0); A.cg_long.assign(n, std::vector<uint32_t>());
    if (n) {
        if (n * (uint64_t)ALN_CG_CAP >= (1ull << 32)) return fsv_fail(ctx, FSV_EUNSUP, "too many DP events in one batch");
        TRY(run_nw(ctx, W, A.tasks, A.bt, A.rows, A.P));
        TRY(download(ctx, A.cg_n.data(), W.cg_n, n));
        FSV_HIP(ctx, hipMemcpy2DAsync(A.cg_head.data(), CG_HEAD * 4, W.cg.p, (size_t)ALN_CG_CAP * 4, CG_HEAD * 4, n, hipMemcpyDeviceToHost, ctx->stream));
        FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
        bool any = false;
        for (size_t t = 0; t < n; t++)
            if (A.cg_n[t] != 0xffffffffu && A.cg_n[t] > CG_HEAD) {
                A.cg_long[t].resize(A.cg_n[t]);
                FSV_HIP(ctx, hipMemcpyAsync(A.cg_long[t].data(), W.cg.p + t * (size_t)ALN_CG_CAP, (size_t)A.cg_n[t] * 4, hipMemcpyDeviceToHost, ctx->stream));
                any = true;
            }
        if (any) FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    A.trace("dp");
    return FSV_OK;
}

// depth 0: every oversize event becomes a (query, target) pair of a second pass, its two sides cut out of this pass's store
int box_pass(Pass &A, AlnWs &W)
{
    fsv_ctx *ctx = A.ctx; const PassIn &S = A.S;
    if (!W.sub) W.sub.reset(new AlnWs());
    AlnWs &W2 = *W.sub;
    const uint32_t nb = (uint32_t)A.bigs.size();
    PassIn S2;
    S2.n_refs = nb; S2.n_pairs = nb;
    S2.len.resize(2 * nb); S2.wper.resize(2 * nb); S2.thin.resize(2 * nb); S2.pair_t.resize(nb); S2.pre_status.assign(nb, 0);
    std::vector<BoxSrc> src(2 * nb);
    for (uint32_t b = 0; b < nb; b++) {
        const Big &B = A.bigs[b];
        const uint32_t rq = S.n_refs + B.slot / A.R, rt = S.pair_t[B.slot / A.R];
        S2.len[b] = B.te - B.ts + 1; S2.len[nb + b] = B.qe - B.qs + 1;
        src[b] = BoxSrc{S.word_off[rt], S.len[rt], 0, B.ts};
        src[nb + b] = BoxSrc{S.word_off[rq], S.len[rq], A.O.hdr[B.slot].rev, B.qs};
        S2.pair_t[b] = b;
        seed_window(A.P.w, (uint64_t)std::max(S2.len[b], S2.len[nb + b]), ALN_SUB_PER, S2.wper[b], S2.thin[b]);
        S2.wper[nb + b] = S2.wper[b]; S2.thin[nb + b] = S2.thin[b];
    }
    TRY(lay_out(ctx, S2.len, store_words, STORE_SLACK, S2.word_off));
    const uint32_t w = S2.word_off[2 * nb];
    TRY(upload(ctx, W2.word_off, S2.word_off));
    TRY(upload(ctx, W2.len, S2.len));
    TRY(upload(ctx, W2.box_src, src));
    TRY(store_room(ctx, W2, w, false));
    FSV_LAUNCH(ctx, ctx->stream, k_extract_boxes, dim3(fsv_grid_for(w, 256)), dim3(256), 0, W.store.p, W.nm(), W2.box_src.p, W2.word_off.p, W2.len.p, 2 * nb, w, W2.store.p, W2.nmask.p + FSV_NM_LEAD);
    PassOut O2;
    TRY(align_pass(ctx, W2, S2, A.P, 1, O2, nullptr));
    for (uint32_t b = 0; b < nb; b++) {
        if (O2.status[b] != 0) return fsv_fail(ctx, FSV_EINTERNAL, "a box of an oversize event came back without an alignment");
        A.big_cg[b].swap(O2.body[b]);
    }
    if (A.stats) A.stats->n_boxes += nb;
    A.trace("boxes");
    return FSV_OK;
}

// depth 1: what is still too large inside a box is closed from its corners, the rest one insertion + one deletion
int corner_pass(Pass &A, AlnWs &W)
{
    fsv_ctx *ctx = A.ctx; const size_t nb = A.bigs.size();
    std::vector<CornerTask> ct(nb);
    for (size_t b = 0; b < nb; b++) { const Big &B = A.bigs[b]; ct[b] = CornerTask{B.slot, B.qs, B.qe - B.qs + 1, B.ts, B.te - B.ts + 1}; }
    std::vector<int2> lr(nb);
    TRY(upload(ctx, W.corner, ct));
    TRY(ensure(ctx, W.corner_out, nb));
    FSV_LAUNCH(ctx, ctx->stream, k_corner, dim3((uint32_t)nb), dim3(64), 0, pair_seqs(W), W.hdr.p, W.corner.p, W.corner_out.p, A.P);
    TRY(download(ctx, lr.data(), W.corner_out, nb));
    FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t b = 0; b < nb; b++) {
        const int ql = ct[b].ql, tl = ct[b].tl, l = lr[b].x, r = lr[b].y;
        std::vector<uint32_t> &c = A.big_cg[b];
        push_cg(c, 0, (uint32_t)l); push_cg(c, 1, (uint32_t)(ql - l - r)); push_cg(c, 2, (uint32_t)(tl - l - r)); push_cg(c, 0, (uint32_t)r);
    }
    A.trace("corners");
    return FSV_OK;
}

int oversize_stage(Pass &A, AlnWs &W)
{
    A.big_cg.assign(A.bigs.size(), std::vector<uint32_t>());
    if (A.bigs.empty()) return FSV_OK;
    return A.depth == 0 ? box_pass(A, W) : corner_pass(A, W);
}

// host only: the ops of every record -- M up to an event, the event's runs, ..., M up to the record's last base
void emit_ops(Pass &A)
{
    A.O.status.assign(A.ns, 0); A.O.body.assign(A.ns, std::vector<uint32_t>());
    for (uint32_t p = 0; p < A.ns; p++) {
        int32_t st = A.slot_status(p);
        if (st == 0) {
            const AlnHeader &h = A.O.hdr[p];
            std::vector<uint32_t> &c = A.O.body[p];
            int mstart = h.qbeg;
            for (const EvRef e : A.slot_ev[p]) {
                if (!e.big) {
                    const NwTask &T = A.tasks[e.at];
                    push_cg(c, 0, (uint32_t)(T.qs - mstart));
                    if (A.cg_n[e.at] == 0xffffffffu) { st = FSV_ECAP; break; }
                    push_all(c, A.runs_of(e.at), A.cg_n[e.at]);
                    mstart = T.qs + T.ql;
                } else {
                    const Big &B = A.bigs[e.at];
                    push_cg(c, 0, (uint32_t)(B.qs - mstart));
                    push_all(c, A.big_cg[e.at].data(), A.big_cg[e.at].size());
                    mstart = B.qe + 1;
                }
            }
            if (st == 0) push_cg(c, 0, (uint32_t)(h.qend + 1 - mstart));
        }
        A.O.status[p] = st;
    }
}

// seeds -> chains -> events -> DP -> the ops of every record
int align_pass(fsv_ctx *ctx, AlnWs &W, const PassIn &S, const fsv_aln_params &P, int depth, PassOut &O, fsv_aln_stats *stats)
{
    Pass A(ctx, S, P, depth, O, stats);
    TRY(seed_stage(A, W));
    TRY(chain_stage(A, W));
    TRY(event_stage(A, W));
    Timer tdp(ctx);
    plan_dp(A);
    TRY(dp_stage(A, W));
    TRY(oversize_stage(A, W));
    if (stats) { stats->ms_dp = tdp.stop(); stats->n_events = A.tasks.size(); }
    emit_ops(A);
    return FSV_OK;
}

// ---- the stitcher: plain C++ over vectors but for the one k_gap_shift launch
// Every I / D run of a stitched CIGAR with an M run on either side, in CIGAR order: f(k, qoff, toff) with the run's index and the
// contig / reference offset of its first base (toff counted from tbeg).  The gap queries are collected and their answers applied
// through this one walk, so the two agree in order and count.  f may move bases between c[k - 1] and c[k + 1] (the offsets
// of later gaps are then stale: the shifts are applied without them).
template <class F> void each_flanked_gap(const std::vector<uint32_t> &c, int tbeg, F f)
{
    int toff = tbeg, qoff = 0;
    for (size_t k = 0; k < c.size(); k++) {
        const uint32_t op = c[k] & 0xf; const int l = (int)(c[k] >> 4);
        if ((op == 1 || op == 2) && k > 0 && k + 1 < c.size() && (c[k - 1] & 0xf) == 0 && (c[k + 1] & 0xf) == 0) f(k, qoff, toff);
        if (op == 0 || op == 2) toff += l;
        if (op == 0 || op == 1 || op == 4) qoff += l;
    }
}

// S, the record's ops, S -- one record per used slot of every contig, the primary first -- and, for every gap flanked by M, the
// question how far it could travel left.  A contig with a failed slot has no record; status: per contig.
struct Rec { uint32_t contig, slot; std::vector<uint32_t> c; };
void stitch_records(const PassIn &S, const PassOut &O, std::vector<Rec> &recs, std::vector<GapQuery> &gaps, std::vector<int32_t> &status)
{
    status.assign(S.n_pairs, 0);
    for (uint32_t cp = 0; cp < S.n_pairs; cp++) {
        int32_t st = O.status[cp * O.R];
        const size_t first_rec = recs.size(), first_gap = gaps.size();
        for (uint32_t r = 0; r < O.R && st == 0; r++) {
            const uint32_t p = cp * O.R + r;
            const AlnHeader &h = O.hdr[p];
            if (O.status[p] != 0) { if (O.status[p] != 1) st = O.status[p]; break; }   // slots fill up in order; 1 = an empty slot
            std::vector<uint32_t> c;
            push_cg(c, 4, (uint32_t)h.qbeg);
            push_all(c, O.body[p].data(), O.body[p].size());
            push_cg(c, 4, (uint32_t)(S.len[S.n_refs + cp] - 1 - h.qend));
            each_flanked_gap(c, h.tbeg, [&](size_t k, int qoff, int toff) {
                const bool ins = (c[k] & 0xf) == 1;
                gaps.push_back(GapQuery{p, ins, ins ? qoff : toff, (int)(c[k] >> 4), std::min(toff - h.tbeg, qoff - h.qbeg)});
            });
            recs.push_back(Rec{cp, p, std::move(c)});
        }
        if (st != 0) { recs.resize(first_rec); gaps.resize(first_gap); }
        status[cp] = st;
    }
}

// every flanked gap of c moved left by its answer, at most by the M run in front of it; an M run used up merges its neighbours.
// Takes the answers of c's gaps from `shift` and returns the first answer of the next CIGAR.
const int32_t *shift_gaps_left(std::vector<uint32_t> &c, const int32_t *shift)
{
    bool shrink = false;
    each_flanked_gap(c, 0, [&](size_t k, int, int) {
        const uint32_t prev = c[k - 1] >> 4, l = std::min<uint32_t>(prev, (uint32_t)*shift++);
        c[k - 1] -= l << 4; c[k + 1] += l << 4;
        shrink |= l == prev;
    });
    if (shrink) {
        std::vector<uint32_t> d;
        push_all(d, c.data(), c.size());
        c.swap(d);
    }
    return shift;
}

// the records of the batch into the caller's buffers, every gap at its leftmost position
int stitch(fsv_ctx *ctx, AlnWs &W, const PassIn &S, const PassOut &O, fsv_alns *out)
{
    std::vector<Rec> recs;
    std::vector<GapQuery> gaps;
    std::vector<int32_t> status;
    stitch_records(S, O, recs, gaps, status);
    std::vector<int32_t> max_shift(gaps.size());
    if (!gaps.empty()) {
        TRY(upload(ctx, W.gaps, gaps));
        TRY(ensure(ctx, W.gap_shift, gaps.size()));
        FSV_LAUNCH(ctx, ctx->stream, k_gap_shift, dim3((uint32_t)gaps.size()), dim3(64), 0, pair_seqs(W), W.hdr.p, W.gaps.p, W.gap_shift.p);
        TRY(download(ctx, max_shift.data(), W.gap_shift, gaps.size()));
        FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    const int32_t *shift = max_shift.data();
    for (Rec &rc : recs) {
        std::vector<uint32_t> &c = rc.c;
        shift = shift_gaps_left(c, shift);
        const AlnHeader &h = O.hdr[rc.slot];
        if (out->n_rec >= out->rec_cap) return fsv_fail(ctx, FSV_ECAP, "record buffer too small (rec_cap >= 5 x n_contigs holds every case)");
        if (out->n_cigar + c.size() > out->cigar_cap) return fsv_fail(ctx, FSV_ECAP, "cigar buffer too small");
        fsv_aln_rec &rr = out->rec[out->n_rec++];
        rr.ref_start = h.tbeg; rr.ref_end = h.tend + 1; rr.q_start = h.qbeg; rr.q_end = h.qend + 1; rr.n_cigar = (uint32_t)c.size();
        rr.n_chain = (uint32_t)h.n_chain; rr.cigar_off = out->n_cigar; rr.contig = rc.contig; rr.rev = (uint8_t)h.rev; rr.mapq = 60; rr.pad[0] = rr.pad[1] = 0;
        memcpy(out->cigar + out->n_cigar, c.data(), c.size() * 4);
        out->n_cigar += c.size();
        W.stats.algo_bytes += c.size() * 4;
    }
    for (uint32_t cp = 0; cp < S.n_pairs; cp++) {
        out->contig_status[cp] = status[cp];
        W.stats.algo_bytes += (uint64_t)(S.len[S.n_refs + cp] + S.len[S.pair_t[cp]] + 3) / 4;
    }
    return FSV_OK;
}

} // namespace

extern "C" void fsv_aln_default_params(fsv_aln_params *P)
{
    if (!P) return;
    P->k = 19; P->w = 19; P->min_anchors = 3; P->lookback = 64; P->max_gap = 50000;
    P->a = 1; P->b = 19; P->q = 39; P->e = 3; P->q2 = 81; P->e2 = 1;
    P->pad = 24; P->max_mm_run = 4; P->xdrop = 100; P->max_cells = 1 << 26;
}

extern "C" int fsv_aln_last_stats(const fsv_ctx *ctx, fsv_aln_stats *out)
{
    if (!ctx || !out || !ctx->aln_ws) return FSV_EINVAL;
    *out = ((const AlnWs *)ctx->aln_ws)->stats;
    return FSV_OK;
}

static int check_aln_params(fsv_ctx *ctx, const fsv_aln_params &P)
{
    if (P.k < 1 || P.k > 31 || P.w < 1 || P.w > 255 || P.lookback != 64 || P.min_anchors < 2 || P.pad < 0 || P.a < 0 || P.b < 0 || P.q < 0 || P.e < 0 || P.max_cells < 1 || P.max_gap < 0 || P.xdrop < 0)
        return fsv_fail(ctx, FSV_EINVAL, "fsv_aln_params out of range");
    return FSV_OK;
}

static int nw_impl(fsv_ctx *ctx, const char *target, int32_t tl, const char *query, int32_t ql, const fsv_aln_params *params, int32_t *score,
                   uint32_t *cigar, uint32_t cigar_cap, uint32_t *n_cigar)
{
    if (!ctx || !target || !query || tl < 1 || ql < 1 || !score || !cigar || !n_cigar) return FSV_EINVAL;
    fsv_aln_params P;
    if (params) P = *params; else fsv_aln_default_params(&P);
    TRY(check_aln_params(ctx, P));
    if ((int64_t)tl * ql > P.max_cells) return fsv_fail(ctx, FSV_EUNSUP, "event larger than max_cells");
    FSV_HIP(ctx, hipSetDevice(ctx->device));
    AlnWs &W = *aln_ws_get(ctx);
    W.resident = AlnWs::Resident();
    std::vector<uint32_t> word_off; std::vector<int32_t> len;
    TRY(pack_pairs(ctx, W, {query, target}, {(uint64_t)ql, (uint64_t)tl}, word_off, len));
    std::vector<AlnHeader> hdr(1); memset(&hdr[0], 0, sizeof(AlnHeader));
    TRY(upload(ctx, W.hdr, hdr));
    TRY(upload(ctx, W.pair_q, std::vector<uint32_t>{0u}));
    TRY(upload(ctx, W.pair_t, std::vector<uint32_t>{1u}));
    std::vector<NwTask> tasks(1);
    tasks[0] = NwTask{0u, 0, ql, 0, tl, 0u, 0ull, 0ull, 0u, 0u};
    TRY(run_nw(ctx, W, tasks, nw_bt_bytes(ql, tl), nw_class(ql, tl) == 2 ? 11ull * ql : 0, P));
    uint32_t n = 0; int32_t sc = 0;
    TRY(download(ctx, &n, W.cg_n, 1));
    TRY(download(ctx, &sc, W.scores, 1));
    FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (n == 0xffffffffu || n > cigar_cap) return FSV_ECAP;
    TRY(download(ctx, cigar, W.cg, n));
    FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *n_cigar = n; *score = sc;
    return FSV_OK;
}

// The batch as one pass's input: the reference windows first, then the contigs (seq / slen: where each sequence's text is, null
// for contigs that are on the device already).  Every window is sketched once with w = max(P.w, L/3000 + 1), L = the longest
// sequence of its group, and its contigs use the same w.
static int batch_input(fsv_ctx *ctx, const char *contig_seq, const uint64_t *contig_off, uint32_t n_contigs, const uint32_t *contig_ref,
                       const char *ref_seq, const uint64_t *ref_off, uint32_t n_refs, const fsv_aln_params &P, PassIn &S,
                       std::vector<const char *> &seq, std::vector<uint64_t> &slen)
{
    const uint32_t np = n_contigs, nr = n_refs + n_contigs;
    S.n_refs = n_refs; S.n_pairs = np;
    seq.resize(nr); slen.resize(nr);
    S.wper.resize(nr); S.thin.assign(nr, 1); S.pair_t.resize(np); S.pre_status.assign(np, 0);
    std::vector<uint64_t> group_len(n_refs, 0);
    for (uint32_t r = 0; r < n_refs; r++) {
        seq[r] = ref_seq + ref_off[r]; slen[r] = ref_off[r + 1] - ref_off[r];
        if (slen[r] == 0) return fsv_fail(ctx, FSV_EINVAL, "empty reference window");
        group_len[r] = slen[r];
    }
    for (uint32_t p = 0; p < np; p++) {
        if (contig_ref[p] >= n_refs) return fsv_fail(ctx, FSV_EINVAL, "contig_ref out of range");
        seq[n_refs + p] = contig_seq ? contig_seq + contig_off[p] : nullptr; slen[n_refs + p] = contig_off[p + 1] - contig_off[p];
        if (slen[n_refs + p] == 0) return fsv_fail(ctx, FSV_EINVAL, "empty contig");
        group_len[contig_ref[p]] = std::max(group_len[contig_ref[p]], slen[n_refs + p]);
        S.pair_t[p] = contig_ref[p];
    }
    // seeds of long windows: w grows with the longest sequence of the group; beyond w = 255 (~760 kb: the whole-genome BED has a
    // 1.15 Mb region) the minimizers are thinned by hash instead (k_thin_seeds), so any window below 2^23 bases is aligned
    for (uint32_t r = 0; r < n_refs; r++) seed_window(P.w, group_len[r], 3000, S.wper[r], S.thin[r]);
    for (uint32_t p = 0; p < np; p++) {
        const uint32_t r = contig_ref[p];
        const uint64_t L = group_len[r];
        S.wper[n_refs + p] = S.wper[r]; S.thin[n_refs + p] = S.thin[r];
        if (L >= (1u << 23) || (!(P.k & 1) && L / 3000 + 1 > 64)) S.pre_status[p] = FSV_EUNSUP; // the replay kernel (even k) holds w <= 64
        else if (slen[n_refs + p] < (uint64_t)P.k || slen[r] < (uint64_t)P.k) S.pre_status[p] = 1;
    }
    return FSV_OK;
}

static int align_batch_impl(fsv_ctx *ctx, const char *contig_seq, const uint64_t *contig_off, uint32_t n_contigs, const uint32_t *contig_ref,
                            const char *ref_seq, const uint64_t *ref_off, uint32_t n_refs, const fsv_aln_params *params, fsv_alns *out)
{
    if (!ctx || !out || !out->rec || !out->cigar || !out->contig_status) return FSV_EINVAL;
    out->n_rec = 0; out->n_cigar = 0;
    if (n_contigs == 0) return FSV_OK;
    // contig_seq == NULL: align the contigs of the last fsv_assemble_batch on this context straight from device memory
    const bool from_dev = contig_seq == nullptr;
    if (from_dev) {
        if (!ctx->last_contigs_dev || ctx->last_contig_off.size() != (size_t)n_contigs + 1) return fsv_fail(ctx, FSV_EINVAL, "no assembled contigs of that count on this context");
        contig_off = ctx->last_contig_off.data();
    }
    if (!contig_off || !contig_ref || !ref_seq || !ref_off) return FSV_EINVAL;
    if (out->rec_cap < n_contigs) return fsv_fail(ctx, FSV_ECAP, "rec_cap must be >= n_contigs");
    fsv_aln_params P;
    if (params) P = *params; else fsv_aln_default_params(&P);
    TRY(check_aln_params(ctx, P));
    FSV_HIP(ctx, hipSetDevice(ctx->device));
    AlnWs &W = *aln_ws_get(ctx);
    memset(&W.stats, 0, sizeof(W.stats));
    W.resident = AlnWs::Resident();
    Timer ttot(ctx);
    PassIn S;
    std::vector<const char *> seq; std::vector<uint64_t> slen;
    TRY(batch_input(ctx, contig_seq, contig_off, n_contigs, contig_ref, ref_seq, ref_off, n_refs, P, S, seq, slen));
    TRY(pack_pairs(ctx, W, seq, slen, S.word_off, S.len, from_dev ? ctx->last_contigs_dev + contig_off[0] : nullptr, n_refs));
    PassOut O;
    TRY(align_pass(ctx, W, S, P, 0, O, &W.stats));
    W.stats.n_pairs = n_contigs;
    TRY(stitch(ctx, W, S, O, out));
    W.stats.ms_total = ttot.stop();
    W.resident.n_refs = n_refs; W.resident.n_contigs = n_contigs; W.resident.len = S.len; W.resident.pair_t = S.pair_t;
    return FSV_OK;
}

// ---- fsv_aln_tags
constexpr int64_t TAG_TASK_COLS = 1 << 15;   // a record of more columns is cut into tasks of about this many, at op boundaries

// One record against its sequences' lengths.  Returns FSV_EUNSUP for an op outside M / I / D / S / H (the call fails), FSV_EINVAL for a
// CIGAR that does not fit (that record fails), else FSV_OK with the record's tasks appended.
static int tag_tasks_of(const fsv_aln_rec &r, const fsv_alns *alns, uint32_t n_contigs, const int32_t *len, uint32_t n_refs, const uint32_t *pair_t,
                        std::vector<TagTask> &tasks, std::vector<uint32_t> &tq, std::vector<uint32_t> &tt)
{
    if (r.cigar_off > alns->n_cigar || r.n_cigar > alns->n_cigar - r.cigar_off) return FSV_EINVAL;
    const uint32_t *c = alns->cigar + r.cigar_off;
    int64_t qsum = 0, tsum = 0;
    for (uint32_t k = 0; k < r.n_cigar; k++) {
        const uint32_t op = c[k] & 0xf; const int64_t l = c[k] >> 4;
        if (op != 0 && op != 1 && op != 2 && op != 4 && op != 5) return FSV_EUNSUP;
        if (op != 2) qsum += l;
        if (op == 0 || op == 2) tsum += l;
    }
    if (r.contig >= n_contigs) return FSV_EINVAL;
    const int64_t lenq = len[n_refs + r.contig], lent = len[pair_t[r.contig]];
    if (qsum != lenq || r.ref_start < 0 || (int64_t)r.ref_start + tsum != (int64_t)r.ref_end || (int64_t)r.ref_end > lent) return FSV_EINVAL;
    // tasks: cut in front of an op once the task holds TAG_TASK_COLS columns
    int64_t qp = 0, tp = r.ref_start, cols = 0;
    TagTask T{r.rev ? 1 : 0, 0, (int32_t)tp, (uint32_t)r.cigar_off, 0};
    for (uint32_t k = 0; k < r.n_cigar; k++) {
        const uint32_t op = c[k] & 0xf; const int64_t l = c[k] >> 4;
        if (cols >= TAG_TASK_COLS) {
            tasks.push_back(T); tq.push_back(n_refs + r.contig); tt.push_back(pair_t[r.contig]);
            T.q0 = (int32_t)qp; T.t0 = (int32_t)tp; T.op_off = (uint32_t)(r.cigar_off + k); T.n_ops = 0; cols = 0;
        }
        T.n_ops++;
        if (op != 2) qp += l;
        if (op == 0 || op == 2) tp += l;
        if (op <= 2) cols += l;
    }
    tasks.push_back(T); tq.push_back(n_refs + r.contig); tt.push_back(pair_t[r.contig]);
    return FSV_OK;
}

static int aln_tags_impl(fsv_ctx *ctx, const char *contig_seq, const uint64_t *contig_off, uint32_t n_contigs, const uint32_t *contig_ref,
                         const char *ref_seq, const uint64_t *ref_off, uint32_t n_refs, const fsv_alns *alns, struct fsv_aln_tags *out)
{
    if (!ctx || !alns || !out || !out->nm || !out->cs_off || !out->rec_status || (alns->n_rec && (!alns->rec || !alns->cigar))) return FSV_EINVAL;
    if ((contig_seq == nullptr) != (ref_seq == nullptr)) return fsv_fail(ctx, FSV_EINVAL, "contig_seq and ref_seq: both or neither");
    out->cs_bytes = 0; out->ms = 0;
    const uint32_t n_rec = alns->n_rec;
    if (alns->n_cigar >= (1ull << 32)) return fsv_fail(ctx, FSV_EUNSUP, "more than 2^32 CIGAR ops; split the batch");
    const bool resident = contig_seq == nullptr;
    AlnWs *Wp = (AlnWs *)ctx->aln_ws;
    std::vector<int32_t> len; std::vector<uint32_t> pair_t;
    std::vector<const char *> seq; std::vector<uint64_t> slen;
    if (resident) {
        if (!Wp || Wp->resident.n_contigs == 0 || Wp->resident.n_contigs != n_contigs || Wp->resident.n_refs != n_refs)
            return fsv_fail(ctx, FSV_EINVAL, "no sequences of an fsv_align_batch with these counts on this context");
        len = Wp->resident.len; pair_t = Wp->resident.pair_t;
    } else {
        if (!contig_off || !contig_ref || !ref_off || n_contigs == 0 || n_refs == 0) return FSV_EINVAL;
        seq.resize((size_t)n_refs + n_contigs); slen.resize(seq.size()); len.resize(seq.size()); pair_t.resize(n_contigs);
        for (uint32_t r = 0; r < n_refs; r++) { seq[r] = ref_seq + ref_off[r]; slen[r] = ref_off[r + 1] - ref_off[r]; }
        for (uint32_t p = 0; p < n_contigs; p++) {
            if (contig_ref[p] >= n_refs) return fsv_fail(ctx, FSV_EINVAL, "contig_ref out of range");
            seq[n_refs + p] = contig_seq + contig_off[p]; slen[n_refs + p] = contig_off[p + 1] - contig_off[p]; pair_t[p] = contig_ref[p];
        }
        for (size_t r = 0; r < seq.size(); r++) {
            if (slen[r] == 0 || slen[r] >= (1ull << 31)) return fsv_fail(ctx, FSV_EINVAL, "empty sequence, or one of 2^31 bases or more");
            len[r] = (int32_t)slen[r];
        }
    }
    // every record is checked before anything is launched; a record that does not fit its sequences never reaches a kernel
    std::vector<TagTask> tasks; std::vector<uint32_t> tq, tt, first_task(n_rec + 1, 0);
    for (uint32_t i = 0; i < n_rec; i++) {
        first_task[i] = (uint32_t)tasks.size();
        const int rc = tag_tasks_of(alns->rec[i], alns, n_contigs, len.data(), n_refs, pair_t.data(), tasks, tq, tt);
        if (rc == FSV_EUNSUP) return fsv_fail(ctx, FSV_EUNSUP, "a CIGAR op outside M / I / D / S / H");
        out->rec_status[i] = rc; out->nm[i] = rc == FSV_OK ? 0 : -1;
    }
    first_task[n_rec] = (uint32_t)tasks.size();
    const uint32_t nt = (uint32_t)tasks.size();
    for (uint32_t i = 0; i <= n_rec; i++) out->cs_off[i] = 0;
    if (nt == 0) return FSV_OK;
    FSV_HIP(ctx, hipSetDevice(ctx->device));
    AlnWs &W = *aln_ws_get(ctx);
    if (!resident) {
        W.resident = AlnWs::Resident();
        std::vector<uint32_t> word_off;
        TRY(pack_pairs(ctx, W, seq, slen, word_off, len));
    }
    TRY(upload(ctx, W.tag_q, tq));
    TRY(upload(ctx, W.tag_t, tt));
    TRY(upload(ctx, W.tag_tasks, tasks));
    TRY(ensure(ctx, W.tag_cg, (size_t)alns->n_cigar));
    FSV_HIP(ctx, hipMemcpyAsync(W.tag_cg.p, alns->cigar, (size_t)alns->n_cigar * 4, hipMemcpyHostToDevice, ctx->stream));
    TRY(ensure(ctx, W.tag_cnt, nt));
    TRY(ensure(ctx, W.tag_off, (size_t)nt + 1));
    TRY(ensure(ctx, W.tag_nm, nt));
    const PairSeqs S{W.store.p, W.nm(), W.word_off.p, W.len.p, W.tag_q.p, W.tag_t.p};
    Timer tc(ctx);
    FSV_LAUNCH(ctx, ctx->stream, k_aln_tags<false>, dim3(nt), dim3(64), 0, S, W.tag_tasks.p, W.tag_cg.p, (const uint64_t *)nullptr, (char *)nullptr, W.tag_cnt.p, W.tag_nm.p);
    FSV_LAUNCH(ctx, ctx->stream, k_aln_tags_scan, dim3(1), dim3(64), 0, W.tag_cnt.p, nt, W.tag_off.p);
    out->ms = tc.stop();
    std::vector<uint64_t> off((size_t)nt + 1); std::vector<int32_t> nm(nt);
    TRY(download(ctx, off.data(), W.tag_off, (size_t)nt + 1));
    TRY(download(ctx, nm.data(), W.tag_nm, nt));
    FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (uint32_t i = 0; i < n_rec; i++) {
        out->cs_off[i] = off[first_task[i]];
        for (uint32_t t = first_task[i]; t < first_task[i + 1]; t++) out->nm[i] += nm[t];
    }
    out->cs_off[n_rec] = off[nt];
    out->cs_bytes = off[nt];
    if (!out->cs) return FSV_OK;       // the sizing call
    if (out->cs_cap < out->cs_bytes) return fsv_fail(ctx, FSV_ECAP, "cs buffer too small (cs_bytes says how many are needed)");
    if (out->cs_bytes == 0) return FSV_OK;
    TRY(ensure(ctx, W.tag_cs, out->cs_bytes));
    Timer te(ctx);
    FSV_LAUNCH(ctx, ctx->stream, k_aln_tags<true>, dim3(nt), dim3(64), 0, S, W.tag_tasks.p, W.tag_cg.p, W.tag_off.p, W.tag_cs.p, (uint64_t *)nullptr, (int32_t *)nullptr);
    out->ms += te.stop();
    TRY(download(ctx, out->cs, W.tag_cs, out->cs_bytes));
    FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return FSV_OK;
}

extern "C" int fsv_nw(fsv_ctx *ctx, const char *target, int32_t tl, const char *query, int32_t ql, const fsv_aln_params *params, int32_t *score,
                      uint32_t *cigar, uint32_t cigar_cap, uint32_t *n_cigar)
{
    FSV_GUARD(ctx, nw_impl(ctx, target, tl, query, ql, params, score, cigar, cigar_cap, n_cigar));
}

extern "C" int fsv_align_batch(fsv_ctx *ctx, const char *contig_seq, const uint64_t *contig_off, uint32_t n_contigs, const uint32_t *contig_ref,
                               const char *ref_seq, const uint64_t *ref_off, uint32_t n_refs, const fsv_aln_params *params, fsv_alns *out)
{
    FSV_GUARD(ctx, align_batch_impl(ctx, contig_seq, contig_off, n_contigs, contig_ref, ref_seq, ref_off, n_refs, params, out));
}

extern "C" int fsv_aln_tags(fsv_ctx *ctx, const char *contig_seq, const uint64_t *contig_off, uint32_t n_contigs, const uint32_t *contig_ref,
                            const char *ref_seq, const uint64_t *ref_off, uint32_t n_refs, const fsv_alns *alns, struct fsv_aln_tags *out)
{
    FSV_GUARD(ctx, aln_tags_impl(ctx, contig_seq, contig_off, n_contigs, contig_ref, ref_seq, ref_off, n_refs, alns, out));
}

#include "aln_mapq.h"
