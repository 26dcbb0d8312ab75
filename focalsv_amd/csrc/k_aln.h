// k_aln.h -- the aligner's kernels (what they compute: aln.hip's table of contents).  Included by aln.hip only.
//
// The pieces the kernels share, each written once:
//   PairSeqs, PairView                 a batch's sequences as one kernel argument; one slot's (contig, window) pair and its bases
//   ChainLds, chain_contig / chain_box k_chain_aln's LDS state with the steps on it, and its two bodies
//   seq_of_word                        which sequence of a store owns a word (k_extract_boxes, k_pack_ascii)
//   NwRows, nw_cell, nw_backtrack      the event DP's rolling rows, its recurrence and its traceback walk
//   NwJob, nw_finish                   what every DP kernel sets up from its task, and how it ends
//   nw_sweep_lds, lds_barrier          the anti-diagonal sweep with the rows in LDS (k_nw, k_nw_rows)
//   wave_incl_sum / wave_incl_max (fsv_internal.h), mz_lower_bound (k_sketch.h)
#pragma once
#include "k_sketch.h"

namespace {

#define ALN_AMAX 8192
#define ALN_CHAIN_STRIDE (ALN_AMAX + 8)   // anchors of one record slot (a box's chain carries its two fixed end pairs as well)
#define ALN_MAX_REC 5       // records per contig: up to ALN_MAJ_REC chains on its majority strand, the part behind a cut, one chain of the other strand
#define ALN_MAJ_REC 3       // the primary chain and up to two supplementary ones on the same strand
#define ALN_SUP_MIN 200     // chain score a supplementary chain needs
#define ALN_SUB_OCC 2       // an event larger than max_cells is seeded again: minimizers occurring at most this often in each side of its box
#define ALN_SUB_PER 1500    // ... with a minimizer window of max(w, L / 1500 + 1), L = the box's longer side
#define ALN_EV_CAP 2048      // events per pair
#define ALN_CG_CAP 1024      // CIGAR runs per event
#define NW_LDS_Q 3072        // query length up to which the rolling DP rows live in LDS (11 x 4 B x 3072 = 132 KB of the CU's 160)
#define NW_NEG (-(1 << 29))

struct AlnHeader { int32_t qbeg, tbeg, qend, tend, n_events, n_chain, rev, status; uint32_t ev_off, pad; };   // ev_off: first event in the packed list
struct AlnEvent { int32_t qs, qe, ts, te; };   // inclusive
struct NwTask { uint32_t pair; int32_t qs, ql, ts, tl; uint32_t cg_off; uint64_t bt_off; uint64_t row_off; uint32_t out_idx, pad; };

__device__ __forceinline__ int ilog2_u32(uint32_t v) { return 31 - __clz((int)v); }

// ------------------------------------------------------------------------------------------------ chain
// k_chain_aln: one block (one wavefront) per contig; its records go to the slots p0 .. p0 + R - 1 (pair_q / pair_t / hdr / chain are per slot).
//   SUB = false: a contig against its reference window (oracle/aln.c:orc_aln_chains).  Seeds unique in both sequences; the
//     best chain on the contig's majority strand is the primary record, what it leaves uncovered is chained again (up to
//     ALN_MAJ_REC chains); then the anchors of the other strand are chained once -- an inverted piece of the contig: minimap2
//     reports it as a reverse-strand supplementary record and breaks the alignment around it, and DipPAV's split rule only pairs
//     consecutive records of one strand (extract_contig_signature_CCS.py:286), so an inversion yields no call.  When that
//     chain's span on the contig lies strictly between the k-mers of two consecutive anchors of a majority chain (both parts
//     keeping min_anchors anchors) the majority chain is cut there and the part behind the cut becomes one more record.
//   SUB = true: the box of an event larger than max_cells, seeded again on its own (oracle/aln.c:sub_align): minimizers that
//     occur at most twice in each side (k_uniq with max_occ = 2), every pair of equal hash on the same strand an anchor, one
//     chain, written between the two fixed base pairs (-1, -1) and (lenq - 1, lent - 1) -- the outer chain's anchors.

// the score anchor (qe, te) reaches behind anchor (qj, tj), whose own chain scores fj; ok: the two may be linked at all
__device__ __forceinline__ int chain_cand(int qe, int te, int qj, int tj, int fj, const fsv_aln_params &P, bool &ok)
{
    const int dq = qe - qj, dt = te - tj;
    ok = false;
    if (dq <= 0 || dt <= 0) return 0;
    const int gap = dq > dt ? dq - dt : dt - dq;
    if (gap > P.max_gap) return 0;
    int sc = min(min(dq, dt), P.k);
    if (gap) sc -= (gap >> 7) + (ilog2_u32((uint32_t)gap) >> 1) + 1;
    ok = true;
    return sc + fj;
}

// The block's LDS: the anchors and what the chain DP knows of them.  Every step below is taken by all 64 lanes together.
struct ChainLds {
    uint64_t key[ALN_AMAX];     // anchors, contig coordinate << 32 | reference coordinate, sorted
    int32_t f[ALN_AMAX];        // chain scores
    uint16_t aux[ALN_AMAX];     // predecessors (0xffff: none); while a contig's anchors are gathered: span | strand << 8

    // the DP step of anchor i as the sequential loop does it
    __device__ __forceinline__ void dp_step_seq(int i, int lane, const fsv_aln_params &P)
    {
        const uint64_t ki = key[i];
        const int qe = (int)(ki >> 32), te = (int)(uint32_t)ki;
        const int j = i - 1 - lane;
        bool ok = false; int cand = 0;
        if (j >= 0) { const uint64_t kj = key[j]; cand = chain_cand(qe, te, (int)(kj >> 32), (int)(uint32_t)kj, f[j], P, ok); }
        // scores can drop below zero here (gap penalty), so bias before packing; lanes without a legal predecessor sit out
        const int mine = ok ? ((cand + (1 << 20)) * 64 + (63 - lane)) : -1; // < 2^27
        const int bestp = wave_max_i32(mine);
        const int bests = bestp < 0 ? -(1 << 30) : (int)(bestp >> 6) - (1 << 20);
        if (bests > P.k) { if (mine == bestp) { f[i] = bests; aux[i] = (uint16_t)j; } }
        else if (lane == 0) { f[i] = P.k; aux[i] = 0xffff; }
        __syncthreads();
    }

    // chain DP over the n anchors in key, sorted by (contig, reference) coordinate: look back 64 anchors, the best-scoring
    // predecessor, the nearer one on ties (oracle/aln.c:chain_dp); returns the best chain's last anchor (the first on ties),
    // predecessors in aux, scores in f.  A contig against its own reference window is co-linear except at
    // its SVs, so 64 anchors are settled at once as in the assembler's k_chain: hypothesis "every anchor links to its
    // predecessor" (the scores are a prefix sum), proof that no other predecessor beats it (cand(i, j) <= f[j] + k: only the j
    // with f[j] + k > f[i] are evaluated), one sequential step where it fails.  Round 1 walked the anchors one by one, a
    // barrier and three LDS round trips each (4.3 ms for 50 kb contigs).
    __device__ __forceinline__ int chain_dp(int n, int lane, const fsv_aln_params &P)
    {
        if (n > 0) dp_step_seq(0, lane, P);
        for (int i0 = 1; i0 < n;) {
            const int nb = min(64, n - i0), i = i0 + lane;
            const bool in = lane < nb;
            int qe = 0, te = 0, sc1 = 0; bool ok1 = false;
            if (in) {
                const uint64_t ki = key[i], kp = key[i - 1];
                qe = (int)(ki >> 32); te = (int)(uint32_t)ki;
                sc1 = chain_cand(qe, te, (int)(kp >> 32), (int)(uint32_t)kp, 0, P, ok1);
            }
            const int fi = f[i0 - 1] + wave_incl_sum(ok1 ? sc1 : 0, lane);
            bool bad = in && !(ok1 && fi > P.k);
            __syncthreads();
            if (in) f[i] = fi;
            __syncthreads();
            for (int d = 2; d <= 64; d++) {
                const int j = i - d;
                const bool live = in && !bad && j >= 0;
                if (!__any(live)) break;
                int fj = 0;
                if (live) fj = f[j];
                const bool need = live && fj + P.k > fi;
                if (__any(need)) {
                    if (need) {
                        bool ok2; const uint64_t kj = key[j];
                        const int c2 = chain_cand(qe, te, (int)(kj >> 32), (int)(uint32_t)kj, fj, P, ok2);
                        if (ok2 && c2 > fi) bad = true;
                    }
                }
            }
            const uint64_t badm = __ballot(bad);
            const int good = badm ? (int)__ffsll((long long)badm) - 1 : nb;
            if (lane < good) aux[i] = (uint16_t)(i - 1);
            __syncthreads();
            i0 += good;
            if (good < nb) { dp_step_seq(i0, lane, P); i0++; }
        }
        long long bk = -1;
        for (int i = lane; i < n; i += 64) { long long v = (long long)f[i] * 16384 + (16383 - i); bk = v > bk ? v : bk; }
        bk = wave_max_i64(bk);
        return 16383 - (int)(bk & 16383);
    }

    // anchors of the chain that ends at `best`: how many, and the first one
    __device__ __forceinline__ void chain_len(int best, int lane, int &cnt, int &first) const
    {
        cnt = 0; first = best;
        if (lane == 0) { int c = best; while (c != 0xffff) { cnt++; first = c; c = aux[c]; } }
        cnt = __shfl(cnt, 0, 64); first = __shfl(first, 0, 64);
    }

    // one lane: the cnt anchors of that chain to out[0 .. cnt - 1], in order
    __device__ __forceinline__ void chain_write(uint64_t *out, int best, int cnt) const
    {
        int c = best, k2 = cnt;
        while (c != 0xffff) { out[--k2] = key[c]; c = aux[c]; }
    }
};

// what both bodies know of their contig (or box): the two minimizer lists, the record slots p0 .. p0 + R - 1 and their chain buffers
struct ChainJob {
    int lane; uint32_t p0, R;
    int lenq, lent, nq, nt;
    const fsv_mz *mq, *mt;      // contig: position-sorted copy, reference: hash-sorted
    uint64_t *chain_out; AlnHeader *hdr;
    __device__ __forceinline__ uint64_t *out(uint32_t rec) const { return chain_out + (size_t)(p0 + rec) * ALN_CHAIN_STRIDE; }
};

// SUB = true.  h: the empty header every slot starts with
__device__ __forceinline__ void chain_box(ChainLds &L, const ChainJob &J, AlnHeader h, const fsv_aln_params &P)
{
    const int lane = J.lane;
    int n = 0;
    for (int base = 0; base < J.nq; base += 64) {
        const int i = base + lane;
        int c = 0; uint64_t k0 = 0, k1 = 0;
        if (i < J.nq) {
            const fsv_mz a = J.mq[i];
            const int l2 = mz_lower_bound(J.mt, J.nt, a.hash);
            for (int e = 0; e < 2 && l2 + e < J.nt; e++) {     // the list holds a hash at most twice, the lower position first
                const fsv_mz b = J.mt[l2 + e];
                if (b.hash != a.hash) break;
                if (b.rev == a.rev) { const uint64_t key = (uint64_t)a.pos << 32 | b.pos; if (c == 0) k0 = key; else k1 = key; c++; }
            }
        }
        const uint64_t m1 = __ballot(c >= 1), m2 = __ballot(c >= 2), below = (1ull << lane) - 1;
        const int at = n + __popcll(m1 & below) + __popcll(m2 & below);
        if (c >= 1 && at < ALN_AMAX) L.key[at] = k0;
        if (c >= 2 && at + 1 < ALN_AMAX) L.key[at + 1] = k1;
        n += __popcll(m1) + __popcll(m2);
    }
    if (n > ALN_AMAX) n = ALN_AMAX;
    __syncthreads();
    int cnt = 0, first = 0, best = 0;
    if (n >= P.min_anchors) { best = L.chain_dp(n, lane, P); L.chain_len(best, lane, cnt, first); }
    if (lane == 0) {
        uint64_t *out = J.out(0);
        int keep = 0;
        if (cnt >= P.min_anchors) {
            L.chain_write(out + 1, best, cnt);
            keep = cnt;     // strictly in front of the box's last base pair
            while (keep > 0 && ((int)(out[keep] >> 32) >= J.lenq - 1 || (int)(uint32_t)out[keep] >= J.lent - 1)) keep--;
        }
        out[0] = ~0ull;                                                             // (-1, -1)
        out[keep + 1] = (uint64_t)(uint32_t)(J.lenq - 1) << 32 | (uint32_t)(J.lent - 1);
        h.n_chain = keep + 2; h.status = 0;
        J.hdr[J.p0] = h;
    }
}

// SUB = false
__device__ __forceinline__ void chain_contig(ChainLds &L, const ChainJob &J, AlnHeader h, const fsv_aln_params &P)
{
    __shared__ int s_cnt[ALN_MAX_REC];      // anchors of the majority strand's chains, for the cut
    const int lane = J.lane, lenq = J.lenq;
    const uint32_t p0 = J.p0, R = J.R;
    int n = 0, nrev = 0, nfwd = 0;
    for (int base = 0; base < J.nq; base += 64) {
        int i = base + lane;
        bool hit = false; uint64_t key = 0; uint16_t aux = 0;
        if (i < J.nq) {
            fsv_mz a = J.mq[i];
            const int l2 = mz_lower_bound(J.mt, J.nt, a.hash);
            if (l2 < J.nt) { fsv_mz b = J.mt[l2]; if (b.hash == a.hash) { hit = true; key = (uint64_t)a.pos << 32 | b.pos; aux = (uint16_t)(a.span | ((a.rev ^ b.rev) << 8)); } }
        }
        uint64_t m = __ballot(hit);
        int at = n + __popcll(m & ((1ull << lane) - 1));
        if (hit && at < ALN_AMAX) { L.key[at] = key; L.aux[at] = aux; }
        nrev += __popcll(__ballot(hit && (aux >> 8)));
        nfwd += __popcll(__ballot(hit && !(aux >> 8)));
        n += __popcll(m);
    }
    if (n > ALN_AMAX) n = ALN_AMAX;
    __syncthreads();
    const int rev = nrev > nfwd;
    h.rev = rev;
    // the majority strand's anchors stay in LDS (compacted in place); the others wait in the last slot's chain buffer
    uint64_t *tmp = J.out(R - 1);
    int m2 = 0, nb = 0;
    for (int base = 0; base < n; base += 64) {
        int i = base + lane;
        bool keep = false, oth = false; uint64_t key = 0;
        if (i < n) {
            const uint16_t aux = L.aux[i];
            const int strand = aux >> 8;
            key = L.key[i];
            // on the reverse strand the contig coordinate is that of the reverse complement
            if (strand) { int qp = (int)(key >> 32), span = aux & 0xff; qp = (lenq - 1) - (qp - span + 1); key = (uint64_t)(uint32_t)qp << 32 | (uint32_t)key; }
            keep = strand == rev; oth = !keep;
        }
        const uint64_t mk = __ballot(keep), mo = __ballot(oth), below = (1ull << lane) - 1;
        const int at = m2 + __popcll(mk & below), ao = nb + __popcll(mo & below);
        __syncthreads();
        if (keep) L.key[at] = key;
        if (oth) tmp[ao] = key;
        m2 += __popcll(mk); nb += __popcll(mo);
        __syncthreads();
    }
    n = m2;
    if (n < P.min_anchors) return;
    // anchors arrive in contig order; on the reverse strand the contig coordinate was mirrored, so the order is reversed
    if (rev) {
        for (int i = lane; i < n / 2; i += 64) { const uint64_t a = L.key[i], b = L.key[n - 1 - i]; L.key[i] = b; L.key[n - 1 - i] = a; }
        __syncthreads();
    }
    // The best chain is the primary alignment.  What it leaves uncovered is chained again (minimap2 reports such pieces as
    // supplementary alignments, and DipPAV calls the SVs beyond the chaining gap from consecutive records of one contig,
    // extract_contig_signature_CCS.py:251-327): the anchors inside the query interval of a chain are taken out -- they are a
    // contiguous run, the list is in query order -- and the rest goes through the same DP, up to ALN_MAJ_REC chains.
    int n_rec = 0;
    for (int rec = 0; rec < ALN_MAJ_REC && rec < (int)R && n >= P.min_anchors; rec++) {
        const int best = L.chain_dp(n, lane, P);
        int cnt, first;
        L.chain_len(best, lane, cnt, first);
        if (cnt < P.min_anchors || (rec > 0 && L.f[best] < ALN_SUP_MIN)) break;
        if (lane == 0) {
            L.chain_write(J.out(rec), best, cnt);
            h.n_chain = cnt; h.status = 0;
            J.hdr[p0 + rec] = h;
            s_cnt[rec] = cnt;
        }
        n_rec++;
        // drop the anchors whose query coordinate lies in [q(first), q(best)]: indices lo .. hi of the sorted list
        const int qlo = (int)(L.key[first] >> 32), qhi = (int)(L.key[best] >> 32);
        int lo = n, hi = -1;
        for (int i = lane; i < n; i += 64) { const int qe = (int)(L.key[i] >> 32); if (qe >= qlo && qe <= qhi) { lo = min(lo, i); hi = max(hi, i); } }
        lo = -wave_max_i32(-lo); hi = wave_max_i32(hi);
        __syncthreads();
        const int tail = n - 1 - hi;
        for (int base = 0; base < tail; base += 64) {   // move the tail down, front to back (ascending: no overlap hazard inside a pass)
            const int i = base + lane;
            uint64_t v = 0;
            if (i < tail) v = L.key[hi + 1 + i];
            __syncthreads();
            if (i < tail) L.key[lo + i] = v;
            __syncthreads();
        }
        n = lo + tail;
    }
    // the other strand, once
    if (n_rec == 0 || n_rec >= (int)R || nb < P.min_anchors) return;
    const int mrev = !rev;
    __threadfence_block();      // tmp and the chains above were written with plain stores by other lanes
    __syncthreads();
    for (int i = lane; i < nb; i += 64) L.key[i] = tmp[mrev ? nb - 1 - i : i];
    __syncthreads();
    const int best = L.chain_dp(nb, lane, P);
    int cnt, first;
    L.chain_len(best, lane, cnt, first);
    if (cnt < P.min_anchors || L.f[best] < ALN_SUP_MIN) return;
    // span of the chain's k-mers on the contig, in the majority strand's coordinates
    const int lo_a = (lenq - 1) - (int)(L.key[best] >> 32), hi_a = (lenq - 1) - ((int)(L.key[first] >> 32) - P.k + 1);
    int cut_r = -1, cut_s = -1;
    for (int r = 0; r < n_rec && cut_r < 0; r++) {
        const uint64_t *c = J.out(r);
        const int cr = s_cnt[r];
        for (int base = P.min_anchors - 1; base + 1 + P.min_anchors <= cr; base += 64) {
            const int s = base + lane;
            const bool ok = s + 1 + P.min_anchors <= cr && (int)(c[s] >> 32) < lo_a && hi_a < (int)(c[s + 1] >> 32) - P.k + 1;
            const uint64_t m = __ballot(ok);
            if (m) { cut_r = r; cut_s = base + (int)__ffsll((long long)m) - 1; break; }
        }
    }
    if (cut_r >= 0 && n_rec + 1 < (int)R) {
        // the part behind the cut becomes the next record
        const int tail = s_cnt[cut_r] - (cut_s + 1);
        const uint64_t *src = J.out(cut_r) + cut_s + 1;
        uint64_t *dst = J.out(n_rec);
        for (int i = lane; i < tail; i += 64) dst[i] = src[i];
        if (lane == 0) {
            h.rev = rev; h.status = 0;
            h.n_chain = cut_s + 1; J.hdr[p0 + cut_r] = h;
            h.n_chain = tail; J.hdr[p0 + n_rec] = h;
        }
        n_rec++;
    }
    if (lane == 0) {
        L.chain_write(J.out(n_rec), best, cnt);
        h.rev = mrev; h.n_chain = cnt; h.status = 0;
        J.hdr[p0 + n_rec] = h;
    }
}

template <bool SUB>
__global__ __launch_bounds__(64) void k_chain_aln(const int32_t *__restrict__ read_len,
                                                  const fsv_mz *__restrict__ mz, const uint32_t *__restrict__ mz_off,
                                                  const uint32_t *__restrict__ mz_cnt, const uint32_t *__restrict__ pair_q,
                                                  const uint32_t *__restrict__ pair_t, uint64_t *__restrict__ chain_out,
                                                  AlnHeader *__restrict__ hdr, uint32_t R, fsv_aln_params P)
{
    __shared__ ChainLds L;
    const int lane = threadIdx.x;
    const uint32_t p0 = blockIdx.x * R, rq = pair_q[p0], rt = pair_t[p0];
    const int nq = (int)mz_cnt[rq], nt = (int)mz_cnt[rt];
    const ChainJob J{lane, p0, R, read_len[rq], read_len[rt], nq, nt, mz + mz_off[rq] + nq, mz + mz_off[rt], chain_out, hdr};
    AlnHeader h; h.qbeg = h.tbeg = h.qend = h.tend = 0; h.n_events = 0; h.n_chain = 0; h.rev = 0; h.status = 1; h.ev_off = 0; h.pad = 0;
    if (lane < (int)R) hdr[p0 + lane] = h;   // every slot starts out empty
    if (SUB) chain_box(L, J, h, P);
    else chain_contig(L, J, h, P);
}

// ------------------------------------------------------------------------------------------------ seed thinning
// Windows beyond ~760 kb would need a minimizer window above 255 to keep a seed list below ALN_AMAX; instead w stays 255 and
// every m-th minimizer by hash survives, on the reference window and its contigs alike (oracle/aln.c does the same).  One
// block per sequence compacts its raw list in place (the order of a raw list is arbitrary: k_uniq sorts).
__global__ __launch_bounds__(256) void k_thin_seeds(fsv_mz *__restrict__ mz, const uint32_t *__restrict__ mz_off, uint32_t *__restrict__ mz_cnt,
                                                    const uint16_t *__restrict__ thin)
{
    __shared__ uint32_t s_w[4];
    const uint32_t r = blockIdx.x, m = thin[r];
    if (m <= 1) return;
    fsv_mz *a = mz + mz_off[r];
    const uint32_t n = min(mz_cnt[r], mz_off[r + 1] - mz_off[r]);
    uint32_t kept = 0;
    for (uint32_t base = 0; base < n; base += 256) {
        const uint32_t i = base + threadIdx.x;
        fsv_mz v = mz_make(0, 0, 0, 0);
        bool keep = false;
        if (i < n) { v = a[i]; keep = (v.hash >> 11) % (uint64_t)m == 0; }
        // rank inside the chunk.  The barrier inside is also: every thread has read its a[i] before anyone overwrites a slot at or below it
        uint32_t all;
        const uint32_t at = block_rank_256(keep, s_w, &all);
        if (keep) a[kept + at] = v;     // destination index <= i: only slots already read
        kept += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) mz_cnt[r] = kept;
}

// ------------------------------------------------------------------------------------------------ events
// query base of the strand-oriented contig
__device__ __forceinline__ uint32_t qbase(const uint32_t *__restrict__ store, uint32_t qw, int lenq, int rev, int p) { return fsv_base_at(store, qw, lenq, rev, p); }
// target base of a reference window: 0-3, or 4 where the window has an N (nm: one word per 16 bases, bit j = base j is an N; nullptr:
// the batch has no N at all).  An N pairs with nothing (no padding, no gap-free run across it, no exact match) and costs
// FSV_SC_AMBI in a score, as in minimap2 (sc_ambi = 1: the alignment runs through a short run of N as 'M').  In the 2-bit store an
// N holds a base hashed from its position (k_pack_ascii): the seeds of an N run then look like random sequence, unique and
// matching nothing, where minimap2 skips k-mers with an N.
#define FSV_SC_AMBI 1
// the mask array starts four words into its buffer; the word in front of it says whether any window of the batch has an N at all
// (k_pack_ascii sets it): a kernel drops the mask at its start when there is none, and then pays nothing for it
#define FSV_NM_LEAD 4
__device__ __forceinline__ const uint32_t *nm_active(const uint32_t *__restrict__ nm) { return (nm && nm[-FSV_NM_LEAD]) ? nm : nullptr; }
__device__ __forceinline__ uint32_t tbase(const uint32_t *__restrict__ store, const uint32_t *__restrict__ nm, uint32_t tw, int p)
{
    if (nm && ((nm[tw + ((uint32_t)p >> 4)] >> ((uint32_t)p & 15u)) & 1u)) return 4u;
    return fsv_base_fwd(store, tw, p);
}
__device__ __forceinline__ int pair_score(uint32_t qb, uint32_t tb, const fsv_aln_params &P) { return tb > 3u ? -FSV_SC_AMBI : (qb == tb ? P.a : -P.b); }
__host__ __device__ __forceinline__ uint32_t n_substitute(uint32_t pos)
{
    uint32_t x = pos * 0x9E3779B1u; x ^= x >> 15; x *= 0x85EBCA77u; x ^= x >> 13;
    return x >> 30;
}

// The sequences of a batch and its record slots' (query, target): one kernel argument of every kernel that reads bases.
struct PairSeqs { const uint32_t *store, *nm_all, *word_off; const int32_t *read_len; const uint32_t *pair_q, *pair_t; };
// One slot's pair, the contig on strand rev: built once per block.  The mask is dropped here when the batch has no N (nm_active).
struct PairView {
    const uint32_t *store, *nm; uint32_t qw, tw; int lenq, lent, rev;
    __device__ __forceinline__ PairView(const PairSeqs &S, uint32_t slot, int rev_)
        : store(S.store), nm(nm_active(S.nm_all)), qw(S.word_off[S.pair_q[slot]]), tw(S.word_off[S.pair_t[slot]]),
          lenq(S.read_len[S.pair_q[slot]]), lent(S.read_len[S.pair_t[slot]]), rev(rev_) {}
    __device__ __forceinline__ uint32_t q(int p) const { return qbase(store, qw, lenq, rev, p); }
    __device__ __forceinline__ uint32_t t(int p) const { return tbase(store, nm, tw, p); }
    __device__ __forceinline__ int score(int qp, int tp, const fsv_aln_params &P) const { return pair_score(q(qp), t(tp), P); }
};

// GLOBAL: the box of an oversize event (k_chain_aln<true>): the chain carries its two fixed end pairs, the walk runs from the
// box's first base pair to its last (no X-drop extension, no clips).
// An event of more than max_cells cells is not handed to the DP: it is listed with qs = -1 - qs, WITHOUT its padding (the box
// between the two anchors) -- the host has it seeded again (first level) or closed from its corners (k_corner, inside a box).
template <bool GLOBAL>
__global__ __launch_bounds__(256) void k_aln_events(PairSeqs S, const uint64_t *__restrict__ chain,
                                                    AlnHeader *__restrict__ hdr, AlnEvent *__restrict__ events, AlnEvent *__restrict__ packed,
                                                    uint32_t *__restrict__ n_packed, fsv_aln_params P)
{
    __shared__ uint8_t s_cls[ALN_CHAIN_STRIDE];
    const uint32_t p = blockIdx.x;
    AlnHeader h = hdr[p];
    if (h.status != 0) return;
    const PairView V(S, p, h.rev);
    const int lenq = V.lenq, lent = V.lent, nch = h.n_chain, nseg = nch - 1;
    const uint64_t *c = chain + (size_t)p * ALN_CHAIN_STRIDE;
    // segment classes between consecutive anchors: 0 identical, 1 few mismatches ('M'), 2 needs DP
    for (int s = threadIdx.x; s < nseg; s += blockDim.x) {
        const int q0 = (int)(c[s] >> 32), t0 = (int)(uint32_t)c[s], dq = (int)(c[s + 1] >> 32) - q0, dt = (int)(uint32_t)c[s + 1] - t0;
        uint8_t cls = 2;
        if (dq == dt) {
            int mm = 0;
            for (int k2 = 1; k2 <= dq && mm <= P.max_mm_run; k2++) mm += V.q(q0 + k2) != V.t(t0 + k2);
            cls = mm == 0 ? 0 : (mm <= P.max_mm_run ? 1 : 2);
        }
        s_cls[s] = cls;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
#define CQ(i) ((int)(c[i] >> 32))
#define CT(i) ((int)(uint32_t)c[i])
    int qbeg = 0, tbeg = 0, qend = lenq - 1, tend = lent - 1;
    if (!GLOBAL) {
        const int qs0 = CQ(0) - P.k + 1, ts0 = CT(0) - P.k + 1;
        int x = 0, best = 0, bi = 0;
        for (int i = 1; qs0 - i >= 0 && ts0 - i >= 0; i++) {
            x += V.score(qs0 - i, ts0 - i, P);
            if (x > best) { best = x; bi = i; }
            if (best - x > P.xdrop) break;
        }
        qbeg = qs0 - bi; tbeg = ts0 - bi;
        x = 0; best = 0; bi = 0;
        for (int i = 1; CQ(nch - 1) + i < lenq && CT(nch - 1) + i < lent; i++) {
            x += V.score(CQ(nch - 1) + i, CT(nch - 1) + i, P);
            if (x > best) { best = x; bi = i; }
            if (best - x > P.xdrop) break;
        }
        qend = CQ(nch - 1) + bi; tend = CT(nch - 1) + bi;
    }
    AlnEvent *ev = events + (size_t)p * ALN_EV_CAP;
    int ne = 0, mstart_q = qbeg, s = 0, status = 0;
    while (s < nseg) {
        if (s_cls[s] < 2) { s++; continue; }
        int e = s;
        while (e + 1 < nseg && s_cls[e + 1] == 2) e++;
        int eqs = CQ(s) + 1, eqe = CQ(e + 1), ets = CT(s) + 1, ete = CT(e + 1);
        int lp = 0, rp = 0;
        int lim_l = min(eqs - mstart_q, P.pad);
        while (lp < lim_l && V.q(eqs - 1 - lp) == V.t(ets - 1 - lp)) lp++;
        int lim_r = P.pad;
        if (eqe + lim_r > qend) lim_r = qend - eqe;
        if (ete + lim_r > tend) lim_r = tend - ete;
        { int nx = e + 1; while (nx < nseg && s_cls[nx] < 2) nx++; if (nx < nseg && eqe + lim_r > CQ(nx)) lim_r = CQ(nx) - eqe; }
        while (rp < lim_r && V.q(eqe + 1 + rp) == V.t(ete + 1 + rp)) rp++;
        if (ne >= ALN_EV_CAP) { status = FSV_ECAP; break; }
        if ((long long)(eqe - eqs + 1 + lp + rp) * (ete - ets + 1 + lp + rp) > P.max_cells) {
            ev[ne].qs = -1 - eqs; ev[ne].qe = eqe; ev[ne].ts = ets; ev[ne].te = ete; ne++;
        } else {
            eqs -= lp; ets -= lp; eqe += rp; ete += rp;
            ev[ne].qs = eqs; ev[ne].qe = eqe; ev[ne].ts = ets; ev[ne].te = ete; ne++;
        }
        mstart_q = eqe + 1;
        s = e + 1;
    }
#undef CQ
#undef CT
    h.qbeg = qbeg; h.tbeg = tbeg; h.qend = qend; h.tend = tend; h.n_events = ne; h.status = status;
    // the pair's events also go to a list packed over all pairs (any order; the header says where): one D2H copy for the batch
    if (status == 0 && ne > 0) {
        h.ev_off = atomicAdd(n_packed, (uint32_t)ne);
        for (int e = 0; e < ne; e++) packed[h.ev_off + e] = ev[e];
    }
    hdr[p] = h;
}

// ------------------------------------------------------------------------------------------------ oversize events
// The two sides of an event's box as sequences of their own (strand-oriented, word-aligned) in a second store, where the
// seeding / chaining / event kernels see them as an ordinary (contig, window) pair.  One thread per output word.
struct BoxSrc { uint32_t src_word; int32_t src_len, rev, start; };     // source read (word offset, length, strand), first base of the box side
// the sequence that owns word w of a store of n sequences laid end to end (word_off[r]: the first word of sequence r)
__device__ __forceinline__ uint32_t seq_of_word(const uint32_t *__restrict__ word_off, uint32_t n, uint32_t w)
{
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) { uint32_t mid = (lo + hi) >> 1; if (word_off[mid] <= w) lo = mid; else hi = mid; }
    return lo;
}
__global__ __launch_bounds__(256) void k_extract_boxes(const uint32_t *__restrict__ src_store, const uint32_t *__restrict__ src_nm, const BoxSrc *__restrict__ box,
                                                       const uint32_t *__restrict__ word_off, const int32_t *__restrict__ read_len,
                                                       uint32_t n_seq, uint32_t total_words, uint32_t *__restrict__ words, uint32_t *__restrict__ nm_out)
{
    const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= total_words) return;
    const uint32_t lo = seq_of_word(word_off, n_seq, w);
    const BoxSrc b = box[lo];
    const int len = read_len[lo], b0 = (int)(w - word_off[lo]) * 16;
    uint32_t v = 0;
    for (int j = 0; j < 16 && b0 + j < len; j++) v |= fsv_base_at(src_store, b.src_word, b.src_len, b.rev, b.start + b0 + j) << (2 * j);
    words[w] = v;
    if (w == 0) nm_out[-FSV_NM_LEAD] = src_nm[-FSV_NM_LEAD];
    if (src_nm[-FSV_NM_LEAD]) {      // the N positions of the side (only a reference window has any; it is never read on the other strand)
        uint32_t m = 0;
        if (!b.rev) for (int j = 0; j < 16 && b0 + j < len; j++) { const int sp = b.start + b0 + j; m |= ((src_nm[b.src_word + ((uint32_t)sp >> 4)] >> ((uint32_t)sp & 15u)) & 1u) << j; }
        nm_out[w] = m;
    }
}

// An event of a box's inner walk that is still larger than max_cells (nothing in it could be seeded: unrelated sequence, or a
// tandem array of short units) is closed from its two corners: gap-free X-drop extensions, the rest one insertion + one
// deletion (oracle/aln.c:corner_event).  One wavefront per event, 64 positions per step: the running score is a prefix sum,
// the running best a prefix maximum, the first position where best - score > xdrop ends the run.
struct CornerTask { uint32_t pair; int32_t qs, ql, ts, tl; };
__global__ __launch_bounds__(64) void k_corner(PairSeqs S, const AlnHeader *__restrict__ hdr,
                                               const CornerTask *__restrict__ tasks, int2 *__restrict__ out, fsv_aln_params P)
{
    const CornerTask T = tasks[blockIdx.x];
    const int lane = threadIdx.x;
    const PairView V(S, T.pair, hdr[T.pair].rev);
    const int lim = min(T.ql, T.tl);
    int res[2] = {0, 0};
    for (int side = 0; side < 2; side++) {
        const int n = side == 0 ? lim : lim - res[0];
        int x0 = 0, best = 0, len = 0;       // score and best score in front of the current step, bases taken at the best
        for (int base = 0; base < n; base += 64) {
            const int i = base + lane;
            int d = 0;
            if (i < n) {
                const int qp = side == 0 ? T.qs + i : T.qs + T.ql - 1 - i, tp = side == 0 ? T.ts + i : T.ts + T.tl - 1 - i;
                d = V.score(qp, tp, P);
            }
            const int x = wave_incl_sum(d, lane) + x0;
            const int m = max(wave_incl_max(i < n ? x : -(1 << 30), lane), best);
            const uint64_t brk = __ballot(i < n && m - x > P.xdrop);
            const int last = brk ? (int)__ffsll((long long)brk) - 1 : 63;      // lanes up to here are part of the run
            const int mb = __shfl(m, last, 64);                                // the best up to the end of the run (or of the step)
            if (mb > best) {
                const uint64_t at = __ballot(i < n && lane <= last && x == mb);
                len = base + (int)__ffsll((long long)at);                       // first position that reaches it
                best = mb;
            }
            if (brk) break;
            x0 = __shfl(x, 63, 64);
        }
        res[side] = len;
    }
    if (lane == 0) out[blockIdx.x] = make_int2(res[0], res[1]);
}

// ------------------------------------------------------------------------------------------------ gap left alignment
// minimap2 moves every I/D of a finished CIGAR to its leftmost position (mm_fix_cigar: a deletion while the reference base
// entering the gap on the left equals the one leaving it on the right, an insertion the same on the query) -- restated in
// oracle/aln.c:shift_gaps_left.  How far a gap could travel depends on the sequence alone, so the device answers that for
// all gaps of the batch at once (one wavefront per gap, 64 positions per step); the host then applies the shifts in CIGAR
// order, each bounded by the M run in front of it.
struct GapQuery { uint32_t slot; int32_t is_ins, off, len, cap; };
__global__ __launch_bounds__(64) void k_gap_shift(PairSeqs S, const AlnHeader *__restrict__ hdr,
                                                  const GapQuery *__restrict__ gaps, int32_t *__restrict__ max_shift)
{
    const GapQuery g = gaps[blockIdx.x];
    const int lane = threadIdx.x;
    const PairView V(S, g.slot, hdr[g.slot].rev);
    int res = g.cap;
    for (int base = 0; base < g.cap; base += 64) {
        const int l = base + lane;
        bool stop = true;
        if (l < g.cap) {
            const int a = g.off - 1 - l, b = g.off + g.len - 1 - l;
            stop = g.is_ins ? V.q(a) != V.q(b) : V.t(a) != V.t(b);
        }
        const uint64_t m = __ballot(stop);
        if (m) { res = base + (int)__ffsll((long long)m) - 1; break; }
    }
    if (lane == 0) max_shift[blockIdx.x] = res;
}

// ------------------------------------------------------------------------------------------------ NM / cs tags
// k_aln_tags: the base-by-base comparison behind a record's NM and cs tags (minimap2 --cs, short form; the grammar and the N and
// strand conventions: focalsv_hip.h, fsv_aln_tags).  One wavefront per task; a task is a run of consecutive ops of one record (the
// host cuts a long record at op boundaries, where no token crosses: a run of identical columns ends with its M op).  The CIGAR is
// walked wave-uniformly.  An M op is compared 64 columns per ballot; the lanes that differ each write their own token -- the
// `:<n>` of the identical columns in front of them, then `*<ref><query>` -- at an offset from a prefix sum of the token lengths,
// so a dense stretch of mismatches costs no more steps than a clean one.  I / D bases are copied a lane each.  The same walk runs
// twice: EMIT = false counts bytes and NM per task, k_aln_tags_scan turns the counts into offsets, EMIT = true writes.
// The host has checked every record against its sequences' lengths: no position of a task lies outside them.
struct TagTask { int32_t rev, q0, t0; uint32_t op_off, n_ops; };   // q0 / t0: strand-oriented contig / window position of the first op
__device__ __forceinline__ int dec_digits(uint32_t v)
{
    int n = 1;
    for (uint32_t p = 10; n < 10 && v >= p; p *= 10) n++;
    return n;
}
// ':' and the nd digits of v
__device__ __forceinline__ void put_run(char *__restrict__ o, uint32_t v, int nd)
{
    o[0] = ':';
    for (int i = nd; i >= 1; i--) { o[i] = (char)('0' + v % 10u); v /= 10u; }
}
// base of the strand-oriented contig, 4 where the contig itself has an N (the mask covers every sequence of the store)
__device__ __forceinline__ uint32_t tag_qbase(const PairView &V, int p)
{
    if (V.nm) {
        const uint32_t f = (uint32_t)(V.rev ? V.lenq - 1 - p : p);
        if ((V.nm[V.qw + (f >> 4)] >> (f & 15u)) & 1u) return 4u;
    }
    return V.q(p);
}
__device__ __forceinline__ char tag_char(uint32_t b) { return (char)(0x6e74676361ull >> (8u * b)); }   // "acgtn"

template <bool EMIT>
__global__ __launch_bounds__(64) void k_aln_tags(PairSeqs S, const TagTask *__restrict__ tasks, const uint32_t *__restrict__ cigar,
                                                 const uint64_t *__restrict__ off, char *__restrict__ cs,
                                                 uint64_t *__restrict__ n_bytes, int32_t *__restrict__ n_diff)
{
    const TagTask T = tasks[blockIdx.x];
    const int lane = threadIdx.x;
    const PairView V(S, blockIdx.x, T.rev);
    const uint32_t *cg = cigar + T.op_off;
    char *out = EMIT ? cs + off[blockIdx.x] : nullptr;
    int qp = T.q0, tp = T.t0, nm = 0;
    uint64_t at = 0;
    for (uint32_t k = 0; k < T.n_ops; k++) {
        const uint32_t op = cg[k] & 0xf;
        const int len = (int)(cg[k] >> 4);
        if (op == 0) {
            uint32_t run = 0;       // identical columns since the last token of this op
            for (int base = 0; base < len; base += 64) {
                const int n = min(64, len - base);
                bool diff = false; uint32_t qb = 0, tb = 0;
                if (lane < n) { qb = tag_qbase(V, qp + base + lane); tb = V.t(tp + base + lane); diff = qb != tb || tb > 3u || qb > 3u; }
                const uint64_t m = __ballot(diff);
                if (!m) { run += (uint32_t)n; continue; }
                const uint64_t below = m & ((1ull << lane) - 1ull);
                const uint32_t gap = below ? (uint32_t)(lane - (63 - __clzll((long long)below)) - 1) : run + (uint32_t)lane;
                const int nd = gap ? dec_digits(gap) : 0;
                const int tl = diff ? (gap ? 1 + nd : 0) + 3 : 0;
                const int incl = wave_incl_sum(tl, lane);
                if (EMIT && diff) {
                    char *o = out + at + (uint32_t)(incl - tl);
                    if (gap) { put_run(o, gap, nd); o += 1 + nd; }
                    o[0] = '*'; o[1] = tag_char(tb); o[2] = tag_char(qb);
                }
                at += (uint32_t)__shfl(incl, 63, 64);
                nm += __popcll(m);
                run = (uint32_t)(n - 1 - (63 - __clzll((long long)m)));
            }
            if (run) {
                const int nd = dec_digits(run);
                if (EMIT && lane == 0) put_run(out + at, run, nd);
                at += 1u + (uint32_t)nd;
            }
            qp += len; tp += len;
        } else if (op == 1 || op == 2) {
            if (len) {
                if (EMIT) {
                    if (lane == 0) out[at] = op == 1 ? '+' : '-';
                    for (int i = lane; i < len; i += 64) out[at + 1 + (uint32_t)i] = tag_char(op == 1 ? tag_qbase(V, qp + i) : V.t(tp + i));
                }
                at += 1u + (uint32_t)len; nm += len;
                if (op == 1) qp += len; else tp += len;
            }
        } else qp += len;       // S / H: the clipped bases of the contig
    }
    if (!EMIT && lane == 0) { n_bytes[blockIdx.x] = at; n_diff[blockIdx.x] = nm; }
}

// exclusive scan of the tasks' byte counts (one wavefront): off[i] the first byte of task i, off[n] the total
__global__ __launch_bounds__(64) void k_aln_tags_scan(const uint64_t *__restrict__ cnt, uint32_t n, uint64_t *__restrict__ off)
{
    const int lane = threadIdx.x;
    uint64_t carry = 0;
    for (uint32_t b = 0; b < n; b += 64) {
        const uint32_t i = b + (uint32_t)lane;
        const uint64_t c = i < n ? cnt[i] : 0;
        uint64_t v = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const uint64_t u = __shfl_up(v, o, 64); if (lane >= o) v += u; }
        if (i < n) off[i] = carry + v - c;
        carry += __shfl(v, 63, 64);
    }
    if (lane == 0) off[n] = carry;
}

// ------------------------------------------------------------------------------------------------ NW
// One workgroup per event, cells of one anti-diagonal in parallel.  Rolling rows indexed by the query position:
//   H on diagonals d-1 and d-2, and the E/F/E2/F2 values *leaving* each cell of diagonal d-1.
// Per cell one traceback byte with ksw2's layout (ksw2.h:115-118), stored diagonal-major (byte (i+j)*ql + j: the cells of
// a diagonal are adjacent, so a wave's stores coalesce); k_nw_rows, whose target side is the short one, stores byte
// (i+j)*tl + i instead -- a 30 kb insertion against 50 reference bases then takes 1.5 MB of traceback, not 900.
struct NwRows {
    int32_t *rows; int stride;
    __device__ __forceinline__ int32_t *H(int d) const { return rows + (size_t)(((d) % 3 + 3) % 3) * stride; }
    __device__ __forceinline__ int32_t *E(int d) const { return rows + (size_t)(3 + (d & 1)) * stride; }
    __device__ __forceinline__ int32_t *F(int d) const { return rows + (size_t)(5 + (d & 1)) * stride; }
    __device__ __forceinline__ int32_t *E2(int d) const { return rows + (size_t)(7 + (d & 1)) * stride; }
    __device__ __forceinline__ int32_t *F2(int d) const { return rows + (size_t)(9 + (d & 1)) * stride; }
};

// cell (i, j) of diagonal d = i + j (ksw_extz2's recurrence, ksw2_extz2_sse.c; boundary: a gap of length l before the
// first cell costs min(q + e*l, q2 + e2*l))
// BYROW: the rolling rows are indexed by the target row i instead of the query column j (k_nw_rows: events with a short target side)
template <bool BYROW = false>
__device__ __forceinline__ void nw_cell(const NwRows &R, int d, int i, int j, uint32_t tb, uint32_t qb, bool two, const fsv_aln_params &P,
                                        uint8_t *__restrict__ bt, int bt_stride)
{
    const int xc = BYROW ? i : j;             // this cell's slot
    const int xd = xc - 1;                    // the diagonal neighbour (i-1, j-1)
    const int xe = BYROW ? i - 1 : j;         // E comes from (i-1, j)
    const int xf = BYROW ? i : j - 1;         // F comes from (i, j-1)
    int32_t hdiag, a, b, a2 = NW_NEG, b2 = NW_NEG;
    if (i == 0 && j == 0) hdiag = 0;
    else if (i == 0) { int g1 = -(P.q + P.e * j), g2 = two ? -(P.q2 + P.e2 * j) : NW_NEG; hdiag = max(g1, g2); }
    else if (j == 0) { int g1 = -(P.q + P.e * i), g2 = two ? -(P.q2 + P.e2 * i) : NW_NEG; hdiag = max(g1, g2); }
    else hdiag = R.H(d - 2)[xd];
    if (i == 0) {
        int g1 = -(P.q + P.e * (j + 1)), g2 = two ? -(P.q2 + P.e2 * (j + 1)) : NW_NEG;
        const int hup = max(g1, g2); // H(-1, j)
        a = hup - P.q - P.e; if (two) a2 = hup - P.q2 - P.e2;
    } else { a = R.E(d - 1)[xe]; if (two) a2 = R.E2(d - 1)[xe]; }
    if (j == 0) {
        int g1 = -(P.q + P.e * (i + 1)), g2 = two ? -(P.q2 + P.e2 * (i + 1)) : NW_NEG;
        const int hleft = max(g1, g2); // H(i, -1)
        b = hleft - P.q - P.e; if (two) b2 = hleft - P.q2 - P.e2;
    } else { b = R.F(d - 1)[xf]; if (two) b2 = R.F2(d - 1)[xf]; }
    int32_t h = hdiag + pair_score(qb, tb, P);
    uint8_t dd = 0;
    if (a > h) { h = a; dd = 1; }
    if (b > h) { h = b; dd = 2; }
    if (two && a2 > h) { h = a2; dd = 3; }
    if (two && b2 > h) { h = b2; dd = 4; }
    int32_t o = h - P.q;
    if (a > o) { dd |= 0x08; R.E(d)[xc] = a - P.e; } else R.E(d)[xc] = o - P.e;
    if (b > o) { dd |= 0x10; R.F(d)[xc] = b - P.e; } else R.F(d)[xc] = o - P.e;
    if (two) {
        o = h - P.q2;
        if (a2 > o) { dd |= 0x20; R.E2(d)[xc] = a2 - P.e2; } else R.E2(d)[xc] = o - P.e2;
        if (b2 > o) { dd |= 0x40; R.F2(d)[xc] = b2 - P.e2; } else R.F2(d)[xc] = o - P.e2;
    }
    R.H(d)[xc] = h;
    bt[(size_t)d * bt_stride + xc] = dd;    // diagonal-major; within a diagonal by column, or by row for a short target side
}

// ksw_backtrack (ksw2.h:120-150) by thread 0, emitted end-to-start then reversed in place.  The traceback bytes come through
// an LDS tile of NW_TD diagonals x NW_TC columns that the whole workgroup loads around the current cell: one memory latency
// per >= 16 steps instead of one per step.
#define NW_TD 32
#define NW_TC 32
template <bool BYROW = false>
__device__ __forceinline__ void nw_backtrack(const uint8_t *__restrict__ bt, int ql, int tl, uint32_t *__restrict__ cg, uint32_t *__restrict__ cg_n_out,
                                             uint8_t (*s_bt)[NW_TC], int *s_walk)
{
    const int bt_stride = BYROW ? tl : ql;
    const int tid = threadIdx.x, nt = blockDim.x;
    if (tid == 0) { s_walk[0] = tl - 1; s_walk[1] = ql - 1; s_walk[2] = 0; s_walk[3] = 0; s_walk[4] = 0; }
    __syncthreads();
    for (;;) {
        const int i0 = s_walk[0], j0 = s_walk[1];
        if (i0 < 0 || j0 < 0) break;
        const int dtop = i0 + j0, jtop = j0;    // tile: diagonals dtop-NW_TD+1 .. dtop, columns jtop-NW_TC+1 .. jtop
        for (int idx = tid; idx < NW_TD * NW_TC; idx += nt) {
            const int rd = idx / NW_TC, rc = idx % NW_TC;
            const int d = dtop - rd, j = jtop - rc, i = d - j;
            s_bt[rd][rc] = (d >= 0 && j >= 0 && i >= 0 && i < tl) ? bt[(size_t)d * bt_stride + (BYROW ? i : j)] : (uint8_t)0;
        }
        __syncthreads();
        if (tid == 0) {
            int i = i0, j = j0, state = s_walk[2], n = s_walk[3];
            bool over = s_walk[4] != 0;
            while (i >= 0 && j >= 0) {
                const int rd = dtop - (i + j), rc = jtop - j;
                if (rd >= NW_TD || rc >= NW_TC) break;   // left the tile
                const uint8_t dd = s_bt[rd][rc];
                if (state == 0) state = dd & 7;
                else if (!((dd >> (state + 2)) & 1)) state = 0;
                if (state == 0) state = dd & 7;
                uint32_t op;
                if (state == 0) { op = 0; i--; j--; }
                else if (state == 1 || state == 3) { op = 2; i--; }
                else { op = 1; j--; }
                if (n && (cg[n - 1] & 0xf) == op) cg[n - 1] += 1u << 4;
                else if (n < ALN_CG_CAP) cg[n++] = 1u << 4 | op;
                else over = true;
            }
            s_walk[0] = i; s_walk[1] = j; s_walk[2] = state; s_walk[3] = n; s_walk[4] = over ? 1 : 0;
        }
        __syncthreads();
    }
    if (tid != 0) return;
    int i = s_walk[0], j = s_walk[1], n = s_walk[3];
    bool over = s_walk[4] != 0;
    auto put = [&](uint32_t op, uint32_t len) {
        if (n && (cg[n - 1] & 0xf) == op) cg[n - 1] += len << 4;
        else if (n < ALN_CG_CAP) cg[n++] = len << 4 | op;
        else over = true;
    };
    if (i >= 0) put(2, (uint32_t)(i + 1));
    if (j >= 0) put(1, (uint32_t)(j + 1));
    for (int k2 = 0; k2 < n / 2; k2++) { uint32_t t = cg[k2]; cg[k2] = cg[n - 1 - k2]; cg[n - 1 - k2] = t; }
    *cg_n_out = over ? 0xffffffffu : (uint32_t)n;
}

// What every DP kernel sets up from its block's task: the pair's view, the event's two lengths, one or two gap costs, its traceback bytes
struct NwJob {
    const NwTask T; const PairView V; const int ql, tl; const bool two; uint8_t *const bt;
    __device__ __forceinline__ NwJob(const PairSeqs &S, const AlnHeader *__restrict__ hdr, const NwTask *__restrict__ tasks, uint8_t *__restrict__ bt_all, const fsv_aln_params &P)
        : T(tasks[blockIdx.x]), V(S, T.pair, hdr[T.pair].rev), ql(T.ql), tl(T.tl), two(P.q2 >= 0), bt(bt_all + T.bt_off) {}
};
// where the kernels leave their results: CIGAR runs (ALN_CG_CAP per task), their number and the score per task
struct NwOut { uint32_t *cg_all, *cg_n; int32_t *scores; };
// ... and how every one of them ends, the whole workgroup behind a barrier that has drained its stores: the score of the last cell, the backtrack
template <bool BYROW>
__device__ __forceinline__ void nw_finish(const NwJob &J, const NwRows &R, const NwOut &O)
{
    __shared__ uint8_t s_bt[NW_TD][NW_TC];
    __shared__ int s_walk[8];
    if (threadIdx.x == 0) O.scores[J.T.out_idx] = R.H(J.ql + J.tl - 2)[(BYROW ? J.tl : J.ql) - 1];
    nw_backtrack<BYROW>(J.bt, J.ql, J.tl, O.cg_all + J.T.cg_off, O.cg_n + J.T.out_idx, s_bt, s_walk);
}

// the next diagonal needs this one's LDS rows, not its traceback bytes: __syncthreads() would also drain the global
// stores (vmcnt), a memory round trip per diagonal; they are drained once, by the barrier in front of the backtrack
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// The sweep with the rolling rows in LDS (11 x CAP x 4 B), for an owner axis of up to CAP cells: thread t owns the cells t, t+NT, ...
// of that axis for the whole sweep, so their bases sit in registers; the bases of the other axis that the sweep is crossing sit
// in an LDS ring that the workgroup refills every CH diagonals.  No global load on the per-diagonal critical path.
//   BYROW = false (k_nw): the owner axis is the query (columns), the ring holds target bases, traceback byte (i+j)*ql + j
//   BYROW = true (k_nw_rows): the owner axis is the target (rows), the ring holds query bases, traceback byte (i+j)*tl + i
template <int CAP, int NT, bool BYROW>
__device__ __forceinline__ void nw_sweep_lds(const NwJob &J, const NwRows &R, const fsv_aln_params &P)
{
    constexpr int C = CAP / NT;
    constexpr int CH = CAP >= 1024 ? 256 : 64;
    constexpr int RING = CAP >= 2048 ? 4096 : 2 * CAP;   // ring of the other axis' bases (power of two >= CAP + CH)
    __shared__ uint8_t s_ring[RING];
    const int tid = threadIdx.x;
    const int n_own = BYROW ? J.tl : J.ql, n_oth = BYROW ? J.ql : J.tl;
    const PairView &V = J.V;
    uint32_t ob[C];
#pragma unroll
    for (int m = 0; m < C; m++) { const int x = tid + m * NT; ob[m] = x >= n_own ? 0u : BYROW ? V.t(J.T.ts + x) : V.q(J.T.qs + x); }
    for (int d = 0; d <= J.ql + J.tl - 2; d++) {
        if (d % CH == 0) {
            // cells d .. d+CH-1 of the other axis enter the sweep during the next CH diagonals; those below d-n_own+1 have left it
            for (int y = d + tid; y < min(d + CH, n_oth); y += NT) s_ring[y & (RING - 1)] = (uint8_t)(BYROW ? V.q(J.T.qs + y) : V.t(J.T.ts + y));
            __syncthreads();
        }
#pragma unroll
        for (int m = 0; m < C; m++) {
            const int x = tid + m * NT, y = d - x;
            if (x < n_own && y >= 0 && y < n_oth) {
                const uint32_t rb = s_ring[y & (RING - 1)];
                nw_cell<BYROW>(R, d, BYROW ? x : y, BYROW ? y : x, BYROW ? ob[m] : rb, BYROW ? rb : ob[m], J.two, P, J.bt, n_own);
            }
        }
        lds_barrier();
    }
    __syncthreads();
}

// Queries up to QCAP bases against any target: thread t owns the query columns t, t+NT, ...
template <int QCAP, int NT>
__global__ __launch_bounds__(NT) void k_nw(PairSeqs S, const AlnHeader *__restrict__ hdr, const NwTask *__restrict__ tasks, uint8_t *__restrict__ bt_all,
                                           NwOut O, fsv_aln_params P)
{
    __shared__ int32_t s_rows[11 * QCAP];
    const NwJob J(S, hdr, tasks, bt_all, P);
    const NwRows R{s_rows, QCAP};
    nw_sweep_lds<QCAP, NT, false>(J, R, P);
    nw_finish<false>(J, R, O);
}

// The transposed case -- a long query against a short target (an insertion: ~50 reference bases of padding against the inserted
// kilobases): thread t owns the target rows t, t+NT, ..., the rolling rows are indexed by row, the query bases come through the LDS
// ring.  With the rows of such an event in ONE wavefront a diagonal costs a single-wave barrier; round 1 sent these events to
// k_nw<3072, 1024>, where each of their ~2 000 diagonals paid a 16-wave barrier for a few dozen cells (7.3 ms per bench step).
template <int RCAP, int NT>
__global__ __launch_bounds__(NT) void k_nw_rows(PairSeqs S, const AlnHeader *__restrict__ hdr, const NwTask *__restrict__ tasks, uint8_t *__restrict__ bt_all,
                                                NwOut O, fsv_aln_params P)
{
    __shared__ int32_t s_rows[11 * RCAP];
    const NwJob J(S, hdr, tasks, bt_all, P);
    const NwRows R{s_rows, RCAP};
    nw_sweep_lds<RCAP, NT, true>(J, R, P);
    nw_finish<true>(J, R, O);
}

// Any query length: rolling rows in HBM, bases fetched per cell (events with queries above NW_LDS_Q bases: rare, slow path)
__global__ __launch_bounds__(256) void k_nw_any(PairSeqs S, const AlnHeader *__restrict__ hdr, const NwTask *__restrict__ tasks, uint8_t *__restrict__ bt_all,
                                                int32_t *__restrict__ rows_all, NwOut O, fsv_aln_params P)
{
    const NwJob J(S, hdr, tasks, bt_all, P);
    const int ql = J.ql, tl = J.tl;
    const NwRows R{rows_all + J.T.row_off, ql};
    for (int d = 0; d <= ql + tl - 2; d++) {
        const int jlo = max(0, d - (tl - 1)), jhi = min(ql - 1, d);
        for (int j = jlo + (int)threadIdx.x; j <= jhi; j += blockDim.x) {
            const int i = d - j;
            nw_cell(R, d, i, j, J.V.t(J.T.ts + i), J.V.q(J.T.qs + j), J.two, P, J.bt, ql);
        }
        __threadfence_block();
        __syncthreads();
    }
    nw_finish<false>(J, R, O);
}

// ASCII -> 2-bit store on the device: one thread per output word, 16 source bytes each.  An N (anything but ACGT) gets a base hashed
// from its position and its bit in the mask word; the word in front of the mask array says whether the batch has any (nm_active)
__global__ __launch_bounds__(256) void k_pack_ascii(const char *__restrict__ ascii, const uint64_t *__restrict__ asc_off,
                                                    const uint32_t *__restrict__ word_off, const int32_t *__restrict__ read_len,
                                                    uint32_t n_reads, uint32_t total_words, uint32_t *__restrict__ words, uint32_t *__restrict__ nm_out)
{
    const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= total_words) return;
    const uint32_t r = seq_of_word(word_off, n_reads, w);
    const int len = read_len[r];
    const int b0 = (int)(w - word_off[r]) * 16;
    const char *src = ascii + asc_off[r] + b0;
    uint32_t v = 0, m = 0;
    for (int j = 0; j < 16 && b0 + j < len; j++) {
        const char c = src[j];
        uint32_t code = (c == 'C' || c == 'c') ? 1u : (c == 'G' || c == 'g') ? 2u : (c == 'T' || c == 't') ? 3u : 0u;
        if (code == 0u && c != 'A' && c != 'a') { code = n_substitute((uint32_t)(b0 + j)); m |= 1u << j; }     // N (anything else): see tbase
        v |= code << (2 * j);
    }
    words[w] = v;
    nm_out[w] = m;
    if (m) atomicOr(&nm_out[-FSV_NM_LEAD], 1u);      // (rare: a window with an N)
}

} // namespace
