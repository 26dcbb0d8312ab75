// k_chain.h -- the chain stage of the per-read-set assembly: the pair table, where a pair's per-anchor arrays live (the LDS tile, the HBM
// slab), chain_core, the four k_chain* kernels and chain_lds_bytes.  Included by asm_kernels.h after its shared constants and PhaseClock.
#pragma once
#include <type_traits>

namespace {

// ------------------------------------------------------------------------------------------------ k_chain

struct ChainArgs {
    const uint32_t *store;
    const uint32_t *word_off;
    const int32_t *read_len;
    const uint32_t *set_start;   // n_sets + 1
    const uint32_t *pair_base;   // n_sets + 1: ordered-pair slots
    const uint32_t *upair_base;  // n_sets + 1: unordered pairs (one block each)
    const uint32_t *pair_list;   // optional: block b works on unordered pair pair_list[b] (nullptr: pair b)
    const uint32_t *n_list_dev;  // with pair_list: its length, left on the device by the kernel that built it (blocks beyond it return)
    const uint4 *upair_tab;      // per unordered pair: {first read of the set, q | t << 16, slot (q,t), slot (t,q)}  (k_pair_tab)
    int32_t amax;                // anchors per pair held in LDS (multiple of 64, <= FSV_AMAX): sizes the dynamic LDS
    const fsv_mz *mz;
    const uint32_t *mz_off;
    const uint32_t *mz_cnt;
    fsv_ovl *ovl;                // one slot per ordered pair
    fsv_wtask *tasks;
    uint32_t *task_counter;
    uint32_t task_cap;
    uint32_t *overflow;          // set to 1 when the task array is full
    uint32_t *warn;              // per read
    uint32_t *set_cols;          // per read, used at the first read of every set: K5 columns emitted for the set (statistics)
    const uint8_t *thr_tab;      // 376 entries: threshold for a window of that length
    uint32_t n_sets;
    int32_t k_score, min_anchors, min_ovlp, bw, emit_tasks;
    int32_t primary_only;        // 1 (without tasks only): the slot of (q, t) alone is written -- the overlap of t on q is chained from t's side by a second launch
    unsigned long long *stamps;  // diagnostic (FSV_CHAIN_STAMPS=1): shader cycles per phase summed over the waves, else nullptr
    uint32_t *wide_list, *n_wide; // pairs whose two lists both have more than amax entries (only they can have more than amax anchors) are
                                  // set aside here and chained by k_chain_wide_list with the large tile; nullptr: chain every pair here
    uint4 *spill_list; uint32_t *n_spill;   // full_lists = 1: a pair with more anchors than the tile in use is not cut but set aside here, as its pair-table
                                            // record (roles as chained), and chained by k_chain_spill in HBM; nullptr: cut and flagged FSV_W_ANCHOR_TRUNC
};

// The unordered pairs of every set, enumerated once per batch: block b of k_chain reads one 16-byte record instead of
// searching the set table and inverting the triangular index (a dozen dependent global loads per block).
// the pair table with the roles of the two reads swapped (the final pass's gapped re-chain chains a pair from either side)
__global__ void k_pair_tab_swap(const uint4 *__restrict__ tab, uint32_t n_upairs, uint4 *__restrict__ out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_upairs) return;
    const uint4 v = tab[i];
    out[i] = make_uint4(v.x, (v.y >> 16) | (v.y << 16), v.w, v.z);
}

__global__ void k_pair_tab(const uint32_t *__restrict__ set_start, const uint32_t *__restrict__ pair_base, const uint32_t *__restrict__ upair_base,
                           uint32_t n_sets, uint32_t n_upairs, uint4 *__restrict__ tab, uint32_t *__restrict__ pair_read)
{
    const uint32_t up = blockIdx.x * blockDim.x + threadIdx.x;
    if (up >= n_upairs) return;
    uint32_t lo = 0, hi = n_sets;
    while (hi - lo > 1) { uint32_t mid = (lo + hi) >> 1; if (upair_base[mid] <= up) lo = mid; else hi = mid; }
    const uint32_t s = lo, r0 = set_start[s], ns = set_start[s + 1] - r0;
    const uint32_t idx = up - upair_base[s];
    // row q holds the pairs (q, q+1..ns-1): rows start at q*(2ns-q-1)/2
    uint32_t q = (uint32_t)((2.0 * ns - 1.0 - sqrt((2.0 * ns - 1.0) * (2.0 * ns - 1.0) - 8.0 * (double)idx)) * 0.5);
    while (q > 0 && (uint64_t)q * (2ull * ns - q - 1) / 2 > idx) q--;
    while ((uint64_t)(q + 1) * (2ull * ns - q - 2) / 2 <= idx) q++;
    const uint32_t t = q + 1 + (idx - (uint32_t)((uint64_t)q * (2ull * ns - q - 1) / 2));
    tab[up] = make_uint4(r0, q | t << 16, pair_base[s] + q * (ns - 1) + (t - 1), pair_base[s] + t * (ns - 1) + q);
    // the query read of either ordered slot (k_bnd_tasks: one load instead of a search of the set table)
    pair_read[pair_base[s] + q * (ns - 1) + (t - 1)] = r0 + q;
    pair_read[pair_base[s] + t * (ns - 1) + q] = r0 + t;
}

// candidate (i <- j) of the chain DP: score or -1, with the chain's indel sum / span it would give (chain_core)
__device__ __forceinline__ int chain_eval(const int bw, const int kk, int qe, int te, int qj, int tj, int indj, int slj, int fj, int &ti, int &tl)
{
    const int dq = qe - qj, dt = te - tj;
    if (dq <= 0 || dt <= 0) return -1;
    const int gap = dq > dt ? dq - dt : dt - dq;
    ti = indj + gap; tl = slj + dq;
    // 64-bit divisions cost ~150 VALU ops on gfx950; the operands fit 32 bits for every read below 2^17 bases (a legal
    // ti <= tl*bw/1000 <= 2621, sc <= 63; ti is tested too: the block hypothesis sums up to 64 gaps before it asks): same quotient either way
    if (tl < (1 << 17) && gap < (1 << 17) && ti < (1 << 17) && bw <= 20) {
        if ((uint32_t)ti * 1000u > (uint32_t)tl * (uint32_t)bw) return -1;
        int sc = min(min(dq, dt), kk);
        if (ti) sc -= (int)(((uint32_t)ti * (uint32_t)sc * 1000u) / ((uint32_t)tl * (uint32_t)bw));
        return sc + fj;
    }
    if ((long long)ti * 1000 > (long long)tl * bw) return -1;
    int sc = min(min(dq, dt), kk);
    if (ti) sc -= (int)(((long long)ti * sc * 1000) / ((long long)tl * bw));
    return sc + fj;
}

// the window tasks of both directions of an overlap (o: q on t, om: its mirror) from its chain: ch_q(e) / ch_t(e) give chain anchor e's
// coordinates in start-to-end order, 0 <= e < cnt, wherever the caller keeps the chain (LDS tile or HBM slab)
template <class CQ, class CT>
__device__ __forceinline__ void chain_window_tasks(const ChainArgs &A, const CQ ch_q, const CT ch_t, const int cnt, const int lane, const fsv_ovl &o, const fsv_ovl &om,
                                                   const uint32_t first_win, const uint32_t xw, const uint32_t yw, const int lenq, const int lent, const int rev,
                                                   const uint32_t p, const uint32_t pm, const int xs, const int xe)
{
    {
        const int w0 = xs / FSV_WINDOW;
        for (int j = lane; j < o.n_win; j += 64) {
            const int gs = (w0 + j) * FSV_WINDOW, ge = gs + FSV_WINDOW - 1;
            const int x_start = max(gs, xs);
            const int x_len = min(ge, xe) - x_start + 1;
            // diagonal of the last chain anchor with qe <= x_start, else of the first one
            int lo2 = 0, hi2 = cnt;
            while (lo2 < hi2) { int mid = (lo2 + hi2) >> 1; if (ch_q(mid) <= x_start) lo2 = mid + 1; else hi2 = mid; }
            const int e = lo2 == 0 ? 0 : lo2 - 1;
            const int diag = ch_t(e) - ch_q(e);
            fsv_wtask w;
            w.x_word = xw; w.y_word = yw; w.x_start = x_start; w.y_start = x_start + diag; w.y_len = lent;
            w.x_len = (uint16_t)x_len; w.k = A.thr_tab[x_len]; w.y_rev = (uint8_t)rev; w.ovl = p; w.win = (uint32_t)j;
            A.tasks[first_win + j] = w;
        }
    }
    {
        // mirrored direction: query t, target q.  Mirrored anchor of e: same strand (ct_e, cq_e) in the same order;
        // reverse strand (lent-1-ct_e, lenq-1-cq_e) in reversed order.
        const int mxs = om.x_s, mxe = om.x_e, w0 = mxs / FSV_WINDOW;
        for (int j = lane; j < om.n_win; j += 64) {
            const int gs = (w0 + j) * FSV_WINDOW, ge = gs + FSV_WINDOW - 1;
            const int x_start = max(gs, mxs);
            const int x_len = min(ge, mxe) - x_start + 1;
            int diag;
            if (!rev) {
                int lo2 = 0, hi2 = cnt; // last anchor with ct <= x_start
                while (lo2 < hi2) { int mid = (lo2 + hi2) >> 1; if (ch_t(mid) <= x_start) lo2 = mid + 1; else hi2 = mid; }
                const int e = lo2 == 0 ? 0 : lo2 - 1;
                diag = ch_q(e) - ch_t(e);
            } else {
                // mirrored query coordinate lent-1-ct_e decreases with e: the last mirrored anchor with coordinate <= x_start is the
                // smallest e with ct_e >= lent-1-x_start; none -> the first mirrored anchor (e = cnt-1)
                const int thr = lent - 1 - x_start;
                int lo2 = 0, hi2 = cnt; // first e with ct_e >= thr
                while (lo2 < hi2) { int mid = (lo2 + hi2) >> 1; if (ch_t(mid) < thr) lo2 = mid + 1; else hi2 = mid; }
                const int e = lo2 == cnt ? cnt - 1 : lo2;
                diag = (lenq - 1 - ch_q(e)) - (lent - 1 - ch_t(e));
            }
            fsv_wtask w;
            w.x_word = yw; w.y_word = xw; w.x_start = x_start; w.y_start = x_start + diag; w.y_len = lenq;
            w.x_len = (uint16_t)x_len; w.k = A.thr_tab[x_len]; w.y_rev = (uint8_t)rev; w.ovl = pm; w.win = (uint32_t)j;
            A.tasks[om.first_win + j] = w;
        }
    }
}

// A pair of the pair table as the chain kernels take it: the record, the two reads' lengths and list sizes, and the two lists
// (query: the position-sorted copy, target: hash-sorted)
struct ChainPair { uint4 pt; int lenq, lent, nq, nt; const fsv_mz *mq, *mt; };
__device__ __forceinline__ ChainPair chain_pair_of(const ChainArgs &A, const uint4 pt)
{
    const uint32_t rq = pt.x + (pt.y & 0xffffu), rt = pt.x + (pt.y >> 16);
    ChainPair P;
    P.pt = pt;
    P.lenq = A.read_len[rq]; P.lent = A.read_len[rt];
    P.nq = (int)A.mz_cnt[rq]; P.nt = (int)A.mz_cnt[rt];
    P.mq = A.mz + A.mz_off[rq] + P.nq; P.mt = A.mz + A.mz_off[rt];
    return P;
}

// ---- where a pair's per-anchor arrays live and how they are packed: chain_core is written once over one of these.  A storage type
// supplies the key packing, the arrays (or typed accessors), the "no predecessor" value, the width of the repair step's packed maximum
// and whether phase stamps exist.


// The LDS tile.  SHORT (every read of the batch shorter than 65 536 bases -- all HiFi data): 12 B per anchor -- the anchor's two
// positions as 16-bit halves of one word, score / run start / predecessor / chain entry as 16-bit values (a chain of at most
// 1 024 anchors scores at most 1 024 x 63), the anchors' strands in a 128-byte bitmap, and the target's sorted hashes staged
// in the 8 B the DP arrays do not need yet (position / span / strand of a hit come from the L2-resident list).  Round 1 used
// 24 B (64-bit keys, 32-bit DP arrays, 12-byte staged records), which capped the kernel at 1-2 waves per SIMD on the batch's
// longest lists; the long layout is kept for batches with a read of 65 536 bases or more.
//   SHORT: key | f | ind | pred | chain, 2 B each behind the 4-byte keys (8 B: the staged target hashes lie over all four) | strand bitmap
//   long:  key | f | ind | (4 B only used by the staged records) | pred | chain
// sl, the chain span per anchor, lives in arrays that are free during the DP: over chain (SHORT), over the staging area (long).
template <bool SHORT>
struct ChainTile {
    using key_t = typename std::conditional<SHORT, uint32_t, uint64_t>::type;   // qe << 16 | te   or   qe << 32 | te
    using dp_t = typename std::conditional<SHORT, uint16_t, int32_t>::type;
    using idx_t = uint16_t;
    using pack_t = int;             // candidate score * 64 + lane: a tile's scores stay far below 2^25
    using Clock = PhaseClock<true>;
    static constexpr int NONE = 0xffff;
    static constexpr int KSH = SHORT ? 16 : 32;
    static constexpr uint64_t KMASK = SHORT ? 0xffffull : 0xffffffffull;
    int cap;                        // anchors the tile holds
    key_t *key;
    unsigned char *rest;            // behind the keys: the staged target list until the DP starts, then the arrays below
    dp_t *f, *ind, *sl;
    idx_t *pred, *chain;            // long: pred holds t span | strand << 8 until the compaction, then the predecessor index
    uint32_t *strand_bits;          // SHORT only: one strand bit per anchor (cap / 8 B)
    __device__ __forceinline__ ChainTile(unsigned char *s_raw, const int amax)
    {
        cap = amax;
        key = (key_t *)s_raw;
        rest = s_raw + sizeof(key_t) * (size_t)amax;
        f = (dp_t *)rest; ind = f + amax;
        pred = (idx_t *)(rest + (SHORT ? 4 : 12) * (size_t)amax);
        chain = pred + amax;
        sl = SHORT ? (dp_t *)chain : (dp_t *)(rest + 8 * (size_t)amax);
        strand_bits = (uint32_t *)(rest + (SHORT ? 8 : 16) * (size_t)amax);
    }
    static __device__ __forceinline__ key_t make_key(uint32_t q_, uint32_t t_) { return (key_t)(((uint64_t)q_ << KSH) | (uint64_t)t_); }
    __device__ __forceinline__ int q(int i) const { return (int)((uint64_t)key[i] >> KSH); }
    __device__ __forceinline__ int t(int i) const { return (int)((uint64_t)key[i] & KMASK); }
    __device__ __forceinline__ int strand(int i) const { return SHORT ? (int)((strand_bits[i >> 5] >> (i & 31)) & 1u) : (int)(pred[i] >> 8); }
    __device__ __forceinline__ void put_anchor(int at, key_t k, uint32_t srev, uint32_t tspan) const
    {
        key[at] = k;
        if (SHORT) { if (srev) atomicOr(&strand_bits[at >> 5], 1u << (at & 31)); }
        else pred[at] = (uint16_t)(tspan | (srev << 8));
    }
    static __device__ __forceinline__ pack_t wave_max(pack_t v) { return wave_max_i32(v); }
};

// The slab in HBM (k_chain_spill): 64-bit keys whatever the read lengths, 32-bit scores and indices with -1 as "none", a strand byte --
// 29 B per anchor in FSV_SPILL_BYTES
#define FSV_SPILL_BYTES 32   // slab bytes per anchor
struct ChainSlab {
    using key_t = uint64_t;
    using dp_t = int32_t;
    using idx_t = int32_t;
    using pack_t = long long;       // slab scores can pass 2^25
    using Clock = PhaseClock<false>;
    static constexpr int NONE = -1;
    int cap;
    key_t *key;
    dp_t *f, *ind, *sl;
    idx_t *pred, *chain;
    uint8_t *strand_byte;
    __device__ __forceinline__ ChainSlab(unsigned char *slab, const uint32_t cap_)
    {
        cap = (int)cap_;
        key = (uint64_t *)slab;
        f = (int32_t *)(slab + 8 * (size_t)cap_); ind = f + cap_; sl = ind + cap_; pred = sl + cap_; chain = pred + cap_;
        strand_byte = (uint8_t *)(chain + cap_);
    }
    static __device__ __forceinline__ key_t make_key(uint32_t q_, uint32_t t_) { return ((uint64_t)q_ << 32) | (uint64_t)t_; }
    __device__ __forceinline__ int q(int i) const { return (int)(key[i] >> 32); }
    __device__ __forceinline__ int t(int i) const { return (int)(key[i] & 0xffffffffull); }
    __device__ __forceinline__ int strand(int i) const { return (int)strand_byte[i]; }
    __device__ __forceinline__ void put_anchor(int at, key_t k, uint32_t srev, uint32_t) const { key[at] = k; strand_byte[at] = (uint8_t)srev; }
    static __device__ __forceinline__ pack_t wave_max(pack_t v) { return wave_max_i64(v); }
};

// ---- step 1's shared pieces

// the anchor's query coordinate.  A reverse-strand anchor is kept as hifiasm chains such a pair (Hash_Table.cpp:619-676, x_pos_strand = 1):
// the query on its reverse strand -- the k-mer's last base there -- and the target forward; the chain's indel budget runs from that end
__device__ __forceinline__ uint32_t chain_anchor_q(const uint4 av, const uint32_t srev, const int lenq)
{
    const uint32_t qrev = (uint32_t)(lenq - 1) - (av.z - ((av.w >> 8) & 0xffu) + 1);   // (computed either way: a select, not a branch per lookup)
    return srev ? qrev : av.z;
}

// q minimizer av looked up in the target's hash-sorted list in memory (the slab path's every lookup; the tile path's when the list is not
// in LDS): a hit gives the anchor's two coordinates, its strand and the target k-mer's span
__device__ __forceinline__ bool chain_lookup_mem(const fsv_mz *mt, const int nt, const uint4 av, const int lenq, uint32_t &aq, uint32_t &at, uint32_t &srev, uint32_t &tspan)
{
    const uint64_t ah = (uint64_t)av.x | (uint64_t)av.y << 32;
    const int l2 = mz_lower_bound(mt, nt, ah);
    if (!(l2 < nt && mt[l2].hash == ah)) return false;
    const fsv_mz b = mt[l2];
    srev = (av.w & 0xffu) ^ b.rev; tspan = b.span;
    aq = chain_anchor_q(av, srev, lenq); at = b.pos;
    return true;
}

// a batch of up to 64 lookups appended to the anchor list in lane order (entries beyond the storage's capacity are counted, not stored)
template <class S>
__device__ __forceinline__ void chain_commit(const S &st, const int lane, const bool hit, const typename S::key_t key, const uint32_t srev, const uint32_t tspan,
                                             int &n, int &nrev, int &nfwd)
{
    const uint64_t m = __ballot(hit);
    const int at = n + __popcll(m & ((1ull << lane) - 1));
    if (hit && at < st.cap) st.put_anchor(at, key, srev, tspan);
    nrev += __popcll(__ballot(hit && srev));
    nfwd += __popcll(__ballot(hit && !srev));
    n += __popcll(m);
}

// ---- steps 2-7: from the anchor list (n anchors in lookup order in st, nrev / nfwd of them on either strand) to both ordered slots and
// both window-task lists.  One wavefront; lane is the caller's lane index.
template <class S>
__device__ __forceinline__ void chain_core(const ChainArgs &A, const S &st, const ChainPair &P, int n, const int nrev, const int nfwd, const int lane, typename S::Clock &clk)
{
    using key_t = typename S::key_t;
    using dp_t = typename S::dp_t;
    using idx_t = typename S::idx_t;
    using pack_t = typename S::pack_t;
    const uint4 pt = P.pt;
    const int lenq = P.lenq, lent = P.lent;
    const uint32_t q = pt.y & 0xffffu, t = pt.y >> 16;
    const uint32_t p = pt.z, pm = pt.w;     // ordered slots (q, t) and (t, q)
    const uint32_t rq = pt.x + q, rt = pt.x + t;
    fsv_ovl o;
    o.q = q; o.t = t; o.x_s = o.x_e = o.y_s = o.y_e = 0; o.score = 0; o.n_chain = 0; o.chain_off = 0; o.first_win = 0; o.n_win = 0;
    o.align_len = 0; o.err_sum = 0; o.rev = 0; o.is_match = 0; o.exact = 0; o.valid = 0;
    fsv_ovl om = o; // the mirrored overlap (t on q)
    om.q = t; om.t = q;
    auto put_both = [&]() { if (lane == 0) { A.ovl[p] = o; if (!A.primary_only) A.ovl[pm] = om; } };
    // 2. majority strand, compaction
    const int rev = nrev > nfwd;
    int m2 = 0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        bool keep = false; key_t key = 0;
        if (i < n) { key = st.key[i]; keep = st.strand(i) == rev; }
        const uint64_t m = __ballot(keep);
        const int at = m2 + __popcll(m & ((1ull << lane) - 1));
        __syncthreads();
        if (keep) st.key[at] = key;
        m2 += __popcll(m);
        __syncthreads();
    }
    n = m2;
    if (n < A.min_anchors) { put_both(); clk.mark(A.stamps, lane, 2); return; }
    // 3. anchors are in query order: q's minimizers were walked by position and both compactions keep the order (query positions
    //    are distinct, so (qe, te) order == qe order) -- for a reverse-strand pair that is decreasing order on the query's reverse
    //    strand, so the list is turned around
    if (rev) {
        for (int i = lane; i < n / 2; i += 64) { const key_t a0 = st.key[i], a1 = st.key[n - 1 - i]; st.key[i] = a1; st.key[n - 1 - i] = a0; }
        __syncthreads();
    }
    // 4. chain DP: lane l examines predecessor i-1-l (nearest first on ties).
    //    Fast path: when every anchor sits on one diagonal (error-free reads: correction rounds 2, 3 and the final pass)
    //    the DP provably links each anchor to its nearest predecessor -- gap 0 means no indel penalty, and
    //    f[i-1] + min(d_i,k) >= f[j] + min(qe_i - qe_j, k) for every j < i-1 because min(.,k) is sub-additive, with the
    //    nearest predecessor winning ties -- so the chain is the whole list and the score a running sum.
    clk.mark(A.stamps, lane, 3);
    bool colinear;
    {
        const int d0 = st.t(0) - st.q(0);
        bool same = true;
        for (int i = lane; i < n; i += 64) same = same && (st.t(i) - st.q(i) == d0);
        colinear = __all(same);
    }
    if (colinear) {
        int acc = 0;
        for (int i = 1 + lane; i < n; i += 64) acc += min(st.q(i) - st.q(i - 1), A.k_score);
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
        for (int i = lane; i < n; i += 64) { st.pred[i] = (idx_t)(i == 0 ? S::NONE : i - 1); st.f[i] = (dp_t)(i == n - 1 ? A.k_score + acc : 0); }
        __syncthreads();
    } else {
        // Reads with errors: the anchors leave the diagonal at every indel, and the DP of the reference (Hash_Table.cpp:425-616 as
        // restated in oracle/asm.c: look back 64 anchors, link to the best-scoring predecessor, the nearer one on ties) is a chain
        // of n dependent steps.  But it almost always links an anchor to the one just before it, so 64 anchors are settled at once:
        //   hypothesis   every anchor of the block links to its predecessor; the chain's indel sum, span and score are then
        //                prefix sums over the block (three wave scans);
        //   proof        cand(i, j) <= f[j] + k for any other predecessor j, so only the j with f[j] + k > f[i] can beat the
        //                hypothesis (usually none, or i-2): those candidates are evaluated exactly as the DP does;
        //   repair       the first anchor whose hypothesis fails (an illegal link, a better candidate) and the few behind it go
        //                through the sequential step -- the 64 predecessors in registers, lane l = anchor i-1-l, handed on by
        //                DPP wave_shr -- and the blocks resume after them.
        // By induction over the anchors the result is the sequential DP's, bit for bit (tests/test_gpu_chain.py and
        // tests/test_gpu_long_chain.py: every record and window task against the oracle, on the pairs of tests/chain_cases.py).
        const int kk = A.k_score;
        auto eval = [&](int qe, int te, int qj, int tj, int indj, int slj, int fj, int &ti, int &tl) { return chain_eval(A.bw, kk, qe, te, qj, tj, indj, slj, fj, ti, tl); };
        if (lane == 0) { st.f[0] = (dp_t)kk; st.pred[0] = (idx_t)S::NONE; st.ind[0] = 0; st.sl[0] = 0; }
        __syncthreads();
        int i0 = 1;
        while (i0 < n) {
            const int nb = min(64, n - i0), i = i0 + lane;
            const bool in = lane < nb;
            int qe = 0, te = 0, dq = 0, dt = 0, gap = 0;
            if (in) { qe = st.q(i); te = st.t(i); dq = qe - st.q(i - 1); dt = te - st.t(i - 1); gap = dq > dt ? dq - dt : dt - dq; }
            const int ti = (int)st.ind[i0 - 1] + wave_incl_sum(gap, lane), tl = (int)st.sl[i0 - 1] + wave_incl_sum(dq, lane);
            bool legal = in && dq > 0 && dt > 0;
            int sc = 0;
            if (legal) {
                int t2, l2;
                const int c = eval(qe, te, qe - dq, te - dt, ti - gap, tl - dq, 0, t2, l2);
                legal = c >= 0; sc = c;
            }
            const int fi = (int)st.f[i0 - 1] + wave_incl_sum(legal ? sc : 0, lane);
            bool bad = in && !(legal && fi > kk);
            __syncthreads();
            if (in) { st.f[i] = (dp_t)fi; st.ind[i] = (dp_t)ti; st.sl[i] = (dp_t)tl; }
            __syncthreads();
            // The look-back stops where no earlier anchor can matter any more: P[j] = max f over the 64 anchors before the block
            // and the block up to j never decreases with j, so once P[i-d] + k <= f[i] nothing at distance d or beyond can beat
            // the hypothesis.  Scores grow by ~35 an anchor, so that is after two or three steps -- the loop used to run all 63
            // (a dependent LDS read each) whenever the block had that many predecessors: most of the round-1 DP's time.
            // f and P of the 128 anchors sit in registers; distance d is a lane rotation.
            const int pj0 = i0 - 64 + lane;
            const int pf = pj0 >= 0 ? (int)st.f[pj0] : 0, cf = in ? fi : 0;
            int pP = pf, cP = cf;
            for (int off = 1; off < 64; off <<= 1) {
                const int o1 = __shfl_up(pP, off, 64), o2 = __shfl_up(cP, off, 64);
                if (lane >= off) { pP = max(pP, o1); cP = max(cP, o2); }
            }
            cP = max(cP, __shfl(pP, 63, 64));
            bool live = in && !bad;
            for (int d = 2; d <= 64; d++) {
                const int j = i - d, src = (lane - d) & 63;
                const int f_c = __shfl(cf, src, 64), f_p = __shfl(pf, src, 64), P_c = __shfl(cP, src, 64), P_p = __shfl(pP, src, 64);
                const int fj = lane >= d ? f_c : f_p, Pj = lane >= d ? P_c : P_p;
                live = live && !bad && j >= 0 && Pj + kk > fi;
                if (!__any(live)) break;
                const bool need = live && fj + kk > fi;
                if (__any(need)) {
                    if (need) {
                        int t2, l2;
                        if (eval(qe, te, st.q(j), st.t(j), (int)st.ind[j], (int)st.sl[j], fj, t2, l2) > fi) bad = true;
                    }
                }
            }
            const uint64_t badm = __ballot(bad);
            const int good = badm ? (int)__ffsll((long long)badm) - 1 : nb;     // anchors i0 .. i0 + good - 1 stand
            if (lane < good) st.pred[i] = (idx_t)(i - 1);
            __syncthreads();
            i0 += good;
            if (good == nb) continue;
            // sequential steps for the anchor that broke the hypothesis and up to seven behind it
            const int s1 = min(n, i0 + 8);
            int pq = 0, pt2 = 0, rind = 0, rsl = 0, rf = 0;
            { const int j = i0 - 1 - lane; if (j >= 0) { pq = st.q(j); pt2 = st.t(j); rind = (int)st.ind[j]; rsl = (int)st.sl[j]; rf = (int)st.f[j]; } }
            for (int is = i0; is < s1; is++) {
                const int qe2 = st.q(is), te2 = st.t(is);
                const int j = is - 1 - lane;
                int cand = -1, ti2 = 0, tl2 = 0;
                if (j >= 0) cand = eval(qe2, te2, pq, pt2, rind, rsl, rf, ti2, tl2);
                // pack so that the max prefers the higher score, then the nearer predecessor
                const pack_t packed = cand < 0 ? (pack_t)-1 : (pack_t)cand * 64 + (63 - lane);
                const pack_t bestp = S::wave_max(packed);
                const int bests = bestp < 0 ? -1 : (int)(bestp >> 6);
                int nf = kk, nind = 0, nsl = 0, npred = S::NONE;
                if (bests > kk) {
                    const int wl = 63 - (int)(bestp & 63);
                    nf = bests; npred = is - 1 - wl;
                    nind = __builtin_amdgcn_readlane(ti2, wl); nsl = __builtin_amdgcn_readlane(tl2, wl);
                }
                if (lane == 0) { st.f[is] = (dp_t)nf; st.pred[is] = (idx_t)npred; st.ind[is] = (dp_t)nind; st.sl[is] = (dp_t)nsl; }
                pq = __builtin_amdgcn_update_dpp(qe2, pq, 0x138, 0xF, 0xF, false);    // wave_shr:1, lane 0 <- the new anchor
                pt2 = __builtin_amdgcn_update_dpp(te2, pt2, 0x138, 0xF, 0xF, false);
                rind = __builtin_amdgcn_update_dpp(nind, rind, 0x138, 0xF, 0xF, false);
                rsl = __builtin_amdgcn_update_dpp(nsl, rsl, 0x138, 0xF, 0xF, false);
                rf = __builtin_amdgcn_update_dpp(nf, rf, 0x138, 0xF, 0xF, false);
            }
            __syncthreads();
            i0 = s1;
        }
        __syncthreads();
    }
    clk.mark(A.stamps, lane, 4);
    // 5. best chain end: highest score, smallest index on ties
    long long bk = -1;
    for (int i = lane; i < n; i += 64) { const long long v = ((long long)st.f[i] << 32) | (long long)(0x7fffffff - i); bk = v > bk ? v : bk; }
    bk = wave_max_i64(bk);
    const int best = 0x7fffffff - (int)(bk & 0xffffffffll);
    // 6. walk back, chain stored end-to-start in st.chain.  A step-by-step walk is ~n dependent reads; instead every
    //    anchor learns the start of its run of "predecessor == previous anchor" links (a max-scan; st.ind is free after the
    //    DP) and the walk copies whole runs, one dependent step per break in the chain.
    int cnt = 0;
    if (colinear) {
        for (int e = lane; e <= best; e += 64) st.chain[e] = (idx_t)(best - e);
        cnt = best + 1;
    } else {
        int carry = 0;
        for (int base = 0; base < n; base += 64) {
            const int i = base + lane;
            int v = (i < n && i > 0 && st.pred[i] == (idx_t)(i - 1)) ? -1 : i; // run start candidate
            if (i >= n) v = -1;
            for (int off = 1; off < 64; off <<= 1) { const int o2 = __shfl_up(v, off, 64); if (lane >= off) v = max(v, o2); }   // (wave_incl_max: written out, the call reorders the k_chain kernels' code)
            v = max(v, carry);
            if (i < n) st.ind[i] = (dp_t)v;
            carry = __shfl(v, 63, 64);
        }
        __syncthreads();
        int c = best;
        while (c != S::NONE) {
            const int r = st.ind[c];
            for (int e = lane; e <= c - r; e += 64) st.chain[cnt + e] = (idx_t)(c - e);
            cnt += c - r + 1;
            c = st.pred[r];
        }
    }
    __syncthreads();
    clk.mark(A.stamps, lane, 5);
    if (cnt < A.min_anchors) { put_both(); return; }
    const int first = st.chain[cnt - 1];
    int xs = st.q(first), ys = st.t(first);
    int xe = st.q(best), ye = st.t(best);
    { int m = min(xs, ys); xs -= m; ys -= m; int r = min(lenq - 1 - xe, lent - 1 - ye); xe += r; ye += r; }
    if (xe - xs + 1 < A.min_ovlp) { put_both(); return; }
    const int score_best = st.f[best];
    if (rev) {
        // everything downstream works with the query forward and the target on its reverse strand: mirror the overlap and every
        // anchor, and turn the chain list around so that it still runs end-to-start in query order
        { const int t0 = xs; xs = (lenq - 1) - xe; xe = (lenq - 1) - t0; }
        { const int t0 = ys; ys = (lent - 1) - ye; ye = (lent - 1) - t0; }
        __syncthreads();
        for (int i = lane; i < n; i += 64) {
            const int kq = st.q(i), kt2 = st.t(i);
            st.key[i] = S::make_key((uint32_t)((lenq - 1) - kq), (uint32_t)((lent - 1) - kt2));
        }
        for (int e = lane; e < cnt / 2; e += 64) { const idx_t c0 = st.chain[e], c1 = st.chain[cnt - 1 - e]; st.chain[e] = c1; st.chain[cnt - 1 - e] = c0; }
        __syncthreads();
    }
    o.x_s = xs; o.x_e = xe; o.y_s = ys; o.y_e = ye; o.rev = (uint8_t)rev; o.score = score_best; o.n_chain = cnt; o.valid = 1;
    o.n_win = xe / FSV_WINDOW - xs / FSV_WINDOW + 1;
    // mirror: same anchors seen from t; on the reverse strand both coordinates are measured from the other read end
    om.rev = (uint8_t)rev; om.score = o.score; om.n_chain = cnt; om.valid = 1;
    if (!rev) { om.x_s = ys; om.x_e = ye; om.y_s = xs; om.y_e = xe; }
    else { om.x_s = lent - 1 - ye; om.x_e = lent - 1 - ys; om.y_s = lenq - 1 - xe; om.y_e = lenq - 1 - xs; }
    om.n_win = om.x_e / FSV_WINDOW - om.x_s / FSV_WINDOW + 1;
    if (!A.emit_tasks) { o.n_win = 0; om.n_win = 0; put_both(); return; }
    // 7. window tasks of both directions
    uint32_t first_win = 0;
    if (lane == 0) {
        first_win = atomicAdd(A.task_counter, (uint32_t)(o.n_win + om.n_win));
        // statistics: DP columns of the windows handed to K5, both directions; one counter per set (indexed by the set's first
        // read) -- a single shared counter costs ~10 ns per pair in same-address atomics
        atomicAdd(&A.set_cols[pt.x], (uint32_t)(xe - xs + 1) + (uint32_t)(om.x_e - om.x_s + 1));
    }
    first_win = __shfl(first_win, 0, 64);
    if ((uint64_t)first_win + (uint32_t)(o.n_win + om.n_win) > A.task_cap) {
        if (lane == 0) { atomicExch(A.overflow, 1u); o.valid = 0; o.n_win = 0; om.valid = 0; om.n_win = 0; A.ovl[p] = o; A.ovl[pm] = om; }
        return;
    }
    o.first_win = (int32_t)first_win;
    om.first_win = (int32_t)(first_win + (uint32_t)o.n_win);
    const uint32_t xw = A.word_off[rq], yw = A.word_off[rt];
    chain_window_tasks(A, [&](int e) { return st.q(st.chain[cnt - 1 - e]); }, [&](int e) { return st.t(st.chain[cnt - 1 - e]); }, cnt, lane, o, om, first_win, xw, yw, lenq, lent, rev, p, pm, xs, xe);
    put_both();
    clk.mark(A.stamps, lane, 6);
}

// One wavefront per UNORDERED read pair (q < t) of a set: the chain is computed with q as the query and the overlap of t on
// q is its mirror image (oracle/asm.c collect_overlaps); both ordered slots and both window-task lists are written here.
// This is step 1 for the LDS tile -- the anchors -- and chain_core on them.
#define FSV_CHAIN_QR 12   // the query list sits in registers when it has at most 64 x this many entries (768: reads up to ~27 kb; 16 would cost the third wave per SIMD)
template <bool SHORT>
__device__ __forceinline__ void chain_pair(const ChainArgs &A, unsigned char *s_raw, const ChainPair &P, const uint4 (&qa)[FSV_CHAIN_QR])
{
    using Tile = ChainTile<SHORT>;
    const int AMAX = A.amax;
    const Tile st(s_raw, AMAX);
    const int lenq = P.lenq, lent = P.lent, nq = P.nq, nt = P.nt;
    const fsv_mz *const mt = P.mt;
    int lane_ = threadIdx.x;
    // (opaque to the optimiser: called in a loop, the compiler otherwise hoists every lane-derived constant of the body out of it
    // and holds them in ~80 extra registers -- two waves per SIMD instead of three)
    asm volatile("" : "+v"(lane_));
    const int lane = lane_;
    typename Tile::Clock clk(A.stamps && (blockIdx.x & 63u) == 0u);

    // 1. anchors: every q minimizer is looked up in t's sorted unique list.  All global loads are issued up front -- t's
    //    hashes go to LDS (the long layout also stages {pos, span, strand}: 12 B per entry in the DP arrays, free until the
    //    DP), q's records to registers (16 B per lane per 64 minimizers) -- so a pair pays one memory latency instead of two
    //    per batch of 64 lookups; the ~10 probes of a lookup are LDS reads.
    uint64_t *s_th = (uint64_t *)st.rest;
    uint32_t *s_tp = (uint32_t *)(st.rest + 8 * (size_t)AMAX);   // long layout only (staging them for SHORT too -- 16 B per anchor, 9 pairs per CU -- was slower)
    const bool t_in_lds = nt <= AMAX && lent < (1 << 23);
    const uint4 *mq4 = (const uint4 *)P.mq, *mt4 = (const uint4 *)mt;
    constexpr int QR = FSV_CHAIN_QR;
    const bool q_in_regs = nq <= 64 * FSV_CHAIN_QR;   // (the caller loaded them)
    if (t_in_lds) {
        // eight loads in flight per lane: written as a plain loop the compiler waits for every load before it issues the next
        // (s_waitcnt vmcnt(0) in front of each LDS write) -- seven dependent round trips for a 15 kb read's list, which was
        // most of the kernel's time
        for (int base = 0; base < nt; base += 512) {
            if (SHORT) {
                uint2 v[8];
#pragma unroll
                for (int u = 0; u < 8; u++) { const int i = base + u * 64 + lane; if (i < nt) v[u] = *reinterpret_cast<const uint2 *>(mt4 + i); }
#pragma unroll
                for (int u = 0; u < 8; u++) { const int i = base + u * 64 + lane; if (i < nt) s_th[i] = (uint64_t)v[u].x | (uint64_t)v[u].y << 32; }
            } else {
                uint4 v[8];
#pragma unroll
                for (int u = 0; u < 8; u++) { const int i = base + u * 64 + lane; if (i < nt) v[u] = mt4[i]; }
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    const int i = base + u * 64 + lane;
                    if (i < nt) {
                        s_th[i] = (uint64_t)v[u].x | (uint64_t)v[u].y << 32;
                        s_tp[i] = v[u].z | (v[u].w & 0xffu) << 31 | ((v[u].w >> 8) & 0xffu) << 23; // pos < 2^23 | span << 23 | strand << 31
                    }
                }
            }
        }
    }
    if (SHORT) for (int i = lane; i < AMAX / 32; i += 64) st.strand_bits[i] = 0u;
    __syncthreads();
    // the hashes are uniform, so their top six bits cut the sorted list into 64 buckets of a few entries each: one search per
    // lane finds the bucket bounds, and a lookup then needs ~3 probes instead of log2(nt) ~ 9 (the lookups were nearly all of
    // the kernel's instructions: every q minimizer against every t list of the set, overlapping or not)
    __shared__ uint32_t s_bk[65];
    if (t_in_lds) {
        int l2 = 0, h2 = nt;
        while (l2 < h2) { const int mid = (l2 + h2) >> 1; if ((uint32_t)(s_th[mid] >> 58) < (uint32_t)lane) l2 = mid + 1; else h2 = mid; }
        s_bk[lane] = (uint32_t)l2;
        if (lane == 0) s_bk[64] = (uint32_t)nt;
        __syncthreads();
    }
    clk.mark(A.stamps, lane, 0);
    int n = 0, nrev = 0, nfwd = 0;
    auto lookup = [&](int i, const uint4 av) {
        bool hit = false; typename Tile::key_t key = 0; uint32_t srev = 0, tspan = 0;
        if (i < nq) {
            if (t_in_lds) {
                const uint64_t ah = (uint64_t)av.x | (uint64_t)av.y << 32;
                int l2 = (int)s_bk[av.y >> 26], h2 = (int)s_bk[(av.y >> 26) + 1];
                while (l2 < h2) { int mid = (l2 + h2) >> 1; if (s_th[mid] < ah) l2 = mid + 1; else h2 = mid; }
                if (l2 < nt && s_th[l2] == ah) {
                    const uint32_t arev = av.w & 0xffu;
                    uint32_t tpos;
                    if (SHORT) { const uint4 b = mt4[l2]; tpos = b.z; srev = arev ^ (b.w & 0xffu); tspan = (b.w >> 8) & 0xffu; }
                    else { const uint32_t tp = s_tp[l2]; tpos = tp & 0x7fffffu; srev = arev ^ (tp >> 31); tspan = (tp >> 23) & 0xffu; }
                    hit = true; key = Tile::make_key(chain_anchor_q(av, srev, lenq), tpos);   // (packed here, under the hit: packed after the branches it cost the ONT batches' k_chain 1.3 %)
                }
            } else {
                uint32_t aq, at;
                hit = chain_lookup_mem(mt, nt, av, lenq, aq, at, srev, tspan);
                if (hit) key = Tile::make_key(aq, at);
            }
        }
        chain_commit(st, lane, hit, key, srev, tspan, n, nrev, nfwd);
    };
    if (q_in_regs && t_in_lds) {
        // four batches of 64 lookups at a time: their probe chains are independent, so the four LDS reads of a step (and the
        // four fetches of the hits' records) are in flight together -- one batch at a time a wave spent ~1 700 cycles per batch
        // on dependent LDS / memory latency (FSV_CHAIN_STAMPS)
#pragma unroll
        for (int u0 = 0; u0 < QR; u0 += 4) {
            if (u0 * 64 < nq) {
                int l[4], h[4];
                uint64_t ah[4];
                bool val[4];
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const uint4 av = qa[u0 + j];
                    val[j] = (u0 + j) * 64 + lane < nq;
                    ah[j] = (uint64_t)av.x | (uint64_t)av.y << 32;
                    const uint32_t b = av.y >> 26;
                    l[j] = val[j] ? (int)s_bk[b] : 0; h[j] = val[j] ? (int)s_bk[b + 1] : 0;
                }
                for (;;) {
                    bool more = false;
                    uint64_t v[4];
                    int mid[4];
#pragma unroll
                    for (int j = 0; j < 4; j++) { mid[j] = (l[j] + h[j]) >> 1; v[j] = s_th[mid[j]]; }   // (mid <= nt <= AMAX: inside the tile)
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const bool act = l[j] < h[j], lt = v[j] < ah[j];
                        l[j] = act && lt ? mid[j] + 1 : l[j]; h[j] = act && !lt ? mid[j] : h[j];
                        more |= act;
                    }
                    if (!__any(more)) break;
                }
                uint64_t c[4];
#pragma unroll
                for (int j = 0; j < 4; j++) c[j] = s_th[l[j]];
                // (an array of structs, not three arrays: as arrays the compiler keeps hit and w in one vector register group each, and
                // writing a fetched record into its element makes every fetch wait for its data before the next is issued)
                struct { uint32_t z, w; bool hit; } tr[4];   // the target's position; strand | span << 8
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    tr[j].z = 0; tr[j].w = 0;
                    tr[j].hit = val[j] && l[j] < nt && c[j] == ah[j];
                    if (SHORT) { if (tr[j].hit) { const uint2 b = *reinterpret_cast<const uint2 *>(reinterpret_cast<const char *>(mt4 + l[j]) + 8); tr[j].z = b.x; tr[j].w = b.y; } }
                    else if (tr[j].hit) { const uint32_t tp = s_tp[l[j]]; tr[j].z = tp & 0x7fffffu; tr[j].w = (tp >> 31) | ((tp >> 23) & 0xffu) << 8; }
                }
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if ((u0 + j) * 64 < nq) {
                        const uint4 av = qa[u0 + j];
                        const uint32_t srev = (av.w & 0xffu) ^ (tr[j].w & 0xffu);
                        chain_commit(st, lane, tr[j].hit, Tile::make_key(chain_anchor_q(av, srev, lenq), tr[j].z), tr[j].hit ? srev : 0u, (tr[j].w >> 8) & 0xffu, n, nrev, nfwd);
                    }
            }
        }
    } else
        for (int base = 0; base < nq; base += 64) { const int i = base + lane; lookup(i, i < nq ? mq4[i] : make_uint4(0, 0, 0, 0)); }
    if (n > AMAX) {
        if (A.spill_list) { if (lane == 0) A.spill_list[atomicAdd(A.n_spill, 1u)] = P.pt; return; }   // (no slot written: k_chain_spill writes them)
        if (lane == 0) atomicOr(&A.warn[P.pt.x + (P.pt.y & 0xffffu)], (uint32_t)FSV_W_ANCHOR_TRUNC);
        n = AMAX;
    }
    __syncthreads();
    clk.mark(A.stamps, lane, 1);
    chain_core(A, st, P, n, nrev, nfwd, lane, clk);
}

__device__ __forceinline__ void chain_load_query(uint4 (&qa)[FSV_CHAIN_QR], const fsv_mz *mq, int nq)
{
    const uint4 *mq4 = (const uint4 *)mq;
    int lane = threadIdx.x;
    asm volatile("" : "+v"(lane));   // (see chain_pair)
    if (nq <= 64 * FSV_CHAIN_QR) {
#pragma unroll
        for (int u = 0; u < FSV_CHAIN_QR; u++) { const int i = u * 64 + lane; qa[u] = i < nq ? mq4[i] : make_uint4(0, 0, 0, 0); }
    }
}

// one block per listed pair (the re-chaining of a few pairs with another band width)
template <bool SHORT>
__global__ __launch_bounds__(64) void k_chain(ChainArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    if (A.pair_list && A.n_list_dev && blockIdx.x >= *A.n_list_dev) return;
    const ChainPair P = chain_pair_of(A, A.upair_tab[A.pair_list ? A.pair_list[blockIdx.x] : blockIdx.x]);
    if (A.wide_list && min(P.nq, P.nt) > A.amax) {
        if (threadIdx.x == 0) A.wide_list[atomicAdd(A.n_wide, 1u)] = A.pair_list ? A.pair_list[blockIdx.x] : blockIdx.x;
        return;
    }
    uint4 qa[FSV_CHAIN_QR];
    chain_load_query(qa, P.mq, P.nq);
    chain_pair<SHORT>(A, s_raw, P, qa);
}

// the pairs set aside by the kernels above (long reads: more than 1 024 minimizers in both lists), with the large tile; a small
// fixed grid walks the list, which is empty for reads below ~25 kb
template <bool SHORT>
__global__ __launch_bounds__(64) void k_chain_wide_list(ChainArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    const uint32_t n = *A.n_wide;
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        const ChainPair P = chain_pair_of(A, A.upair_tab[A.wide_list[i]]);
        uint4 qa[FSV_CHAIN_QR];
        chain_load_query(qa, P.mq, P.nq);
        chain_pair<SHORT>(A, s_raw, P, qa);
        __syncthreads();
    }
}

// The full pass: one block per FSV_CHAIN_CH consecutive pairs of the pair table (row-major: the pairs of a chunk nearly always
// share their query).  A block per pair paid three dependent memory round trips before its first lookup (pair record -> lengths /
// counts / offsets -> the two lists: two thirds of the kernel's wave cycles, FSV_CHAIN_STAMPS); here the chunk's records and
// its targets' lengths, counts and offsets arrive in two trips for all its pairs, and a pair waits for one round trip -- the two
// lists.  (One block per whole row was slower: rows have 0 .. ns-1 pairs.)
#define FSV_CHAIN_CH 8
template <bool SHORT>
__global__ __launch_bounds__(64) void k_chain_chunks(ChainArgs A, uint32_t n_upairs)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    const int lane = threadIdx.x;
    uint32_t chunk;
    if (!xcd_block((n_upairs + FSV_CHAIN_CH - 1) / FSV_CHAIN_CH, chunk)) return;
    const uint32_t first = chunk * FSV_CHAIN_CH;
    const int np = (int)min((uint32_t)FSV_CHAIN_CH, n_upairs - first);
    uint4 ptv = make_uint4(0, 0, 0, 0);
    int lent_v = 0, nt_v = 0;
    uint32_t offt_v = 0;
    if (lane < np) {
        ptv = A.upair_tab[first + lane];
        const uint32_t rt = ptv.x + (ptv.y >> 16);
        lent_v = A.read_len[rt]; nt_v = (int)A.mz_cnt[rt]; offt_v = A.mz_off[rt];
    }
    // q's list stays in registers while the query does not change (half the list traffic; FSV_CHAIN_QR keeps the kernel at three
    // waves per SIMD with it)
    uint32_t cur_rq = 0xffffffffu;
    int lenq = 0, nq = 0;
    uint32_t offq = 0;
    uint4 qa[FSV_CHAIN_QR];
#pragma nounroll
    for (int i = 0; i < np; i++) {
        // readlane: the pair's values are wave-uniform and must live in scalar registers
#define RL(v_) ((uint32_t)__builtin_amdgcn_readlane((int)(v_), i))
        const uint4 pt = make_uint4(RL(ptv.x), RL(ptv.y), RL(ptv.z), RL(ptv.w));
        const int lent = (int)RL(lent_v), nt = (int)RL(nt_v);
        const uint32_t offt = RL(offt_v);
#undef RL
        const uint32_t rq = pt.x + (pt.y & 0xffffu);
        if (rq != cur_rq) {
            cur_rq = rq;
            lenq = __builtin_amdgcn_readfirstlane(A.read_len[rq]); nq = __builtin_amdgcn_readfirstlane((int)A.mz_cnt[rq]);
            offq = (uint32_t)__builtin_amdgcn_readfirstlane((int)A.mz_off[rq]);
            chain_load_query(qa, A.mz + offq + nq, nq);   // the position-sorted copy
        }
        if (A.wide_list && min(nq, nt) > A.amax) {     // only such a pair can have more anchors than this tile holds
            if (lane == 0) A.wide_list[atomicAdd(A.n_wide, 1u)] = first + (uint32_t)i;
            continue;
        }
        const ChainPair P = {pt, lenq, lent, nq, nt, A.mz + offq + nq, A.mz + offt};
        chain_pair<SHORT>(A, s_raw, P, qa);
        __syncthreads();   // the next pair reuses the tile
    }
}

// ------------------------------------------------------------------------------------------------ k_chain_spill (full_lists = 1)
// The pairs chain_pair set aside because their anchors exceed its LDS tile: a small fixed grid walks A.spill_list, one wavefront per pair,
// with the per-anchor arrays in the block's slab in HBM (ChainSlab; cap anchors: the host sizes it from the batch's longest minimizer
// slot, and a pair has at most min(nq, nt) anchors), which stays in L2.  Step 1 here is a plain binary search of the target's list in
// memory per query minimizer; the rest is chain_core.
#define FSV_SPILL_GRID 32
__device__ __forceinline__ void chain_pair_spill(const ChainArgs &A, const uint4 pt, unsigned char *slab, const uint32_t cap)
{
    const ChainSlab st(slab, cap);
    const ChainPair P = chain_pair_of(A, pt);
    const int lane = threadIdx.x;
    const uint4 *mq4 = (const uint4 *)P.mq;
    ChainSlab::Clock clk(false);
    int n = 0, nrev = 0, nfwd = 0;
    for (int base = 0; base < P.nq; base += 64) {
        const int i = base + lane;
        bool hit = false; uint32_t aq = 0, at = 0, srev = 0, tspan = 0;
        if (i < P.nq) hit = chain_lookup_mem(P.mt, P.nt, mq4[i], P.lenq, aq, at, srev, tspan);
        chain_commit(st, lane, hit, ChainSlab::make_key(aq, at), srev, tspan, n, nrev, nfwd);
    }
    if (n > st.cap) { if (lane == 0) atomicOr(&A.warn[pt.x + (pt.y & 0xffffu)], (uint32_t)FSV_W_INTERNAL); n = st.cap; }   // cannot happen: n <= min(nq, nt) <= a slot
    __syncthreads();
    chain_core(A, st, P, n, nrev, nfwd, lane, clk);
}

__global__ __launch_bounds__(64) void k_chain_spill(ChainArgs A, unsigned char *slab, uint32_t cap, uint32_t *spilled)
{
    const uint32_t n = *A.n_spill;
    if (blockIdx.x == 0 && threadIdx.x == 0 && n) atomicAdd(spilled, n);   // statistics: pairs chained here, summed over the pass's launches
    unsigned char *const mine = slab + (size_t)blockIdx.x * cap * FSV_SPILL_BYTES;
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        chain_pair_spill(A, A.spill_list[i], mine, cap);
        __threadfence_block();
        __syncthreads();   // the next pair reuses the slab
    }
}

// LDS bytes of a k_chain block
__host__ __device__ inline size_t chain_lds_bytes(bool short_reads, int amax) { return short_reads ? (size_t)amax * 12 + (size_t)amax / 8 : (size_t)amax * 24; }

} // namespace
