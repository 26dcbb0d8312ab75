// asm_kernels.h -- device kernels of the per-read-set assembly (gfx950).  Included by asm.hip; the sketch kernels, which the
// aligner shares, are in k_sketch.h, the consensus family (k_consensus ... the second pass) in k_consensus.h.
//
// Stage map (reference = hifiasm-0.14 under software/, restated in oracle/asm.c which these kernels
// must match bit for bit):
//   k_sketch          ha_sketch                                  sketch.cpp:39-137
//   k_uniq            per-read index (hash occurs once)          htab.cpp:917-998 restated
//   k_chain           anchors, chain_DP, extension, window list  anchor.cpp:60-178; Hash_Table.cpp:425-616, 83-243; Correct.cpp:306-531
//   k5 (bpm_device.h) Reserve_Banded_BPM                         Levenshtein_distance.h:274-461
//   k_rescue_accept   recalcate_window_advance (right pass), 0.9 / 0.03 filters   Correct.cpp:2629-3023, 725
//   k_path_fast/_dp   try_cigar, Reserve_Banded_BPM_PATH, generate_cigar          Levenshtein_distance.h:465-888; Correct.cpp:1302-1536
//   k_consensus       window_consensus / get_seq_from_Graph as a column vote       Correct.cpp:4010-4195
//   k_newlen/k_repack worker_ec_save (+ reverse complement)      Assembly.cpp:706-767
//   k_exact           if_exact_match                             Assembly.cpp:894-974
//   k_stitch          ma_ug_seq                                  Overlaps.cpp:8969-9034
#pragma once
#include "bpm_device.h"
#include "k_sketch.h"
#include <type_traits>

#define FSV_AMAX       1024  // anchors per read pair held in LDS
#define FSV_AMAX_WIDE_LONG 2560  // ... the same second pass in the long layout (24 B per anchor: 60 KB, a workgroup's LDS limit without opting in to more)
#define FSV_AMAX_WIDE  4096  // ... for ONT-profile batches: k = 15 minimizers every ~8 bases, corrected reads share all of them (a 25 kb overlap: ~3 000)
#define FSV_PATH_CAP    416  // ops per window path: x_len (<= 375) + y-only ops (<= k <= 31)
#define FSV_CW_STRIDE   448  // bytes reserved per corrected grid window
#define FSV_INS_MAXLEN   12
#define FSV_SB_MAXERR    7   // k_path_sb: distances it holds in one word per column (2 x 7 + 1 rows x 2 bits)
#define FSV_SB_QUADS ((FSV_WINDOW + 3) / 4)
#define FSV_FR_MAXERR    3   // k_path_fr: distances it walks without the DP matrix
#define FSV_EV_CAP_WIDE 2048 // ... for ONT-profile batches (wide bands): ~25 inserted-base events per overlap and window
#define FSV_EV_CAP     256   // insertion events per grid window in LDS (overlaps x indel rate x 375 x 2 -- HiFi at 30x: a few dozen, 48 reads at 1.2 % indels: 462; more sets
                             // the read's warning bit 8 and drops the excess, or with deep_sets = 1 sends the window to k_consensus_deep)

// fsv_wpath (include/focalsv_hip.h): 128 bytes per window task; state 2 = queued for the DP kernel (internal)
static_assert(sizeof(fsv_wpath) == 128, "fsv_wpath layout");

namespace { // (every translation unit that includes this header gets its own copy of the kernels)

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

// Phase stamps of a diagnostic run: shader cycles since the last mark (or restart) added to stamps[phase] and one to stamps[8 + phase],
// by the wave's lane 0.  FSV_CHAIN_STAMPS=1: the tile kernels, one block in 64 (the atomics must not become the load; the slab's clock
// is empty); FSV_K6_STAMPS=1: k_path_sb<true> and k_path_fr<E, true>, every block.  PhaseClock<false> is empty: no stamp code at all.
template <bool ON> struct PhaseClock {
    bool on; unsigned long long tm;
    __device__ __forceinline__ explicit PhaseClock(const bool sample) : on(sample), tm(0ull) { restart(); }
    __device__ __forceinline__ void restart() { if (on) tm = __builtin_amdgcn_s_memtime(); }
    __device__ __forceinline__ void mark(unsigned long long *stamps, const int lane, const int i)
    {
        if (on) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); if (lane == 0) { atomicAdd(&stamps[i], t_ - tm); atomicAdd(&stamps[8 + i], 1ull); } tm = t_; }
    }
};
template <> struct PhaseClock<false> {
    __device__ __forceinline__ explicit PhaseClock(bool) {}
    __device__ __forceinline__ void restart() {}
    __device__ __forceinline__ void mark(unsigned long long *, int, int) {}
};

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

// ------------------------------------------------------------------------------------------------ k_rescue_accept
// One lane per overlap slot: right-extension rescue of unmatched windows (Correct.cpp:2655-2744),
// then the 0.9 coverage filter and the 0.03 error-rate filter (Correct.cpp:2899-3021, 725).
__device__ __forceinline__ int double_thr(int pre, int x_len, int k_cap)
{
    if (pre == 0 && x_len >= 4) pre = 1;
    int t = pre * 2;
    if (x_len >= 300 && t < k_cap) t = k_cap;
    if (t > k_cap) t = k_cap;
    return t;
}

// WIDE: the batch's error model allows thresholds above 31 (k_cap up to 95): the re-runs go through the wide-band BPM
// DEFER (fsv_asm_params.partial_charge): the error-rate test is left to k_charge_tasks / k_charge_accept, which need the windows' paths
// first -- an overlap that passes the 0.9 coverage filter gets is_match = 1 for K6's sake (k_path_fast gates on it) while its accepted
// bit in ovl_c stays clear; nothing but K6 runs between this verdict and the final one
template <bool WIDE, bool DEFER = false>
__global__ __launch_bounds__(64) void k_rescue_accept(const uint32_t *__restrict__ store, fsv_ovl *__restrict__ ovl, uint32_t n_pairs,
                                                      fsv_wtask *__restrict__ tasks, fsv_wres *__restrict__ res,
                                                      unsigned long long *__restrict__ stat_cols, uint4 *__restrict__ ovl_c, int k_cap, int accept_err_pm,
                                                      uint32_t *__restrict__ left_list, uint32_t *__restrict__ n_left)
{
    const uint32_t p = blockIdx.x * 64 + threadIdx.x;
    if (p >= n_pairs) return;
    fsv_ovl o = ovl[p];
    // ovl_c: what the consensus needs of an overlap, 16 B instead of 56: {x_s, first window task, n_win | accepted << 31, -}
    if (!o.valid) { ovl_c[p] = make_uint4(0u, 0u, 0u, 0u); return; }
    fsv_wtask *T = tasks + o.first_win;
    fsv_wres *R = res + o.first_win;
    int align = 0;
    unsigned long long cols = 0;
    // one pass settles an overlap whose windows all matched (nearly all of them): aligned length, total length and error sum;
    // four windows per trip so that their loads are in flight together (a lane walks ~20 windows, a memory round trip each)
    int n_bad = 0;
    long long tlen0 = 0, terr0 = 0;
#pragma unroll 4
    for (int j = 0; j < o.n_win; j++) {
        const int e = R[j].err, xl = T[j].x_len;
        if (e >= 0) { align += xl; terr0 += e; } else n_bad++;
        tlen0 += xl;
    }
    for (int j = n_bad ? o.n_win - 1 : -1; j >= 0; j--) {
        if (R[j].err < 0) continue;
        int next = R[j].y_beg + R[j].end_site - R[j].extra_begin + 1;
        for (int k2 = j + 1; k2 < o.n_win && R[k2].err < 0; k2++) {
            fsv_wtask u = T[k2];
            if (next >= u.y_len) break;
            u.k = (uint8_t)double_thr(u.k, u.x_len, k_cap);
            u.y_start = next;
            fsv_wres r;
            if (!bpm_window_geometry(u, r, k_cap)) break;
            if ((u.x_len + 2 * u.k - r.extra_begin - r.extra_end) + u.k < u.x_len) break;
            if (WIDE) { WideNoSink none; bpm_run_wide(store, u, r, none, k_cap); }
            else bpm_run(store, u, r, BpmNoSink());
            cols += u.x_len;
            if (r.err < 0) break;
            T[k2] = u; R[k2] = r;
            align += u.x_len;
            next = r.y_beg + r.end_site - r.extra_begin + 1;
        }
    }
    if (n_bad && left_list) {
        // an unmatched window left of a matched one: the left-extension pass (k_left_rescue) decides about this overlap
        bool left = false;
        for (int j = 1; j < o.n_win && !left; j++) left = R[j].err >= 0 && R[j - 1].err < 0;
        if (left) {
            left_list[atomicAdd(n_left, 1u)] = p;
            o.is_match = 0; ovl[p] = o;
            ovl_c[p] = make_uint4((uint32_t)o.x_s, (uint32_t)o.first_win, (uint32_t)o.n_win, 0u);
            if (cols) atomicAdd(stat_cols, cols);
            return;
        }
    }
    long long tlen = tlen0, terr = terr0;
    if (n_bad) {   // the rescue may have changed results and window lengths never change: only the error sum is taken again
        terr = 0;
#pragma unroll 4
        for (int j = 0; j < o.n_win; j++) { const int e = R[j].err; terr += e >= 0 ? e : T[j].x_len; }
    }
    o.align_len = align; o.err_sum = (int32_t)terr;
    // DEFER: the 0.9 filter alone, and the accepted bit of ovl_c stays clear until k_charge_tasks / k_charge_accept have spoken
    const bool covered = (long long)(o.x_e - o.x_s + 1) * 9 <= (long long)align * 10;
    o.is_match = (covered && (DEFER || terr * 1000 <= tlen * accept_err_pm)) ? 1 : 0;
    ovl[p] = o;
    ovl_c[p] = make_uint4((uint32_t)o.x_s, (uint32_t)o.first_win, (uint32_t)o.n_win | (o.is_match && !DEFER ? 0x80000000u : 0u), 0u);
    if (cols) atomicAdd(stat_cols, cols);
}

// ------------------------------------------------------------------------------------------------ K6 paths
// Fast paths of Reserve_Banded_BPM_PATH (Levenshtein_distance.h:516-531): err == 0, or a gap-free placement with
// exactly err mismatches (try_cigar).  Everything else is queued for one of the walk kernels.
struct PathLists {      // task lists and their device-side lengths: 0-2 k_path_fr<1..3>, 3 k_path_sb, 4 k_path_dp<32>, 5 k_path_dp<64>, 6 k_path_wide,
    uint32_t *list[8], *cnt[8];   // 7 (may be null): windows whose alignment may touch the edge of its band (k_fix_boundary looks at them again)
};
// The record of a window's path, for the gap-free placement (path_gapfree) and for the walked paths (path_finish): the y interval
// [start, end] in padded-window columns, the distance after generate_cigar and plen ops, of which word(wd) gives the wd-th sixteen,
// start-to-end.  pad: bit 0 = an op other than a match among the first ten, bit 1 = among the last ten (tail10: those fields) -- what
// scan_cigar (Correct.cpp:1070) over ten columns from either end asks about (calculate_boundary_cigars :2360; k_bcig_tasks reads the
// header only); bit 2 = raw0: the alignment started in the padded window's first column before generate_cigar moved it (fix_boundary's
// question).  with_ops false (path_gapfree, distance 0: every op a match): the record carries no ops -- its consumers (k_consensus,
// k_het) look at err first and never read them, and in the later correction rounds nearly every window is one: 24 bytes out instead of 128.
template <class Words>
__device__ __forceinline__ void path_record(fsv_wpath *__restrict__ P, const fsv_wtask &t, int start, int end, int plen, int err, bool raw0, uint32_t tail10,
                                            bool with_ops, Words word)
{
    uint32_t head10 = 0;
    if (with_ops) {
        uint2 *dst = reinterpret_cast<uint2 *>(P->ops); // ops sit at byte 24 of the record: 8-byte aligned
        for (int i = 0; i < FSV_PATH_CAP / 32; i++) {
            const uint32_t v0 = word(2 * i), v1 = word(2 * i + 1);
            if (i == 0) head10 = v0 & 0xfffffu;
            dst[i] = make_uint2(v0, v1);
        }
    }
    P->ry_start = t.y_start - t.k + start;
    P->ry_end = t.y_start - t.k + end;
    P->path_len = (int16_t)plen; P->err = (int16_t)err; P->state = 1; P->y_rev = t.y_rev;
    P->pad = (uint16_t)((head10 ? 1u : 0u) | (tail10 ? 2u : 0u) | (raw0 ? 4u : 0u)); P->y_word = t.y_word; P->y_len = t.y_len;
}

// try_cigar (Levenshtein_distance.h:465-507): the gap-free placement on the end diagonal K5 reported.  When its mismatches are the
// window's distance that is the path (generate_cigar then only trims mismatches at the two ends into x-only ops): the record is
// written and true returned; false: the window needs a walk.  One lane per window, no cross-lane traffic.
__device__ __forceinline__ bool path_gapfree(const uint32_t *__restrict__ store, const fsv_wtask &t, const fsv_wres &r, fsv_wpath *__restrict__ P, bool write_clean_ops)
{
    const int n = t.x_len;
    const int start = r.end_site - n + 1;
    // mismatch map of the gap-free placement, 16 columns per word; field value 1 == op "mismatch"
    uint32_t ops32[26];
#pragma unroll
    for (int i = 0; i < 26; i++) ops32[i] = 0;
    bool ok = r.err == 0;
    if (!ok && start >= 0) {
        int mm = 0;
        const int win0 = t.y_start - t.k;
#pragma unroll
        for (int c = 0; c < 6; c++) {
            if (c * 64 < n) {
                uint32_t xb4[4], yb4[4], yv4[4];
                fetch64_x(store, t.x_word, t.x_start + c * 64, xb4);
                fetch64(store, t.y_word, t.y_len, t.y_rev, win0 + start + c * 64, yb4, yv4);
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int b = c * 4 + q;
                    if (b * 16 < n) {
                        uint32_t d = mismatch_fields16(xb4[q], yb4[q], yv4[q]);
                        // columns past the window do not count
                        const int lim = min(16, n - b * 16);
                        if (lim < 16) d &= (1u << (2 * lim)) - 1u;
                        ops32[b] = d;
                        mm += __popc(d);
                    }
                }
            }
        }
        ok = (mm == r.err);
    }
    if (!ok) return false;
    // gap-free path.  generate_cigar (Correct.cpp:1387-1536) turns mismatches at either end into x-only ops (3) and
    // moves the y interval inwards -- the alignment end first, then its start; there are no gaps to shift.
    int s2 = start, e2 = r.end_site;
    if (r.err > 0) {
        for (int i = n - 1; i >= 0 && ((ops32[i >> 4] >> ((i & 15) << 1)) & 3u) == 1u; i--) { ops32[i >> 4] |= 3u << ((i & 15) << 1); e2--; }
        for (int i = 0; i < n && ((ops32[i >> 4] >> ((i & 15) << 1)) & 3u) == 1u; i++) { ops32[i >> 4] |= 3u << ((i & 15) << 1); s2++; }
    }
    uint32_t tail10 = 0;
    if (r.err > 0) {
        const int a = max(n - 10, 0), wi = a >> 4, sh = (a & 15) << 1;
        const uint32_t lo = ops32[wi] >> sh, hi = (sh && wi + 1 < 26) ? ops32[wi + 1] << (32 - sh) : 0u;
        tail10 = (lo | hi) & 0xfffffu;
    }
    path_record(P, t, s2, e2, n, r.err, r.err > 0 && start == 0, tail10, r.err > 0 || write_clean_ops, [&](int wd) { return ops32[wd]; });
    return true;
}

__global__ __launch_bounds__(256) void k_path_fast(const uint32_t *__restrict__ store, const fsv_ovl *__restrict__ ovl,
                                                   const fsv_wtask *__restrict__ tasks, const fsv_wres *__restrict__ res, uint32_t n_tasks,
                                                   fsv_wpath *__restrict__ paths, PathLists L, bool write_clean_ops, const uint32_t *__restrict__ n_dev)
{
    if (n_dev) n_tasks = min(*n_dev, n_tasks);   // the grid covers the task bound; the count stays on the device (no host round trip), clamped to the bound
    uint32_t blk;
    if (!xcd_block((n_tasks + 255u) >> 8, blk)) return;
    const uint32_t tid = blk * blockDim.x + threadIdx.x;
    if (tid >= n_tasks) return;
    const fsv_wtask t = tasks[tid];
    const fsv_wres r = res[tid];
    fsv_wpath *P = paths + tid;
    if (r.err < 0 || !ovl[t.ovl].is_match) { P->state = 0; return; }
    const bool ok = path_gapfree(store, t, r, P, write_clean_ops);
    // fix_boundary's candidates, from what K5 knows: the alignment ends in the padded window's last column, or could start in its first
    // one (it starts at end - (n - 1) - (inserted - deleted bases), and the distance bounds that difference)
    if (L.cnt[7] && r.err > 0 && t.k <= FSV_K_MAX && (r.end_site == (int)t.x_len + 2 * (int)t.k - 1 || r.end_site - ((int)t.x_len - 1) <= r.err))
        L.list[7][atomicAdd(L.cnt[7], 1u)] = tid;
    // Not settled here: queued for one of the walk kernels, each list homogeneous -- first-pass bands (k <= 15) by distance: the walk
    // without the matrix up to 3 (nine in ten; a list per distance), the sub-band matrix up to 7, the general kernel beyond; the doubled thresholds of the
    // rescue pass (k <= 31); bands above 63 rows (k_path_wide).  One atomic instruction per wave: a class's first lane reserves its slots.
    {
        const int cls = ok ? -1 : (t.k <= FSV_K_MAX && r.err <= FSV_FR_MAXERR) ? r.err - 1 : t.k <= 15 ? (r.err <= FSV_SB_MAXERR ? 3 : 4) : t.k <= FSV_K_MAX ? 5 : 6;
        if (__any(cls >= 0)) {
            const int lane = (int)(threadIdx.x & 63u);
            unsigned long long mine = 0ull;
#pragma unroll
            for (int c = 0; c < 7; c++) {
                const unsigned long long m = __ballot(cls == c);
                if (cls == c) mine = m;
            }
            const int leader = mine ? __ffsll((long long)mine) - 1 : lane;      // the class's first lane reserves for all of them
            uint32_t base = 0, *cnt = L.cnt[0], *list = L.list[0];
#pragma unroll
            for (int c = 1; c < 7; c++) { cnt = cls == c ? L.cnt[c] : cnt; list = cls == c ? L.list[c] : list; }
            if (cls >= 0 && lane == leader) base = atomicAdd(cnt, (uint32_t)__popcll(mine));
            const uint32_t at = __shfl(base, leader, 64) + (uint32_t)__popcll(mine & ((1ull << lane) - 1ull));
            if (cls >= 0) { P->state = 2; list[at] = tid; }
        }
    }
}

// One lane's walk back through the DP (Levenshtein_distance.h:757-888) as every K6 kernel records it: the path in the lane's column of
// the block's LDS array s_ops[28][64] -- 2 bits per op (0 diagonal over a match, 1 diagonal over a mismatch, 2 up, 3 left), stored
// end-to-start, 448 ops -- and where the walk stands: the ops so far, the y column of the padded window the alignment would start in if
// the rest were matches, the x column, the errors left, the band row (absolute, or relative to the rows a kernel keeps), the last op.
// The ops are gathered in a register that goes to LDS once per 16 steps.
struct PathWalk {
    static constexpr int WORDS = 28, CAP = WORDS * 16;
    uint32_t (*ops)[64]; int lane;
    int plen, start, ci, cur, row, dir;
    uint32_t acc;
    __device__ __forceinline__ PathWalk(uint32_t (*s_ops)[64], int lane64) : ops(s_ops), lane(lane64) {}
    // a window of n columns whose alignment ends in window column `end` on band row `row_` with distance `err`
    __device__ __forceinline__ void clear(int n, int end, int err, int row_)
    {
        for (int i = 0; i < WORDS; i++) ops[i][lane] = 0;
        plen = 0; start = end; ci = n - 1; cur = err; row = row_; dir = 0; acc = 0;
    }
    // one step: the op is recorded and the walk moves -- "up" stays in its column, "left" keeps its y base, every op but a match spends an error
    __device__ __forceinline__ void put(uint32_t code)
    {
        acc |= code << ((plen & 15) << 1);
        if ((plen & 15) == 15) { ops[plen >> 4][lane] = acc; acc = 0; }
        plen++;
        cur -= (int)(code != 0u);
        start -= (int)(code != 3u);
        row += (int)(code == 3u) - (int)(code == 2u);
        ci -= (int)(code != 2u);
        dir = (int)code;
    }
    // a run of matches: the fields are already 0, a word that fills up with them goes out
    __device__ __forceinline__ void matches(int steps)
    {
        const int np = plen + steps;
        if ((np >> 4) != (plen >> 4)) { ops[plen >> 4][lane] = acc; acc = 0; }
        plen = np; start -= steps; ci -= steps; dir = 0;
    }
    __device__ __forceinline__ void flush() { if (plen & 15) ops[plen >> 4][lane] = acc; }
    // the recorded path, for generate_cigar: op i (0 = the alignment's last), a word of 16 of them
    __device__ __forceinline__ uint32_t word(int wi) const { return ops[wi][lane]; }
    __device__ __forceinline__ uint32_t get(int i) const { return (ops[i >> 4][lane] >> ((i & 15) << 1)) & 3u; }
    __device__ __forceinline__ void set(int i, uint32_t v)
    {
        const int wi = i >> 4, sh = (i & 15) << 1;
        ops[wi][lane] = (ops[wi][lane] & ~(3u << sh)) | (v << sh);
    }
};

// The end of K6, shared by all the walks: the all-match rest of the walk, generate_cigar's end trimming and greedy gap left-shift
// (Correct.cpp:1302-1536) on the path in LDS, and the record.
__device__ __forceinline__ void path_finish(const uint32_t *__restrict__ store, const fsv_wtask &t, fsv_wpath *__restrict__ P, PathWalk &w, int end, int err)
{
    int plen = w.plen, start = w.start, dir = w.dir;
    const int col = w.ci + 1;
    if (col > 0) { start -= col; plen += col; dir = 0; } // the rest of the path is matches: the fields are already 0
    // a record holds FSV_PATH_CAP ops (x_len + k <= 406 for hifiasm's thresholds: never reached); a longer path -- a wide-band
    // window with more than 41 inserted bases -- leaves the window without a path, as oracle/asm.c:window_path does
    if (plen > FSV_PATH_CAP) { P->state = 0; return; }
    if (dir != 3) start++;
    const bool raw0 = err > 0 && start == 0;      // before generate_cigar moves the start
    // generate_cigar: the path is stored end-to-start
    if (err > 0) {
        int stop = -1;
        for (int i = 0; i < plen && w.get(i) == 1; i++) { w.set(i, 3); end--; stop = i; }
        for (int i = plen - 1; i >= 0 && w.get(i) == 1; i--) { w.set(i, 3); start++; }
        int xi = 0, yi = 0;
        BaseCache xc, yc;
        for (int i = plen - 1; i > stop;) {
            // runs of match / mismatch ops are skipped a path word at a time: a gap op is a field with its high bit set
            const int f = i & 15;
            const uint32_t wv = w.word(i >> 4);
            const uint32_t m = wv & 0xAAAAAAAAu & (f == 15 ? 0xffffffffu : ((1u << (2 * f + 2)) - 1u));
            const int skip = min(m == 0u ? f + 1 : f - ((31 - __clz(m)) >> 1), i - stop);
            if (skip > 0) { xi += skip; yi += skip; i -= skip; continue; }
            const uint32_t op = (wv >> (2 * f)) & 3u;
            // shift this gap towards the alignment start while the bases it passes still pair up (move_gap_greedy)
            int pi = i + 1, x2 = xi, y2 = yi;
            if (op == 3) y2--; else x2--;
            for (; pi < plen && x2 >= 0 && y2 >= 0; pi++, x2--, y2--) {
                const uint32_t pv = w.get(pi);
                // the shift reads bases at falling positions: one 16-base word per 16 steps instead of two dependent global loads
                // per step (a gap inside a homopolymer travels a long way, and the whole wave waits for its slowest lane)
                const bool same = xc.get(store, t.x_word, t.x_start + x2) == yc.ycol(store, t, start + y2);
                if (pv >= 2 || (pv == 0 && !same)) break;
                if (pv == 1 && same) { w.set(pi - 1, 0); err--; }
                else w.set(pi - 1, pv);
                w.set(pi, op);
            }
            if (op == 2) yi++; else xi++;
            i--;
        }
    }
    // the record holds the ops start-to-end: its word wd is the path's fields plen-16-16wd .. plen-1-16wd in reverse order
    auto packed = [&](int wd) -> uint32_t {
        const int a = plen - 16 - 16 * wd;
        uint32_t v = 0;
        if (a >= 0) {
            const int wi = a >> 4, sh = (a & 15) << 1;
            const uint32_t w0 = w.word(wi), w1 = (sh && wi + 1 < PathWalk::WORDS) ? w.word(wi + 1) : 0u;
            v = sh ? (w0 >> sh) | (w1 << (32 - sh)) : w0;
        } else if (a > -16) v = w.word(0) << ((-a) << 1);
        return rev_fields2(v);
    };
    path_record(P, t, start, end, plen, err, raw0, w.word(0) & 0xfffffu, true, packed);
}

// General K6 (any band up to 63 rows, any distance): forward pass keeping {D0, VP, VN} of every column in a per-lane scratch, the
// reference's walk back on those words, then path_finish.  Since round 2
// this is the fallback: first-pass windows (k <= 15) at distance <= FSV_SB_MAXERR go through k_path_sb below, which keeps
// 4 bytes per column instead of 12 and walks without a dependent global load per step; what is left for this kernel are
// the doubled-threshold rescue windows (k > 15) and distances above 7 -- a fraction of a percent of the HiFi windows.
// WordT = uint32_t for bands of at most 31 diagonals (k <= 15): the walk back only looks at bits below the band width, so the
// low halves of D0 / VP / VN are all it needs and the scratch traffic halves; uint64_t for the doubled thresholds (k <= 31).
// LANES: the lanes that share the scratch -- 64: a block's slice in HBM, [column][word][lane] (k_path_dp); 1: one lane's columns in LDS
// (k_fix_boundary, k_left_rescue)
template <class WordT, int LANES> struct PathSink {
    WordT *cols; uint32_t lane;
    __device__ __forceinline__ WordT &at(int c, int w) const { return cols[((size_t)c * 3 + w) * LANES + lane]; }
    __device__ __forceinline__ void operator()(int i, uint64_t d0, uint64_t vp, uint64_t vn) const
    {
        at(i + 1, 0) = (WordT)d0; at(i + 1, 1) = (WordT)vp; at(i + 1, 2) = (WordT)vn;
    }
};

// Reserve_Banded_BPM_PATH by one lane for one window: the forward pass with every column's {D0, VP, VN} kept in the lane's scratch, the
// walk back, generate_cigar and the record (path_finish).  The general K6 kernel's body; fix_boundary and k_left_rescue call it too.
template <class WordT, int LANES>
__device__ __forceinline__ void path_general(const uint32_t *__restrict__ store, const fsv_wtask &t, fsv_wpath *__restrict__ P, uint32_t (*s_ops)[64],
                                             int lane64, WordT *cols_slice)
{
    const int n = t.x_len, k = t.k, band = 2 * k + 1;
    fsv_wres r;
    const PathSink<WordT, LANES> sink{cols_slice, LANES == 1 ? 0u : (uint32_t)lane64};
    bpm_run(store, t, r, sink);
    if (r.err < 0) { P->state = 0; return; } // cannot happen: K5 matched this window
    PathWalk w(s_ops, lane64);
    w.clear(n, r.end_site, r.err, band - (n + 2 * k - r.end_site));
    // the kernel is instruction-bound (4-5 waves per SIMD keep the issue slots full), so the walk is written for few
    // instructions: WordT-wide bit tests (only band bits are read) and the column it leaves behind handed to the next step
    // instead of re-read (scratch column c + 1 holds x column c)
    WordT vp = sink.at(n, 1), vn = sink.at(n, 2);
    while (w.ci >= 0 && w.cur != 0) {
        const int row = w.row, cur = w.cur;
        const WordT d0 = sink.at(w.ci + 1, 0);
        const WordT vpi = w.ci > 0 ? sink.at(w.ci, 1) : (WordT)0, vni = w.ci > 0 ? sink.at(w.ci, 2) : (WordT)0;
        const WordT hn = vpi & d0, hp = vni | ~(vpi | d0);
        const int diag = cur - (int)((~(d0 >> row)) & 1u);
        const bool can_up = row != 0, can_left = row == 0 || row != band - 1;
        int left = cur, up = cur;
        if (can_left) left = cur - (int)((hp >> row) & 1u) + (int)((hn >> row) & 1u);
        if (can_up) up = cur - (int)((vp >> (row - 1)) & 1u) + (int)((vn >> (row - 1)) & 1u);
        // ties: diagonal, then up, then left; a neighbour that is cheaper is so by exactly one
        int best = diag;
        uint32_t code = diag != cur ? 1u : 0u;
        if (can_up && up < best) { best = up; code = 2u; }
        if (can_left && left < best) code = 3u;
        if (code != 2u) { vp = vpi; vn = vni; }
        w.put(code);
    }
    w.flush();
    path_finish(store, t, P, w, r.end_site, r.err);
}

template <class WordT>
__global__ __launch_bounds__(64) void k_path_dp(const uint32_t *__restrict__ store, const fsv_wtask *__restrict__ tasks,
                                                const uint32_t *__restrict__ dp_list, const uint32_t *__restrict__ n_dev,
                                                fsv_wpath *__restrict__ paths, WordT *__restrict__ cols)
{
    __shared__ uint32_t s_ops[PathWalk::WORDS][64];
    const int lane64 = threadIdx.x;
    const uint32_t n_list = *n_dev;     // the list's length as the kernel before left it: no host round trip
    // persistent blocks: the grid is sized to what the device holds at once and every block strides through the list, so the
    // scratch is a few hundred MB whatever the number of windows, and the whole list is one launch; a block's slice of the scratch is
    // reused for every task it takes
    for (uint32_t li = blockIdx.x * 64 + threadIdx.x; li < n_list; li += gridDim.x * 64) {
        const uint32_t tid = dp_list[li];
        const fsv_wtask t = tasks[tid];
        path_general<WordT, 64>(store, t, paths + tid, s_ops, lane64, cols + (size_t)blockIdx.x * (FSV_WINDOW + 2) * 3 * 64);
    }
}

// ------------------------------------------------------------------------------------------------ fix_boundary
// fix_boundary (Correct.cpp:1676-1795; for the windows' final cigars :2968 and in the left-extension pass :2858): an alignment that
// starts in the first column of its padded window, or ends in its last one, may have been cut off by the band -- the window is aligned
// once more with the band shifted by k towards that side (from the old region's first base / so that the x interval ends at the old
// alignment's last base), without a hint, and the new alignment stands when it has fewer errors.  t / r / the record at P: the window
// as K6 left it; they are replaced when the new alignment stands.  One lane, its column scratch `cols` in LDS.
// oracle/asm.c:window_path is the same, statement for statement.
__device__ __forceinline__ void fix_boundary_dev(const uint32_t *__restrict__ store, fsv_wtask &t, fsv_wres &r, fsv_wpath *__restrict__ P, uint32_t (*s_ops)[64],
                                                 uint64_t *cols, int k_cap)
{
    const uint4 h = *reinterpret_cast<const uint4 *>(P);
    if ((h.w & 0xffu) != 1u || r.err <= 0 || t.k > FSV_K_MAX || (r.extra_begin & 0x4000)) return;     // (bit 14 of extra_begin: moved once already)
    const int n = t.x_len, k = t.k, wlen = n + 2 * k;
    const bool raw0 = ((h.w >> 16) & 4u) != 0u;
    fsv_wtask t2 = t;
    if (raw0) { if (r.extra_begin != 0) return; t2.y_start = r.y_beg; }
    else if (r.end_site == wlen - 1) { if (r.extra_end != 0) return; t2.y_start = (r.y_beg + r.end_site) - n + 1; }
    else return;
    fsv_wres r2;
    if (!bpm_window_geometry(t2, r2, k_cap)) return;
    if (r2.y_beg == r.y_beg) return;
    bpm_run(store, t2, r2, BpmNoSink());
    if (r2.err < 0 || r2.err >= r.err) return;
    path_general<uint64_t, 1>(store, t2, P, s_ops, 0, cols);
    r2.extra_begin = (int16_t)(r2.extra_begin | 0x4000);
    t = t2; r = r2;
}

// the candidates k_path_fast listed, one block (one working lane, LDS scratch: see k_left_rescue) each
__global__ __launch_bounds__(64) void k_fix_boundary(const uint32_t *__restrict__ store, const uint32_t *__restrict__ list, const uint32_t *__restrict__ n_list_dev,
                                                     fsv_wtask *__restrict__ tasks, fsv_wres *__restrict__ res, fsv_wpath *__restrict__ paths, int k_cap,
                                                     uint32_t *__restrict__ n_fixed)
{
    __shared__ uint32_t s_ops[PathWalk::WORDS][64];
    __shared__ uint64_t s_cols[(FSV_WINDOW + 2) * 3];
    if (threadIdx.x != 0) return;
    const uint32_t n_list = *n_list_dev;
    for (uint32_t li = blockIdx.x; li < n_list; li += gridDim.x) {
        const uint32_t tid = list[li];
        fsv_wtask t = tasks[tid];
        fsv_wres r = res[tid];
        const int y0 = t.y_start;
        fix_boundary_dev(store, t, r, paths + tid, s_ops, s_cols, k_cap);
        if (t.y_start != y0) { tasks[tid] = t; res[tid] = r; if (n_fixed) atomicAdd(n_fixed, 1u); }
    }
}

// ------------------------------------------------------------------------------------------------ k_left_rescue
// recalcate_window_advance's left pass (Correct.cpp:2745-2905), for the overlaps k_rescue_accept set aside: a matched window whose
// left neighbour is unmatched gets its path first -- its real start on y -- and the unmatched windows to its left are tried again one
// after the other, each placed so that it ends right in front of the window to its right, with the doubled threshold and its path at
// once (the next one needs its start).  Then the overlap is accepted or not, as k_rescue_accept does: a window whose path was
// computed here counts with its distance after generate_cigar, as in hifiasm.  One block (one working lane) per listed overlap, a
// persistent grid over the list; oracle/asm.c:align_overlaps (left_rescue) statement for statement.
// DEFER: as in k_rescue_accept -- the 0.9 filter alone decides here, provisionally.
template <bool DEFER = false>
__global__ __launch_bounds__(64) void k_left_rescue(const uint32_t *__restrict__ store, fsv_ovl *__restrict__ ovl, const uint32_t *__restrict__ list,
                                                    const uint32_t *__restrict__ n_list_dev, fsv_wtask *__restrict__ tasks, fsv_wres *__restrict__ res,
                                                    fsv_wpath *__restrict__ paths, uint4 *__restrict__ ovl_c, int k_cap, int accept_err_pm)
{
    // One lane of a block works, with the column scratch of its window in LDS: the walk back is a chain of dependent reads of that
    // scratch, column after column -- 1.3 ms for a single window from HBM, whatever the number of overlaps listed (a few thousand in the
    // first round, a dozen later); 40 us from LDS.
    __shared__ uint32_t s_ops[PathWalk::WORDS][64];
    __shared__ uint64_t s_cols[(FSV_WINDOW + 2) * 3];
    if (threadIdx.x != 0) return;
    const uint32_t n_list = *n_list_dev;
    for (uint32_t li = blockIdx.x; li < n_list; li += gridDim.x) {
        const uint32_t p = list[li];
        fsv_ovl o = ovl[p];
        fsv_wtask *T = tasks + o.first_win;
        fsv_wres *R = res + o.first_win;
        fsv_wpath *PP = paths + o.first_win;
        long long post = 0;          // sum over the windows whose path was computed here of (distance after generate_cigar - K5's distance)
        auto window_path = [&](fsv_wtask &t, fsv_wres &r, fsv_wpath *P) {
            if (!path_gapfree(store, t, r, P, true)) path_general<uint64_t, 1>(store, t, P, s_ops, 0, s_cols);
            fix_boundary_dev(store, t, r, P, s_ops, s_cols, k_cap);
        };
        for (int j = 1; j < o.n_win; j++) {
            if (R[j].err < 0 || R[j - 1].err >= 0) continue;
            fsv_wtask tj = T[j];
            fsv_wres rj = R[j];
            window_path(tj, rj, PP + j);
            if (tj.y_start != T[j].y_start) { T[j] = tj; R[j] = rj; }      // (fix_boundary moved the window)
            const uint4 hj = *reinterpret_cast<const uint4 *>(PP + j);
            if ((hj.w & 0xffu) != 1u) { R[j].err = -1; continue; }       // (a path longer than a record holds: the window is unused, as in window_path)
            post += (int)(int16_t)(hj.z >> 16) - rj.err;
            int total_y_end = (int)hj.x - 1;
            for (int k2 = j - 1; k2 >= 0 && R[k2].err < 0; k2--) {
                fsv_wtask u = T[k2];
                u.k = (uint8_t)double_thr(u.k, u.x_len, k_cap);
                if (total_y_end <= 0) break;
                u.y_start = total_y_end - (int)u.x_len + 1;
                fsv_wres r;
                if (!bpm_window_geometry(u, r, k_cap)) break;
                if ((u.x_len + 2 * u.k - r.extra_begin - r.extra_end) + u.k < u.x_len) break;
                bpm_run(store, u, r, BpmNoSink());
                if (r.err < 0) break;
                window_path(u, r, PP + k2);
                const uint4 hk = *reinterpret_cast<const uint4 *>(PP + k2);
                if ((hk.w & 0xffu) != 1u) break;
                T[k2] = u; R[k2] = r;
                post += (int)(int16_t)(hk.z >> 16) - r.err;
                total_y_end = (int)hk.x - 1;
            }
        }
        int align = 0;
        long long tlen = 0, terr = post;
        for (int j = 0; j < o.n_win; j++) {
            const int e = R[j].err, xl = T[j].x_len;
            if (e >= 0) { align += xl; terr += e; } else terr += xl;
            tlen += xl;
        }
        o.align_len = align; o.err_sum = (int32_t)terr;
        const bool covered = (long long)(o.x_e - o.x_s + 1) * 9 <= (long long)align * 10;
        o.is_match = (covered && (DEFER || terr * 1000 <= tlen * accept_err_pm)) ? 1 : 0;
        ovl[p] = o;
        ovl_c[p] = make_uint4((uint32_t)o.x_s, (uint32_t)o.first_win, (uint32_t)o.n_win | (o.is_match && !DEFER ? 0x80000000u : 0u), 0u);
    }
}

// ------------------------------------------------------------------------------------------------ partial charge (opt-in)
// non_trim_error_rate (Correct.cpp:725-845), for fsv_asm_params.partial_charge = 1; oracle/asm.c:align_overlaps with partial_charge
// (the acceptance test and unmatched_charge) statement for statement.  The rescue kernels ran with DEFER: every overlap that passed the
// 0.9 coverage filter carries is_match = 1 and K6 (path_stage, fix_boundary included) has left its matched windows' paths.  Now
//   k_charge_tasks   one lane per overlap slot: the error sum over the matched windows' distances AFTER generate_cigar (the path headers),
//                    as the reference has them when it sums up (Correct.cpp:2920-3003).  No unmatched window: the verdict, here.  Otherwise
//                    two extension tasks per unmatched window -- from the left neighbour's exact end, to the right neighbour's exact start,
//                    doubled threshold -- at the fixed slots 2 x window task + direction, and the overlap goes on the list;
//   k_bpm_ext        one lane per extension task (bpm_ext_run, bpm_device.h);
//   k_charge_accept  one lane per listed overlap: its windows in order with the running total (the float branch of the charge reads it),
//                    then the verdict.
// An overlap rejected in the end gets the path state of all its windows cleared, which is how k_path_fast leaves a rejected overlap's
// windows on the default path: the consensus, partition and junction kernels that look at the path state alone see no difference.
struct ChargeArgs {
    fsv_ovl *ovl; uint32_t n_pairs;
    const fsv_wtask *tasks; const fsv_wres *res; fsv_wpath *paths; uint4 *ovl_c;
    fsv_wtask *ext_tasks;            // slot 2 x (window task) + direction; .win: the direction, .ovl: the window task
    const fsv_wext *ext_res;         // the same slots
    uint32_t *ext_list, *n_ext;      // the slots that hold a task, in no particular order (results sit at fixed slots)
    uint32_t *ovl_list, *n_ovl;      // overlap slots waiting for k_charge_accept
    unsigned long long *stats;       // fsv_charge_stats' five counters, in its order
    int k_cap, accept_err_pm;
};
enum { CH_OVERLAPS = 0, CH_WINDOWS = 1, CH_EXT = 2, CH_ACCEPTED = 3, CH_FLIPPED = 4 };

// a window counts as matched when K5 (or a rescue pass) aligned it and K6 left a path (a path too long for a record leaves the window
// unused, as oracle/asm.c:window_path does; with thresholds up to 31 there is none)
__device__ __forceinline__ bool charge_matched(const fsv_wres *R, const fsv_wpath *P, uint4 &h)
{
    h = *reinterpret_cast<const uint4 *>(P);
    return R->err >= 0 && (h.w & 0xffu) == 1u;
}

__device__ __forceinline__ void charge_verdict(const ChargeArgs &A, uint32_t p, fsv_ovl &o, long long tlen, long long terr)
{
    o.err_sum = (int32_t)terr;
    o.is_match = ((long long)(o.x_e - o.x_s + 1) * 9 <= (long long)o.align_len * 10 && terr * 1000 <= tlen * A.accept_err_pm) ? 1 : 0;
    A.ovl[p] = o;
    A.ovl_c[p] = make_uint4((uint32_t)o.x_s, (uint32_t)o.first_win, (uint32_t)o.n_win | (o.is_match ? 0x80000000u : 0u), 0u);
    if (!o.is_match) for (int j = 0; j < o.n_win; j++) A.paths[o.first_win + j].state = 0;
}

__global__ __launch_bounds__(64) void k_charge_tasks(ChargeArgs A)
{
    const uint32_t p = blockIdx.x * 64 + threadIdx.x;
    if (p >= A.n_pairs) return;
    fsv_ovl o = A.ovl[p];
    if (!o.valid || !o.is_match) return;      // (no overlap, or below the 0.9 filter: ovl_c says "not accepted" already, no path was made)
    const fsv_wtask *T = A.tasks + o.first_win;
    const fsv_wres *R = A.res + o.first_win;
    const fsv_wpath *PP = A.paths + o.first_win;
    long long tlen = 0, terr = 0;
    int n_bad = 0;
    for (int j = 0; j < o.n_win; j++) {
        uint4 h;
        tlen += T[j].x_len;
        if (charge_matched(R + j, PP + j, h)) terr += (int)(int16_t)(h.z >> 16); else n_bad++;
    }
    if (!n_bad) { charge_verdict(A, p, o, tlen, terr); return; }
    o.is_match = 0;                           // until k_charge_accept has spoken
    A.ovl[p] = o;
    A.ovl_list[atomicAdd(A.n_ovl, 1u)] = p;
    atomicAdd(A.stats + CH_OVERLAPS, 1ull);
    atomicAdd(A.stats + CH_WINDOWS, (unsigned long long)n_bad);
    uint4 h, hl = make_uint4(0u, 0u, 0u, 0u);
    bool left = false, cur = charge_matched(R, PP, h);
    for (int j = 0; j < o.n_win; j++) {
        // h / cur: window j; hl / left: window j - 1; hr / right: window j + 1
        uint4 hr = make_uint4(0u, 0u, 0u, 0u);
        const bool right = j + 1 < o.n_win && charge_matched(R + j + 1, PP + j + 1, hr);
        if (!cur && R[j].y_beg >= 0) {
            fsv_wtask t = T[j];
            const int n = t.x_len, k0 = t.k;
            int yb0 = left ? (int)hl.y + 1 : -1, yb1 = right ? (int)hr.x - n : -1;     // ry_end + 1 / ry_start - n
            if (yb0 < 0 && yb1 < 0) yb0 = yb1 = R[j].y_beg + k0 - R[j].extra_begin;
            if (yb0 < 0) yb0 = yb1;
            if (yb1 < 0) yb1 = yb0;
            const uint32_t tid = (uint32_t)o.first_win + (uint32_t)j;
            t.k = (uint8_t)double_thr(k0, n, A.k_cap);
            t.ovl = tid;
            const uint32_t at = atomicAdd(A.n_ext, 2u);
            t.y_start = yb0; t.win = 0u; A.ext_tasks[2 * tid] = t; A.ext_list[at] = 2 * tid;
            t.y_start = yb1; t.win = 1u; A.ext_tasks[2 * tid + 1] = t; A.ext_list[at + 1] = 2 * tid + 1;
        }
        hl = h; left = cur; h = hr; cur = right;
    }
}

// list == null: task i sits in slot i (fsv_bpm_extensions); n_list_dev == null: n_tasks is the count
__global__ __launch_bounds__(64) void k_bpm_ext(const uint32_t *__restrict__ store, const fsv_wtask *__restrict__ tasks, const uint32_t *__restrict__ list,
                                                const uint32_t *__restrict__ n_list_dev, uint32_t n_tasks, int k_cap, fsv_wext *__restrict__ out,
                                                unsigned long long *__restrict__ n_run)
{
    if (n_list_dev) n_tasks = min(*n_list_dev, n_tasks);
    unsigned int ran = 0;
    for (uint32_t i = blockIdx.x * 64 + threadIdx.x; i < n_tasks; i += gridDim.x * 64) {
        const uint32_t slot = list ? list[i] : i;
        const fsv_wtask t = tasks[slot];
        fsv_wext r;
        ran += bpm_ext_run(store, t, (int)(t.win & 1u), k_cap, r) ? 1u : 0u;
        out[slot] = r;
    }
    if (n_run && ran) atomicAdd(n_run, (unsigned long long)ran);
}

__global__ __launch_bounds__(64) void k_charge_accept(ChargeArgs A)
{
    const uint32_t li = blockIdx.x * 64 + threadIdx.x;
    if (li >= min(*A.n_ovl, A.n_pairs)) return;
    const uint32_t p = A.ovl_list[li];
    fsv_ovl o = A.ovl[p];
    const fsv_wtask *T = A.tasks + o.first_win;
    const fsv_wres *R = A.res + o.first_win;
    const fsv_wpath *PP = A.paths + o.first_win;
    long long tlen = 0, terr = 0, full = 0;
    for (int j = 0; j < o.n_win; j++) {
        uint4 h;
        const int n = T[j].x_len;
        tlen += n;
        if (charge_matched(R + j, PP + j, h)) { const int e = (int)(int16_t)(h.z >> 16); terr += e; full += e; continue; }
        full += n;
        if (R[j].y_beg < 0) { terr += n; continue; }       // the window lies outside y
        const fsv_wext e0 = A.ext_res[2 * ((size_t)o.first_win + j)], e1 = A.ext_res[2 * ((size_t)o.first_win + j) + 1];
        terr = fsv_partial_charge_hd(n, e0.t_end >= 0 ? e0.t_end + 1 : 0, e0.t_end >= 0 ? e0.err : 0, e1.t_end >= 0 ? e1.t_end + 1 : 0,
                                     e1.t_end >= 0 ? e1.err : 0, terr);
    }
    charge_verdict(A, p, o, tlen, terr);
    if (o.is_match) {
        atomicAdd(A.stats + CH_ACCEPTED, 1ull);
        if (full * 1000 > tlen * A.accept_err_pm) atomicAdd(A.stats + CH_FLIPPED, 1ull);
    }
}

// ---- the walk kernels' task: a listed window, its record, and what K5 found for it -- the end site, the distance, and the band row
// the alignment ends on
struct PathTask { fsv_wtask t; fsv_wpath *P; int n, k, band, end, err, row0; };
__device__ __forceinline__ PathTask path_task_of(const fsv_wtask *__restrict__ tasks, const fsv_wres *__restrict__ res, fsv_wpath *__restrict__ paths, const uint32_t tid)
{
    PathTask T;
    T.t = tasks[tid];
    const fsv_wres r0 = res[tid];
    T.P = paths + tid;
    T.n = T.t.x_len; T.k = T.t.k; T.band = 2 * T.k + 1;
    T.end = r0.end_site; T.err = r0.err;
    T.row0 = T.band - (T.n + 2 * T.k - T.end);
    return T;
}
// a walk kernel's forward pass is K5's DP once more: it reproduces (end site, distance), or the window is left without a path (cannot happen)
__device__ __forceinline__ bool path_same_dp(const PathTask &T, const fsv_wres &r)
{
    if (r.err == T.err && r.end_site == T.end) return true;
    T.P->state = 0;
    return false;
}

// ---- K6 for first-pass windows: k <= 15, distance 4 .. FSV_SB_MAXERR (3 and below: k_path_fr further down) ----------------
// What the walk back (Levenshtein_distance.h:757-888) asks of a DP cell is which way it leaves it -- 0 diagonal over a match,
// 1 diagonal over a mismatch, 2 up, 3 left; ties: diagonal, then up, then left -- and that is known while the column is
// computed: a cell whose D0 bit is clear is a mismatch (the diagonal is one cheaper than the cell, nothing beats it);
// otherwise "up" is cheaper exactly when the column's new VP has the bit of the row below set, and "left" when HP has the
// cell's bit (the top band row has no left neighbour).  And the walk never strays further than `err` rows from the end row:
// every up / left step spends one of the err errors it has left.  K5 already gave (end site, err) for the window, so the
// forward pass keeps two bits for each of the 2 x 7 + 1 rows around the end row: ONE 32-bit word per column (bits 0-15 the
// low code bit of rows row0-7 .. row0+8, bits 16-31 the high one) instead of three band-wide words.  Columns go to the scratch
// four at a time ([block][column quad][lane] as uint4: 1 KB per wave store); the walk reads them back a quad ahead of where it
// stands, so no step waits on memory -- round 1's walk was a chain of ~375 dependent loads per window (62 % of its wave cycles
// parked in s_waitcnt, profiles/r01_i_pmc_sq_summary.txt).  Scratch traffic: 1.5 KB per window, written once, read once.
struct SubbandSink {
    uint4 *slot;             // this lane's uint4 of quad 0; quad q sits 64 x q further
    uint32_t sr, sl, lmask;  // band word -> sub-band: (w >> sr) << sl; rows that may step left
    uint32_t a0, a1, a2, a3;
    __device__ __forceinline__ void operator()(int blk, int j, uint32_t d0, uint32_t hp, uint32_t vp, uint32_t)
    {
        const uint32_t u = vp << 1, l = hp & lmask;
        const uint32_t w1 = d0 & (u | l), w0 = ~d0 | (l & ~u);
        const uint32_t word = (((w0 >> sr) << sl) & 0xffffu) | (((w1 >> sr) << sl) << 16);
        if ((j & 3) == 0) a0 = word; else if ((j & 3) == 1) a1 = word; else if ((j & 3) == 2) a2 = word; else a3 = word;
        if ((j & 3) == 3) slot[(size_t)((blk + j) >> 2) * 64] = make_uint4(a0, a1, a2, a3);
    }
    __device__ __forceinline__ void flush(int n) { if (n & 3) slot[(size_t)(n >> 2) * 64] = make_uint4(a0, a1, a2, a3); }
};

__device__ __forceinline__ uint32_t quad_elem(const uint4 &q, int e) { return e == 0 ? q.x : e == 1 ? q.y : e == 2 ? q.z : q.w; }

// STAMP: diagnostic build only (FSV_K6_STAMPS=1): shader-clock cycles of the three phases summed over the waves' trips into `stamps`
template <bool STAMP>
__global__ __launch_bounds__(64) void k_path_sb(const uint32_t *__restrict__ store, const fsv_wtask *__restrict__ tasks, const fsv_wres *__restrict__ res,
                                                const uint32_t *__restrict__ dp_list, const uint32_t *__restrict__ n_dev,
                                                fsv_wpath *__restrict__ paths, uint4 *__restrict__ cols, unsigned long long *__restrict__ stamps)
{
    PhaseClock<STAMP> clk(true);
    __shared__ uint32_t s_ops[PathWalk::WORDS][64];
    const int lane64 = threadIdx.x;
    const uint32_t n_list = *n_dev;
    uint4 *slot = cols + (size_t)blockIdx.x * FSV_SB_QUADS * 64 + lane64;   // persistent blocks: the slice is reused for every task
    for (uint32_t li = blockIdx.x * 64 + threadIdx.x; li < n_list; li += gridDim.x * 64) {
        const PathTask T = path_task_of(tasks, res, paths, dp_list[li]);
        constexpr int ME = FSV_SB_MAXERR, QSH = 2;
        const int lo = T.row0 - ME;
        SubbandSink sink;
        sink.slot = slot; sink.sr = (uint32_t)max(lo, 0); sink.sl = (uint32_t)max(-lo, 0);
        sink.lmask = T.band == 1 ? 1u : (1u << (T.band - 1)) - 1u;
        sink.a0 = sink.a1 = sink.a2 = sink.a3 = 0;
        fsv_wres r;
        clk.restart();
        bpm_run32(store, T.t, r, sink);
        clk.mark(stamps, lane64, 0);
        if (!path_same_dp(T, r)) continue;
        PathWalk w(s_ops, lane64);
        w.clear(T.n, T.end, T.err, ME);      // the row: relative to the sub-band
        // The walk, a quad of columns per phase: every lane walks until it leaves its current quad (four column steps plus its
        // "up" steps), then all lanes move one quad down together.  Six quads rotate through registers and the one just left
        // is refilled with the quad six below, so a quad is requested five phases before it is walked and no lane ever waits
        // for a load another lane has just issued (with a per-lane "switch when I cross" every crossing waited out the full
        // memory latency of the neighbour's request: 1 500 cycles per step, FSV_K6_STAMPS).
        int qi = w.ci >> QSH;
        auto quad = [&](int q) { return q >= 0 ? slot[(size_t)q * 64] : make_uint4(0, 0, 0, 0); };
        uint4 qa = quad(qi), qb = quad(qi - 1), qc = quad(qi - 2), qd = quad(qi - 3), qe = quad(qi - 4), qf = quad(qi - 5);
        auto phase = [&](const uint4 &q4) {
            while (w.cur != 0 && w.ci >= 0 && (w.ci >> QSH) == qi) {
                // A match step keeps the band row and moves one column left, so a run of matches is a run of zero codes at ONE
                // bit position of consecutive columns' words: the columns of this quad whose code at the row is not 0 are found with a few
                // shifts, and the matches in front of the first of them are taken in one step (round 2 walked them one by one, ~40
                // instructions each: half of K6's time by the cycle stamps, 375 steps for the 1-3 deviations of a HiFi window).
                const int rel = w.row;
                uint32_t nz;
                nz = (((q4.x >> rel) | (q4.x >> (rel + 16))) & 1u) | ((((q4.y >> rel) | (q4.y >> (rel + 16))) & 1u) << 1) |
                     ((((q4.z >> rel) | (q4.z >> (rel + 16))) & 1u) << 2) | ((((q4.w >> rel) | (q4.w >> (rel + 16))) & 1u) << 3);
                const int cl = w.ci & 3;
                const uint32_t m = nz & ((2u << cl) - 1u);          // deviating columns at or below this one
                const int steps = m ? cl - (31 - __clz((int)m)) : cl + 1;
                if (steps) {
                    w.matches(steps);
                    if (!m) continue;                                   // the rest of the quad matched
                }
                const uint32_t cw = quad_elem(q4, w.ci & 3);
                w.put(((cw >> rel) & 1u) | (((cw >> (16 + rel)) & 1u) << 1));
            }
        };
        // (six quads in rotation since round 3: a quad is requested five phases before it is walked.  With three -- two phases, ~800
        // cycles of walking -- every phase still waited out most of a memory round trip: the stamps showed half of K6's time in the walk)
        while (__any(w.cur != 0 && w.ci >= 0)) {
            phase(qa); qi--; qa = quad(qi - 5);
            phase(qb); qi--; qb = quad(qi - 5);
            phase(qc); qi--; qc = quad(qi - 5);
            phase(qd); qi--; qd = quad(qi - 5);
            phase(qe); qi--; qe = quad(qi - 5);
            phase(qf); qi--; qf = quad(qi - 5);
        }
        w.flush();
        clk.mark(stamps, lane64, 1);
        path_finish(store, T.t, T.P, w, T.end, T.err);
        clk.mark(stamps, lane64, 2);
    }
}

// ---- K6 without the matrix: distance <= FSV_FR_MAXERR ------------------------------------------------------------------------
// The walk back (Levenshtein_distance.h:757-888) asks three things of the cell (column c, band row r) it stands on, whose
// distance `cur` it knows: is the diagonal neighbour (c-1, r) one cheaper (a mismatch), else is the upper one (c, r-1), else the
// left one (c-1, r+1); none of them: a match, one column down the same row.  A band row is a diagonal of the alignment
// matrix and the distance never falls along a diagonal, so "cell (c, r) is within s errors" is c <= F[s][r], the furthest
// column row r reaches with s errors -- Landau-Vishkin's table, started from the free start of the DP (every band row at
// column -1 with distance 0) and clipped to the band:
//     F[0][r] = last column of the run of matches from column 0 on row r
//     F[s][r] = the run of matches behind max(F[s-1][r] + 1, F[s-1][r-1], F[s-1][r+1] + 1)      (mismatch, up, left)
// The walk starts on the end row with the window's distance e (K5 gave both) and spends an error with every move off a match,
// so the cell it stands on with `cur` left is at most e - cur rows from the end row and the three neighbours it tests sit on
// level cur - 1 at most e - cur + 1 rows away: a triangle of (2e+1) + (2e-1) + .. + 3 table entries (15 for e = 3), each a
// word-wise comparison of packed bases, instead of 375 columns of the recurrence and their 750-byte scratch.  Between two
// errors the walk is one subtraction: it matches down its row to the first column where a neighbour opens.
// tests/test_gpu_k6.py holds this kernel to the oracle's matrix walk.
// first column in [cs, cs + 64) (none at or past n) whose x base differs from the y base at strand position ypos + column, as an offset from cs
__device__ __forceinline__ int diag_mismatch16(uint32_t xb, uint32_t yb, uint32_t yvalid)
{
    const uint32_t d = mismatch_fields16(xb, yb, yvalid);     // columns outside read y never match
    return d ? (__ffs((int)d) - 1) >> 1 : 16;
}
__device__ __forceinline__ int diag_probe64(const uint32_t *__restrict__ store, const fsv_wtask &t, int ypos, int cs, int n)
{
    uint32_t xb4[4], yb4[4], yv4[4];
    fetch64_x(store, t.x_word, t.x_start + cs, xb4);
    fetch64(store, t.y_word, t.y_len, t.y_rev, ypos + cs, yb4, yv4);
    int m = 64;
#pragma unroll
    for (int q = 3; q >= 0; q--) { const int f = diag_mismatch16(xb4[q], yb4[q], yv4[q]); if (f < 16) m = q * 16 + f; }
    return min(m, n - cs);
}

// E = the windows' distance (one list per distance: a wave's lanes then have the same number of table entries to fill)
// STAMP: diagnostic build only (FSV_K6_STAMPS=1): shader-clock cycles of table / walk / finish summed over the waves' trips into `stamps`
template <int E, bool STAMP = false>
__global__ __launch_bounds__(64) void k_path_fr(const uint32_t *__restrict__ store, const fsv_wtask *__restrict__ tasks, const fsv_wres *__restrict__ res,
                                                const uint32_t *__restrict__ dp_list, const uint32_t *__restrict__ n_dev, fsv_wpath *__restrict__ paths,
                                                unsigned long long *__restrict__ stamps = nullptr)
{
    PhaseClock<STAMP> clk(true);
    __shared__ uint32_t s_ops[PathWalk::WORDS][64];
    constexpr int NJ = 2 * E + 1;
    const int lane64 = threadIdx.x;
    const uint32_t n_list = *n_dev;
    for (uint32_t li = blockIdx.x * 64 + threadIdx.x; li < n_list; li += gridDim.x * 64) {
        clk.restart();
        const PathTask T = path_task_of(tasks, res, paths, dp_list[li]);
        const fsv_wtask &t = T.t;
        const int n = T.n, band = T.band, row0 = T.row0, win0 = t.y_start - T.k;
        // Q[s][j + E] = F[s][row0 + j] + 1: the first column of the row that is NOT within s errors; -1 = no such row (outside the
        // band or the triangle): F = -2 is below every column the walk can ask about
        int Q[E][NJ];
        // the rows in `run` lengthen their runs of matches, 64 columns a trip, every lane working on its lowest running row: the
        // wave makes as many trips as its busiest lane has chunks to compare (row after row it made the sum of the rows' longest)
        auto extend = [&](int (&q)[NJ], uint32_t run) {
            while (__any(run != 0u)) {
                if (run) {
                    const int jj = __ffs((int)run) - 1;
                    int c = 0;
#pragma unroll
                    for (int i = 0; i < NJ; i++) c = i == jj ? q[i] : c;
                    const int m = diag_probe64(store, t, win0 + row0 + jj - E, c, n);
                    c += m;
#pragma unroll
                    for (int i = 0; i < NJ; i++) q[i] = i == jj ? c : q[i];
                    if (m < 64 || c >= n) run &= run - 1u;
                }
            }
        };
        {
            // level 0, first 64 columns: every row starts at column 0 and the rows' y bases overlap -- one fetch for all of them
            uint32_t xb4[4], yb[5], yv[5];
            fetch64_x(store, t.x_word, t.x_start, xb4);
            {
                uint32_t b4[4], v4[4];
                fetch64(store, t.y_word, t.y_len, t.y_rev, win0 + row0 - E, b4, v4);
                const Bases16 b5 = fetch16(store, t.y_word, t.y_len, t.y_rev, win0 + row0 - E + 64);
#pragma unroll
                for (int q = 0; q < 4; q++) { yb[q] = b4[q]; yv[q] = v4[q] & 0xffffu; }
                yb[4] = b5.bits; yv[4] = b5.valid & 0xffffu;
            }
            uint32_t run = 0;
#pragma unroll
            for (int jj = 0; jj < NJ; jj++) {
                const int row = row0 + jj - E;
                int m = -1;
                if (row >= 0 && row < band) {
                    m = 64;
#pragma unroll
                    for (int q = 3; q >= 0; q--) {
                        const int f = diag_mismatch16(xb4[q], __builtin_amdgcn_alignbit(yb[q + 1], yb[q], 2 * jj), ((yv[q] | yv[q + 1] << 16) >> jj) & 0xffffu);
                        if (f < 16) m = q * 16 + f;
                    }
                    m = min(m, n);
                    if (m == 64 && n > 64) run |= 1u << jj;
                }
                Q[0][jj] = m;
            }
            extend(Q[0], run);
        }
#pragma unroll
        for (int s = 1; s < E; s++) {
            uint32_t run = 0;
#pragma unroll
            for (int jj = 0; jj < NJ; jj++) {
                const int row = row0 + jj - E;
                int c = -1;
                if (abs(jj - E) <= E - s && row >= 0 && row < band) {
                    // the furthest cell of the row within s errors before its matches: behind a mismatch on the row, an "up" move
                    // from the row below (same column), a "left" move from the row above (next column)
                    const int up = jj > 0 ? Q[s - 1][jj - 1] - 1 : -2, left = jj + 1 < NJ ? Q[s - 1][jj + 1] : -2;
                    c = min(n - 1, max(Q[s - 1][jj], max(up, left))) + 1;
                    if (c < n) run |= 1u << jj;
                }
                Q[s][jj] = c;
            }
            extend(Q[s], run);
        }
        clk.mark(stamps, lane64, 0);
        PathWalk w(s_ops, lane64);
        w.clear(n, T.end, E, E);        // the row: an index into a level of Q
#pragma unroll
        for (int s = E - 1; s >= 0; s--) {      // the walk has s + 1 errors left: its neighbours are judged on level s
            int fa = -1, fb = -2, fc = -1;      // first columns (from the end) where the mismatch / up / left move is open
#pragma unroll
            for (int i = 0; i < NJ; i++) { fa = i == w.row ? Q[s][i] : fa; fb = i == w.row - 1 ? Q[s][i] - 1 : fb; fc = i == w.row + 1 ? Q[s][i] : fc; }
            const int cstop = min(w.ci, max(fa, max(fb, fc)));    // fa >= 0: column 0 is a mismatch at the latest
            w.matches(w.ci - cstop);
            w.put(w.ci <= fa ? 1u : w.ci <= fb ? 2u : 3u);
        }
        w.flush();
        clk.mark(stamps, lane64, 1);
        path_finish(store, t, T.P, w, T.end, E);
        clk.mark(stamps, lane64, 2);
    }
}

// ---- K6 for wide bands (k > 31, up to 95): the ONT profile ---------------------------------------------------------------------
// The walk codes of k_path_sb for every band row: two planes x six 32-bit limbs per column (48 B) in a per-lane slice of an HBM
// scratch ([block][column][12][lane]).  The distance of such a window is of the order of its band (tens of errors), so there is
// no narrow sub-band to keep, and the walk reads the two words of its row's limb at every step.  First version: correct, not
// tuned (the forward pass is ~130 lane-ops per column, the walk a dependent load per step).
struct WideCodeSink {
    uint32_t *cols; uint32_t lane; int band;
    __device__ __forceinline__ void operator()(int col, const uint32_t *d0, const uint32_t *hp, const uint32_t *vp)
    {
        uint32_t *c = cols + (size_t)col * 2 * FSV_WL * 64 + lane;
#pragma unroll
        for (int l = 0; l < FSV_WL; l++) {
            const uint32_t u = vp[l] << 1 | (l ? vp[l - 1] >> 31 : 0u);
            // the top band row has no left neighbour
            const int tb = band - 1 - 32 * l;
            const uint32_t lm = band == 1 ? 1u : (tb >= 32 ? 0xffffffffu : (tb <= 0 ? 0u : ((1u << tb) - 1u)));
            const uint32_t lf = hp[l] & lm;
            c[(size_t)l * 64] = ~d0[l] | (lf & ~u);              // low code bit
            c[(size_t)(FSV_WL + l) * 64] = d0[l] & (u | lf);     // high code bit
        }
    }
};

__global__ __launch_bounds__(64) void k_path_wide(const uint32_t *__restrict__ store, const fsv_wtask *__restrict__ tasks, const fsv_wres *__restrict__ res,
                                                  const uint32_t *__restrict__ dp_list, const uint32_t *__restrict__ n_dev,
                                                  fsv_wpath *__restrict__ paths, uint32_t *__restrict__ cols, int k_cap)
{
    __shared__ uint32_t s_ops[PathWalk::WORDS][64];
    const int lane64 = threadIdx.x;
    const uint32_t n_list = *n_dev;
    uint32_t *slot = cols + (size_t)blockIdx.x * FSV_WINDOW * 2 * FSV_WL * 64;
    for (uint32_t li = blockIdx.x * 64 + threadIdx.x; li < n_list; li += gridDim.x * 64) {
        const PathTask T = path_task_of(tasks, res, paths, dp_list[li]);
        WideCodeSink sink{slot, (uint32_t)lane64, T.band};
        fsv_wres r;
        bpm_run_wide(store, T.t, r, sink, k_cap);
        if (!path_same_dp(T, r)) continue;
        PathWalk w(s_ops, lane64);
        w.clear(T.n, T.end, T.err, T.row0);
        bool fits = true;
        // The walk, column by column for the whole wavefront: the two code words a lane needs at a column (those of its row's limb)
        // are requested FOUR columns ahead, at a point every lane passes together, and held in four register pairs that an unrolled
        // loop uses in turn -- round 2's walk was a dependent pair of loads per step (~400 steps of full memory latency per window:
        // 314 ms per ONT step).  A lane whose row has moved to another limb by the time it reaches a column (a limb is 32 rows; the
        // row drifts by one per gap) loads that column's words directly.
        auto ld = [&](int c, int lm, uint32_t &lo, uint32_t &hi) {
            if (c >= 0) { const uint32_t *p = slot + (size_t)c * 2 * FSV_WL * 64 + lane64; lo = p[(size_t)lm * 64]; hi = p[(size_t)(FSV_WL + lm) * 64]; }
        };
        auto column = [&](int c, uint32_t &lo, uint32_t &hi, int &lmx) {
            if (c >= 0 && w.ci == c && w.cur != 0 && fits) {
                while (true) {
                    const int lm = w.row >> 5, bt = w.row & 31;
                    if (lm != lmx) { ld(c, lm, lo, hi); lmx = lm; }
                    if (w.plen >= PathWalk::CAP - 1) { fits = false; break; }        // the path buffer is full; such a path is dropped below anyway
                    w.put(((lo >> bt) & 1u) | (((hi >> bt) & 1u) << 1));
                    if (w.dir != 2 || w.cur == 0) break;     // "up" stays in its column
                }
            }
            lmx = w.row >> 5;
            ld(c - 4, lmx, lo, hi);          // (every lane, walking or not: the request is issued where the whole wave passes)
        };
        const int c0 = FSV_WINDOW - 1;       // every window has at most FSV_WINDOW columns; a shorter one idles until the loop reaches its last column
        uint32_t lo0 = 0, hi0 = 0, lo1 = 0, hi1 = 0, lo2 = 0, hi2 = 0, lo3 = 0, hi3 = 0;
        int lm0 = w.row >> 5, lm1 = lm0, lm2 = lm0, lm3 = lm0;
        ld(c0, lm0, lo0, hi0); ld(c0 - 1, lm1, lo1, hi1); ld(c0 - 2, lm2, lo2, hi2); ld(c0 - 3, lm3, lo3, hi3);
        for (int c = c0; c >= 0; c -= 4) {
            if (!__any(w.cur != 0 && w.ci >= 0 && fits)) break;
            column(c, lo0, hi0, lm0);
            column(c - 1, lo1, hi1, lm1);
            column(c - 2, lo2, hi2, lm2);
            column(c - 3, lo3, hi3, lm3);
        }
        w.flush();
        if (!fits) { T.P->state = 0; continue; }
        path_finish(store, T.t, T.P, w, T.end, T.err);
    }
}

} // namespace
#include "k_consensus.h"
namespace {

// ------------------------------------------------------------------------------------------------ k_newlen / k_repack
__global__ void k_newlen(const uint32_t *__restrict__ gwin_off, const uint16_t *__restrict__ cwin_len, uint32_t n_reads, int32_t *__restrict__ new_len,
                         uint32_t *__restrict__ lb = nullptr)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_reads) return;
    int32_t L = 0;
    for (uint32_t g = gwin_off[r]; g < gwin_off[r + 1]; g++) { if (lb) lb[g] = (uint32_t)L; L += cwin_len[g]; }   // lb: where window g starts in the corrected read
    new_len[r] = L;
}

// One workgroup per read, a thread per output word: 16 bases gathered from the corrected windows of the read (optionally
// reverse-complemented).  The windows' starts in the corrected read (k_newlen's lb) are staged in LDS and searched there; with one
// thread per word of the whole store every thread searched the read table (15 dependent loads) and then walked its read's windows
// one dependent load at a time.
#define FSV_RP_WIN 1024
__global__ __launch_bounds__(256) void k_repack(const uint32_t *__restrict__ gwin_off, const uint32_t *__restrict__ lb,
                                                const uint8_t *__restrict__ cwin, const uint32_t *__restrict__ new_word_off,
                                                const int32_t *__restrict__ new_len, uint32_t n_reads, int rc,
                                                uint32_t *__restrict__ out, const uint32_t *__restrict__ only = nullptr)
{
    __shared__ int s_lb[FSV_RP_WIN + 1];
    const uint32_t r = blockIdx.x;
    if (r >= n_reads) return;
    if (only && !only[r]) return;      // the second pass only looks at reads some overlap deviates from
    const uint32_t g0 = gwin_off[r], nw = gwin_off[r + 1] - g0;
    const int len = new_len[r];
    const uint32_t w0 = new_word_off[r], slot = new_word_off[r + 1] - w0;
    const bool in_lds = nw <= FSV_RP_WIN;
    if (in_lds) {
        for (uint32_t i = threadIdx.x; i < nw; i += 256) s_lb[i] = (int)lb[g0 + i];
        if (threadIdx.x == 0) s_lb[nw] = len;
    }
    __syncthreads();
    auto LB = [&](uint32_t i) -> int { return in_lds ? s_lb[i] : (i < nw ? (int)lb[g0 + i] : len); };
    for (uint32_t w = threadIdx.x; w < slot; w += 256) {
        const int b0 = (int)w * 16;
        uint32_t v = 0;
        if (b0 < len && nw) {
            int src = rc ? len - 1 - b0 : b0;
            // the window holding the first source base: the last one that starts at or before it (empty windows share their start
            // with the next one), then step window by window
            uint32_t g = 0, hi = nw;
            while (hi - g > 1) { const uint32_t mid = (g + hi) >> 1; if (LB(mid) <= src) g = mid; else hi = mid; }
            for (int j = 0; j < 16 && b0 + j < len; j++) {
                uint32_t code = cwin[(size_t)(g0 + g) * FSV_CW_STRIDE + (src - LB(g))];
                if (rc) {
                    code = 3u - code;
                    src--;
                    while (g > 0 && src < LB(g)) g--;
                } else {
                    src++;
                    while (g + 1 < nw && src >= LB(g + 1)) g++;
                }
                v |= code << (2 * j);
            }
        }
        out[w0 + w] = v;
    }
}

// ------------------------------------------------------------------------------------------------ k_exact
// if_exact_match (Assembly.cpp:894-974): the two overlap intervals must be the same string.  One wavefront per unordered
// pair: the overlap of t on q covers the same bases as the overlap of q on t, so one comparison decides both slots.
// The comparison issues four 16-base fetches per lane before it looks at any of them (the early exit costs a memory
// round trip per test, and most valid overlaps of the final pass are exact).
// An exact overlap as the host layout reads it (32 B; q, t are read indices inside the set).
struct fsv_hit { uint32_t q, t; int32_t x_s, x_e, y_s, y_e; uint32_t rev, slot; };   // slot: the overlap slot; bit 31 set = exact

__global__ __launch_bounds__(64) void k_exact(const uint32_t *__restrict__ store, const uint32_t *__restrict__ word_off,
                                              const int32_t *__restrict__ read_len, const uint32_t *__restrict__ read_set,
                                              const uint32_t *__restrict__ pair_base, const uint4 *__restrict__ upair_tab,
                                              const fsv_ovl *__restrict__ ovl, fsv_hit *__restrict__ hits, uint32_t *__restrict__ set_hits,
                                              uint8_t *__restrict__ exact_flag)
{
    const uint4 pt = upair_tab[blockIdx.x];
    const int lane = threadIdx.x;
    fsv_ovl o = ovl[pt.z];
    if (lane == 0) exact_flag[blockIdx.x] = 0;
    if (!o.valid) return;
    const uint32_t rq = pt.x + o.q, rt = pt.x + o.t;
    const int L = o.x_e - o.x_s + 1;
    bool same = (L == o.y_e - o.y_s + 1);
    if (same) {
        const uint32_t xw = word_off[rq], yw = word_off[rt];
        const int ylen = read_len[rt];
        uint32_t acc = 0;
        for (int i0 = lane * 16; i0 < L; i0 += 4 * 64 * 16) {
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int i = i0 + u * 64 * 16;
                if (i < L) {
                    const uint32_t xb = fetch16_x(store, xw, o.x_s + i);
                    const Bases16 yb = fetch16(store, yw, ylen, o.rev, o.y_s + i);
                    uint32_t d = xb ^ yb.bits;
                    const int lim = min(16, L - i);
                    if (lim < 16) d &= (1u << (2 * lim)) - 1u;
                    acc |= d;
                }
            }
            if (__any(acc != 0u)) break;
        }
        same = !__any(acc != 0u);
    }
    if (!same) return;
    if (lane == 0) exact_flag[blockIdx.x] = 1;
    // exact hits are gathered per set for the host layout (a few per cent of the slots): the set's hit segment starts at its
    // first ordered-pair slot and a per-set counter hands out places -- one atomic per pair, spread over the sets' addresses
    const uint32_t s = read_set[pt.x];
    uint32_t at = 0;
    if (lane == 0) at = atomicAdd(&set_hits[s], 2u);
    at = __shfl(at, 0, 64);
    if (lane < 2) {
        const uint32_t slot = lane ? pt.w : pt.z;
        if (lane) o = ovl[slot];
        fsv_hit h; h.q = o.q; h.t = o.t; h.x_s = o.x_s; h.x_e = o.x_e; h.y_s = o.y_s; h.y_e = o.y_e; h.rev = o.rev; h.slot = slot | 0x80000000u;   // bit 31: an exact overlap (hifiasm's el)
        hits[pair_base[s] + at + lane] = h;
    }
}

// the per-set hit segments, packed back to back for one D2H copy: one block per set, 8 words per record
__global__ __launch_bounds__(256) void k_hits_compact(const fsv_hit *__restrict__ hits, const uint32_t *__restrict__ pair_base,
                                                      const uint32_t *__restrict__ hit_first, fsv_hit *__restrict__ out)
{
    const uint32_t s = blockIdx.x;
    const uint32_t n = (hit_first[s + 1] - hit_first[s]) * 8u;
    const uint32_t *src = (const uint32_t *)(hits + pair_base[s]);
    uint32_t *dst = (uint32_t *)(out + hit_first[s]);
    for (uint32_t i = threadIdx.x; i < n; i += 256) dst[i] = src[i];
}

// Inexact overlaps for the layout (update_overlaps, Assembly.cpp:975-1083 as called by worker_ov_final :1284-1306): a pair
// without an exact overlap whose overlap the last correction round verified is chained again with hifiasm's final bandwidth
// (0.001, gapped coordinates) and accepted per direction when strand and coordinates agree with the verified overlap (both
// ends of either read within 10 % of the longer span).
__global__ void k_inexact_list(const uint4 *__restrict__ upair_tab, const uint8_t *__restrict__ exact_flag, const fsv_ovl *__restrict__ prev,
                               uint32_t n_upairs, uint32_t *__restrict__ list, uint32_t *__restrict__ n_list)
{
    const uint32_t up = blockIdx.x * blockDim.x + threadIdx.x;
    if (up >= n_upairs || exact_flag[up]) return;
    const uint4 pt = upair_tab[up];
    const fsv_ovl a = prev[pt.z], b = prev[pt.w];
    if ((a.valid && a.is_match == 1) || (b.valid && b.is_match == 1)) list[atomicAdd(n_list, 1u)] = up;
}

__global__ void k_accept_inexact(const uint4 *__restrict__ upair_tab, const uint32_t *__restrict__ list, uint32_t n_list,
                                 const fsv_ovl *__restrict__ ovl, const fsv_ovl *__restrict__ prev, const uint32_t *__restrict__ read_set,
                                 const uint32_t *__restrict__ pair_base, fsv_hit *__restrict__ hits, uint32_t *__restrict__ set_hits,
                                 const uint32_t *__restrict__ n_dev = nullptr)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (n_dev) n_list = *n_dev;
    if (i >= 2 * n_list) return;
    const uint4 pt = upair_tab[list[i >> 1]];
    const uint32_t slot = (i & 1) ? pt.w : pt.z;
    const fsv_ovl o = ovl[slot], pv = prev[slot];
    if (!o.valid || !pv.valid || pv.is_match != 1 || pv.rev != o.rev) return;
    const int lx = pv.x_e - pv.x_s + 1, ly = pv.y_e - pv.y_s + 1, L = max(lx, ly) / 10;
    const bool ok = (abs(o.x_s - pv.x_s) < L && abs(o.x_e - pv.x_e) < L) || (abs(o.y_s - pv.y_s) < L && abs(o.y_e - pv.y_e) < L);
    if (!ok) return;
    const uint32_t s = read_set[pt.x];
    fsv_hit h; h.q = o.q; h.t = o.t; h.x_s = o.x_s; h.x_e = o.x_e; h.y_s = o.y_s; h.y_e = o.y_e; h.rev = o.rev; h.slot = slot;
    hits[pair_base[s] + atomicAdd(&set_hits[s], 1u)] = h;
}

// ------------------------------------------------------------------------------------------------ k_stitch
struct fsv_piece { uint32_t read; uint32_t rev; uint32_t len; uint32_t pad; uint64_t dst; };
__global__ __launch_bounds__(256) void k_stitch(const uint32_t *__restrict__ store, const uint32_t *__restrict__ word_off,
                                                const int32_t *__restrict__ read_len, const fsv_piece *__restrict__ pieces, char *__restrict__ out)
{
    const fsv_piece pc = pieces[blockIdx.x];
    const uint32_t w = word_off[pc.read];
    const int len = read_len[pc.read];
    for (uint32_t i = threadIdx.x; i < pc.len; i += blockDim.x) out[pc.dst + i] = "ACGT"[fsv_base_at(store, w, len, (int)pc.rev, (int)i)];
}

__global__ void k_unpack_reads(const uint32_t *__restrict__ store, const uint32_t *__restrict__ word_off, const int32_t *__restrict__ read_len,
                               const uint64_t *__restrict__ dst_off, char *__restrict__ out)
{
    const uint32_t r = blockIdx.x;
    const uint32_t w = word_off[r];
    const int len = read_len[r];
    for (int i = threadIdx.x; i < len; i += blockDim.x) out[dst_off[r] + i] = "ACGT"[fsv_base_fwd(store, w, i)];
}

} // namespace
