// k_sketch.h -- minimizer sketch and per-read index: k_sketch (replay, even k), k_sketch_fast (position-parallel, odd k),
// k_uniq / k_uniq_walk / k_uniq_long.  Included by asm.hip (through asm_kernels.h) and by aln.hip; each of the two translation units gets its own
// copy of these kernels and of nothing else.
//
// The pieces the kernels share, each written once:
//   mz_pack / mz_unpack / mz_make   an fsv_mz as the (hash, pos | rev << 32 | span << 40) pair the LDS sorts move
//   mz_lower_bound                  a hash looked up in a hash-sorted list (the chain kernels of both translation units)
//   MzList, mz_emit                 a read's list in its slot: claim an entry, store the record or flag the truncation (both sketch kernels)
//   flt_set_of, flt_dummy           the read's filter set (KmerSet, fsv_internal.h) and "is this hash filtered"; nothing without FLT
//   bitonic_lds                     the bitonic network over a view (ByHashPos, ByPos: uniq_read's two arrays; LongTile: sort_long's records)
//   occurs_once, uniq_totals        the index's keep rule and its three statistics
//   block_offset_256 / block_rank_256 (fsv_internal.h)   a thread's place among the kept of its block
#pragma once
#include "fsv_internal.h"

#define FSV_UQ_MAX     4096  // minimizers per read sorted in LDS

namespace {

__device__ __forceinline__ uint64_t mix64(uint64_t key)
{
    key = ~key + (key << 21);
    key = key ^ key >> 24;
    key = (key + (key << 3)) + (key << 8);
    key = key ^ key >> 14;
    key = (key + (key << 2)) + (key << 4);
    key = key ^ key >> 28;
    key = key + (key << 31);
    return key;
}

// ------------------------------------------------------------------------------------------------ records and lists
__device__ __forceinline__ fsv_mz mz_make(uint64_t hash, uint32_t pos, uint32_t rev, uint32_t span)
{
    fsv_mz m; m.hash = hash; m.pos = pos; m.rev = (uint8_t)rev; m.span = (uint8_t)span; m.pad = 0;
    return m;
}
// pay = pos | rev << 32 | span << 40: its low word orders by position
__device__ __forceinline__ void mz_pack(const fsv_mz m, uint64_t *hash, uint64_t *pay) { *hash = m.hash; *pay = (uint64_t)m.pos | (uint64_t)m.rev << 32 | (uint64_t)m.span << 40; }
__device__ __forceinline__ fsv_mz mz_unpack(uint64_t hash, uint64_t pay) { return mz_make(hash, (uint32_t)pay, (uint8_t)(pay >> 32), (uint8_t)(pay >> 40)); }
// the first of the nt entries of a hash-sorted list whose hash is not below `hash` (nt: there is none)
__device__ __forceinline__ int mz_lower_bound(const fsv_mz *mt, const int nt, const uint64_t hash)
{
    int l2 = 0, h2 = nt;
    while (l2 < h2) { const int mid = (l2 + h2) >> 1; if (mt[mid].hash < hash) l2 = mid + 1; else h2 = mid; }
    return l2;
}

// a read's list while the sketch fills it: `cap` entries at out, the count (which runs past the cap when the list is cut) and the read's warning word
struct MzList { fsv_mz *out; uint32_t cap; uint32_t *cnt, *warn; };
__device__ __forceinline__ void mz_emit(const MzList &L, const fsv_mz rec)
{
    const uint32_t at = atomicAdd(L.cnt, 1u);
    if (at < L.cap) L.out[at] = rec;
    else atomicOr(L.warn, (uint32_t)FSV_W_MZ_TRUNC);
}

// ------------------------------------------------------------------------------------------------ the high-count k-mer filter
// hifiasm's ha_ft_isflt inside ha_sketch (sketch.cpp:89): an entry whose hash is in its read set's filter set is the dummy entry -- it
// keeps its slot in the window and is never a candidate.  One KmerSet (fsv_internal.h) per read set, back to back in HBM (k_flt_build,
// k_kmer.h): set s owns slots [off[s], off[s + 1]), a power of two or none.  The filter is a template parameter of the two sketch
// kernels: without it the view is an empty struct and the kernels hold no filter code.
template <bool FLT> struct FltView { static constexpr bool on = false; };
template <> struct FltView<true> {
    static constexpr bool on = true;
    const unsigned long long *keys; const uint64_t *off; const uint32_t *read_set;
    __device__ __forceinline__ KmerSet set_of(uint32_t r) const { const uint32_t s = read_set[r]; const uint64_t base = off[s]; return KmerSet{base, off[s + 1] - base}; }
};
struct SketchFilter { const unsigned long long *keys = nullptr; const uint64_t *off = nullptr; const uint32_t *read_set = nullptr; };   // host side; keys == nullptr: no filter
// the launch with or without the filter: fn is called with the view the kernel takes (its type names the instantiation)
template <class Fn> int with_filter(const SketchFilter &f, Fn fn) { return f.keys ? fn(FltView<true>{f.keys, f.off, f.read_set}) : fn(FltView<false>{}); }

// the filter set of read r's read set (no slots: no probe), and whether it turns hash h into the dummy
template <bool FLT> __device__ __forceinline__ KmerSet flt_set_of(const FltView<FLT> &F, uint32_t r)
{
    if constexpr (FLT) return F.set_of(r); else return KmerSet{0, 0};
}
template <bool FLT> __device__ __forceinline__ bool flt_dummy(const FltView<FLT> &F, const KmerSet &S, uint64_t h)
{
    if constexpr (FLT) return S.size && S.has(F.keys, h); else return false;
}

// ------------------------------------------------------------------------------------------------ k_sketch
// One wavefront per read.  The minimizer recurrence is sequential, but what it emits at a position only depends on
// the w entries around it (and on the k HPC bases behind them), so every lane replays the recurrence over its own 1/64
// of the read plus a warm-up of w+k+4 homopolymer runs in front and w+2 runs behind, and keeps only the minimizers whose
// end position falls inside its own slice.  Output order is arbitrary (k_uniq sorts).
//
// The reference keeps a w-slot ring and rescans it whenever the minimum slides out (two passes over w slots); in SIMT
// some lane rescans at almost every step, so the whole wave would pay ~2w LDS reads per step.  The replay therefore
// uses a monotone deque (hashes non-decreasing front to back, ties kept) that holds exactly the window elements which
// can still become a minimum.  ha_sketch emits an element exactly once iff it equals the minimum of some window that
// ends at or after the first full one -- as the "best" when that is replaced / slides out / the read ends, or as an
// "identical k-mer" copy when a rescan (or the first full window) finds it (sketch.cpp:101-135) -- so here an element
// is emitted the moment it joins the deque's front run.  The one irregular step is the first full window (l == w+k-1):
// copies of the previous partial window's minimum are emitted and that minimum itself is dropped silently if the
// incoming k-mer ties or beats it (sketch.cpp:101-106 run before 116-118 with l < w+k); replicated literally below.
// Dynamic LDS: [w x 64 hashes][read words][w x 64 pos|span][w x 64 time|flag|rev][64 x 64 run lengths, 16 bits each].
__host__ __device__ inline size_t sketch_lds_bytes(int w, uint32_t read_words) { return (size_t)read_words * 4 + (size_t)w * 64 * 14 + 64 * 64 * 2 + 16; }

struct WordCache { // sequential base access through one cached 16-base word
    const uint32_t *p; uint32_t w; int idx;
    __device__ __forceinline__ uint32_t get(int i) { const int wi = i >> 4; if (wi != idx) { w = p[wi]; idx = wi; } return (w >> ((i & 15) << 1)) & 3u; }
};

// One lane's monotone deque: its column of three arrays [w_max][64] in dynamic LDS (the pointers are the lane's column), entries
// (head + j) mod w, j < cnt.  The arrays are laid out for the launch's largest window while a lane wraps at its own w.
struct LaneDeque {
    uint64_t *hash;   // the entry's hash, NONE for a dummy
    uint32_t *ps;     // pos << 8 | span
    uint16_t *tf;     // (entry time & 0x3fff) << 2 | rev << 1 | emitted
    int w, head, cnt;
    __device__ __forceinline__ int slot(int j) const { const int x = head + j; return x >= w ? x - w : x; }
    __device__ __forceinline__ uint64_t hash_at(int sl) const { return hash[sl * 64]; }
    __device__ __forceinline__ uint64_t front() const { return hash[head * 64]; }
    // drop what has left the window of the last w entries (entry times modulo 2^14: windows are at most 64 entries long)
    __device__ __forceinline__ void expire(int tcur) { while (cnt > 0 && (((tcur - (int)(tf[head * 64] >> 2)) & 0x3fff) >= w)) { head = slot(1); cnt--; } }
    // keep hashes non-decreasing front to back (ties stay: they are the "identical k-mers")
    __device__ __forceinline__ void push(uint64_t h, uint32_t pos_span, int tcur, uint32_t rev)
    {
        while (cnt > 0 && hash_at(slot(cnt - 1)) > h) cnt--;
        const int sl = slot(cnt);
        hash[sl * 64] = h; ps[sl * 64] = pos_span; tf[sl * 64] = (uint16_t)((uint32_t)tcur << 2 | rev << 1);
        cnt++;
    }
    // entries at the front that share the front's hash (cnt > 0)
    __device__ __forceinline__ int front_run() const { const uint64_t m = front(); int run = 1; while (run < cnt && hash_at(slot(run)) == m) run++; return run; }
    __device__ __forceinline__ bool emitted(int sl) const { return tf[sl * 64] & 1u; }
    __device__ __forceinline__ void mark(int sl) { tf[sl * 64] = (uint16_t)(tf[sl * 64] | 1u); }
    __device__ __forceinline__ fsv_mz record(int sl) const { const uint32_t p = ps[sl * 64]; return mz_make(hash[sl * 64], p >> 8, (tf[sl * 64] >> 1) & 1u, p & 0xffu); }
};

// One lane's ring of the last k homopolymer run lengths (its column of [64][64] 16-bit words) and their sum, the k-mer's span.
// Lengths saturate at 256: exact up to 255 (with k = 1 a run of 255 is a minimizer of span 255), and one run of 256 or more puts the
// span at >= 256 (= no minimizer) whatever k is.
struct RunRing {
    uint16_t *q; int head, cnt, span;
    __device__ __forceinline__ int push(int run, int k)
    {
        const int rs = min(run, 256);
        q[((head + cnt++) & 63) * 64] = (uint16_t)rs;
        span += rs;
        if (cnt > k) { span -= q[head * 64]; head = (head + 1) & 63; cnt--; }
        return span;
    }
};

template <bool FLT>
__global__ __launch_bounds__(64) void k_sketch(const uint32_t *__restrict__ store, const uint32_t *__restrict__ word_off,
                                               const int32_t *__restrict__ read_len, const uint32_t *__restrict__ mz_off,
                                               fsv_mz *__restrict__ mz, uint32_t *__restrict__ mz_cnt, uint32_t n_reads, int w, int k,
                                               int hpc, uint32_t *__restrict__ warn, const uint8_t *__restrict__ w_per_read, int w_max,
                                               uint32_t lds_words, const FltView<FLT> F)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t s_dyn[];
    const int lane = threadIdx.x;
    const uint32_t r = blockIdx.x;
    if (r >= n_reads) return;
    const uint32_t woff = word_off[r];
    const int len = read_len[r];
    const MzList L{mz + mz_off[r], mz_off[r + 1] - mz_off[r], &mz_cnt[r], &warn[r]};
    if (w_per_read) w = w_per_read[r];
    [[maybe_unused]] const KmerSet fset = flt_set_of(F, r);
    uint64_t *d_hash = (uint64_t *)s_dyn;                               // [w_max][64]
    uint32_t *s_words = (uint32_t *)(d_hash + (size_t)w_max * 64);      // [lds_words]
    uint32_t *d_ps = s_words + lds_words;                               // [w_max][64]   pos << 8 | span
    uint16_t *d_tf = (uint16_t *)(d_ps + (size_t)w_max * 64);           // [w_max][64]   (time & 0x3fff) << 2 | rev << 1 | emitted
    uint16_t *q_run = d_tf + (size_t)w_max * 64;                        // [64][64]      run lengths, saturating at 256
    const uint32_t nwords = ((uint32_t)len + 15u) >> 4;
    const bool staged = nwords <= lds_words;
    if (staged) for (uint32_t i = lane; i < nwords; i += 64) s_words[i] = store[woff + i];
    __syncthreads();
    WordCache B{staged ? (const uint32_t *)s_words : store + woff, 0u, -1};
    // For even k palindromic k-mers are skipped (sketch.cpp:84), so a fixed warm-up cannot guarantee w entries: lane 0 then
    // replays the whole read from base 0 (exact, 64x less parallel; hifiasm's k = 51 and minimap2's 19 are odd and use k_sketch_fast).
    const bool single = (k & 1) == 0;
    const int c0 = single ? 0 : (int)((long long)len * lane / 64), c1 = single ? (lane == 0 ? len : 0) : (int)((long long)len * (lane + 1) / 64);
    if (c1 <= c0) return;
    int b0 = c0;
    if (hpc) {
        while (b0 > 0 && B.get(b0 - 1) == B.get(b0)) b0--;
        for (int n = 0; n < w + k + 4 && b0 > 0; n++) {
            b0--;
            const uint32_t c = B.get(b0);
            while (b0 > 0 && B.get(b0 - 1) == c) b0--;
        }
    } else {
        b0 = max(0, c0 - (w + k + 4));
    }
    const uint64_t NONE = ~0ull;
    const uint64_t mask = (1ull << k) - 1;
    uint64_t km0 = 0, km1 = 0, km2 = 0, km3 = 0;
    LaneDeque D{d_hash + lane, d_ps + lane, d_tf + lane, w, 0, 0};
    RunRing Q{q_run + lane, 0, 0, 0};
    int span = 0;
    int l = b0 > 0 ? w + k + 1 : 0; // past the start-up phase every "l >= ..." test of the reference holds
    int tail = -1;                  // runs still to replay once the slice is done
    // report the entry in slot sl if it ends inside the lane's slice; it counts as emitted either way
    auto emit_slot = [&](int sl) {
        const fsv_mz m = D.record(sl);
        if ((int)m.pos >= c0 && (int)m.pos < c1) mz_emit(L, m);
        D.mark(sl);
    };

    int i = b0;
    for (; i < len; i++) {
        if (i >= c1) { if (tail < 0) tail = w + 2; if (tail-- == 0) break; }
        const uint32_t c = B.get(i);
        uint64_t cur_h = NONE; uint32_t cur_ps = 0; uint32_t cur_rev = 0;
        if (hpc) {
            int run = 1;
            while (i + run < len && B.get(i + run) == c) run++;
            i += run - 1;
            span = Q.push(run, k);
        } else {
            span = l + 1 < k ? l + 1 : k;
        }
        km0 = (km0 << 1 | (uint64_t)(c & 1u)) & mask;
        km1 = (km1 << 1 | (uint64_t)(c >> 1)) & mask;
        km2 = km2 >> 1 | (uint64_t)(1u - (c & 1u)) << (k - 1);
        km3 = km3 >> 1 | (uint64_t)(1u - (c >> 1)) << (k - 1);
        if (km1 == km3) continue; // palindrome: not an entry (sketch.cpp:84)
        const int z = km1 < km3 ? 0 : 1;
        ++l;
        if (l >= k && span < 256) {
            cur_h = z ? mix64(km2) + mix64(km3) : mix64(km0) + mix64(km1);
            cur_ps = ((uint32_t)i << 8) | (uint32_t)span;
            cur_rev = (uint32_t)z;
            if (flt_dummy(F, fset, cur_h)) { cur_h = NONE; cur_ps = 0; cur_rev = 0; }   // a filtered k-mer: the dummy, in its slot
        }
        const int tcur = l & 0x3fff; // entry time, modulo 2^14
        D.expire(tcur);
        if (l == w + k - 1 && D.cnt > 0 && D.front() != NONE) {
            // first full window (only lanes that replay from base 0 get here): copies of the partial window's minimum
            // are emitted (sketch.cpp:101-106); the minimum itself is lost if the incoming k-mer ties or beats it (:116-118)
            const uint64_t m = D.front();
            const int run = D.front_run();
            for (int j = 0; j + 1 < run; j++) emit_slot(D.slot(j));
            if (cur_h <= m) D.mark(D.slot(run - 1));
        }
        D.push(cur_h, cur_ps, tcur, cur_rev);
        if (l >= w + k - 1) {
            const uint64_t m = D.front();
            if (m != NONE)
                for (int j = 0; j < D.cnt; j++) {
                    const int sl = D.slot(j);
                    if (D.hash_at(sl) != m) break;
                    if (!D.emitted(sl)) emit_slot(sl);
                }
        }
    }
    // a read shorter than one window: only the last minimum is reported (sketch.cpp:134-135)
    if (i >= len && l < w + k - 1 && D.cnt > 0 && D.front() != NONE) emit_slot(D.slot(D.front_run() - 1));
}

// ------------------------------------------------------------------------------------------------ the bitonic network in LDS
// Sorts the np elements (a power of two) behind a view with the block's 256 threads: one compare-exchange per thread and trip,
// pair t = (i, i | st), a barrier per step.  A view gives before(a, b) -- does element a go in front of element b -- and swap(a, b).
template <class View>
__device__ __forceinline__ void bitonic_lds(View v, const uint32_t np)
{
    for (uint32_t sz = 2; sz <= np; sz <<= 1)
        for (uint32_t st = sz >> 1; st > 0; st >>= 1) {
            for (uint32_t t = threadIdx.x; t < np / 2; t += 256) {
                const uint32_t i = ((t & ~(st - 1)) << 1) | (t & (st - 1)), j = i | st;
                const bool up = (i & sz) == 0;
                if (v.before(j, i) == up) v.swap(i, j);
            }
            __syncthreads();
        }
}
// uniq_read's pair of arrays by (hash, position).  The comparison is written without a branch on purpose: all four words are then read
// in front of it, in flight together, and the swap finds them in registers.  With `||` / `&&` the compiler reads the payloads under the
// tie only and the swap reads them again, a second trip to LDS for half of all pairs (k_uniq<8192> 14 % slower).
struct ByHashPos {
    uint64_t *hash, *pay;
    __device__ __forceinline__ bool before(uint32_t a, uint32_t b) const
    {
        const uint64_t ha = hash[a], hb = hash[b], pa = pay[a], pb = pay[b];
        return (ha < hb) | ((ha == hb) & ((uint32_t)pa < (uint32_t)pb));
    }
    __device__ __forceinline__ void swap(uint32_t a, uint32_t b) const { const uint64_t ha = hash[a], hb = hash[b], pa = pay[a], pb = pay[b]; hash[a] = hb; hash[b] = ha; pay[a] = pb; pay[b] = pa; }
};
// ... and by position, the ~0ull padding last: only the payload is read for the comparison, the hash on a swap
struct ByPos {
    uint64_t *hash, *pay;
    __device__ __forceinline__ bool before(uint32_t a, uint32_t b) const
    {
        const uint64_t pa = pay[a], pb = pay[b];
        if (pb == ~0ull) return pa != ~0ull;
        if (pa == ~0ull) return false;
        return (uint32_t)pa < (uint32_t)pb || ((uint32_t)pa == (uint32_t)pb && pa < pb);
    }
    __device__ __forceinline__ void swap(uint32_t a, uint32_t b) const { ByHashPos{hash, pay}.swap(a, b); }
};

// ------------------------------------------------------------------------------------------------ what the index keeps
// does the hash at i of a hash-sorted list of n occur once -- or, with max_occ > 1 (the aligner's second seeding of an oversize
// event), at most max_occ times?  hash_at(j): the hash at j
template <class HashAt>
__device__ __forceinline__ bool occurs_once(HashAt hash_at, uint32_t i, uint32_t n, uint32_t max_occ = 1u)
{
    const uint64_t h = hash_at(i);
    bool u = (i == 0 || hash_at(i - 1) != h) && (i + 1 >= n || hash_at(i + 1) != h);
    if (max_occ > 1u && !u) {
        uint32_t run = 1;
        for (uint32_t d = 1; d <= max_occ && i >= d && hash_at(i - d) == h; d++) run++;
        for (uint32_t d = 1; d <= max_occ && i + d < n && hash_at(i + d) == h; d++) run++;
        u = run <= max_occ;
    }
    return u;
}
// statistics of the launch: unique minimizers; minimizers the sketch produced; bases of the reads it sketched
__device__ __forceinline__ void uniq_totals(unsigned long long *total, uint32_t unique, uint32_t raw, uint32_t slot)
{
    atomicAdd(total, (unsigned long long)unique);
    atomicAdd(total + 3, (unsigned long long)raw);              // CT_MZRAW (asm.hip)
    atomicAdd(total + 4, (unsigned long long)(slot - 64u));     // CT_BASES: a slot holds len + 64 entries
}

// ------------------------------------------------------------------------------------------------ k_uniq
// One workgroup per read: bitonic sort of (hash, pos) in LDS, keep hashes that occur exactly once.
template <int UQ_MAX>
__device__ __forceinline__ void uniq_read(const uint32_t r, fsv_mz *__restrict__ mz, const uint32_t *__restrict__ mz_off, uint32_t *__restrict__ mz_cnt,
                                          uint32_t *__restrict__ warn, const uint32_t *__restrict__ only_changed, uint32_t lo_cnt, uint32_t hi_cnt,
                                          unsigned long long *__restrict__ total, const uint32_t max_occ = 1u)
{
    __shared__ uint64_t s_hash[UQ_MAX];
    __shared__ uint64_t s_pay[UQ_MAX]; // pos | rev << 32 | span << 40
    __shared__ uint32_t s_w[4];
    const int tid = threadIdx.x;
    if (only_changed && !only_changed[r]) return;   // lists of an unchanged read are already in place
    // The sort holds a read's list in LDS, so the kernel is instantiated for short and for long lists (many reads per CU for
    // the former) and launched once per size class: lo_cnt < raw count <= hi_cnt.  The small class runs first -- it replaces
    // the raw count by the unique count, which can only be smaller, so the large class skips what the small one has done.
    { const uint32_t raw = mz_cnt[r]; if (raw <= lo_cnt || raw > hi_cnt) return; }
    fsv_mz *a = mz + mz_off[r];
    const uint32_t slot_cap = mz_off[r + 1] - mz_off[r];
    uint32_t n = min(mz_cnt[r], slot_cap); // k_sketch counts past the cap when it truncates
    const uint32_t n_raw = n;
    if (n > UQ_MAX) { if (tid == 0) atomicOr(&warn[r], (uint32_t)FSV_W_MZ_TRUNC); n = UQ_MAX; }
    uint32_t np = 1;
    while (np < n) np <<= 1;
    for (uint32_t i = tid; i < np; i += 256) {
        if (i < n) mz_pack(a[i], &s_hash[i], &s_pay[i]);
        else { s_hash[i] = ~0ull; s_pay[i] = ~0ull; }
    }
    __syncthreads();
    bitonic_lds(ByHashPos{s_hash, s_pay}, np);
    // unique flags + block compaction (each thread owns a contiguous chunk; its survivors wait in registers until every
    // thread has read its chunk, because they move towards lower indices, i.e. into other threads' chunks)
    const uint32_t per = (n + 255) / 256;
    const uint32_t lo = min(n, tid * per), hi = min(n, lo + per);
    uint64_t kh[UQ_MAX / 256], kp[UQ_MAX / 256];
    uint32_t cnt = 0;
#pragma unroll
    for (uint32_t j = 0; j < UQ_MAX / 256; j++) {
        const uint32_t i = lo + j;
        if (i < hi && occurs_once([&](uint32_t x) { return s_hash[x]; }, i, n, max_occ)) { kh[cnt] = s_hash[i]; kp[cnt] = s_pay[i]; cnt++; }
    }
    uint32_t m;
    const uint32_t o0 = block_offset_256(cnt, s_w, &m);   // (its barrier: every chunk has been read)
    if (tid == 0) {
        mz_cnt[r] = m;
        if (total) uniq_totals(total, m, n_raw, slot_cap);
    }
#pragma unroll
    for (uint32_t j = 0; j < UQ_MAX / 256; j++)
        if (j < cnt) { s_hash[o0 + j] = kh[j]; s_pay[o0 + j] = kp[j]; }
    __syncthreads();
    // [0, m): sorted by hash (the "target" role: binary-searched)
    for (uint32_t i = tid; i < m; i += 256) a[i] = mz_unpack(s_hash[i], s_pay[i]);
    // [m, 2m): the same minimizers sorted by position (the "query" role: anchors then come out in query order and the
    // chain kernels need no per-pair sort)
    if (2 * m <= slot_cap) {
        uint32_t mp = 1;
        while (mp < m) mp <<= 1;
        for (uint32_t i = m + tid; i < mp; i += 256) { s_hash[i] = ~0ull; s_pay[i] = ~0ull; }
        __syncthreads();
        bitonic_lds(ByPos{s_hash, s_pay}, mp);
        for (uint32_t i = tid; i < m; i += 256) a[m + i] = mz_unpack(s_hash[i], s_pay[i]);
    } else if (tid == 0) atomicOr(&warn[r], (uint32_t)FSV_W_INTERNAL); // cannot happen: at most one minimizer per base and slots hold len + 64
}

template <int UQ_MAX>
__global__ __launch_bounds__(256) void k_uniq(fsv_mz *__restrict__ mz, const uint32_t *__restrict__ mz_off, uint32_t *__restrict__ mz_cnt,
                                              uint32_t *__restrict__ warn, const uint32_t *__restrict__ only_changed = nullptr,
                                              uint32_t lo_cnt = 0u, uint32_t hi_cnt = 0xffffffffu, unsigned long long *__restrict__ total = nullptr,
                                              uint32_t max_occ = 1u)
{
    uniq_read<UQ_MAX>(blockIdx.x, mz, mz_off, mz_cnt, warn, only_changed, lo_cnt, hi_cnt, total, max_occ);
}

// the same for a size class that is usually empty (lists above 1 024 entries in a HiFi batch): a few blocks walk all reads, so the
// 64 KB of LDS a block of this instantiation needs are claimed a few hundred times, not once per read (under three lanes the
// one-block-per-read launch averaged 2.8 ms against 0.01 alone: every block waited for LDS only to find its read in the other class)
template <int UQ_MAX>
__global__ __launch_bounds__(256) void k_uniq_walk(fsv_mz *__restrict__ mz, const uint32_t *__restrict__ mz_off, uint32_t *__restrict__ mz_cnt,
                                                   uint32_t *__restrict__ warn, const uint32_t *__restrict__ only_changed, uint32_t lo_cnt, uint32_t hi_cnt,
                                                   unsigned long long *__restrict__ total, uint32_t n_reads)
{
    for (uint32_t r = blockIdx.x; r < n_reads; r += gridDim.x) {
        uniq_read<UQ_MAX>(r, mz, mz_off, mz_cnt, warn, only_changed, lo_cnt, hi_cnt, total);
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ k_uniq_long (full_lists = 1)
// The third size class: lists above FSV_UQ_MAX entries, which no LDS tile holds.  A few blocks walk the reads as k_uniq_walk does and skip
// by count what the two classes in front have done (they leave such a list alone when the option is on).  A list is sorted tile by tile
// in LDS (bitonic_lds on 16-byte records), then the sorted tiles are merged pairwise through HBM, doubling the run
// length per pass: merge path -- every thread finds by binary search where its FSV_UQ_SEG outputs start in the two runs and merges them
// sequentially.  The passes go back and forth between the read's slot and the block's slab in the workspace (two buffers of the longest
// slot each: the slot's own tail would do as the second buffer only while 2n fits, and nothing bounds n below one entry per base), which
// stays in L2.  The sketch emits through an atomic counter, so the raw list is in no particular order: the position-sorted copy of the
// survivors is a second sort of the same kind, by position alone.  Hashes that occur once are found on the sorted list in HBM, so a run
// of equal hashes may straddle any tile or merge boundary.
#define FSV_UQ_SEG 16    // outputs per thread and merge step; divides every run length (multiples of FSV_UQ_MAX)
#define FSV_UQ_LONG_GRID 32

__device__ __forceinline__ uint64_t mz_hash(const uint4 e) { return (uint64_t)e.x | (uint64_t)e.y << 32; }
// the two orders: (hash, position), or position alone (positions are distinct inside a read, so both are total)
template <bool BY_POS> __device__ __forceinline__ bool mz_less(const uint4 a, const uint4 b)
{
    if (BY_POS) return a.z < b.z;
    const uint64_t ha = mz_hash(a), hb = mz_hash(b);
    return ha < hb || (ha == hb && a.z < b.z);
}
// sort_long's tile of records in either order
template <bool BY_POS> struct LongTile {
    uint4 *e;
    __device__ __forceinline__ bool before(uint32_t a, uint32_t b) const { return mz_less<BY_POS>(e[a], e[b]); }
    __device__ __forceinline__ void swap(uint32_t a, uint32_t b) const { const uint4 ea = e[a], eb = e[b]; e[a] = eb; e[b] = ea; }
};

// sorts a[0, n) with b[0, n) as the other buffer; returns the one that holds the result.  s_e: FSV_UQ_MAX records of LDS
template <bool BY_POS>
__device__ __forceinline__ uint4 *sort_long(uint4 *a, uint4 *b, const uint32_t n, uint4 *s_e)
{
    const uint32_t tid = threadIdx.x;
    for (uint32_t base = 0; base < n; base += FSV_UQ_MAX) {
        const uint32_t nt = min((uint32_t)FSV_UQ_MAX, n - base);
        uint32_t np = 1;
        while (np < nt) np <<= 1;
        for (uint32_t i = tid; i < np; i += 256) s_e[i] = i < nt ? a[base + i] : make_uint4(~0u, ~0u, ~0u, ~0u);   // (the dummy hash / no position: last in either order)
        __syncthreads();
        bitonic_lds(LongTile<BY_POS>{s_e}, np);
        for (uint32_t i = tid; i < nt; i += 256) a[base + i] = s_e[i];
        __syncthreads();
    }
    uint4 *src = a, *dst = b;
    for (uint32_t wd = FSV_UQ_MAX; wd < n; wd <<= 1) {
        __threadfence_block();
        __syncthreads();
        const uint32_t n_seg = (n + FSV_UQ_SEG - 1) / FSV_UQ_SEG;
        for (uint32_t g = tid; g < n_seg; g += 256) {
            const uint32_t o0 = g * FSV_UQ_SEG;
            const uint32_t lo = o0 & ~(2u * wd - 1u), mid = min(lo + wd, n), hi = min(lo + 2u * wd, n);   // runs [lo, mid) and [mid, hi)
            const uint32_t nx = mid - lo, ny = hi - mid, d = o0 - lo;
            const uint4 *X = src + lo, *Y = src + mid;
            // the split of output d: i entries of X and d - i of Y in front of it -- the smallest i with X[i] > Y[d - i - 1]
            uint32_t il = d > ny ? d - ny : 0u, ih = min(d, nx);
            while (il < ih) { const uint32_t i = (il + ih) >> 1; if (mz_less<BY_POS>(X[i], Y[d - i - 1])) il = i + 1; else ih = i; }
            uint32_t i = il, j = d - il;
            const uint32_t o1 = min(o0 + (uint32_t)FSV_UQ_SEG, hi);
            bool hx = i < nx, hy = j < ny;
            uint4 x = make_uint4(0, 0, 0, 0), y = x;
            if (hx) x = X[i];
            if (hy) y = Y[j];
            for (uint32_t o = o0; o < o1; o++) {
                const bool tx = hx && (!hy || mz_less<BY_POS>(x, y));
                dst[o] = tx ? x : y;
                if (tx) { i++; hx = i < nx; if (hx) x = X[i]; }
                else { j++; hy = j < ny; if (hy) y = Y[j]; }
            }
        }
        uint4 *t = src; src = dst; dst = t;
    }
    __threadfence_block();
    __syncthreads();
    return src;
}

// ws: FSV_UQ_LONG_GRID slabs of 2 x ws_stride records, ws_stride >= the longest slot of the batch
__global__ __launch_bounds__(256) void k_uniq_long(fsv_mz *mz, const uint32_t *__restrict__ mz_off, uint32_t *mz_cnt, uint32_t *__restrict__ warn,
                                                   const uint32_t *__restrict__ only_changed, unsigned long long *__restrict__ total, uint32_t n_reads,
                                                   uint4 *ws, uint32_t ws_stride, uint32_t *__restrict__ n_done)
{
    __shared__ uint4 s_e[FSV_UQ_MAX];
    __shared__ uint32_t s_w[4];
    const uint32_t tid = threadIdx.x;
    uint4 *const w0 = ws + (size_t)blockIdx.x * 2u * ws_stride, *const w1 = w0 + ws_stride;
    for (uint32_t r = blockIdx.x; r < n_reads; r += gridDim.x) {
        if (only_changed && !only_changed[r]) continue;   // lists of an unchanged read are already in place
        const uint32_t cap = mz_off[r + 1] - mz_off[r];
        const uint32_t raw = mz_cnt[r];
        if (raw <= FSV_UQ_MAX) continue;                   // the other two classes' (what they left is their unique count: smaller still)
        const uint32_t n = min(raw, cap);                  // k_sketch counts past the cap when it truncates
        if (n > ws_stride) { if (tid == 0) atomicOr(&warn[r], (uint32_t)FSV_W_INTERNAL); continue; }   // cannot happen: the host sizes the slabs from the slots
        uint4 *const slot = (uint4 *)(mz + mz_off[r]);
        const uint4 *S = sort_long<false>(slot, w0, n, s_e);
        // hashes that occur once, in hash order, to w1
        uint32_t m = 0;
        for (uint32_t base = 0; base < n; base += 256) {
            const uint32_t i = base + tid;
            const bool u = i < n && occurs_once([&](uint32_t x) { return mz_hash(S[x]); }, i, n);
            uint32_t all;
            const uint32_t at = block_rank_256(u, s_w, &all);
            if (u) w1[m + at] = S[i];
            m += all;
            __syncthreads();
        }
        __threadfence_block();
        __syncthreads();
        // [0, m): sorted by hash (the "target" role)
        for (uint32_t i = tid; i < m; i += 256) slot[i] = w1[i];
        // [m, 2m): the same minimizers sorted by position (the "query" role)
        const uint4 *P = sort_long<true>(w1, w0, m, s_e);
        if (2u * m <= cap) for (uint32_t i = tid; i < m; i += 256) slot[m + i] = P[i];
        else if (tid == 0) atomicOr(&warn[r], (uint32_t)FSV_W_INTERNAL);   // more than half a slot of unique minimizers: cannot happen (w <= 2 only, and the host then sizes the slots for it: mz_slots)
        if (tid == 0) {
            mz_cnt[r] = m;
            if (n_done) atomicAdd(n_done, 1u);   // statistics: lists this class indexed
            if (total) uniq_totals(total, m, n, cap);
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ k_sketch_fast
// Position-parallel form of ha_sketch (sketch.cpp:39-137) for odd k (hifiasm's 51, minimap2's 19): no sequential replay.
//   phase 0  hpc_compress: homopolymer compression in parallel: run ends are found per 16-base word, a block scan gives every kept
//            base its entry index; the compressed bases go to two bit planes, the run-end positions to an array
//            (per-read slices of an HBM scratch, L2-resident for the block that wrote them) -- the HpcPlanes view;
//   phase 1  stage_hashes: every entry's k-mer is cut out of the bit planes with funnel shifts (forward strand = bit-reversed,
//            reverse strand = complemented), hashed, and the span is a difference of two run-end positions;
//   phase 2  window_minima, start_anomaly, report: ha_sketch reports an entry iff it equals the minimum of some window of w entries
//            that ends at or after the first full one (as the window's "best" or as an identical-k-mer copy); window minima and the
//            test are brute-force scans of an LDS tile.  The irregular first full window (l == w+k-1: copies of the previous
//            partial window's minimum are reported, that minimum itself only if the incoming k-mer is larger) and reads
//            shorter than one window (only the last minimum) are handled explicitly.
// Equivalent to the monotone-deque replay in k_sketch (which stays for even k); both are checked against the oracle.
// The phases speak through two structs.  Whoever moves phase 0 off HBM replaces hpc_compress and the three accessors of HpcPlanes
// (span, cut, entry_hash).
#define SKF_T 1024
#define SKF_NW_MAX (SKF_T + 2 * 256)            // a tile with its halo of w - 1 entries on either side, w <= 255
#define SKF_V ((SKF_NW_MAX + 255) / 256)        // elements of the doubling passes per thread
#define SKF_NONE (~0ull)

// a read's entries after phase 0: entry e is the e-th kept base (the last base of its homopolymer run, or every base without compression)
template <bool FLT> struct HpcPlanes {
    uint32_t *ends;          // entry -> index of the run's last base
    uint32_t *low, *high;    // bit planes of the compressed bases, bit e = entry e (zeroed by the host)
    int k; uint64_t kmask; int hpc;
    int M;                   // entries
    FltView<FLT> F; KmerSet fset;   // the read set's filter set (no slots: no probe)
    // bases the k-mer that ends at entry e covers
    __device__ __forceinline__ int span(int e) const { return hpc ? (int)ends[e] - (e - k >= 0 ? (int)ends[e - k] : -1) : k; }
    // k consecutive plane bits starting at entry a (a >= 0), bit i = entry a+i
    __device__ __forceinline__ uint64_t cut(const uint32_t *pl, int a) const
    {
        const int wd = a >> 5, sh = a & 31;
        const uint64_t lo64 = (uint64_t)pl[wd] | (uint64_t)pl[wd + 1] << 32;
        uint64_t v = lo64 >> sh;
        if (sh) v |= (uint64_t)pl[wd + 2] << (64 - sh);
        return v & kmask;
    }
    // the hash of the k-mer that ends at entry e and its strand, or SKF_NONE for a dummy (no entry, span of 256 or more, filtered)
    __device__ __forceinline__ uint64_t entry_hash(int e, int *z_out) const
    {
        if (e < k - 1 || e >= M) return SKF_NONE;
        if (span(e) >= 256) return SKF_NONE;
        const uint64_t lo = cut(low, e - k + 1), hi = cut(high, e - k + 1);
        // forward strand: oldest base in the top bit; reverse strand: complement, oldest base in bit 0
        const uint64_t f0 = __brevll(lo) >> (64 - k), f1 = __brevll(hi) >> (64 - k);
        const uint64_t r0 = ~lo & kmask, r1 = ~hi & kmask;
        const int z = f1 < r1 ? 0 : 1;
        if (z_out) *z_out = z;
        const uint64_t h = mix64(z ? r0 : f0) + mix64(z ? r1 : f1);   // the strand is chosen first: two hashes per entry, not four
        // a filtered k-mer is the dummy, in its slot.  The probe's first load goes out as soon as the hash exists and hits a set of a few
        // KB that every block of the read set walks (L2); report() comes through here too, so what it writes has passed the filter
        if (flt_dummy(F, fset, h)) return SKF_NONE;
        return h;
    }
};

// the block's LDS: two tiles of 12 KB, the start anomaly, the short read's minimizer, the scan's wave totals
struct SkfTile {
    uint64_t h[SKF_NW_MAX];      // h[i]: hash of entry t0 - (w - 1) + i
    uint64_t wmin[SKF_NW_MAX];   // window minima, then the sliding maxima of the masked minima
    uint64_t am, ah;             // start anomaly: minimum of the partial window, hash of entry T0
    int abest, short_at;         // its rightmost position; the single minimizer of a read shorter than one window
    uint32_t scan[4];
};

// phase 0: fills P.ends / P.low / P.high and sets P.M
template <bool FLT>
__device__ __forceinline__ void hpc_compress(HpcPlanes<FLT> &P, SkfTile &T, const uint32_t *__restrict__ words, const int len)
{
    const int tid = threadIdx.x;
    const int nwords = (len + 15) >> 4;
    uint32_t carry = 0;   // entries in front of this trip's 256 words
    for (int wbase = 0; wbase < nwords; wbase += 256) {
        const int wi = wbase + tid;
        uint32_t flags = 0, word = 0;
        int nb = 0;
        if (wi < nwords) {
            word = words[wi];
            nb = min(16, len - wi * 16);
            if (P.hpc) {
                const uint32_t nextb = (wi + 1 < nwords) ? (words[wi + 1] & 3u) : 4u;
                // base j ends a run when it differs from base j+1 (the read's last base always does)
                const uint32_t shifted = (word >> 2) | (nextb << 30);
                uint32_t d = word ^ shifted;
                d = (d | (d >> 1)) & 0x55555555u; // field j non-zero <=> base j != base j+1
                // even bits -> 16-bit mask; the read's last base always ends a run
                d = (d | (d >> 1)) & 0x33333333u; d = (d | (d >> 2)) & 0x0f0f0f0fu; d = (d | (d >> 4)) & 0x00ff00ffu; d = (d | (d >> 8)) & 0xffffu;
                flags = nb >= 16 ? d : (d & ((1u << nb) - 1u));
                if (len - 1 - wi * 16 < 16) flags |= 1u << (len - 1 - wi * 16);
            } else flags = nb >= 16 ? 0xffffu : ((1u << nb) - 1u);
        }
        const uint32_t cnt = __popc(flags);
        uint32_t trip_total;
        const uint32_t base = carry + block_offset_256(cnt, T.scan, &trip_total);
        if (cnt) {
            uint32_t lo = 0, hi = 0, rank = 0;
            for (int j = 0; j < nb; j++)
                if ((flags >> j) & 1u) {
                    const uint32_t b = (word >> (2 * j)) & 3u;
                    lo |= (b & 1u) << rank; hi |= (b >> 1) << rank;
                    P.ends[base + rank] = (uint32_t)(wi * 16 + j);
                    rank++;
                }
            const uint32_t wd = base >> 5, sh = base & 31u;
            atomicOr(&P.low[wd], lo << sh); atomicOr(&P.high[wd], hi << sh);
            if (sh + cnt > 32) { atomicOr(&P.low[wd + 1], lo >> (32 - sh)); atomicOr(&P.high[wd + 1], hi >> (32 - sh)); }
        }
        carry += trip_total;
        __syncthreads();
    }
    P.M = (int)carry;
    __threadfence_block();
    __syncthreads();
}

// phase 1: T.h[i] = hash of entry e0 + i for the NW entries of a tile and its halo
template <bool FLT>
__device__ __forceinline__ void stage_hashes(const HpcPlanes<FLT> &P, SkfTile &T, const int e0, const int NW)
{
    for (int idx = threadIdx.x; idx < NW; idx += 256) T.h[idx] = P.entry_hash(e0 + idx, nullptr);
    __syncthreads();
}

// one doubling pass: T.wmin[i] = op(own[i], src[i + d]) for every i < NW.  Every thread keeps its own elements v[] in registers between
// the passes and only reads its partner's from the tile.
__device__ __forceinline__ void doubling_pass(SkfTile &T, uint64_t (&v)[SKF_V], const uint64_t *src, const int d, const bool is_max, const int NW)
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int c = 0; c < SKF_V; c++) {
        const int i = tid + 256 * c;
        if (i < NW) {
            const uint64_t b = i + d < NW ? src[i + d] : (is_max ? 0ull : SKF_NONE);
            v[c] = is_max ? max(v[c], b) : min(v[c], b);
        }
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < SKF_V; c++) { const int i = tid + 256 * c; if (i < NW) T.wmin[i] = v[c]; }
    __syncthreads();
}

// window minima: T.wmin[i] = min over entries (t0+i)-(w-1) .. (t0+i) = min(T.h[i .. i+w-1]), by doubling: after the
// pass with distance d an element covers 2d entries; two overlapping power-of-two ranges make the window of w (p2: the largest power of two <= w)
__device__ __forceinline__ void window_minima(SkfTile &T, uint64_t (&v)[SKF_V], const int NW, const int w, const int p2)
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int c = 0; c < SKF_V; c++) { const int i = tid + 256 * c; v[c] = i < NW ? T.h[i] : SKF_NONE; }
    if (w == 1) doubling_pass(T, v, T.h, 0, false, NW);
    else {
        doubling_pass(T, v, T.h, 1, false, NW);
        for (int d = 2; d < p2; d <<= 1) doubling_pass(T, v, T.wmin, d, false, NW);
        if (w > p2) doubling_pass(T, v, T.wmin, w - p2, false, NW);
    }
}

// the read's first tile (T.h[0] = entry e0): what the irregular start needs, found by thread 0
__device__ __forceinline__ void start_anomaly(SkfTile &T, const int M, const int T0, const int w, const int e0)
{
    if (threadIdx.x == 0) {
        T.short_at = -1; T.abest = -1; T.am = SKF_NONE; T.ah = SKF_NONE;
        if (M <= T0) { // shorter than one window: only the last minimum (rightmost on ties)
            uint64_t m = SKF_NONE; int bp = -1;
            for (int p = max(0, M - w); p < M; p++) { const uint64_t h = T.h[p - e0]; if (h != SKF_NONE && h <= m) { m = h; bp = p; } }
            T.short_at = bp;
        } else {
            uint64_t m = SKF_NONE; int bp = -1;
            for (int p = T0 - w + 1; p <= T0 - 1; p++) { const uint64_t h = T.h[p - e0]; if (h != SKF_NONE && h <= m) { m = h; bp = p; } }
            T.am = m; T.abest = bp; T.ah = T.h[T0 - e0];
        }
    }
}

// An entry is reported iff it equals the minimum of one of the windows that contain it and end in [T0, M-1]; every such
// minimum is <= the entry's hash, so the test is "sliding maximum of the (masked) window minima == hash", doubled the same way.
template <bool FLT>
__device__ __forceinline__ void report(const HpcPlanes<FLT> &P, SkfTile &T, uint64_t (&v)[SKF_V], const MzList &L, const int t0, const int T0, const int NW,
                                       const int w, const int p2)
{
    const int tid = threadIdx.x, M = P.M;
    if (M > T0) {
        // in place: every thread rewrites its own elements
#pragma unroll
        for (int c = 0; c < SKF_V; c++) {
            const int i = tid + 256 * c, t = t0 + i;
            if (i < NW && !(t >= T0 && t <= M - 1 && i < SKF_T + w - 1)) { T.wmin[i] = 0ull; v[c] = 0ull; }
        }
        __syncthreads();
        if (w > 1) {
            for (int d = 1; d < p2; d <<= 1) doubling_pass(T, v, T.wmin, d, true, NW);
            if (w > p2) doubling_pass(T, v, T.wmin, w - p2, true, NW);
        }
    }
    for (int pi = tid; pi < SKF_T; pi += 256) {
        const int p = t0 + pi;
        if (p >= M) break;
        const uint64_t hp = T.h[pi + (w - 1)];
        if (hp == SKF_NONE) continue;
        bool e;
        if (M <= T0) e = (p == T.short_at);
        else {
            e = (p + w - 1 >= T0) && T.wmin[pi] == hp;
            if (p >= T0 - w + 1 && p <= T0 - 1 && T.am != SKF_NONE && hp == T.am) e = (p != T.abest) ? true : (T.ah > T.am);
        }
        if (e) {
            int z = 0;
            const uint64_t h = P.entry_hash(p, &z);
            mz_emit(L, mz_make(h, P.ends[p], (uint32_t)z, (uint32_t)P.span(p)));
        }
    }
    __syncthreads();
}

template <bool FLT>
__global__ __launch_bounds__(256) void k_sketch_fast(const uint32_t *__restrict__ store, const uint32_t *__restrict__ word_off,
                                                     const int32_t *__restrict__ read_len, const uint32_t *__restrict__ mz_off,
                                                     fsv_mz *__restrict__ mz, uint32_t *__restrict__ mz_cnt, uint32_t n_reads, int w, int k,
                                                     int hpc, uint32_t *__restrict__ warn, const uint8_t *__restrict__ w_per_read,
                                                     uint32_t *__restrict__ sc_ends, uint32_t *__restrict__ sc_low, uint32_t *__restrict__ sc_high,
                                                     const uint32_t *__restrict__ only_changed, const FltView<FLT> F)
{
    __shared__ SkfTile T;
    const uint32_t r = blockIdx.x;
    if (r >= n_reads) return;
    // a read the last correction round left as it was keeps the minimizers of that round (same sequence, same slot)
    if (only_changed && !only_changed[r]) return;
    const uint32_t woff = word_off[r];
    const MzList L{mz + mz_off[r], mz_off[r + 1] - mz_off[r], &mz_cnt[r], &warn[r]};
    if (w_per_read) w = w_per_read[r];
    if (threadIdx.x == 0) mz_cnt[r] = 0;   // (the first emit comes after several barriers)
    // the read's slices of the scratch: 16 run ends per store word, plane words woff + r .. (one spare word per read in front)
    HpcPlanes<FLT> P{sc_ends + (size_t)woff * 16, sc_low + woff + r, sc_high + woff + r, k, (1ull << k) - 1, hpc, 0, F, flt_set_of(F, r)};
    hpc_compress(P, T, store + woff, read_len[r]);
    const int T0 = w + k - 2;               // entry index of the first full window (l == w+k-1)
    const int NW = SKF_T + 2 * (w - 1);     // a tile and its halo
    int p2 = 1;
    while (p2 * 2 <= w) p2 <<= 1;
    for (int t0 = 0; t0 < P.M; t0 += SKF_T) {
        const int e0 = t0 - (w - 1);        // entry held by T.h[0]
        stage_hashes(P, T, e0, NW);
        uint64_t v[SKF_V];
        window_minima(T, v, NW, w, p2);
        if (t0 == 0) start_anomaly(T, P.M, T0, w, e0);
        __syncthreads();
        report(P, T, v, L, t0, T0, NW, w, p2);
    }
}

// ------------------------------------------------------------------------------------------------ host: the sketch launch
// Sketches n_reads reads of `store` into W.mz / W.mz_cnt (W: a workspace with word_off, len, mz_off, mz, mz_cnt, warn uploaded or
// sized, and the scratch buffers sk_ends / sk_low / sk_high).  Odd k: the position-parallel kernel; even k, or replay: k_sketch.
struct SketchJob {
    const uint32_t *store; uint32_t n_reads; size_t total_words; uint32_t max_words;   // store words of all reads / of the longest one (the replay kernel's LDS tile)
    int w, k, hpc; const uint8_t *wper; int w_max;        // a window per read (or null) and the largest of them
    bool replay;                                          // k_sketch for an odd k as well
    const uint32_t *only_changed;                         // odd k: reads with a zero here keep their list and their count
    SketchFilter flt = {};                                // the read sets' filter sets, or nothing (the aligner, fsv_sketch_reads)
};
template <class Ws> int launch_sketch(fsv_ctx *ctx, Ws &W, const SketchJob &J)
{
    const bool fast = (J.k & 1) && !J.replay;
    if (!(fast && J.only_changed)) TRY(zero(ctx, W.mz_cnt, J.n_reads));   // (with only_changed the kernel zeroes the counts of the others itself)
    if (fast) {
        // per-read scratch for run ends (4 B / base) and two bit planes, planes zeroed per launch
        const size_t plane = J.total_words + J.n_reads + 8;
        TRY(ensure(ctx, W.sk_ends, J.total_words * 16 + 64));
        TRY(ensure_each(ctx, plane, W.sk_low, W.sk_high));
        TRY(zero(ctx, W.sk_low, plane));
        TRY(zero(ctx, W.sk_high, plane));
        return with_filter(J.flt, [&](auto F) -> int {
            FSV_LAUNCH(ctx, ctx->stream, k_sketch_fast<decltype(F)::on>, dim3(J.n_reads), dim3(256), 0, J.store, W.word_off.p, W.len.p, W.mz_off.p, W.mz.p,
                       W.mz_cnt.p, J.n_reads, J.w, J.k, J.hpc, W.warn.p, J.wper, W.sk_ends.p, W.sk_low.p, W.sk_high.p, J.only_changed, F);
            return FSV_OK;
        });
    }
    const uint32_t lds_words = J.max_words < 8192u ? J.max_words : 8192u;
    const size_t lds = sketch_lds_bytes(J.w_max, lds_words);
    return with_filter(J.flt, [&](auto F) -> int {
        FSV_HIP(ctx, hipFuncSetAttribute((const void *)k_sketch<decltype(F)::on>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        FSV_LAUNCH(ctx, ctx->stream, k_sketch<decltype(F)::on>, dim3(J.n_reads), dim3(64), lds, J.store, W.word_off.p, W.len.p, W.mz_off.p, W.mz.p, W.mz_cnt.p,
                   J.n_reads, J.w, J.k, J.hpc, W.warn.p, J.wper, J.w_max, lds_words, F);
        return FSV_OK;
    });
}

// ------------------------------------------------------------------------------------------------ host: the per-read index launch
// The unique-minimizer index of the lists launch_sketch left in W.mz / W.mz_cnt, one launch per size class.  The sort holds a read's
// minimizers in LDS (16 B per entry): one instantiation for lists up to 1 024 entries (many reads per CU), one for lists up to
// FSV_UQ_MAX; each launch skips the reads of the other classes by count, so the host need not know the longest list of the batch.
// full_lists: lists above FSV_UQ_MAX go to k_uniq_long instead of being cut there (W.uq_ws: its slabs, held only by such a call).
struct UniqJob {
    uint32_t n_reads, max_words;          // store words of the longest read: at most one minimizer per base, so shorter reads cannot have a longer list
    const uint32_t *only_changed;         // reads with a zero here keep their index
    unsigned long long *total;            // the launch's statistics (unique, raw, bases), or null
    bool full_lists; uint32_t max_slot, n_long;   // full_lists: the longest slot, the reads above FSV_UQ_MAX bases
    uint32_t *n_long_done;                // ... and a device counter of the lists k_uniq_long indexed, or null
};
// before_long: called in front of the third class's launch, when there is one (the assembly times that kernel on its own)
template <class Ws, class F> int launch_uniq(fsv_ctx *ctx, Ws &W, const UniqJob &J, F before_long)
{
    FSV_LAUNCH(ctx, ctx->stream, k_uniq<1024>, dim3(J.n_reads), dim3(256), 0, W.mz.p, W.mz_off.p, W.mz_cnt.p, W.warn.p, J.only_changed, 0u, 1024u, J.total);
    if (J.max_words * 16u > 1024u)
        FSV_LAUNCH(ctx, ctx->stream, k_uniq_walk<FSV_UQ_MAX>, dim3(std::min<uint32_t>(J.n_reads, 2u * (uint32_t)ctx->n_cu)), dim3(256), 0, W.mz.p, W.mz_off.p,
                   W.mz_cnt.p, W.warn.p, J.only_changed, 1024u, J.full_lists ? (uint32_t)FSV_UQ_MAX : 0xffffffffu, J.total, J.n_reads);
    if (J.full_lists && J.max_words * 16u > (uint32_t)FSV_UQ_MAX && J.n_long) {
        const uint32_t grid = std::min<uint32_t>(J.n_long, FSV_UQ_LONG_GRID);
        TRY(ensure(ctx, W.uq_ws, (size_t)grid * 2u * J.max_slot));
        before_long();
        FSV_LAUNCH(ctx, ctx->stream, k_uniq_long, dim3(grid), dim3(256), 0, W.mz.p, W.mz_off.p, W.mz_cnt.p, W.warn.p, J.only_changed, J.total, J.n_reads,
                   W.uq_ws.p, J.max_slot, J.n_long_done);
    }
    return FSV_OK;
}

} // namespace
