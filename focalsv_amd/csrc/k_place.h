// k_place.h -- chromosome-level mapping quality of contig alignment records (fsv_ref_index_*, fsv_contig_mapq; opt-in).  Included by
// aln.hip only; the host path is aln_mapq.h.
//
//   k_ref_tiles     a chunk of tiles (REF_TILE owned k-mer ends each, REF_HALO bases of context on either side) copied out of the packed
//                   chromosome into a store of their own: the sketch kernel addresses its scratch by store word, and neighbouring tiles overlap
//   k_ref_keep      ownership and N tests on a chunk's sketch; the survivors appended to the entry list (hash, pos | rev << 31)
//   k_ref_count     every entry claims its key's slot (KmerSet::claim, as k_kmer_insert does) and counts itself there
//   k_ref_offsets   exclusive scan of the stored counts over the slots (a key above max_occ keeps its slot and stores nothing); the statistics
//   k_ref_scatter   every entry of a stored key to its place behind the key's offset
//   k_ref_sort      a key's occurrences (at most REF_MAX_OCC) by position: what a lookup returns does not depend on the order of arrival
//   k_ref_lookup / k_ref_gather   the stage hook: counts and occurrences of caller-supplied hashes
//   k_place         one wavefront per alignment record: the record's minimizers looked up, their hits split into own locus / elsewhere forward /
//                   elsewhere reverse, the occurrence cutoff c*, and the best chain score of each class through ChainLds::chain_dp with the
//                   roles of the two coordinates swapped (anchors sorted reference-major)
#pragma once
#include "k_aln.h"

namespace {

#define REF_TILE 65536      // k-mer end positions a tile owns
#define REF_HALO 64         // bases sketched on either side of them (>= w + k - 1 for every (w, k) the index takes)
#define REF_MAX_OCC 64      // largest max_occ
#define REF_W_MAX 32        // largest w: a window of w k-mers fits in the halo
#define PLACE_QMAX 4096     // minimizers of a record before thinning

// the finished index as the kernels that read it see it
struct RefTable {
    const unsigned long long *keys; const uint32_t *cnt, *off, *occ; uint64_t slots; int max_occ;
    // the slot that holds h, or `slots` (no such key); never claims
    __device__ __forceinline__ uint64_t find(uint64_t h) const
    {
        if (h == FSV_KMER_EMPTY) return slots;
        const KmerSet S{0, slots};
        uint64_t slot = S.start(h);
        for (uint64_t probe = 0; probe < slots; probe++) {
            const unsigned long long cur = keys[slot];
            if (cur == h) return slot;
            if (cur == FSV_KMER_EMPTY) return slots;
            slot = (slot + 1) & (slots - 1);
        }
        return slots;
    }
};

// ------------------------------------------------------------------------------------------------ the build
// one thread per word of the chunk's store: tile j of the chunk starts at word src_word[j] of the chromosome's store
__global__ __launch_bounds__(256) void k_ref_tiles(const uint32_t *__restrict__ chrom, const uint32_t *__restrict__ src_word, const uint32_t *__restrict__ word_off,
                                                   uint32_t n_tiles, uint32_t total_words, uint32_t *__restrict__ words)
{
    const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= total_words) return;
    const uint32_t j = seq_of_word(word_off, n_tiles, w);
    words[w] = chrom[src_word[j] + (w - word_off[j])];
}

enum { REF_C_ENT = 0, REF_C_OWNED, REF_C_DROP_N, REF_C_KEYS, REF_C_ABOVE, REF_C_STORED, REF_C_MAXCNT, REF_C_ERR, REF_C_COUNT };

// One block per tile of the chunk.  tile_lo[j]: chromosome position of the tile's first base; own_lo[j]: the first k-mer end it owns (it owns
// REF_TILE of them).  A minimizer whose k bases cover an N (nm: the chromosome's mask, bit per base) is dropped.
__global__ __launch_bounds__(256) void k_ref_keep(const fsv_mz *__restrict__ mz, const uint32_t *__restrict__ mz_off, const uint32_t *__restrict__ mz_cnt,
                                                  const uint32_t *__restrict__ tile_lo, const uint32_t *__restrict__ own_lo, const uint32_t *__restrict__ nm,
                                                  int k, unsigned long long *__restrict__ ent_hash, uint32_t *__restrict__ ent_pos, uint32_t ent_cap,
                                                  uint32_t *__restrict__ counters)
{
    const uint32_t j = blockIdx.x;
    const fsv_mz *a = mz + mz_off[j];
    const uint32_t n = min(mz_cnt[j], mz_off[j + 1] - mz_off[j]);
    const uint32_t lo = tile_lo[j], o0 = own_lo[j];
    uint32_t owned = 0, dropped = 0;
    for (uint32_t i = threadIdx.x; i < n; i += 256) {
        const fsv_mz m = a[i];
        const uint32_t g = lo + m.pos;
        if (g < o0 || g - o0 >= (uint32_t)REF_TILE) continue;
        owned++;
        bool has_n = false;
        for (uint32_t wd = (g - (uint32_t)k + 1) >> 4; wd <= (g >> 4); wd++) {
            const uint32_t b0 = wd << 4;     // bits of this word inside [g - k + 1, g]
            const uint32_t first = max(b0, g - (uint32_t)k + 1) - b0, last = min(b0 + 15u, g) - b0;
            const uint32_t bits = (0xffffu >> (15u - last)) & (0xffffu << first);
            has_n |= (nm[wd] & bits) != 0;
        }
        if (has_n) { dropped++; continue; }
        const uint32_t at = atomicAdd(&counters[REF_C_ENT], 1u);
        if (at < ent_cap) { ent_hash[at] = m.hash; ent_pos[at] = g | (uint32_t)m.rev << 31; }
        else atomicOr(&counters[REF_C_ERR], 1u);
    }
    if (owned) atomicAdd(&counters[REF_C_OWNED], owned);
    if (dropped) atomicAdd(&counters[REF_C_DROP_N], dropped);
}

__global__ __launch_bounds__(256) void k_ref_count(const unsigned long long *__restrict__ ent_hash, uint32_t n_ent, unsigned long long *keys, uint64_t slots,
                                                   uint32_t *cnt, uint32_t *counters)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_ent) return;
    const KmerSet S{0, slots};
    const uint64_t slot = S.claim(keys, ent_hash[i]);
    if (slot < slots) atomicAdd(&cnt[slot], 1u); else atomicOr(&counters[REF_C_ERR], 2u);
}

// One block: off[slot] = stored occurrences of the slots in front of it, 2 048 slots a trip.
__global__ __launch_bounds__(256) void k_ref_offsets(const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ cnt, uint64_t slots, int max_occ,
                                                     uint32_t *__restrict__ off, uint32_t *__restrict__ counters)
{
    __shared__ uint32_t s_w[4];
    uint32_t carry = 0, n_keys = 0, n_above = 0, top = 0;
    for (uint64_t base = 0; base < slots; base += 2048) {
        const uint64_t s0 = base + (uint64_t)threadIdx.x * 8;
        uint32_t c[8], sum = 0;
#pragma unroll
        for (int e = 0; e < 8; e++) {
            c[e] = 0;
            if (s0 + e < slots && keys[s0 + e] != FSV_KMER_EMPTY) {
                const uint32_t v = cnt[s0 + e];
                n_keys++; top = max(top, v);
                if (v > (uint32_t)max_occ) n_above++; else c[e] = v;
            }
            sum += c[e];
        }
        uint32_t trip;
        uint32_t at = carry + block_offset_256(sum, s_w, &trip);
#pragma unroll
        for (int e = 0; e < 8; e++) if (s0 + e < slots) { off[s0 + e] = at; at += c[e]; }
        carry += trip;
        __syncthreads();
    }
    if (n_keys) atomicAdd(&counters[REF_C_KEYS], n_keys);
    if (n_above) atomicAdd(&counters[REF_C_ABOVE], n_above);
    atomicMax(&counters[REF_C_MAXCNT], top);
    if (threadIdx.x == 0) counters[REF_C_STORED] = carry;
}

__global__ __launch_bounds__(256) void k_ref_scatter(const unsigned long long *__restrict__ ent_hash, const uint32_t *__restrict__ ent_pos, uint32_t n_ent,
                                                     RefTable T, uint32_t *fill, uint32_t *__restrict__ occ, uint32_t *counters)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_ent) return;
    const uint64_t slot = T.find(ent_hash[i]);
    if (slot >= T.slots) { atomicOr(&counters[REF_C_ERR], 4u); return; }
    const uint32_t c = T.cnt[slot];
    if (c > (uint32_t)T.max_occ) return;
    const uint32_t at = atomicAdd(&fill[slot], 1u);
    if (at < c) occ[T.off[slot] + at] = ent_pos[i]; else atomicOr(&counters[REF_C_ERR], 4u);
}

// one thread per slot: insertion sort of its key's occurrences by position (a position holds one minimizer, so the order is total)
__global__ __launch_bounds__(256) void k_ref_sort(RefTable T, uint32_t *__restrict__ occ)
{
    const uint64_t slot = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (slot >= T.slots || T.keys[slot] == FSV_KMER_EMPTY) return;
    const uint32_t c = T.cnt[slot];
    if (c < 2 || c > (uint32_t)T.max_occ) return;
    uint32_t *a = occ + T.off[slot];
    for (uint32_t i = 1; i < c; i++) {
        const uint32_t v = a[i];
        uint32_t j = i;
        while (j > 0 && (a[j - 1] & 0x7fffffffu) > (v & 0x7fffffffu)) { a[j] = a[j - 1]; j--; }
        a[j] = v;
    }
}

// ------------------------------------------------------------------------------------------------ the stage hook
__global__ __launch_bounds__(256) void k_ref_lookup(const unsigned long long *__restrict__ hashes, uint32_t n, RefTable T, uint32_t *__restrict__ cnt_out,
                                                    uint32_t *__restrict__ src_off)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t slot = T.find(hashes[i]);
    cnt_out[i] = slot < T.slots ? T.cnt[slot] : 0u;
    src_off[i] = slot < T.slots ? T.off[slot] : 0u;
}
__global__ __launch_bounds__(256) void k_ref_gather(uint32_t n, RefTable T, const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ src_off,
                                                    const uint64_t *__restrict__ dst_off, uint32_t *__restrict__ out)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = cnt[i];
    if (c > (uint32_t)T.max_occ) return;
    for (uint32_t e = 0; e < c; e++) out[dst_off[i] + e] = T.occ[src_off[i] + e];
}

// ------------------------------------------------------------------------------------------------ k_place
// seq: the contig's list in mz / mz_off / mz_cnt; [q_lo, q_hi): the record's interval on the forward contig; [own_lo, own_hi): its interval on
// the chromosome; out: the record's index
struct PlaceTask { uint32_t seq; int32_t len, q_lo, q_hi, rev; uint32_t own_lo, own_hi, out; };
struct PlaceOut { int32_t f1, f2, m, cutoff, thin, flags; };

struct PlaceJob {
    PlaceTask K; const fsv_mz *a; int nq; uint32_t thin; RefTable T;
    // minimizer i of the contig's list, when it belongs to the record's query set and survives the thinning: its key's count and first
    // occurrence; false otherwise, or when the key is unknown or above max_occ
    __device__ __forceinline__ bool seed(int i, fsv_mz &m, uint32_t &c, uint32_t &o) const
    {
        if (i >= nq) return false;
        m = a[i];
        if ((int)m.pos < K.q_lo || (int)m.pos >= K.q_hi) return false;
        if (thin > 1 && (m.hash >> 11) % (uint64_t)thin != 0) return false;
        const uint64_t slot = T.find(m.hash);
        if (slot >= T.slots) return false;
        c = T.cnt[slot]; o = T.off[slot];
        return c >= 1 && c <= (uint32_t)T.max_occ;
    }
    // 0 the record's own locus, 1 elsewhere on the forward relative strand, 2 elsewhere on the reverse one
    __device__ __forceinline__ int cls(const fsv_mz &m, uint32_t v) const
    {
        const uint32_t p = v & 0x7fffffffu; const int rel = (int)(m.rev ^ (v >> 31));
        return (rel == K.rev && p >= K.own_lo && p < K.own_hi) ? 0 : 1 + rel;
    }
};

__global__ __launch_bounds__(64) void k_place(const PlaceTask *__restrict__ tasks, const fsv_mz *__restrict__ mz, const uint32_t *__restrict__ mz_off,
                                              const uint32_t *__restrict__ mz_cnt, RefTable T, PlaceOut *__restrict__ out, fsv_aln_params P)
{
    __shared__ ChainLds L;
    __shared__ int s_hist[3][REF_MAX_OCC];      // hits per class and count value (count c in column c - 1)
    const int lane = threadIdx.x;
    PlaceJob J;
    J.K = tasks[blockIdx.x]; J.T = T;
    J.a = mz + mz_off[J.K.seq];
    J.nq = (int)min(mz_cnt[J.K.seq], mz_off[J.K.seq + 1] - mz_off[J.K.seq]);
    // the query set and its thinning factor
    int n_q = 0;
    for (int base = 0; base < J.nq; base += 64) {
        const int i = base + lane;
        const bool in = i < J.nq && (int)J.a[i].pos >= J.K.q_lo && (int)J.a[i].pos < J.K.q_hi;
        n_q += __popcll(__ballot(in));
    }
    J.thin = (uint32_t)max(1, (n_q + PLACE_QMAX - 1) / PLACE_QMAX);
    for (int i = lane; i < 3 * REF_MAX_OCC; i += 64) (&s_hist[0][0])[i] = 0;
    __syncthreads();
    for (int base = 0; base < J.nq; base += 64) {
        fsv_mz m; uint32_t c = 0, o = 0;
        if (J.seed(base + lane, m, c, o))
            for (uint32_t e = 0; e < c; e++) atomicAdd(&s_hist[J.cls(m, T.occ[o + e])][c - 1], 1);
    }
    __syncthreads();
    // c*: lane c - 1 speaks for count value c
    bool ok = lane < T.max_occ;
    for (int cl = 0; cl < 3; cl++) ok = ok && wave_incl_sum(s_hist[cl][lane], lane) <= ALN_AMAX;
    const int cutoff = max(1, __popcll(__ballot(ok)));     // ok is a prefix of the lanes: the sums only grow
    int score[3] = {0, 0, 0}, m_own = 0;
    for (int cl = 0; cl < 3; cl++) {
        __syncthreads();
        int n = 0;
        for (int base = 0; base < J.nq; base += 64) {
            fsv_mz m; uint32_t c = 0, o = 0;
            const bool live = J.seed(base + lane, m, c, o) && (int)c <= cutoff;
            int mine = 0;
            if (live) for (uint32_t e = 0; e < c; e++) mine += J.cls(m, T.occ[o + e]) == cl;
            const int incl = wave_incl_sum(mine, lane);
            int at = n + incl - mine;
            if (mine) {
                for (uint32_t e = 0; e < c; e++) {
                    const uint32_t v = T.occ[o + e];
                    if (J.cls(m, v) != cl) continue;
                    // on the reverse relative strand the contig coordinate is that of the reverse complement (oracle/aln.c:204)
                    const int qp = (m.rev ^ (v >> 31)) ? (J.K.len - 1) - ((int)m.pos - (int)m.span + 1) : (int)m.pos;
                    if (at < ALN_AMAX) L.key[at] = (uint64_t)(v & 0x7fffffffu) << 32 | (uint32_t)qp;
                    at++;
                }
            }
            n += __shfl(incl, 63, 64);
        }
        n = min(n, ALN_AMAX);
        if (n == 0) continue;
        // reference-major order: the hits of a non-unique seed at one locus sit together, inside the DP's look-back
        int np = 1;
        while (np < n) np <<= 1;
        __syncthreads();
        for (int i = n + lane; i < np; i += 64) L.key[i] = ~0ull;
        __syncthreads();
        for (int sz = 2; sz <= np; sz <<= 1)
            for (int st = sz >> 1; st > 0; st >>= 1) {
                for (int t = lane; t < np / 2; t += 64) {
                    const int i = ((t & ~(st - 1)) << 1) | (t & (st - 1)), j = i | st;
                    const uint64_t x = L.key[i], y = L.key[j];
                    if ((y < x) == ((i & sz) == 0)) { L.key[i] = y; L.key[j] = x; }
                }
                __syncthreads();
            }
        const int best = L.chain_dp(n, lane, P);
        score[cl] = L.f[best];
        if (cl == 0) { int first; L.chain_len(best, lane, m_own, first); }
    }
    if (lane == 0) {
        PlaceOut o;
        o.f1 = score[0]; o.f2 = max(score[1], score[2]); o.m = m_own; o.cutoff = cutoff; o.thin = (int)J.thin;
        o.flags = cutoff < T.max_occ ? FSV_MQ_TRUNC : 0;
        out[J.K.out] = o;
    }
}

} // namespace
