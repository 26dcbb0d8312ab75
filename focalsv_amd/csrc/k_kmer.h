// k_kmer.h -- the per-set k-mer count table (hifiasm's ha_ft_gen / ha_analyze_count, htab.cpp:917-950, hist.cpp:15-96): the verdict on a
// count histogram (host and device), and the kernels that count a read set's sketch entries in an open-addressed table, take the
// histogram of the counts and gather the high-count keys.  The table's keys and the sketch's filter sets are the same open-addressed set,
// KmerSet (fsv_internal.h, with FSV_KMER_EMPTY): k_kmer_insert and k_flt_build claim a key's slot through it, the sketch kernels
// (k_sketch.h) look a hash up in it.  Included by asm.hip; the first part compiles without HIP (a plain C++ program can include this
// header for fsv_kmer_peaks_hd alone).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FSV_KMER_HD __host__ __device__
#else
#define FSV_KMER_HD
#endif

#define FSV_KMER_BINS 4096         // YAK_N_COUNTS: a count saturates at 4095 (YAK_MAX_COUNT)
#define FSV_KMER_START 5           // min_hist_kmer_cnt (CommandLines.cpp:126)
#define FSV_KMER_HIGH_FACTOR 5.0   // high_factor (CommandLines.cpp:132)

// The coverage peaks of a k-mer count histogram: hist[c] = distinct k-mers seen c times, c < n.  Returns the homozygous peak, or -1
// when the histogram never rises behind its lowest point (coverage too low to tell k-mers from errors); *peak_het: the heterozygous
// peak or -1; *low_i: the lowest point; *max_i: the highest peak behind it (-1 without one).  The caller has checked n >= 3 and
// start_cnt < n.
//   lowest point   from max(first, start_cnt) -- first = 1 if any k-mer occurs once, else 2 -- walk right while the histogram does not rise
//   highest peak   the largest bin right of the lowest point, the leftmost on ties
//   left peak      the largest local maximum (>= both neighbours) strictly between the two, the one nearest the highest peak on ties;
//                  dropped when it is below 5 % of the highest peak, or when the valley between them stays above 95 % of it
//   right peak     the largest local maximum right of the highest peak (the last bin aside), the leftmost on ties; dropped by the same
//                  two rules, or when it lies beyond 2.5 x the highest peak's count
// With a right peak the highest peak is the heterozygous one and the right peak the homozygous; otherwise the highest peak is the
// homozygous one and a left peak, if any, the heterozygous.  The three rules compare in double arithmetic.
FSV_KMER_HD inline int fsv_kmer_peaks_hd(const int64_t *hist, int n, int start_cnt, int *peak_het, int *low_i, int *max_i)
{
    *peak_het = -1; *max_i = -1;
    const int first = hist[1] > 0 ? 1 : 2;
    int lo = first > start_cnt ? first : start_cnt;
    while (lo + 1 < n && hist[lo + 1] <= hist[lo]) lo++;
    *low_i = lo;
    if (lo == n - 1) return -1;
    int top = lo + 1;
    for (int i = lo + 2; i < n; i++) if (hist[i] > hist[top]) top = i;
    *max_i = top;
    const int64_t peak = hist[top];
    auto is_local_max = [&](int i) { return hist[i] >= hist[i - 1] && hist[i] >= hist[i + 1]; };
    // the lowest bin strictly between a and b, no higher than the highest peak
    auto valley = [&](int a, int b) { int64_t v = peak; for (int i = a + 1; i < b; i++) if (hist[i] < v) v = hist[i]; return v; };
    int left = -1;
    for (int i = top - 1; i > lo; i--) if (is_local_max(i) && (left < 0 || hist[i] > hist[left])) left = i;
    if (left > 0 && ((double)hist[left] < (double)peak * 0.05 || (double)valley(left, top) > (double)hist[left] * 0.95)) left = -1;
    int right = -1;
    for (int i = top + 1; i < n - 1; i++) if (is_local_max(i) && (right < 0 || hist[i] > hist[right])) right = i;
    if (right > 0 && ((double)hist[right] < (double)peak * 0.05 || (double)valley(top, right) > (double)hist[right] * 0.95 || (double)right > (double)top * 2.5)) right = -1;
    if (right > 0) { *peak_het = top; return right; }
    *peak_het = left;
    return top;
}

// the count from which a k-mer is filtered: (int)(peak_hom x 5.0), at most 4094; -5 without a peak, which filters every k-mer
FSV_KMER_HD inline int fsv_kmer_cutoff(int peak_hom)
{
    const int c = (int)(peak_hom * FSV_KMER_HIGH_FACTOR);
    return c > FSV_KMER_BINS - 2 ? FSV_KMER_BINS - 2 : c;
}

#if defined(__HIPCC__)
#include "fsv_internal.h"

#define FSV_KMER_MIN_SLOTS 1024u   // smallest table
#define FSV_KMER_TILE 4096u        // slots a block of k_kmer_hist / k_kmer_filter walks
#define FSV_KMER_E_FULL 1u         // error flags: a table had no free slot; a filter segment was too short
#define FSV_KMER_E_FLT 2u

namespace {

// slots of a set's table: a power of two, at least twice its entries (0 for a set without entries)
inline uint64_t kmer_table_slots(uint64_t entries)
{
    if (entries == 0) return 0;
    uint64_t n = FSV_KMER_MIN_SLOTS;
    while (n < 2 * entries) n <<= 1;
    return n;
}

// One block per read: every entry of the read's sketch (W.mz, in whatever order the sketch kernel left them) is counted in the table of
// the read's set -- the KmerSet in slots [tab_off[s], tab_off[s + 1]).  A key is claimed (KmerSet::claim: linear probing from the hash's
// own bits, a 64-bit compare-and-swap against the empty value), its count bumped with an atomic add and clamped when read, so thousands of
// adds on one slot (a tandem array) stay exact.  Which slot a key lands in depends on the order of arrival; what is read out of
// the table (histogram, filter set) does not.  The probe is bounded by the table's size: a full table raises FSV_KMER_E_FULL.
__global__ __launch_bounds__(256) void k_kmer_insert(const fsv_mz *__restrict__ mz, const uint32_t *__restrict__ mz_off, const uint32_t *__restrict__ mz_cnt,
                                                     const uint32_t *__restrict__ read_set, const uint64_t *__restrict__ tab_off,
                                                     unsigned long long *keys, uint32_t *cnt, uint32_t n_reads, uint32_t *err)
{
    const uint32_t r = blockIdx.x;
    if (r >= n_reads) return;
    const uint32_t s = read_set[r];
    const KmerSet T{tab_off[s], tab_off[s + 1] - tab_off[s]};
    const uint32_t n = min(mz_cnt[r], mz_off[r + 1] - mz_off[r]);   // (the sketch counts past the slot when it truncates)
    if (n && T.size == 0) { if (threadIdx.x == 0) atomicOr(err, FSV_KMER_E_FULL); return; }
    const fsv_mz *a = mz + mz_off[r];
    for (uint32_t i = threadIdx.x; i < n; i += 256) {
        const unsigned long long h = a[i].hash;
        if (h == FSV_KMER_EMPTY) continue;
        const uint64_t slot = T.claim(keys, h);
        if (slot < T.size) atomicAdd(&cnt[T.base + slot], 1u); else atomicOr(err, FSV_KMER_E_FULL);
    }
}

// a tile of a set's table: slots [tab_off[set] + first, ... + first + len)
struct KmerTile { uint32_t set, len; uint64_t first; };

// One block per tile: the 4 096-bin histogram of the tile's clamped counts in LDS (16 KB), then added to the set's histogram.
__global__ __launch_bounds__(256) void k_kmer_hist(const KmerTile *__restrict__ tiles, const uint64_t *__restrict__ tab_off,
                                                   const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ cnt, uint32_t *__restrict__ hist)
{
    __shared__ uint32_t s_hist[FSV_KMER_BINS];
    const KmerTile t = tiles[blockIdx.x];
    for (uint32_t b = threadIdx.x; b < FSV_KMER_BINS; b += 256) s_hist[b] = 0;
    __syncthreads();
    const uint64_t at = tab_off[t.set] + t.first;
    for (uint32_t i = threadIdx.x; i < t.len; i += 256)
        if (keys[at + i] != FSV_KMER_EMPTY) atomicAdd(&s_hist[min(cnt[at + i], (uint32_t)(FSV_KMER_BINS - 1))], 1u);
    __syncthreads();
    uint32_t *out = hist + (size_t)t.set * FSV_KMER_BINS;
    for (uint32_t b = threadIdx.x; b < FSV_KMER_BINS; b += 256) { const uint32_t v = s_hist[b]; if (v) atomicAdd(&out[b], v); }
}

// One block per tile: the keys whose clamped count reaches the set's cutoff go to the set's segment of the filter list,
// [flt_off[s], flt_off[s + 1]) -- sized by the host from the histogram, so the cursor ends exactly at the segment's length.  Order inside
// a segment is arrival order (the host sorts what it hands out).
__global__ __launch_bounds__(256) void k_kmer_filter(const KmerTile *__restrict__ tiles, const uint64_t *__restrict__ tab_off,
                                                     const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ cnt,
                                                     const int32_t *__restrict__ cutoff, const uint64_t *__restrict__ flt_off, uint32_t *__restrict__ cursor,
                                                     unsigned long long *__restrict__ flt, uint32_t *err)
{
    const KmerTile t = tiles[blockIdx.x];
    const uint64_t at = tab_off[t.set] + t.first;
    const int32_t cut = cutoff[t.set];
    const uint64_t seg = flt_off[t.set], seg_len = flt_off[t.set + 1] - seg;
    for (uint32_t i = threadIdx.x; i < t.len; i += 256) {
        const unsigned long long key = keys[at + i];
        if (key == FSV_KMER_EMPTY || (int32_t)min(cnt[at + i], (uint32_t)(FSV_KMER_BINS - 1)) < cut) continue;
        const uint32_t o = atomicAdd(&cursor[t.set], 1u);
        if (o < seg_len) flt[seg + o] = key; else atomicOr(err, FSV_KMER_E_FLT);
    }
}

// slots of a set's filter set (what the sketch kernels probe, k_sketch.h): a power of two, at least twice its filtered keys; none
// for a set with an empty filter, whose reads then probe nothing
inline uint64_t flt_set_slots(uint64_t keys)
{
    if (keys == 0) return 0;
    uint64_t n = 2;
    while (n < 2 * keys) n <<= 1;
    return n;
}

// One thread per key of the sets' filter lists (flt, segments [flt_off[s], flt_off[s + 1]), any order, duplicates allowed): the key is
// claimed in its set's slots [set_off[s], set_off[s + 1]) of `keys` -- all FSV_KMER_EMPTY before the launch -- as k_kmer_insert claims
// one (KmerSet::claim; where the key lands is of no interest here).  The probe is bounded by the set's size;
// a set that ran full (the host sized it wrongly) or a list that holds the empty value raises FSV_KMER_E_FULL.  A set whose slot range
// is empty while its list is not is one the host leaves unfiltered: its keys are passed over.
__global__ __launch_bounds__(256) void k_flt_build(const unsigned long long *__restrict__ flt, const uint64_t *__restrict__ flt_off,
                                                   const uint64_t *__restrict__ set_off, uint32_t n_sets, unsigned long long *keys, uint32_t *err)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= flt_off[n_sets]) return;
    uint32_t lo = 0, hi = n_sets;              // the set whose segment holds key i: the last s with flt_off[s] <= i
    while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (flt_off[mid] <= i) lo = mid; else hi = mid; }
    const KmerSet S{set_off[lo], set_off[lo + 1] - set_off[lo]};
    const unsigned long long h = flt[i];
    if (S.size == 0) return;                  // a set the host gave no slots (left unfiltered) takes no keys
    if (h == FSV_KMER_EMPTY || S.claim(keys, h) == S.size) atomicOr(err, FSV_KMER_E_FULL);
}

} // namespace
#endif // __HIPCC__
