// asm_kernels.h -- device kernels of the per-read-set assembly (gfx950).  Included by asm.hip.  This file holds the stage map, the
// constants the stages share and the small kernels around the correction rounds (k_newlen / k_repack, k_exact and the hit compaction,
// k_stitch, k_unpack_reads); it includes the stages' own files.
//
// Stage map (reference = hifiasm-0.14 under software/, restated in oracle/asm.c which these kernels
// must match bit for bit):
//   k_sketch          ha_sketch                                  sketch.cpp:39-137                                   k_sketch.h (shared with the aligner)
//   k_uniq            per-read index (hash occurs once)          htab.cpp:917-998 restated                           k_sketch.h
//   k_chain           anchors, chain_DP, extension, window list  anchor.cpp:60-178; Hash_Table.cpp:425-616, 83-243; Correct.cpp:306-531   k_chain.h
//   k5                Reserve_Banded_BPM                         Levenshtein_distance.h:274-461                      bpm_device.h
//   k_rescue_accept   recalcate_window_advance (right pass), 0.9 / 0.03 filters   Correct.cpp:2629-3023, 725         k_verify.h
//   k_path_fast/_dp   try_cigar, Reserve_Banded_BPM_PATH, generate_cigar          Levenshtein_distance.h:465-888; Correct.cpp:1302-1536   k_path.h
//   k_fix_boundary    fix_boundary                               Correct.cpp:1676-1795                               k_verify.h
//   k_left_rescue     recalcate_window_advance (left pass)       Correct.cpp:2745-2905                               k_verify.h
//   k_charge_*        non_trim_error_rate (opt-in)               Correct.cpp:725-845                                 k_verify.h
//   k_consensus       window_consensus / get_seq_from_Graph as a column vote       Correct.cpp:4010-4195             k_consensus.h
//   k_newlen/k_repack worker_ec_save (+ reverse complement)      Assembly.cpp:706-767                                here
//   k_exact           if_exact_match                             Assembly.cpp:894-974                                here
//   k_stitch          ma_ug_seq                                  Overlaps.cpp:8969-9034                              here
#pragma once
#include "bpm_device.h"
#include "k_sketch.h"

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

} // namespace
#include "k_chain.h"
#include "k_path.h"
#include "k_verify.h"
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
