// fsv_internal.h -- shared by the HIP translation units of libfocalsv_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>
#include "focalsv_hip.h"

struct fsv_ctx {
    int device = -1;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int n_cu = 0;
    int clock_khz = 0;
    uint64_t hbm_bytes = 0;
    std::string name;
    std::string last_error;
    void *asm_ws = nullptr;                 // assembly workspace (asm.hip)
    void (*asm_ws_free)(fsv_ctx *) = nullptr;
    // contigs of the last fsv_assemble_batch, still on the device (ASCII, back to back) for a device-resident hand-off to the aligner
    const char *last_contigs_dev = nullptr;
    std::vector<uint64_t> last_contig_off;
    void *aln_ws = nullptr;                 // alignment workspace (aln.hip)
    void (*aln_ws_free)(fsv_ctx *) = nullptr;
    void *ref_ws = nullptr;                 // chromosome index and the workspace of fsv_contig_mapq (aln_mapq.h), or nothing
    void (*ref_ws_free)(fsv_ctx *) = nullptr;
};

#define FSV_HIP(ctx, call)                                                              \
    do {                                                                                \
        hipError_t e_ = (call);                                                         \
        if (e_ != hipSuccess) {                                                         \
            (ctx)->last_error = std::string(#call) + ": " + hipGetErrorString(e_);      \
            return (e_ == hipErrorOutOfMemory) ? FSV_ENOMEM : FSV_EHIP;                 \
        }                                                                               \
    } while (0)

static inline int fsv_fail(fsv_ctx *ctx, int code, const char *msg)
{
    if (ctx) ctx->last_error = msg;
    return code;
}

// ---- device helpers -----------------------------------------------------------------
// 2-bit read store: 16 bases per uint32 word (see focalsv_hip.h).
__device__ __forceinline__ uint32_t fsv_base_fwd(const uint32_t *__restrict__ store, uint32_t word_off, int pos)
{
    return (store[word_off + ((uint32_t)pos >> 4)] >> (((uint32_t)pos & 15u) << 1)) & 3u;
}

// base at strand coordinate p of a read of length len; rev = reverse complement strand.
__device__ __forceinline__ uint32_t fsv_base_at(const uint32_t *__restrict__ store, uint32_t word_off, int len, int rev, int p)
{
    int q = rev ? (len - 1 - p) : p;
    uint32_t b = fsv_base_fwd(store, word_off, q);
    return rev ? (3u - b) : b;
}

// wave-wide max, uniform result.  __shfl_xor goes through the LDS crossbar (ds_bpermute, ~6 dependent round trips);
// DPP row operations reduce each 16-lane row in four VALU ops and the four row results are read as scalars.
__device__ __forceinline__ int wave_max_i32(int v)
{
    const int lowest = -2147483647 - 1;
    v = max(v, __builtin_amdgcn_update_dpp(lowest, v, 0xB1, 0xF, 0xF, false));  // quad_perm [1,0,3,2]
    v = max(v, __builtin_amdgcn_update_dpp(lowest, v, 0x4E, 0xF, 0xF, false));  // quad_perm [2,3,0,1]
    v = max(v, __builtin_amdgcn_update_dpp(lowest, v, 0x141, 0xF, 0xF, false)); // row_half_mirror
    v = max(v, __builtin_amdgcn_update_dpp(lowest, v, 0x140, 0xF, 0xF, false)); // row_mirror
    const int a = __builtin_amdgcn_readlane(v, 0), b = __builtin_amdgcn_readlane(v, 16);
    const int c = __builtin_amdgcn_readlane(v, 32), d = __builtin_amdgcn_readlane(v, 48);
    return max(max(a, b), max(c, d));
}
__device__ __forceinline__ long long wave_max_i64(long long v)
{
    for (int off = 32; off > 0; off >>= 1) { long long o = __shfl_xor(v, off, 64); v = o > v ? o : v; }
    return v;
}

// inclusive prefix sum / prefix maximum over the wavefront's lanes
__device__ __forceinline__ int wave_incl_sum(int v, int lane)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const int o = __shfl_up(v, off, 64); if (lane >= off) v += o; }
    return v;
}
__device__ __forceinline__ int wave_incl_max(int v, int lane)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const int o = __shfl_up(v, off, 64); if (lane >= off) v = max(v, o); }
    return v;
}

// ---- block compaction: a thread's place among the 256 threads (four waves) of its block --------------------------------------------
// The four wave totals go through s_w (four words of LDS); returns what the waves in front of this one hold and sets *total to the
// block's sum.  One barrier inside, between the totals' store and their loads: whatever the block did before the call is done after
// it.  The caller puts a barrier between two calls on the same s_w.  wave_total counts on lane 63 only.
__device__ __forceinline__ uint32_t block_waves_before_256(uint32_t wave_total, uint32_t *s_w, uint32_t *total)
{
    const uint32_t wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 63u) s_w[wv] = wave_total;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (uint32_t v = 0; v < 4; v++) { const uint32_t c = s_w[v]; if (v < wv) before += c; all += c; }
    *total = all;
    return before;
}
// exclusive offset of this thread's count: a shuffle scan inside the wave in front of the wave totals
__device__ __forceinline__ uint32_t block_offset_256(uint32_t cnt, uint32_t *s_w, uint32_t *total)
{
    const uint32_t incl = (uint32_t)wave_incl_sum((int)cnt, (int)(threadIdx.x & 63u));
    return block_waves_before_256(incl, s_w, total) + incl - cnt;
}
// the one-bit case: the rank of a thread that keeps its element (for the others, the kept in front of them) from a ballot
__device__ __forceinline__ uint32_t block_rank_256(bool keep, uint32_t *s_w, uint32_t *total)
{
    const uint64_t bal = __ballot(keep);
    return block_waves_before_256((uint32_t)__popcll(bal), s_w, total) + (uint32_t)__popcll(bal & ((1ull << (threadIdx.x & 63u)) - 1ull));
}

// ---- an open-addressed set of 8-byte keys --------------------------------------------------------------------------------------------
// The k-mer count table's keys (k_kmer_insert) and the sketch's filter sets (k_flt_build, probed by the sketch kernels): slots
// [base, base + size) of a key array, size a power of two (or 0: no set), a free slot holds FSV_KMER_EMPTY, linear probing from bits of
// the key itself (it is mix64 output).  Every probe is bounded by the set's size.
#define FSV_KMER_EMPTY (~0ull)     // no key: hifiasm's dummy hash, which the sketch never emits
struct KmerSet {
    uint64_t base, size;
    __device__ __forceinline__ uint64_t start(uint64_t h) const { return (h ^ (h >> 29)) & (size - 1); }
    // is h a key?  The sets are at most half full, so a probe ends at a free slot after a step or two.
    __device__ __forceinline__ bool has(const unsigned long long *__restrict__ keys, uint64_t h) const
    {
        uint64_t slot = start(h);
        for (uint64_t probe = 0; probe < size; probe++) {
            const unsigned long long cur = keys[base + slot];
            if (cur == h) return true;
            if (cur == FSV_KMER_EMPTY) return false;
            slot = (slot + 1) & (size - 1);
        }
        return false;
    }
    // the slot that holds h, claimed now if nobody had: a 64-bit compare-and-swap against the empty value.  A slot only ever goes from
    // empty to one key, so a stale read of "empty" is settled by the compare-and-swap.  Returns `size` when the set is full.
    __device__ __forceinline__ uint64_t claim(unsigned long long *keys, uint64_t h) const
    {
        uint64_t slot = start(h);
        for (uint64_t probe = 0; probe < size; probe++) {
            unsigned long long cur = keys[base + slot];
            if (cur == FSV_KMER_EMPTY) { cur = atomicCAS(&keys[base + slot], FSV_KMER_EMPTY, h); if (cur == FSV_KMER_EMPTY) cur = h; }
            if (cur == h) return slot;
            slot = (slot + 1) & (size - 1);
        }
        return size;
    }
};

int fsv_live_contexts(int device);   // ctx.hip: contexts alive on a device

// the C entry points never let a C++ exception through (a std::bad_alloc from a vector sized by caller data, a std::system_error
// from a thread that could not start, would otherwise terminate a Python process that came in through ctypes)
#define FSV_GUARD(ctx, call)                                                            \
    try { return (call); }                                                              \
    catch (const std::bad_alloc &) { return fsv_fail(ctx, FSV_ENOMEM, "out of host memory"); } \
    catch (const std::exception &e) { if (ctx) (ctx)->last_error = std::string("exception: ") + e.what(); return FSV_EINTERNAL; } \
    catch (...) { return fsv_fail(ctx, FSV_EINTERNAL, "unknown exception"); }

static inline unsigned fsv_grid_for(uint64_t n, unsigned block) { return (unsigned)((n + block - 1) / block); }

#define TRY(x) do { int rc_ = (x); if (rc_ != FSV_OK) return rc_; } while (0)

// ---- device buffers -------------------------------------------------------------------
// A device allocation of elements of type T that only grows.  It owns its memory: the destructor frees it, so deleting a
// workspace frees its buffers.  cap is in bytes (what the chunking budget adds up); every count below is in elements.
template <class T> struct Dev {
    T *p = nullptr;
    size_t cap = 0;
    Dev() = default;
    Dev(const Dev &) = delete;
    Dev &operator=(const Dev &) = delete;
    ~Dev() { if (p) (void)hipFree(p); }
    void swap(Dev &o) { T *tp = p; p = o.p; o.p = tp; const size_t tc = cap; cap = o.cap; o.cap = tc; }
};

// room for n elements (an eighth more bytes, so that a slowly growing batch does not reallocate every call).  What the buffer
// held is lost when it grows; the stream is drained before the old allocation goes.
template <class T> int ensure(fsv_ctx *ctx, Dev<T> &b, size_t n)
{
    const size_t bytes = n * sizeof(T);
    if (bytes <= b.cap && b.p) return FSV_OK;
    if (b.p) { FSV_HIP(ctx, hipStreamSynchronize(ctx->stream)); FSV_HIP(ctx, hipFree(b.p)); b.p = nullptr; b.cap = 0; }
    const size_t want = bytes + bytes / 8 + 256;
    FSV_HIP(ctx, hipMalloc((void **)&b.p, want));
    b.cap = want;
    return FSV_OK;
}

// n host elements, or a vector, into the buffer (none still leaves a valid pointer behind: kernels are handed b.p whatever the count)
template <class T> int upload(fsv_ctx *ctx, Dev<T> &b, const T *host, size_t n)
{
    TRY(ensure(ctx, b, n ? n : 1));
    if (n) FSV_HIP(ctx, hipMemcpyAsync(b.p, host, n * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    return FSV_OK;
}
template <class T> int upload(fsv_ctx *ctx, Dev<T> &b, const std::vector<T> &v) { return upload(ctx, b, v.data(), v.size()); }

// the first n elements zeroed / copied to the host, on the context's stream
template <class T> int zero(fsv_ctx *ctx, Dev<T> &b, size_t n) { FSV_HIP(ctx, hipMemsetAsync(b.p, 0, n * sizeof(T), ctx->stream)); return FSV_OK; }
template <class T> int download(fsv_ctx *ctx, T *host, const Dev<T> &b, size_t n) { FSV_HIP(ctx, hipMemcpyAsync(host, b.p, n * sizeof(T), hipMemcpyDeviceToHost, ctx->stream)); return FSV_OK; }
// room for n elements in each of several buffers, in the order given
template <class... Ts> int ensure_each(fsv_ctx *ctx, size_t n, Dev<Ts> &...b) { int rc = FSV_OK; (void)(((rc = ensure(ctx, b, n)) == FSV_OK) && ...); return rc; }

// a kernel launch on a stream; every launch is checked on its own
#define FSV_LAUNCH(ctx, stream, kern, grid, block, lds, ...) \
    do { hipLaunchKernelGGL(kern, grid, block, lds, stream, __VA_ARGS__); FSV_HIP(ctx, hipGetLastError()); } while (0)

// ---- host clocks ----------------------------------------------------------------------
// wall-clock milliseconds of a stretch of work on the context's stream: both ends wait for the stream
struct Timer {
    std::chrono::steady_clock::time_point t0; fsv_ctx *ctx;
    explicit Timer(fsv_ctx *c) : ctx(c) { (void)hipStreamSynchronize(c->stream); t0 = std::chrono::steady_clock::now(); }
    double stop() { (void)hipStreamSynchronize(ctx->stream); return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};
// FSV_TRACE: the host's view of a pass, step by step, on stderr -- "[fsv] <who> <step> <ms since the last line>" (each line waits for the stream)
struct Trace {
    fsv_ctx *ctx = nullptr; const char *who = ""; std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void operator()(const char *what)
    {
        if (!getenv("FSV_TRACE")) return;
        (void)hipStreamSynchronize(ctx->stream);
        const auto t = std::chrono::steady_clock::now();
        fprintf(stderr, "[fsv] %s %-14s %.2f ms\n", who, what, std::chrono::duration<double, std::milli>(t - t0).count());
        t0 = t;
    }
};

// K5 with the task count left on the device (k5_bpm.hip): n_tasks sizes the grid, *n_dev is the count the kernel uses
// k_cap: the largest threshold of the batch's error model (31 = hifiasm's; above it every window goes through the wide-band kernel)
int fsv_bpm_windows_dev_n(fsv_ctx *ctx, const uint32_t *store_dev, const fsv_wtask *tasks_dev, uint32_t n_tasks, const uint32_t *n_dev,
                          fsv_wres *res_dev, int k_cap);
