// k_path.h -- the K6 family of the per-read-set assembly: the window path record and its header view (PathHead), the gap-free placement
// (k_path_fast), the walk recorder and path_finish, and the walk kernels k_path_dp / k_path_sb / k_path_fr / k_path_wide.  Included by
// asm_kernels.h after its shared constants and PhaseClock; k_verify.h and k_consensus.h use its helpers.
#pragma once

namespace {

// ------------------------------------------------------------------------------------------------ K6 paths
// Fast paths of Reserve_Banded_BPM_PATH (Levenshtein_distance.h:516-531): err == 0, or a gap-free placement with
// exactly err mismatches (try_cigar).  Everything else is queued for one of the walk kernels.
struct PathLists {      // task lists and their device-side lengths: 0-2 k_path_fr<1..3>, 3 k_path_sb, 4 k_path_dp<32>, 5 k_path_dp<64>, 6 k_path_wide,
    uint32_t *list[8], *cnt[8];   // 7 (may be null): windows whose alignment may touch the edge of its band (k_fix_boundary looks at them again)
};
// The first 16 bytes of an fsv_wpath -- {ry_start, ry_end, path_len | err << 16, state | y_rev << 8 | pad << 16} -- as its readers take
// them: one 16-byte load, then fields.  The pad bits, which path_record sets: PAD_DEV_HEAD = an op other than a match among the path's
// first ten, PAD_DEV_TAIL = among its last ten -- what scan_cigar (Correct.cpp:1070) over ten columns from either end asks about
// (calculate_boundary_cigars :2360; k_bcig_tasks reads the header only); PAD_RAW0 = the alignment started in the padded window's first
// column before generate_cigar moved it (fix_boundary's question).
struct PathHead {
    static constexpr uint32_t PAD_DEV_HEAD = 1u, PAD_DEV_TAIL = 2u, PAD_RAW0 = 4u;
    uint4 h;
    static __device__ __forceinline__ PathHead load(const fsv_wpath *P) { return PathHead{*reinterpret_cast<const uint4 *>(P)}; }
    static __device__ __forceinline__ PathHead none() { return PathHead{make_uint4(0u, 0u, 0u, 0u)}; }
    __device__ __forceinline__ bool present() const { return (h.w & 0xffu) == 1u; }      // state 1: a path (0: none, 2: still queued)
    __device__ __forceinline__ int ry_start() const { return (int)h.x; }
    __device__ __forceinline__ int ry_end() const { return (int)h.y; }
    __device__ __forceinline__ int len() const { return (int)(int16_t)(h.z & 0xffffu); }
    __device__ __forceinline__ int err() const { return (int)(int16_t)(h.z >> 16); }     // the distance after generate_cigar
    __device__ __forceinline__ int y_rev() const { return (int)((h.w >> 8) & 0xffu); }
    __device__ __forceinline__ bool dev_head() const { return ((h.w >> 16) & PAD_DEV_HEAD) != 0u; }
    __device__ __forceinline__ bool dev_tail() const { return ((h.w >> 16) & PAD_DEV_TAIL) != 0u; }
    __device__ __forceinline__ bool raw0() const { return ((h.w >> 16) & PAD_RAW0) != 0u; }
};
// the 8 bytes behind them -- where read y lies in the store and how long it is -- for the readers that walk the ops
struct PathY {
    uint2 w;
    static __device__ __forceinline__ PathY load(const fsv_wpath *P) { return PathY{*reinterpret_cast<const uint2 *>((const uint8_t *)P + 16)}; }
    __device__ __forceinline__ uint32_t y_word() const { return w.x; }
    __device__ __forceinline__ int y_len() const { return (int)w.y; }
};
static_assert(offsetof(fsv_wpath, path_len) == 8 && offsetof(fsv_wpath, err) == 10 && offsetof(fsv_wpath, state) == 12 && offsetof(fsv_wpath, y_rev) == 13 &&
              offsetof(fsv_wpath, pad) == 14 && offsetof(fsv_wpath, y_word) == 16, "PathHead reads fsv_wpath's first 16 bytes");

// The record of a window's path, for the gap-free placement (path_gapfree) and for the walked paths (path_finish): the y interval
// [start, end] in padded-window columns, the distance after generate_cigar and plen ops, of which word(wd) gives the wd-th sixteen,
// start-to-end; tail10: the fields of the last ten ops.  with_ops false (path_gapfree, distance 0: every op a match): the record carries
// no ops -- its consumers (k_consensus, k_het) look at err first and never read them, and in the later correction rounds nearly every
// window is one: 24 bytes out instead of 128.
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
    P->pad = (uint16_t)((head10 ? PathHead::PAD_DEV_HEAD : 0u) | (tail10 ? PathHead::PAD_DEV_TAIL : 0u) | (raw0 ? PathHead::PAD_RAW0 : 0u)); P->y_word = t.y_word; P->y_len = t.y_len;
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
