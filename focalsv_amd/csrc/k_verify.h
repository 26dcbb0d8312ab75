// k_verify.h -- the kernels that give every overlap its verdict between K5 and the consensus: k_rescue_accept (right-extension rescue),
// fix_boundary / k_fix_boundary, k_left_rescue (left-extension rescue) and the partial charge (k_charge_tasks / k_bpm_ext /
// k_charge_accept), on one core: the compact overlap record (OvlC), the window sums, the retry of an unmatched window and the verdict.
// Included by asm_kernels.h after k_path.h, whose path_gapfree / path_general the left pass and fix_boundary call.
#pragma once

namespace {

// ------------------------------------------------------------------------------------------------ the core
// ovl_c: what the consensus needs of an overlap, 16 B instead of 56: {x_s, first window task, n_win | accepted << 31, -}.  A uint4 in
// memory; written by the verdicts below, cleared by k_hap_partition, read by the consensus family.
struct OvlC {
    static constexpr uint32_t ACCEPTED = 0x80000000u;
    uint4 v;
    static __device__ __forceinline__ OvlC of(const fsv_ovl &o, bool accepted)
    {
        return OvlC{make_uint4((uint32_t)o.x_s, (uint32_t)o.first_win, (uint32_t)o.n_win | (accepted ? ACCEPTED : 0u), 0u)};
    }
    static __device__ __forceinline__ OvlC load(const uint4 *slot) { return OvlC{*slot}; }
    static __device__ __forceinline__ OvlC none() { return OvlC{make_uint4(0u, 0u, 0u, 0u)}; }
    __device__ __forceinline__ int x_s() const { return (int)v.x; }
    __device__ __forceinline__ uint32_t first_task() const { return v.y; }
    __device__ __forceinline__ int n_win() const { return (int)(v.z & ~ACCEPTED); }
    __device__ __forceinline__ bool accepted() const { return (v.z >> 31) != 0u; }
    static __device__ __forceinline__ void clear_accepted(uint4 *slot) { slot->z &= ~ACCEPTED; }
};

__device__ __forceinline__ int double_thr(int pre, int x_len, int k_cap)
{
    if (pre == 0 && x_len >= 4) pre = 1;
    int t = pre * 2;
    if (x_len >= 300 && t < k_cap) t = k_cap;
    if (t > k_cap) t = k_cap;
    return t;
}

// An unmatched window tried again (Correct.cpp:2655-2744 to the right, :2745-2905 to the left; the partial charge's extension tasks take
// the threshold alone): the doubled threshold, the new place on y, and K5's DP once more unless the padded window no longer covers the
// window's length.  r: the result, as K5 leaves one.
// WIDE: the batch's error model allows thresholds above 31 (k_cap up to 95): the re-runs go through the wide-band BPM
__device__ __forceinline__ void retry_threshold(fsv_wtask &u, int k_cap) { u.k = (uint8_t)double_thr(u.k, u.x_len, k_cap); }
enum Retry { RETRY_SKIPPED, RETRY_FAILED, RETRY_ALIGNED };     // not run; run without an alignment within the threshold; aligned
template <bool WIDE>
__device__ __forceinline__ Retry retry_window(const uint32_t *__restrict__ store, fsv_wtask &u, int y_start, int k_cap, fsv_wres &r)
{
    retry_threshold(u, k_cap);
    u.y_start = y_start;
    if (!bpm_window_geometry(u, r, k_cap)) return RETRY_SKIPPED;
    if ((u.x_len + 2 * u.k - r.extra_begin - r.extra_end) + u.k < u.x_len) return RETRY_SKIPPED;
    if (WIDE) { WideNoSink none; bpm_run_wide(store, u, r, none, k_cap); }
    else bpm_run(store, u, r, BpmNoSink());
    return r.err < 0 ? RETRY_FAILED : RETRY_ALIGNED;
}

// An overlap's windows summed up: matched length, total length, the matched windows' distances, the unmatched windows.  e: a window's
// distance -- K5's (fsv_wres) in the rescue kernels, the path header's in the partial charge -- or negative for an unmatched window.
struct WindowSums {
    int align = 0, n_bad = 0;
    long long tlen = 0, terr = 0;
    __device__ __forceinline__ void add(int x_len, int e)
    {
        tlen += x_len;
        if (e >= 0) { align += x_len; terr += e; } else n_bad++;
    }
    // an unmatched window that a retry aligned (window lengths never change)
    __device__ __forceinline__ void rescued(int x_len, int e) { align += x_len; terr += e; n_bad--; }
    // the error sum the 0.03 filter asks about: an unmatched window counts with its whole length
    __device__ __forceinline__ long long terr_charged() const { return terr + (tlen - align); }
};

// The verdict (Correct.cpp:2899-3021, 725): the 0.9 coverage filter and the 0.03 error-rate filter.  Sets the overlap's align_len,
// err_sum and is_match and returns its ovl_c record; the caller stores both.
// DEFER (fsv_asm_params.partial_charge): the error-rate test is left to k_charge_tasks / k_charge_accept, which need the windows' paths
// first -- an overlap that passes the 0.9 coverage filter gets is_match = 1 for K6's sake (k_path_fast gates on it) while its accepted
// bit in ovl_c stays clear; nothing but K6 runs between this verdict and the final one
template <bool DEFER>
__device__ __forceinline__ OvlC ovl_verdict(fsv_ovl &o, int align, long long tlen, long long terr, int accept_err_pm)
{
    o.align_len = align; o.err_sum = (int32_t)terr;
    const bool covered = (long long)(o.x_e - o.x_s + 1) * 9 <= (long long)align * 10;
    o.is_match = (covered && (DEFER || terr * 1000 <= tlen * accept_err_pm)) ? 1 : 0;
    return OvlC::of(o, o.is_match && !DEFER);
}

// One working lane per block with its scratch in LDS -- the walk's ops (PathWalk's array: the lane uses column 0) and the column words
// of its window (path_general<uint64_t, 1>) -- and a persistent grid over a device-side list: k_fix_boundary and k_left_rescue.  The walk
// back is a chain of dependent reads of that scratch, column after column -- 1.3 ms for a single window from HBM, whatever the number
// of entries listed (a few thousand in the first round, a dozen later); 40 us from LDS.
struct LaneScratch {
    uint32_t ops[PathWalk::WORDS][64];
    uint64_t cols[(FSV_WINDOW + 2) * 3];
};
template <class F>
__device__ __forceinline__ void for_listed(const uint32_t *__restrict__ list, const uint32_t *__restrict__ n_list_dev, F f)
{
    if (threadIdx.x != 0) return;
    const uint32_t n_list = *n_list_dev;
    for (uint32_t li = blockIdx.x; li < n_list; li += gridDim.x) f(list[li]);
}

// ------------------------------------------------------------------------------------------------ k_rescue_accept
// One lane per overlap slot: right-extension rescue of unmatched windows (Correct.cpp:2655-2744), then the verdict.
template <bool WIDE, bool DEFER = false>
__global__ __launch_bounds__(64) void k_rescue_accept(const uint32_t *__restrict__ store, fsv_ovl *__restrict__ ovl, uint32_t n_pairs,
                                                      fsv_wtask *__restrict__ tasks, fsv_wres *__restrict__ res,
                                                      unsigned long long *__restrict__ stat_cols, uint4 *__restrict__ ovl_c, int k_cap, int accept_err_pm,
                                                      uint32_t *__restrict__ left_list, uint32_t *__restrict__ n_left)
{
    const uint32_t p = blockIdx.x * 64 + threadIdx.x;
    if (p >= n_pairs) return;
    fsv_ovl o = ovl[p];
    if (!o.valid) { ovl_c[p] = OvlC::none().v; return; }
    fsv_wtask *T = tasks + o.first_win;
    fsv_wres *R = res + o.first_win;
    unsigned long long cols = 0;
    // one pass settles an overlap whose windows all matched (nearly all of them): aligned length, total length and error sum;
    // four windows per trip so that their loads are in flight together (a lane walks ~20 windows, a memory round trip each)
    WindowSums S;
#pragma unroll 4
    for (int j = 0; j < o.n_win; j++) S.add(T[j].x_len, R[j].err);
    for (int j = S.n_bad ? o.n_win - 1 : -1; j >= 0; j--) {
        if (R[j].err < 0) continue;
        int next = R[j].y_beg + R[j].end_site - R[j].extra_begin + 1;
        for (int k2 = j + 1; k2 < o.n_win && R[k2].err < 0; k2++) {
            fsv_wtask u = T[k2];
            if (next >= u.y_len) break;
            fsv_wres r;
            const Retry tried = retry_window<WIDE>(store, u, next, k_cap, r);
            if (tried != RETRY_SKIPPED) cols += u.x_len;
            if (tried != RETRY_ALIGNED) break;
            T[k2] = u; R[k2] = r;
            S.rescued(u.x_len, r.err);
            next = r.y_beg + r.end_site - r.extra_begin + 1;
        }
    }
    if (S.n_bad && left_list) {
        // an unmatched window left of a matched one: the left-extension pass (k_left_rescue) decides about this overlap
        bool left = false;
        for (int j = 1; j < o.n_win && !left; j++) left = R[j].err >= 0 && R[j - 1].err < 0;
        if (left) {
            left_list[atomicAdd(n_left, 1u)] = p;
            o.is_match = 0; ovl[p] = o;
            ovl_c[p] = OvlC::of(o, false).v;
            if (cols) atomicAdd(stat_cols, cols);
            return;
        }
    }
    const OvlC oc = ovl_verdict<DEFER>(o, S.align, S.tlen, S.terr_charged(), accept_err_pm);
    ovl[p] = o;
    ovl_c[p] = oc.v;
    if (cols) atomicAdd(stat_cols, cols);
}

// ------------------------------------------------------------------------------------------------ fix_boundary
// fix_boundary (Correct.cpp:1676-1795; for the windows' final cigars :2968 and in the left-extension pass :2858): an alignment that
// starts in the first column of its padded window, or ends in its last one, may have been cut off by the band -- the window is aligned
// once more with the band shifted by k towards that side (from the old region's first base / so that the x interval ends at the old
// alignment's last base), without a hint, and the new alignment stands when it has fewer errors.  t / r / the record at P: the window
// as K6 left it; they are replaced when the new alignment stands.  One lane, its scratch in LDS.
// oracle/asm.c:window_path is the same, statement for statement.
__device__ __forceinline__ void fix_boundary_dev(const uint32_t *__restrict__ store, fsv_wtask &t, fsv_wres &r, fsv_wpath *__restrict__ P, LaneScratch &s, int k_cap)
{
    const PathHead h = PathHead::load(P);
    if (!h.present() || r.err <= 0 || t.k > FSV_K_MAX || (r.extra_begin & 0x4000)) return;     // (bit 14 of extra_begin: moved once already)
    const int n = t.x_len, k = t.k, wlen = n + 2 * k;
    fsv_wtask t2 = t;
    if (h.raw0()) { if (r.extra_begin != 0) return; t2.y_start = r.y_beg; }
    else if (r.end_site == wlen - 1) { if (r.extra_end != 0) return; t2.y_start = (r.y_beg + r.end_site) - n + 1; }
    else return;
    fsv_wres r2;
    if (!bpm_window_geometry(t2, r2, k_cap)) return;
    if (r2.y_beg == r.y_beg) return;
    bpm_run(store, t2, r2, BpmNoSink());
    if (r2.err < 0 || r2.err >= r.err) return;
    path_general<uint64_t, 1>(store, t2, P, s.ops, 0, s.cols);
    r2.extra_begin = (int16_t)(r2.extra_begin | 0x4000);
    t = t2; r = r2;
}

// the candidates k_path_fast listed, one block each
__global__ __launch_bounds__(64) void k_fix_boundary(const uint32_t *__restrict__ store, const uint32_t *__restrict__ list, const uint32_t *__restrict__ n_list_dev,
                                                     fsv_wtask *__restrict__ tasks, fsv_wres *__restrict__ res, fsv_wpath *__restrict__ paths, int k_cap,
                                                     uint32_t *__restrict__ n_fixed)
{
    __shared__ LaneScratch s;
    for_listed(list, n_list_dev, [&](const uint32_t tid) {
        fsv_wtask t = tasks[tid];
        fsv_wres r = res[tid];
        const int y0 = t.y_start;
        fix_boundary_dev(store, t, r, paths + tid, s, k_cap);
        if (t.y_start != y0) { tasks[tid] = t; res[tid] = r; if (n_fixed) atomicAdd(n_fixed, 1u); }
    });
}

// ------------------------------------------------------------------------------------------------ k_left_rescue
// recalcate_window_advance's left pass (Correct.cpp:2745-2905), for the overlaps k_rescue_accept set aside: a matched window whose
// left neighbour is unmatched gets its path first -- its real start on y -- and the unmatched windows to its left are tried again one
// after the other, each placed so that it ends right in front of the window to its right, with the doubled threshold and its path at
// once (the next one needs its start).  Then the overlap is accepted or not, as k_rescue_accept does: a window whose path was
// computed here counts with its distance after generate_cigar, as in hifiasm.  One block (one working lane) per listed overlap;
// oracle/asm.c:align_overlaps (left_rescue) statement for statement.
// DEFER: as in ovl_verdict -- the 0.9 filter alone decides here, provisionally.
template <bool DEFER = false>
__global__ __launch_bounds__(64) void k_left_rescue(const uint32_t *__restrict__ store, fsv_ovl *__restrict__ ovl, const uint32_t *__restrict__ list,
                                                    const uint32_t *__restrict__ n_list_dev, fsv_wtask *__restrict__ tasks, fsv_wres *__restrict__ res,
                                                    fsv_wpath *__restrict__ paths, uint4 *__restrict__ ovl_c, int k_cap, int accept_err_pm)
{
    __shared__ LaneScratch s;
    for_listed(list, n_list_dev, [&](const uint32_t p) {
        fsv_ovl o = ovl[p];
        fsv_wtask *T = tasks + o.first_win;
        fsv_wres *R = res + o.first_win;
        fsv_wpath *PP = paths + o.first_win;
        long long post = 0;          // sum over the windows whose path was computed here of (distance after generate_cigar - K5's distance)
        // the window's path, as K6 and k_fix_boundary would leave it: its header
        auto window_path = [&](fsv_wtask &t, fsv_wres &r, fsv_wpath *P) {
            if (!path_gapfree(store, t, r, P, true)) path_general<uint64_t, 1>(store, t, P, s.ops, 0, s.cols);
            fix_boundary_dev(store, t, r, P, s, k_cap);
            return PathHead::load(P);
        };
        for (int j = 1; j < o.n_win; j++) {
            if (R[j].err < 0 || R[j - 1].err >= 0) continue;
            fsv_wtask tj = T[j];
            fsv_wres rj = R[j];
            const PathHead hj = window_path(tj, rj, PP + j);
            if (tj.y_start != T[j].y_start) { T[j] = tj; R[j] = rj; }      // (fix_boundary moved the window)
            if (!hj.present()) { R[j].err = -1; continue; }       // (a path longer than a record holds: the window is unused, as in window_path)
            post += hj.err() - rj.err;
            int total_y_end = hj.ry_start() - 1;
            for (int k2 = j - 1; k2 >= 0 && R[k2].err < 0; k2--) {
                fsv_wtask u = T[k2];
                if (total_y_end <= 0) break;
                fsv_wres r;
                if (retry_window<false>(store, u, total_y_end - (int)u.x_len + 1, k_cap, r) != RETRY_ALIGNED) break;
                const PathHead hk = window_path(u, r, PP + k2);
                if (!hk.present()) break;
                T[k2] = u; R[k2] = r;
                post += hk.err() - r.err;
                total_y_end = hk.ry_start() - 1;
            }
        }
        WindowSums S;
        for (int j = 0; j < o.n_win; j++) S.add(T[j].x_len, R[j].err);
        const OvlC oc = ovl_verdict<DEFER>(o, S.align, S.tlen, post + S.terr_charged(), accept_err_pm);
        ovl[p] = o;
        ovl_c[p] = oc.v;
    });
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
__device__ __forceinline__ bool charge_matched(const fsv_wres *R, const fsv_wpath *P, PathHead &h)
{
    h = PathHead::load(P);
    return R->err >= 0 && h.present();
}

__device__ __forceinline__ void charge_verdict(const ChargeArgs &A, uint32_t p, fsv_ovl &o, long long tlen, long long terr)
{
    const OvlC oc = ovl_verdict<false>(o, o.align_len, tlen, terr, A.accept_err_pm);
    A.ovl[p] = o;
    A.ovl_c[p] = oc.v;
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
    WindowSums S;
    for (int j = 0; j < o.n_win; j++) {
        PathHead h;
        S.add(T[j].x_len, charge_matched(R + j, PP + j, h) ? h.err() : -1);
    }
    if (!S.n_bad) { charge_verdict(A, p, o, S.tlen, S.terr); return; }
    o.is_match = 0;                           // until k_charge_accept has spoken
    A.ovl[p] = o;
    A.ovl_list[atomicAdd(A.n_ovl, 1u)] = p;
    atomicAdd(A.stats + CH_OVERLAPS, 1ull);
    atomicAdd(A.stats + CH_WINDOWS, (unsigned long long)S.n_bad);
    PathHead h, hl = PathHead::none();
    bool left = false, cur = charge_matched(R, PP, h);
    for (int j = 0; j < o.n_win; j++) {
        // h / cur: window j; hl / left: window j - 1; hr / right: window j + 1
        PathHead hr = PathHead::none();
        const bool right = j + 1 < o.n_win && charge_matched(R + j + 1, PP + j + 1, hr);
        if (!cur && R[j].y_beg >= 0) {
            fsv_wtask t = T[j];
            const int n = t.x_len, k0 = t.k;
            int yb0 = left ? hl.ry_end() + 1 : -1, yb1 = right ? hr.ry_start() - n : -1;
            if (yb0 < 0 && yb1 < 0) yb0 = yb1 = R[j].y_beg + k0 - R[j].extra_begin;
            if (yb0 < 0) yb0 = yb1;
            if (yb1 < 0) yb1 = yb0;
            const uint32_t tid = (uint32_t)o.first_win + (uint32_t)j;
            retry_threshold(t, A.k_cap);
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
    // (not WindowSums: the charge of an unmatched window depends on the running error total)
    long long tlen = 0, terr = 0, full = 0;
    for (int j = 0; j < o.n_win; j++) {
        PathHead h;
        const int n = T[j].x_len;
        tlen += n;
        if (charge_matched(R + j, PP + j, h)) { const int e = h.err(); terr += e; full += e; continue; }
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

} // namespace
