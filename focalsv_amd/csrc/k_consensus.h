// k_consensus.h -- the consensus family of the per-read-set assembly: k_consensus / k_consensus_redo, the junction cigars
// (k_bcig_tasks / k_bcig_accept), the haplotype partition (k_snp_sites / k_hap_partition) and the second consensus pass
// (k_bnd_tasks ... k_bnd_apply).  Included by asm_kernels.h after the path kernels, whose helpers and constants it uses.
#pragma once

namespace {

// ------------------------------------------------------------------------------------------------ k_consensus
// One wavefront per (read, 375-bp grid window).  Lanes walk the window paths of the accepted overlaps
// and vote into LDS histograms (per column: A C G T deleted arrived after-insertion); inserted strings are
// kept as (column, key) events.  Then lanes take columns, decide, and the corrected window is written out.
struct ConsArgs {
    const uint32_t *store;
    const uint32_t *word_off;
    const int32_t *read_len;
    const uint32_t *read_set;    // read -> set
    const uint32_t *set_start;
    const uint32_t *pair_base;
    const uint32_t *gwin_off;    // n_reads + 1: first grid window of every read
    const uint32_t *gwin_read;   // n_gwin: read of every grid window
    const uint4 *ovl_c;          // per ordered pair: an OvlC (k_verify.h)
    const uint4 *gwin_tab;       // per grid window: {read, first pair slot of the read, overlaps of the read, window index}  (k_gwin_tab)
    const fsv_wtask *tasks;
    const fsv_wpath *paths;
    uint8_t *cwin;               // FSV_CW_STRIDE bytes per grid window (2-bit codes, one per byte)
    uint16_t *cwin_len;
    uint32_t *warn;
    uint32_t *changed;           // per read: set when the consensus of some window differs from the read (nullptr: not tracked)
    uint32_t n_reads;
    const uint32_t *read_dirty;  // per read: some accepted overlap deviates from it somewhere (k_read_dirty); nullptr: not known
    uint8_t *cov3;               // per grid window: at least three overlaps voted (the window went through window_consensus); nullptr: not kept
    int junction_vote;           // 1: bases skipped between two windows of an overlap are voted as an insertion (the stand-in for the second pass)
    int ins_dag;                 // 1: inserted strings that disagree go through hifiasm's DAG (lane 0); 0: the most frequent string (ONT profile)
    // deep_sets = 1 (nullptr: off): a window with more insertion events than its LDS buffer holds, or with more than 255 overlaps, is not
    // flagged but listed here as {grid window, events} for k_consensus_deep; deep_n counts every attempt, deep_cap entries fit
    uint2 *deep_list; uint32_t *deep_n; uint32_t deep_cap;
};
__device__ __forceinline__ void deep_push(uint2 *list, uint32_t *n, uint32_t cap, uint32_t gw, uint32_t events)
{
    const uint32_t k = atomicAdd(n, 1u);
    if (k < cap) list[k] = make_uint2(gw, events);
}

__device__ __forceinline__ bool vote_wins(int cnt, int total, bool homo)
{
    if (cnt * 5 >= total * 3) return true;
    return homo && cnt * 1000 >= total * 515;
}

// One wavefront per read, one lane per overlap: does some accepted overlap deviate from the read anywhere -- a window at distance
// > 0, or y bases skipped between two consecutive windows (what k_consensus votes as a junction insertion)?  A read no overlap
// deviates from keeps every window as it is; from the second round on that is most reads, and their windows skip the tally.
__global__ __launch_bounds__(64) void k_read_dirty(const uint4 *__restrict__ ovl_c, const fsv_wpath *__restrict__ paths, const uint32_t *__restrict__ read_set,
                                                   const uint32_t *__restrict__ set_start, const uint32_t *__restrict__ pair_base, uint32_t n_reads,
                                                   uint32_t *__restrict__ read_dirty)
{
    const uint32_t r = blockIdx.x;
    if (r >= n_reads) return;
    const uint32_t s = read_set[r], r0 = set_start[s], ns = set_start[s + 1] - r0;
    const uint32_t pbase = pair_base[s] + (r - r0) * (ns - 1), n_ovl = ns - 1;
    bool dirty = false;
    for (uint32_t oi = threadIdx.x; oi < n_ovl; oi += 64) {
        const OvlC oc = OvlC::load(&ovl_c[pbase + oi]);
        if (!oc.accepted()) continue;
        const int n_win = oc.n_win();
        int prev_end = 0; bool prev_ok = false;
        for (int j = 0; j < n_win && !dirty; j++) {
            const PathHead h0 = PathHead::load(paths + (oc.first_task() + (uint32_t)j));
            const bool ok = h0.present();
            if (ok) {
                if (h0.err() != 0) dirty = true;
                if (prev_ok && h0.ry_start() - prev_end - 1 != 0) dirty = true;     // bases of y skipped, or used twice
                prev_end = h0.ry_end();
            }
            prev_ok = ok;
        }
    }
    const bool any = __ballot(dirty) != 0ull;
    if (threadIdx.x == 0) read_dirty[r] = any ? 1u : 0u;
}

// per grid window, once per round: everything k_consensus would otherwise look up through three levels of tables
__global__ void k_gwin_tab(const uint32_t *__restrict__ gwin_read, const uint32_t *__restrict__ gwin_off, const uint32_t *__restrict__ read_set,
                           const uint32_t *__restrict__ set_start, const uint32_t *__restrict__ pair_base, uint32_t n_gwin, uint4 *__restrict__ tab)
{
    const uint32_t gw = blockIdx.x * blockDim.x + threadIdx.x;
    if (gw >= n_gwin) return;
    const uint32_t r = gwin_read[gw], s = read_set[r], r0 = set_start[s], ns = set_start[s + 1] - r0;
    tab[gw] = make_uint4(r, pair_base[s] + (r - r0) * (ns - 1), ns - 1, gw - gwin_off[r]);
}

// EVC: insertion events a window can hold in LDS (FSV_EV_CAP; ONT-profile reads: FSV_EV_CAP_WIDE; beyond it: deep_sets, k_consensus_deep)
// MODE 0: every window.  MODE 1: every window, and a window with a column that split_sub_list would keep as a site of the
// haplotype partition is marked (site_cnt[gw] = FSV_SITE_MARK) -- the consensus written here is then provisional: k_snp_sites and
// k_hap_partition run next, and the windows of a read that lost overlaps to the partition are redone.  MODE 2: that redo.
#define FSV_SITE_MARK 0xffffffffu
// ---- what is inserted in front of a column: hifiasm's DAG of the inserted strings ---------------------------------------------
// build_DAGCon / Merge_DAGCon / generate_best_seq_from_nodes (Correct.cpp:3219-3951), as oracle/asm.c:dagcon_insertion restates
// them: one chain S -> b1 -> ... -> E per distinct string (here in ascending key order) weighted by its count, nodes gone through
// in topological order merging per base the in-nodes with one out-edge and the out-nodes with one in-edge, node weight = sum of the
// out-edges (E: in-edges), greedy walk forward from S's heaviest out-node or backward from E's heaviest in-node.  One lane runs it
// on a scratch in LDS; beyond the bounds (FSV_DG_*) the caller inserts the most frequent string instead, as the oracle does.
#define FSV_DG_N 64
#define FSV_DG_E 128
#define FSV_DG_A 8
#define FSV_DG_D 8
#define FSV_DG_K 64
struct DagLds {
    uint32_t keys[FSV_DG_K];
    uint16_t e_w[FSV_DG_E];
    uint8_t e_from[FSV_DG_E], e_to[FSV_DG_E], e_alive[FSV_DG_E], e_vis[FSV_DG_E];
    uint8_t base[FSV_DG_N], alive[FSV_DG_N], out_n[FSV_DG_N], in_n[FSV_DG_N];
    uint8_t out_e[FSV_DG_N][FSV_DG_A], in_e[FSV_DG_N][FSV_DG_A];
    uint8_t queue[4 * FSV_DG_E];
    uint8_t stk_node[16], stk_bi[16], stk_cons[16];
    int n_node, n_edge, ok;
};

__device__ __forceinline__ int dg_node(DagLds &D, uint8_t b)
{
    const int id = D.n_node;
    if (id >= FSV_DG_N) { D.ok = 0; return FSV_DG_N - 1; }
    D.base[id] = b; D.alive[id] = 1; D.out_n[id] = 0; D.in_n[id] = 0; D.n_node = id + 1;
    return id;
}
__device__ __forceinline__ void dg_edge(DagLds &D, int u, int v, int w, int vis)
{
    const int e = D.n_edge;
    if (e >= FSV_DG_E || D.out_n[u] >= FSV_DG_A || D.in_n[v] >= FSV_DG_A) { D.ok = 0; return; }
    D.e_from[e] = (uint8_t)u; D.e_to[e] = (uint8_t)v; D.e_w[e] = (uint16_t)w; D.e_alive[e] = 1; D.e_vis[e] = (uint8_t)vis; D.n_edge = e + 1;
    D.out_e[u][D.out_n[u]++] = (uint8_t)e; D.in_e[v][D.in_n[v]++] = (uint8_t)e;
}
__device__ __forceinline__ int dg_find(const DagLds &D, int u, int v)
{
    for (int i = 0; i < D.in_n[v]; i++) { const int e = D.in_e[v][i]; if (D.e_alive[e] && D.e_from[e] == u) return e; }
    return -1;
}
__device__ __forceinline__ int dg_outdeg(const DagLds &D, int u) { int c = 0; for (int i = 0; i < D.out_n[u]; i++) c += D.e_alive[D.out_e[u][i]]; return c; }
__device__ __forceinline__ int dg_indeg(const DagLds &D, int u) { int c = 0; for (int i = 0; i < D.in_n[u]; i++) c += D.e_alive[D.in_e[u][i]]; return c; }
__device__ __forceinline__ void dg_delete(DagLds &D, int x)
{
    D.alive[x] = 0; D.base[x] = 'D';
    for (int i = 0; i < D.out_n[x]; i++) D.e_alive[D.out_e[x][i]] = 0;
    for (int i = 0; i < D.in_n[x]; i++) D.e_alive[D.in_e[x][i]] = 0;
    D.out_n[x] = 0; D.in_n[x] = 0;
}
// Merge_Out_Nodes (OUT) / Merge_In_Nodes (!OUT) with the recursion of the reference unrolled onto a small stack: a frame is
// (node, next base); after the merges for one base the merged node is entered before the next base is looked at
template <bool OUT>
__device__ __forceinline__ void dg_merge(DagLds &D, int start)
{
    int sp = 0;
    D.stk_node[0] = (uint8_t)start; D.stk_bi[0] = 0;
    if (!D.alive[start] || (OUT ? dg_outdeg(D, start) : dg_indeg(D, start)) == 0) return;
    while (sp >= 0 && D.ok) {
        const int cur = D.stk_node[sp], bi = D.stk_bi[sp];
        if (bi >= 4) { sp--; continue; }
        D.stk_bi[sp] = (uint8_t)(bi + 1);
        const uint8_t want = (uint8_t)("ACGT"[bi]);
        int flag = 0, weight = 0, cons = -1;
        const int nl = OUT ? D.out_n[cur] : D.in_n[cur];
        for (int i = 0; i < nl; i++) {
            const int e = OUT ? D.out_e[cur][i] : D.in_e[cur][i];
            if (!D.e_alive[e]) continue;
            const int g = OUT ? D.e_to[e] : D.e_from[e];
            if (D.base[g] != want || (OUT ? dg_indeg(D, g) : dg_outdeg(D, g)) != 1) continue;
            if (flag == 0) { flag = 1; cons = g; D.e_vis[e] = 1; weight = D.e_w[e]; }
            else {
                flag++;
                weight += D.e_w[e];
                const int ng = OUT ? D.out_n[g] : D.in_n[g];
                for (int j = 0; j < ng; j++) {
                    const int e2 = OUT ? D.out_e[g][j] : D.in_e[g][j];
                    if (!D.e_alive[e2]) continue;
                    const int o = OUT ? D.e_to[e2] : D.e_from[e2];
                    const int e3 = OUT ? dg_find(D, cons, o) : dg_find(D, o, cons);
                    if (e3 >= 0) { D.e_vis[e3] = 1; D.e_w[e3] = (uint16_t)(D.e_w[e3] + D.e_w[e2]); }
                    else if (OUT) dg_edge(D, cons, o, D.e_w[e2], 1);
                    else dg_edge(D, o, cons, D.e_w[e2], 1);
                }
                dg_delete(D, g);
            }
        }
        if (flag > 1) { const int e = OUT ? dg_find(D, cur, cons) : dg_find(D, cons, cur); if (e >= 0) D.e_w[e] = (uint16_t)weight; }
        if (flag > 0 && D.alive[cons] && (OUT ? dg_outdeg(D, cons) : dg_indeg(D, cons)) != 0) {
            if (sp + 1 >= 16) { D.ok = 0; return; }
            sp++;
            D.stk_node[sp] = (uint8_t)cons; D.stk_bi[sp] = 0;
        }
    }
}
__device__ __forceinline__ int dg_weight(const DagLds &D, int u, bool in)
{
    int w = 0;
    if (in) { for (int i = 0; i < D.in_n[u]; i++) if (D.e_alive[D.in_e[u][i]]) w += D.e_w[D.in_e[u][i]]; }
    else for (int i = 0; i < D.out_n[u]; i++) if (D.e_alive[D.out_e[u][i]]) w += D.e_w[D.out_e[u][i]];
    return w;
}
// D.keys[0 .. nk): the column's inserted strings (len << 24 | 2-bit bases).  Returns max_insertion_count (-1: beyond the bounds)
__device__ __forceinline__ int dag_insertion(DagLds &D, int nk, uint32_t &out_key)
{
    out_key = 0;
    if (nk > FSV_DG_K) return -1;
    for (int z = 1; z < nk; z++) { const uint32_t kv = D.keys[z]; int z2 = z; for (; z2 > 0 && D.keys[z2 - 1] > kv; z2--) D.keys[z2] = D.keys[z2 - 1]; D.keys[z2] = kv; }
    uint32_t distinct[FSV_DG_D]; int cnt[FSV_DG_D], nd = 0;
    for (int i = 0; i < nk; i++) {
        if (nd && distinct[nd - 1] == D.keys[i]) { cnt[nd - 1]++; continue; }
        if (nd == FSV_DG_D) return -1;
        distinct[nd] = D.keys[i]; cnt[nd] = 1; nd++;
    }
    if (nd == 1) { out_key = distinct[0]; return cnt[0]; }      // one string: the chain itself
    D.n_node = 0; D.n_edge = 0; D.ok = 1;
    const int S = dg_node(D, 'S'), E = dg_node(D, 'E');
    for (int i = 0; i < nd; i++) {
        const int len = (int)(distinct[i] >> 24);
        int last = S;
        for (int j = 0; j < len; j++) { const int nn = dg_node(D, (uint8_t)("ACGT"[(distinct[i] >> (2 * j)) & 3u])); dg_edge(D, last, nn, cnt[i], 0); last = nn; }
        if (last != S) dg_edge(D, last, E, cnt[i], 0);
    }
    int qh = 0, qt = 0;
    D.queue[qt++] = (uint8_t)S;
    while (qh < qt && D.ok) {
        const int cur = D.queue[qh++];
        dg_merge<false>(D, cur);
        dg_merge<true>(D, cur);
        if (!D.alive[cur]) continue;
        for (int i = 0; i < D.out_n[cur]; i++) if (D.e_alive[D.out_e[cur][i]]) D.e_vis[D.out_e[cur][i]] = 1;
        for (int i = 0; i < D.out_n[cur]; i++) {
            const int e = D.out_e[cur][i];
            if (!D.e_alive[e]) continue;
            const int o = D.e_to[e];
            bool all = true;
            for (int j = 0; j < D.in_n[o]; j++) if (D.e_alive[D.in_e[o][j]] && !D.e_vis[D.in_e[o][j]]) { all = false; break; }
            if (all) { if (qt < 4 * FSV_DG_E) D.queue[qt++] = (uint8_t)o; else D.ok = 0; }
        }
    }
    if (!D.ok) return -1;
    int best_s = -1, best_e = -1, ws = 0, we = 0;
    for (int i = 0; i < D.out_n[S]; i++) { const int e = D.out_e[S][i]; if (D.e_alive[e]) { const int o = D.e_to[e], w = o == E ? dg_weight(D, E, true) : dg_weight(D, o, false); if (w > ws) { ws = w; best_s = o; } } }
    for (int i = 0; i < D.in_n[E]; i++) { const int e = D.in_e[E][i]; if (D.e_alive[e]) { const int o = D.e_from[e], w = dg_weight(D, o, false); if (w > we) { we = w; best_e = o; } } }
    uint32_t seq = 0; int L = 0;
    if (ws >= we) {
        int cur = best_s;
        while (cur >= 0 && cur != E && L < FSV_DG_N) {
            int mx = 0, nx = -1;
            if (L < FSV_INS_MAXLEN) seq |= (uint32_t)(D.base[cur] == 'A' ? 0u : D.base[cur] == 'C' ? 1u : D.base[cur] == 'G' ? 2u : 3u) << (2 * L);
            L++;
            for (int i = 0; i < D.out_n[cur]; i++) { const int e = D.out_e[cur][i]; if (D.e_alive[e]) { const int o = D.e_to[e], w = o == E ? dg_weight(D, E, true) : dg_weight(D, o, false); if (w > mx) { mx = w; nx = o; } } }
            cur = nx;
        }
    } else {
        // backward: the bases come out last first
        uint8_t rb[FSV_INS_MAXLEN + 4];
        int cur = best_e;
        while (cur >= 0 && cur != S && L < FSV_DG_N) {
            int mx = 0, nx = -1;
            if (L < FSV_INS_MAXLEN + 4) rb[L] = D.base[cur];
            L++;
            for (int i = 0; i < D.in_n[cur]; i++) { const int e = D.in_e[cur][i]; if (D.e_alive[e]) { const int o = D.e_from[e], w = dg_weight(D, o, false); if (w > mx) { mx = w; nx = o; } } }
            cur = nx;
        }
        const int Lc = min(L, FSV_INS_MAXLEN + 4);
        for (int i = 0; i < Lc && i < FSV_INS_MAXLEN; i++) { const uint8_t b = rb[Lc - 1 - i]; seq |= (uint32_t)(b == 'A' ? 0u : b == 'C' ? 1u : b == 'G' ? 2u : 3u) << (2 * i); }
    }
    if (L > FSV_INS_MAXLEN) L = FSV_INS_MAXLEN;
    out_key = ((uint32_t)L << 24) | seq;
    return ws >= we ? ws : we;
}

// get_seq_from_Graph (Correct.cpp:4010-4129) at the node in front of one backbone column, as oracle/asm.c:vote_consensus: the
// edges to the four bases (the backbone's own first; weight minus the votes that arrived "after an insertion" while the node still
// has insertions to place), the inserted strings' DAG, the deletion edge; the heaviest wins if it has 60 % of the total (51.5 % when
// the PREVIOUS backbone base sits in a homopolymer run); an insertion is written and the node looked at again without it.
// W[b]: votes for base b (the backbone's own + 1), Ifl[b]: of those, votes whose previous cigar run was an insertion, dl: votes
// without a partner for the column, ni: overlaps inserting in front of it, (mi, ikey): the DAG's answer.  out[0] = bases written.
__device__ __forceinline__ bool poa_decide(const int W[4], const int Ifl[4], int dl, int ni, int mi, uint32_t ikey, int own, bool homo, uint8_t *out)
{
    uint8_t nb = 0;
    bool kept = true;
    for (int visit = 0; visit < 2; visit++) {
        int maxc = -1, type = 0, edge = own, total = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int b = k == 0 ? own : (k - 1 < own ? k - 1 : k);     // own first, then the others in base order
            if (W[b] == 0) continue;
            const int cw = ni ? W[b] - Ifl[b] : W[b];
            total += cw;
            if (cw > maxc) { maxc = cw; type = 0; edge = b; }
        }
        if (ni) { total += ni; if (mi > maxc) { maxc = mi; type = 1; } }
        if (dl) { total += dl; if (dl > maxc) { maxc = dl; type = 2; } }
        if (maxc * 5 >= total * 3 || (homo && maxc * 1000 >= total * 515)) {
            if (type == 1) { const int L = (int)(ikey >> 24); for (int b = 0; b < L; b++) out[1 + nb++] = (uint8_t)((ikey >> (2 * b)) & 3u); ni = 0; continue; }
            if (type == 2) { kept = false; break; }
            out[1 + nb++] = (uint8_t)edge;
            break;
        }
        out[1 + nb++] = (uint8_t)own;
        break;
    }
    out[0] = nb;
    return kept;
}

// ---- where a window's insertion events live -------------------------------------------------------------------------------------
// An event is (key, link to the next event of its column); the tally goes through one of two stores, as chain_core goes through
// ChainTile and ChainSlab.  EvLds<EVC>: EVC events in LDS with 16-bit links -- the kernels of every call; an event beyond EVC is counted
// and dropped.  EvSlab (deep_sets = 1, k_consensus_deep / k_bnd_consensus_deep): the block's slab in HBM with 32-bit links, sized by
// the host so that no window can fill it (asm.hip: deep_slab_events), and a third array the wave gathers a column's keys into.
// NIL ends a list; ANSWERED marks a column head whose first event holds the insertion consensus; FLW: words per column of Tally::fl.
template <int EVC>
struct EvLds {
    static constexpr bool deep = false;
    static constexpr int FLW = 1;                      // 8 bits per base
    static constexpr uint32_t NIL = 0xffffu, ANSWERED = 0x10000u;
    uint32_t k[EVC];
    uint16_t n[EVC];
    __device__ __forceinline__ uint32_t cap() const { return (uint32_t)EVC; }
    __device__ __forceinline__ uint32_t key(uint32_t i) const { return k[i]; }
    __device__ __forceinline__ uint32_t next(uint32_t i) const { return n[i]; }
    __device__ __forceinline__ void put(uint32_t i, uint32_t key_, uint32_t next_) { k[i] = key_; n[i] = (uint16_t)next_; }
};
struct EvSlab {
    static constexpr bool deep = true;
    static constexpr int FLW = 2;                      // 16 bits per base, as cnt: a field holds the votes of every overlap of a set
    static constexpr uint32_t NIL = 0x7fffffffu, ANSWERED = 0x80000000u;
    uint32_t *k, *n, *g;                               // keys, links, the gathered keys of the column being answered: cap_ entries each
    uint32_t cap_;
    __device__ __forceinline__ uint32_t cap() const { return cap_; }
    __device__ __forceinline__ uint32_t key(uint32_t i) const { return k[i]; }
    __device__ __forceinline__ uint32_t next(uint32_t i) const { return n[i]; }
    __device__ __forceinline__ void put(uint32_t i, uint32_t key_, uint32_t next_) { k[i] = key_; n[i] = next_; }
};

// the most frequent inserted string of a column's event list, the smaller key on a tie
template <class EV>
__device__ __forceinline__ void most_frequent_insertion(const EV &ev, uint32_t head, int &mi, uint32_t &key)
{
    int bc = 0; uint32_t bk = 0;
    for (uint32_t i = head; i != EV::NIL; i = ev.next(i)) {
        const uint32_t k1 = ev.key(i);
        int cn = 0;
        for (uint32_t j2 = head; j2 != EV::NIL; j2 = ev.next(j2)) cn += (ev.key(j2) == k1);
        if (cn > bc || (cn == bc && k1 < bk)) { bc = cn; bk = k1; }
    }
    mi = bc; key = bk;
}
// the same on the nk keys of a column gathered into g, the wave sharing the quadratic count: a lane counts every 64th key against
// all of them, then the lanes' answers meet (most votes, the smaller key on a tie: what the list order gives, whatever that order)
__device__ __forceinline__ void most_frequent_gathered(const uint32_t *g, int nk, int lane, int &mi, uint32_t &key)
{
    int bc = 0; uint32_t bk = 0;
    for (int a = lane; a < nk; a += 64) {
        const uint32_t k1 = g[a];
        int cn = 0;
        for (int j = 0; j < nk; j++) cn += (g[j] == k1);
        if (cn > bc || (cn == bc && k1 < bk)) { bc = cn; bk = k1; }
    }
    for (int d = 32; d >= 1; d >>= 1) {
        const int oc = __shfl_xor(bc, d); const uint32_t ok = __shfl_xor(bk, d);
        if (oc > bc || (oc == bc && ok < bk)) { bc = oc; bk = ok; }
    }
    mi = bc; key = bk;
}

#define FSV_INSLIST 128
#define COV_LO(v) ((int)(int16_t)((v) & 0xffff))
#define COV_HI(v) (((int)(v) - COV_LO(v)) >> 16)

// if_is_homopolymer_strict (Correct.h:447-530) on 2-bit bases: the run that starts right after the site and the run that starts right
// before it, each looked at over at most three bases; the site joins the forward run if it has that base, else the backward run if
// it has that one; a run of three (the site included or merely beside it) makes a homopolymer site, and so do a forward and a
// backward run of the site's own base that add up to three.  B(p): base at read position p (0 <= p < len).
template <class F>
__device__ __forceinline__ bool homo_strict(F B, int site, int len)
{
    const int beg = max(0, site - 3), end = min(len - 1, site + 3);
    const uint32_t own = B(site);
    uint32_t f_ch = 4u, b_ch = 4u;      // 4: no base seen
    int f_len = 0, b_len = 0;
    for (int i = site + 1; i <= end; i++) {
        const uint32_t v = B(i);
        if (f_ch == 4u) { f_ch = v; f_len = 1; } else if (v != f_ch) break; else f_len++;
    }
    for (int i = site - 1; i >= beg; i--) {
        const uint32_t v = B(i);
        if (b_ch == 4u) { b_ch = v; b_len = 1; } else if (v != b_ch) break; else b_len++;
    }
    if (f_ch == own) f_len++;
    else if (b_ch == own) b_len++;
    return f_len >= 3 || b_len >= 3 || (own == f_ch && b_ch == f_ch && f_len + b_len >= 3);
}

// ---- the column tally of one window: its LDS state and the steps every kernel of the family takes on it ------------------------------
// TallyCols is what k_snp_sites needs: per-column counters, the coverage difference array, a row of op words per lane and the
// backbone's bases.  Tally<EV> (k_consensus, k_consensus_redo, k_bnd_consensus) adds the inserted strings, the "after an insertion"
// votes and the lists of the columns to look at.  One __shared__ object per kernel; members are ordered by alignment so that the
// struct has no padding.
__device__ __forceinline__ void load_path_ops(const fsv_wpath *P, uint2 (&pv)[13])
{
    const uint2 *src = reinterpret_cast<const uint2 *>(P->ops);
#pragma unroll
    for (int i = 0; i < 13; i++) pv[i] = src[i];
}
// each lane owns the contiguous columns [c0, c1) of the n a window has
__device__ __forceinline__ void lane_columns(int lane, int n, int &c0, int &c1)
{
    const int per = (n + 63) / 64;
    c0 = min(n, lane * per); c1 = min(n, c0 + per);
}

struct TallyCols {
    uint32_t cnt[FSV_WINDOW + 1][3];   // per column, 16 bits each: votes for A C | G T that differ from the backbone | deleted, arrived-after-insertion
    int32_t cov[FSV_WINDOW + 2];       // coverage difference array -> arrived
    uint32_t path[64][27];             // per lane: the 26 op words of its window path (odd stride); after the tally the DAG scratch, then the output
    uint32_t xraw[28];                 // raw store words covering x[org-16 .. org+n_cols+16), org = the read position of column 0
    uint32_t cover;

    __device__ __forceinline__ void reset(int lane)
    {
        for (int i = lane; i < (FSV_WINDOW + 1) * 3; i += 64) (&cnt[0][0])[i] = 0;
        for (int i = lane; i < FSV_WINDOW + 2; i += 64) cov[i] = 0;
        if (lane == 0) cover = 0;
    }
    // x: the backbone's first store word, len: its length; the first staged word may be -1 at the read start: reads as 0, never used
    __device__ __forceinline__ void stage_backbone(int lane, const uint32_t *__restrict__ x, int org, int len)
    {
        if (lane < 28) { const int wi = (org >> 4) - 1 + lane; xraw[lane] = (wi >= 0 && wi <= ((len + 15) >> 4)) ? x[wi] : 0u; }
    }
    __device__ __forceinline__ uint32_t xb(int org, int p) const { return (xraw[(p >> 4) - ((org >> 4) - 1)] >> ((p & 15) << 1)) & 3u; }
    __device__ __forceinline__ void cnt_add(int c, uint32_t b) { atomicAdd(&cnt[c][b >> 1], 1u << ((b & 1u) << 4)); }
    __device__ __forceinline__ uint32_t cnt_get(int c, uint32_t b) const { return (cnt[c][b >> 1] >> ((b & 1u) << 4)) & 0xffffu; }
    // the lane's row of op words; returns nz: bit w set = word w is not all matches
    __device__ __forceinline__ uint32_t stage_path(int lane, const uint2 (&pv)[13])
    {
        uint32_t nz = 0;
#pragma unroll
        for (int i = 0; i < 13; i++) {
            path[lane][2 * i] = pv[i].x; path[lane][2 * i + 1] = pv[i].y;
            nz |= (pv[i].x ? 1u << (2 * i) : 0u) | (pv[i].y ? 2u << (2 * i) : 0u);
        }
        return nz;
    }
};

// split_sub_list (Correct.cpp:5804) on a column's tallies: of the arrived overlaps occ_0 show the backbone's base, oa[b] another
// base b (occ_1 in all: at least two, hap->flag > snp_threshold), occ2 have no partner for it.  The column is kept as a site of the
// haplotype partition when one other base (alt) dominates.
__device__ __forceinline__ bool split_sub_site(const int oa[4], int occ2, int arrived, int &alt)
{
    const int occ1 = oa[0] + oa[1] + oa[2] + oa[3];
    if (occ1 <= 1) return false;
    const int occ0 = arrived - occ1 - occ2;
    int mx = occ2;
    alt = -1;
#pragma unroll
    for (int b = 0; b < 4; b++) if (oa[b] > mx) { mx = oa[b]; alt = b; }
    if (occ0 == 0 || alt < 0 || mx <= 1) return false;
#pragma unroll
    for (int b = 0; b < 4; b++) if (oa[b] == mx && b != alt) return false;
    return (double)(occ0 + 1 + mx) / (double)(arrived + 1) >= 0.95 && (double)mx / (double)(arrived + 1 - (occ0 + 1)) >= 0.70;
}

template <class EV>
struct Tally : TallyCols {
    uint32_t evhead[FSV_WINDOW + 1];   // insertion events of a column form a list: evhead[column] -> event -> ev.next(event) ...
    uint32_t fl[FSV_WINDOW + 1][EV::FLW];   // votes of the mismatch runs that follow an insertion, 8 (EvSlab: 16) bits per base (the match runs: cov's upper halves)
    uint32_t evn, nins, ndev;
    EV ev;
    uint16_t inslist[FSV_INSLIST];     // columns whose inserted strings disagree
    uint16_t devlist[FSV_WINDOW + 1];  // columns some vote deviates at
    static_assert(sizeof(DagLds) <= sizeof(uint32_t) * 64 * 27 && (FSV_WINDOW + 1) * 14 <= sizeof(uint32_t) * 64 * 27,
                  "the DAG scratch and the decided columns live in the path buffer between the tally and the write-out");

    __device__ __forceinline__ DagLds &dag() { return *reinterpret_cast<DagLds *>(&path[0][0]); }
    // per column: the number of bases written for it (0: deleted), then the bases
    __device__ __forceinline__ uint8_t (*out())[14] { return reinterpret_cast<uint8_t (*)[14]>(&path[0][0]); }

    __device__ __forceinline__ void reset(int lane)
    {
        TallyCols::reset(lane);
        for (int i = lane; i < FSV_WINDOW + 1; i += 64) evhead[i] = EV::NIL;
        for (int i = lane; i < (FSV_WINDOW + 1) * EV::FLW; i += 64) (&fl[0][0])[i] = 0;
        if (lane == 0) { evn = 0; nins = 0; ndev = 0; }
    }
    __device__ __forceinline__ void add_event(int c, uint32_t key)
    {
        const uint32_t e = atomicAdd(&evn, 1u);
        if (e < ev.cap()) ev.put(e, key, atomicExch(&evhead[c], e));
    }
    __device__ __forceinline__ void fl_add(uint32_t c, uint32_t b)
    {
        if (EV::FLW == 1) atomicAdd(&fl[c][0], 1u << (b << 3));
        else atomicAdd(&fl[c][(b >> 1) & (EV::FLW - 1)], 1u << ((b & 1u) << 4));
    }
    __device__ __forceinline__ int fl_get(int c, int b) const
    {
        return EV::FLW == 1 ? (int)((fl[c][0] >> (b << 3)) & 0xffu) : (int)((fl[c][(b >> 1) & (EV::FLW - 1)] >> ((b & 1) << 4)) & 0xffffu);
    }

    // the insertion consensus of every column that has insertions, by lane 0 (a handful per window): the column's keyed events are
    // gathered from its list, the DAG (or, beyond its bounds, the most frequent string) answers, and the answer replaces the list's head
    // event (key, count); EV::ANSWERED in the head marks the column as answered.  EvSlab: the whole wave comes here -- a column can hold
    // hundreds of events, so the walk also gathers its keys into ev.g and the lanes share the count of the most frequent string; with
    // ins_dag 0 that string is the answer
    __device__ __forceinline__ void answer_insertions(int lane, int n_cols, int ins_dag)
    {
        DagLds &D = dag();
        const int n_list = (int)nins, n = n_list > FSV_INSLIST ? n_cols : n_list;      // the list overflowed: every column
        for (int li = 0; li < n; li++) {
            const int c = n_list > FSV_INSLIST ? li : (int)inslist[li];
            const uint32_t head = evhead[c] & (EV::ANSWERED - 1u);
            if (head == EV::NIL || (evhead[c] & EV::ANSWERED)) continue;
            int nk = 0;
            uint32_t key = 0;
            if constexpr (EV::deep) {
                for (uint32_t i = head; i != EV::NIL; i = ev.next(i)) {
                    const uint32_t kv = ev.key(i);
                    if (lane == 0 && nk < FSV_DG_K) D.keys[nk] = kv;
                    if ((nk & 63) == lane) ev.g[nk] = kv;
                    nk++;
                }
                __syncthreads();
                int mi = -1;
                if (ins_dag && lane == 0) mi = dag_insertion(D, nk, key);
                mi = __shfl(mi, 0); key = __shfl(key, 0);
                if (mi < 0) most_frequent_gathered(ev.g, nk, lane, mi, key);
                if (lane == 0) { ev.put(head, key, (uint32_t)mi); evhead[c] |= EV::ANSWERED; }
                __syncthreads();
            } else {
                for (uint32_t i = head; i != EV::NIL; i = ev.next(i)) { if (nk < FSV_DG_K) D.keys[nk] = ev.key(i); nk++; }
                int mi = dag_insertion(D, nk, key);
                if (mi < 0) most_frequent_insertion(ev, head, mi, key);
                ev.put(head, key, (uint32_t)mi);
                evhead[c] |= EV::ANSWERED;
            }
        }
    }

    // From the finished tally to the decided columns out()[0 .. n_cols), the lane owning the columns [c0, c1).  org: read position
    // of column 0, len: the backbone's length, verbatim: every column keeps the backbone's base.  extra(c, arrived, kept) is called
    // for every column that went through poa_decide.  Returns whether a column of this lane's came out different from the backbone;
    // on return the columns are visible to all lanes.
    template <class F>
    __device__ __forceinline__ bool decide_columns(int lane, int c0, int c1, int org, int n_cols, int len, bool verbatim, int ins_dag, F extra)
    {
        // arrived[c] = prefix sum of the difference array (low half: coverage, high half: the flagged match runs; both small signed
        // numbers, so the halves separate exactly)
        int run = 0, frun = 0;
        for (int c = c0; c < c1; c++) {
            const int v = cov[c];
            run += COV_LO(v); frun += COV_HI(v);
            if (cnt_get(c, 5u)) {       // inserted strings that disagree go through the DAG (lane 0, below); one string answers itself
                const uint32_t head = evhead[c];
                bool same = true;
                if (head != EV::NIL) { const uint32_t k0 = ev.key(head); for (uint32_t i = ev.next(head); i != EV::NIL; i = ev.next(i)) if (ev.key(i) != k0) { same = false; break; } }
                // (EvSlab: listed without the DAG too -- the wave then finds the most frequent string together, below)
                if (!same && (ins_dag || EV::deep)) { const uint32_t k = atomicAdd(&nins, 1u); if (k < FSV_INSLIST) inslist[k] = (uint16_t)c; }
            }
        }
        int arrived = wave_incl_sum(run, lane) - run, farrived = wave_incl_sum(frun, lane) - frun;
        __syncthreads();
        if ((EV::deep || lane == 0) && nins) answer_insertions(lane, n_cols, ins_dag);
        __syncthreads();
        uint8_t (*o)[14] = out();      // paths are done
        // Columns nobody deviates at (no vote in cnt: nine in ten even in the first round) keep the backbone's base: poa_decide then
        // sees one edge with all the weight.  The others are listed and decided a lane each -- walked in place, lane = six consecutive
        // columns, nearly every trip had some lane with a deviating column and the whole wave went through the decision six times.
        for (int c = c0; c < c1; c++) {
            arrived += COV_LO(cov[c]);
            farrived += COV_HI(cov[c]);
            o[c][0] = 1; o[c][1] = (uint8_t)xb(org, org + c);
            if (!verbatim && (cnt[c][0] | cnt[c][1] | cnt[c][2]) != 0u) {
                cov[c] = (int32_t)(((uint32_t)arrived & 0xffffu) | ((uint32_t)farrived << 16));     // the lane owns its columns: the difference array is done with
                devlist[atomicAdd(&ndev, 1u)] = (uint16_t)c;
            }
        }
        __syncthreads();
        bool differs = false;
        for (uint32_t e = lane; e < ndev; e += 64) {
            const int c = (int)devlist[e];
            arrived = (int)(int16_t)((uint32_t)cov[c] & 0xffffu); farrived = (int)(int16_t)((uint32_t)cov[c] >> 16);
            const uint32_t own = xb(org, org + c);
            // the node in front of column c (poa_decide); the homopolymer relief looks at the PREVIOUS backbone base
            const bool homo = c > 0 && homo_strict([&](int pp) { return xb(org, pp); }, org + c - 1, len);
            int W[4], Ifl[4], dev = 0;
#pragma unroll
            for (int b = 0; b < 4; b++) { W[b] = (int)cnt_get(c, (uint32_t)b); dev += W[b]; Ifl[b] = fl_get(c, b); }
            const int dl = (int)cnt_get(c, 4u), ni = (int)cnt_get(c, 5u);
#pragma unroll
            for (int b = 0; b < 4; b++) if ((int)own == b) { W[b] += arrived - dev - dl + 1; Ifl[b] = farrived; }
            int mi = 0; uint32_t ikey = 0;
            if (ni) {
                const uint32_t hv = evhead[c], head = hv & (EV::ANSWERED - 1u);
                if (head != EV::NIL) {
                    ikey = ev.key(head);
                    if (hv & EV::ANSWERED) mi = (int)ev.next(head);                              // the DAG's answer (EvSlab: or the wave's)
                    else if (ins_dag || EV::deep) { for (uint32_t i = head; i != EV::NIL; i = ev.next(i)) mi++; }   // one string, mi times
                    else most_frequent_insertion(ev, head, mi, ikey);
                }
            }
            const bool kept = poa_decide(W, Ifl, dl, ni, mi, ikey, (int)own, homo, &o[c][0]);
            extra(c, arrived, kept);
            if (o[c][0] != 1 || o[c][1] != (uint8_t)own) differs = true;
        }
        __syncthreads();
        return differs;
    }
};

// ---- one overlap's votes on the columns of a window: the walk over its 2-bit path --------------------------------------------------
// A match op votes for the backbone's own base, so a path only contributes its deviations.  The walk jumps from deviation to
// deviation (a bit per non-zero path word, count-trailing-zeros inside a word) and does not touch memory: what needs a base of y
// -- a mismatch's vote, the string of an insertion -- is put aside, four at a time, and the y words of all four are requested
// together (a load per deviating op inside the walk was a dependent memory round trip per deviation for the whole wave).
// row: the lane's 26 op words in LDS (fields past plen are 0), nz: bit w set = word w is not all matches.
// pend: an insertion in front of column xs is already pending (the junction vote).  Returns the number of y-only ops (n2).
#define FSV_PEND_N 4
template <class T>
__device__ __forceinline__ void cons_flush(T &S, const uint32_t *__restrict__ store, uint32_t y_word, int y_len, int y_rev, int ry_start,
                                           const uint32_t (&ent)[FSV_PEND_N], int n)
{
    // entry: column | (y position - ry_start) << 9 | L << 19 (0: a mismatch) | flagged << 23
    uint32_t bits[FSV_PEND_N];
#pragma unroll
    for (int i = 0; i < FSV_PEND_N; i++) if (i < n) bits[i] = fetch16(store, y_word, y_len, y_rev, ry_start + (int)((ent[i] >> 9) & 1023u)).bits;
#pragma unroll
    for (int i = 0; i < FSV_PEND_N; i++) {
        if (i >= n) continue;
        const uint32_t e = ent[i], xp = e & 511u, L = (e >> 19) & 15u;
        if (L == 0u) {
            const uint32_t yb = bits[i] & 3u;
            S.cnt_add((int)xp, yb);
            if (e >> 23) S.fl_add(xp, yb);
        } else S.add_event((int)xp, (L << 24) | (bits[i] & ((1u << (2u * L)) - 1u)));
    }
}
template <class T>
__device__ __forceinline__ int cons_walk(T &S, const uint32_t *row, uint32_t nz, int plen, int xs, int xlim, bool pend,
                                         const uint32_t *__restrict__ store, uint32_t y_word, int y_len, int y_rev, int ry_start)
{
    int n2 = 0, n3 = 0, fstart = -1, fmm_pos = -1, np = 0, p = 0;
    uint32_t ent[FSV_PEND_N] = {0u, 0u, 0u, 0u};
    while (true) {
        if (np == FSV_PEND_N) { cons_flush(S, store, y_word, y_len, y_rev, ry_start, ent, np); np = 0; }
        if (!pend) {       // on to the next op that is not a match
            int w = p >> 4;
            if (w >= 26) break;
            uint32_t rest = row[w] >> ((p & 15) << 1);
            if (rest == 0u) {
                const uint32_t m = nz >> (w + 1);
                if (m == 0u) break;
                w += 1 + __builtin_ctz(m);
                p = w << 4;
                rest = row[w];
            }
            p += __builtin_ctz(rest) >> 1;
        }
        if (p >= plen) break;
        const uint32_t op = (row[p >> 4] >> ((p & 15) << 1)) & 3u;
        const int xp = xs + p - n2;
        if (fstart >= 0 && op != 0u) { atomicAdd(&S.cov[fstart], 65536); atomicAdd(&S.cov[xp], -65536); fstart = -1; }   // the match run after an insertion ends here
        if (op == 2u) {     // run of y-only ops in front of column xp
            int L = 1;
            while (p + L < plen && ((row[(p + L) >> 4] >> (((p + L) & 15) << 1)) & 3u) == 2u) L++;
            if (xp < xlim) {
                pend = true;
                if (L <= FSV_INS_MAXLEN) {
                    const uint32_t e = (uint32_t)xp | ((uint32_t)(p - n3) << 9) | ((uint32_t)L << 19);
                    if (np == 0) ent[0] = e; else if (np == 1) ent[1] = e; else if (np == 2) ent[2] = e; else ent[3] = e;
                    np++;
                }
            }
            n2 += L; p += L;
            continue;
        }
        const bool after_ins = pend && p > 0;      // (a junction vote is no cigar run)
        if (pend) { atomicAdd(&S.cnt[xp][2], 1u << 16); pend = false; }
        if (op == 3u) { atomicAdd(&S.cnt[xp][2], 1u); n3++; }
        else if (op == 1u) {
            // add_mismatchEdge_weight (POA.h:492) looks at the previous cigar RUN: every base of the run that follows an insertion
            // counts as "after an insertion", not only the first
            const bool flagged = after_ins || fmm_pos == p;
            const uint32_t e = (uint32_t)xp | ((uint32_t)(p - n3) << 9) | (flagged ? 1u << 23 : 0u);
            if (np == 0) ent[0] = e; else if (np == 1) ent[1] = e; else if (np == 2) ent[2] = e; else ent[3] = e;
            np++;
            if (flagged) fmm_pos = p + 1;
        } else if (after_ins) fstart = xp;
        p++;
    }
    if (fstart >= 0) { atomicAdd(&S.cov[fstart], 65536); atomicAdd(&S.cov[xs + plen - n2], -65536); }
    if (np) cons_flush(S, store, y_word, y_len, y_rev, ry_start, ent, np);
    return n2;
}

struct SiteLists {
    uint32_t *site_cnt;        // per grid window: FSV_SITE_MARK after k_consensus<., 1>, the number of kept sites after k_snp_sites
    uint32_t *win_list;        // marked windows, [0] of win_n
    uint32_t *redo_list;       // windows of the reads that lost an overlap to the partition
    uint32_t *win_n;           // {marked windows, redo windows}
    // per grid window, from k_bcig_accept (nullptr: no junction cigars anywhere): [0] a used junction cigar, or a window cigar it stands in
    // for, has a mismatch in the window; [1] / [2] first / last column at which a used junction cigar shows something else than the
    // window cigar ([1] > [2]: none)
    const int32_t *bc_win;
};
// EV: the event store (above); slab: the block's EvSlab when EV is one
template <class EV, int MODE>
__device__ __forceinline__ void consensus_window(const ConsArgs &A, const uint32_t gw, const SiteLists &L, const EvSlab *slab = nullptr)
{
    // Per-column votes of one 375-bp grid window.  A match op votes for the backbone's own base, so a lane (= one
    // overlap) only contributes (a) its coverage interval, through a difference array, and (b) its deviations --
    // mismatches, deleted columns, insertions -- which it finds by skipping the all-match words of its 2-bit path.
    // Deviations are sparse (HiFi: ~1.5 per window), so their LDS atomics do not collide the way per-step votes would.
    __shared__ Tally<EV> S;
    __shared__ uint32_t s_anydev;      // some overlap deviates from the backbone somewhere in this window
    const int lane = threadIdx.x;
    const uint4 gt = A.gwin_tab[gw];
    const uint32_t r = gt.x, pbase = gt.y, n_ovl = gt.z;
    const int g = (int)gt.w;
    const int xlen = A.read_len[r];
    const int gs = g * FSV_WINDOW, glen = min(FSV_WINDOW, xlen - gs);
    S.stage_backbone(lane, A.store + A.word_off[r], gs, xlen);
    uint8_t *dst = A.cwin + (size_t)gw * FSV_CW_STRIDE;
    if (A.read_dirty && !A.read_dirty[r]) {
        // every accepted overlap of this read matches it base for base (from the second round on: most reads): all votes are for
        // the backbone, whatever the coverage
        __syncthreads();
        for (int c = lane; c < glen; c += 64) dst[c] = (uint8_t)S.xb(gs, gs + c);
        if (lane == 0) { A.cwin_len[gw] = (uint16_t)glen; if (MODE == 1) L.site_cnt[gw] = 0u; }
        return;
    }
    S.reset(lane);
    if constexpr (EV::deep) { if (lane == 0) S.ev = *slab; }
    if (lane == 0) s_anydev = 0;
    __syncthreads();
    for (uint32_t oi = lane; oi < n_ovl; oi += 64) {
        const OvlC oc = OvlC::load(&A.ovl_c[pbase + oi]);
        const int o_x_s = oc.x_s(), o_n_win = oc.n_win();
        const int j = g - o_x_s / FSV_WINDOW;
        if (!oc.accepted() || j < 0 || j >= o_n_win) continue;
        const uint32_t ti = oc.first_task() + (uint32_t)j;
        const fsv_wpath *P = A.paths + ti;
        const PathHead h0 = PathHead::load(P);
        const PathY h1 = PathY::load(P);
        // In a read somebody deviates from (the only reads that get here) most paths carry deviations, so the 104 op bytes are
        // requested together with the header: waiting for the header first to learn whether the path is clean cost a second
        // memory round trip per overlap on the window's critical path
        uint2 pv[13];
        load_path_ops(P, pv);
        atomicAdd(&S.cover, 1u);       // get_available_interval (Correct.cpp:113): every accepted overlap that overlaps the window counts, matched there or not
        if (!h0.present()) continue;
        // a path at distance 0 is all matches: it only adds its coverage interval
        const bool clean_path = h0.err() == 0;
        const uint32_t nz = clean_path ? 0u : S.stage_path(lane, pv);
        const int ry_start = h0.ry_start(), plen = h0.len();
        const uint32_t y_word = h1.y_word(); const int y_len = h1.y_len(), y_rev = h0.y_rev();
        const int xs = max(gs, o_x_s) - gs;
        bool pend = false;
        if (j > 0 && A.junction_vote) {
            const PathHead hp = PathHead::load(A.paths + ti - 1);
            if (hp.present()) {
                const int gap = ry_start - hp.ry_end() - 1;
                if (gap > 0 && xs == 0) {
                    pend = true;
                    if (gap <= FSV_INS_MAXLEN) {
                        uint32_t key = (uint32_t)gap << 24;
                        for (int b = 0; b < gap; b++) key |= fsv_base_at(A.store, y_word, y_len, y_rev, ry_start - gap + b) << (2 * b);
                        S.add_event(0, key);
                    }
                }
            }
        }
        if (pend || nz) s_anydev = 1u;
        int n2 = 0;
        if (clean_path) { if (pend) S.cnt_add(xs, 5u); }      // the first op is a match at column xs
        else n2 = cons_walk(S, S.path[lane], nz, plen, xs, glen, pend, A.store, y_word, y_len, y_rev, ry_start);
        // coverage interval: every x base of the task is consumed exactly once
        atomicAdd(&S.cov[xs], 1);
        atomicAdd(&S.cov[xs + plen - n2], -1);
    }
    __syncthreads();
    // fewer than three overlaps: the reference leaves the window alone; no deviation anywhere: every vote is for the backbone
    const bool verbatim = S.cover < 3u || s_anydev == 0u;
    if (A.cov3 && lane == 0) A.cov3[gw] = S.cover >= 3u ? 1 : 0;
    // more events than the buffer holds: flagged, the excess dropped -- or, with deep_sets, the window is listed for k_consensus_deep
    // (so is one whose fl fields could wrap) and what is written below is provisional
    if constexpr (!EV::deep) {
        if (lane == 0 && (S.evn > S.ev.cap() || (A.deep_list && S.cover > 255u))) {
            if (!A.deep_list) atomicOr(&A.warn[r], (uint32_t)FSV_W_INS_EVENTS);
            else if (!verbatim) deep_push(A.deep_list, A.deep_n, A.deep_cap, gw, S.evn);
        }
    }
    const int bc_lo = (MODE == 1 && L.bc_win) ? L.bc_win[3 * (size_t)gw + 1] : 1, bc_hi = (MODE == 1 && L.bc_win) ? L.bc_win[3 * (size_t)gw + 2] : 0;
    bool site = false;
    int c0, c1;
    lane_columns(lane, glen, c0, c1);
    const bool differs = S.decide_columns(lane, c0, c1, gs, glen, xlen, verbatim, A.ins_dag, [&](int c, int arrived, bool) {
        if (MODE != 1) return;
        int oa[4], alt;
#pragma unroll
        for (int b = 0; b < 4; b++) oa[b] = (int)S.cnt_get(c, (uint32_t)b);
        // (a column with two mismatch votes where some overlap's junction cigar shows something else than its window cigar: the
        // tallies of the partition differ from these -- k_snp_sites decides)
        if (oa[0] + oa[1] + oa[2] + oa[3] > 1 && c >= bc_lo && c <= bc_hi) site = true;
        if (split_sub_site(oa, (int)S.cnt_get(c, 4u), arrived, alt)) site = true;
    });
    if (differs && A.changed) A.changed[r] = 1u;
    if (MODE == 1) {
        // a window a used junction cigar reaches into is looked at by k_snp_sites whatever the window cigars say: what its overlaps
        // show beside the junction is read off that cigar there (markSNP_advance, Correct.cpp:5054)
        const bool any_site = __ballot(site) != 0ull || (L.bc_win && L.bc_win[3 * (size_t)gw]);
        if (lane == 0) {
            L.site_cnt[gw] = any_site ? FSV_SITE_MARK : 0u;
            if (any_site) L.win_list[atomicAdd(&L.win_n[0], 1u)] = gw;
        }
    }
    uint8_t (*s_out)[14] = S.out();
    uint32_t mine = 0;
    for (int c = c0; c < c1; c++) mine += s_out[c][0];
    const int incl = wave_incl_sum((int)mine, lane);
    uint32_t off = (uint32_t)incl - mine;
    const uint32_t tot = (uint32_t)__shfl(incl, 63, 64);
    if (tot > FSV_CW_STRIDE) { // cannot happen with <= 12-base insertions winning at a few columns; keep the read as it is
        for (int c = lane; c < glen; c += 64) dst[c] = (uint8_t)S.xb(gs, gs + c);
        if (lane == 0) { A.cwin_len[gw] = (uint16_t)glen; atomicOr(&A.warn[r], (uint32_t)FSV_W_WINDOW_KEPT); }
        return;
    }
    for (int c = c0; c < c1; c++) for (int b = 0; b < s_out[c][0]; b++) dst[off++] = s_out[c][1 + b];
    if (lane == 0) A.cwin_len[gw] = (uint16_t)tot;
}

template <int EVC, int MODE>
__global__ __launch_bounds__(64) void k_consensus(ConsArgs A, uint32_t n_gwin, SiteLists L)
{
    uint32_t gw;
    if (xcd_block(n_gwin, gw)) consensus_window<EvLds<EVC>, MODE>(A, gw, L);
}

// the redo: a fixed grid walks the list k_hap_partition left
template <int EVC>
__global__ __launch_bounds__(64) void k_consensus_redo(ConsArgs A, SiteLists L)
{
    const uint32_t n = L.win_n[1];
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        consensus_window<EvLds<EVC>, 0>(A, L.redo_list[i], L);
        __syncthreads();
    }
}

// deep_sets = 1, once per round after k_consensus_redo (the partition's accepted bits are final): a fixed grid walks the windows the two
// kernels above listed, a wavefront per entry, and writes each one's cwin / cwin_len / changed again from a tally that drops nothing:
// the events in the block's slab of HBM, fl in 16-bit fields.  A window listed twice (by k_consensus and by the redo) comes out the
// same twice.  MODE 1's site marking reads cnt only and stands.  max_events: the largest event count of a listed window.
struct DeepSlabs {
    uint32_t *base; uint32_t cap;      // per block 3 x cap words: keys, links, gathered keys
    uint32_t *max_events;
    __device__ __forceinline__ EvSlab of_block(uint32_t b) const
    {
        uint32_t *p = base + (size_t)b * 3u * cap;
        return EvSlab{p, p + cap, p + 2 * (size_t)cap, cap};
    }
};
__global__ __launch_bounds__(64) void k_consensus_deep(ConsArgs A, SiteLists L, DeepSlabs D)
{
    const uint32_t n = min(*A.deep_n, A.deep_cap);
    const EvSlab ev = D.of_block(blockIdx.x);
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        const uint2 e = A.deep_list[i];
        if (threadIdx.x == 0) atomicMax(D.max_events, e.y);
        consensus_window<EvSlab, 0>(A, e.x, L, &ev);
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ k_bcig_tasks / k_bcig_accept
// calculate_boundary_cigars (Correct.cpp:2310-2530), for the haplotype partition: the junction between two matched windows of an
// accepted overlap whose alignments do not simply meet (bases of y skipped or used twice, or an error within 10 columns of the
// junction on either side) is aligned once more -- up to 100 columns on each side, doubled threshold, no fix_boundary -- and the
// partition reads the ~50 columns on each side of the junction off that cigar unless it has clearly more errors there than the two
// window cigars (markSNP_advance :5054, addSNPtohaplotype_advance :5351).  k_bcig_tasks writes the junction tasks (one thread per
// window task; K5 and the K6 kernels then run on them as on any task list), k_bcig_accept decides which of the new cigars are used.
// oracle/asm.c:boundary_cigars / window_evidence are the same, statement for statement.
#define FSV_BC_SIDE 100
#define FSV_BC_USELESS 50
#define FSV_BC_SCAN 10
struct BcigArgs {
    const fsv_wtask *tasks; const fsv_wpath *paths; const uint32_t *n_tasks;     // the round's window tasks and their paths
    const uint32_t *pair_read, *read_dirty, *gwin_off; const uint8_t *thr_tab; int k_cap;
    fsv_wtask *tasks2; int32_t *bc_idx; uint32_t *n_tasks2;                      // junction tasks; bc_idx[window task] = the task of the junction behind it or -1
    const fsv_wres *res2; const fsv_wpath *paths2; uint4 *bc_rec; int32_t *bc_win;      // bc_win: see SiteLists
    uint32_t *n_same, *n_used;      // statistics: accepted cigars that show what the window cigars show / that are used
};
// op i of a path record's 2-bit stream, through one cached word
struct OpReader {
    const uint32_t *w; uint32_t cur = 0; int idx = -1;
    __device__ __forceinline__ OpReader(const fsv_wpath *P) : w(reinterpret_cast<const uint32_t *>(P->ops)) {}
    __device__ __forceinline__ uint32_t get(int i) { const int wi = i >> 4; if (wi != idx) { cur = w[wi]; idx = wi; } return (cur >> ((i & 15) << 1)) & 3u; }
};
// scan_cigar (Correct.cpp:1070-1200): errors met while the first (dir 0) / last (dir 1) scan_x columns of x go by; y-only ops count
// whenever they are met.  err0: the path's distance (a distance-0 record carries no ops)
__device__ __forceinline__ int scan_ops(const fsv_wpath *P, int plen, int err0, int scan_x, int dir)
{
    if (err0 == 0) return 0;
    OpReader R(P);
    int x_i = 0, err = 0;
    for (int p = 0; p < plen; p++) {
        const uint32_t op = R.get(dir ? plen - 1 - p : p);
        if (op == 2u) { err++; continue; }
        if (op != 0u) err++;
        if (++x_i >= scan_x) return err;
    }
    return err;
}
// scan_cigar_interval (Correct.cpp:1204-1290): errors over the columns [xb, xe] of x
__device__ __forceinline__ int scan_ops_interval(const fsv_wpath *P, int plen, int err0, int xb, int xe)
{
    if (err0 == 0) return 0;
    OpReader R(P);
    int x_i = 0, err = 0;
    for (int p = 0; p < plen; p++) {
        const uint32_t op = R.get(p);
        if (op == 2u) { err++; continue; }
        if (x_i == xb) err = 0;
        x_i++;
        if (op != 0u) err++;
        if (x_i == xe + 1) return err;
    }
    return err;
}

__global__ void k_bcwin_init(int32_t *__restrict__ bc_win, uint32_t n_gwin)
{
    const uint32_t gw = blockIdx.x * blockDim.x + threadIdx.x;
    if (gw < n_gwin) { bc_win[3 * (size_t)gw] = 0; bc_win[3 * (size_t)gw + 1] = 0x7fffffff; bc_win[3 * (size_t)gw + 2] = -1; }
}

__global__ __launch_bounds__(256) void k_bcig_tasks(BcigArgs A)
{
    const uint32_t n_tasks = min(*A.n_tasks, gridDim.x * blockDim.x);
    uint32_t blk;
    if (!xcd_block((n_tasks + 255u) >> 8, blk)) return;
    const uint32_t ti = blk * blockDim.x + threadIdx.x;
    if (ti >= n_tasks) return;
    A.bc_idx[ti] = -1;
    if (ti + 1 >= n_tasks) return;
    // (the two headers say everything about the junction but where it lies: loaded together with the task, one round trip)
    const fsv_wtask t0 = A.tasks[ti];
    // a clean read (most reads from the second round on): every path at distance 0, every junction met -- its path records (a 128-byte
    // line each for 16 bytes of header) are not even looked at
    if (!A.read_dirty[A.pair_read[t0.ovl]]) return;
    const PathHead h0 = PathHead::load(A.paths + ti), h1 = PathHead::load(A.paths + ti + 1);
    if (!h0.present() || !h1.present()) return;     // (a path only exists for a matched window of an accepted overlap)
    const int y_distance = h1.ry_start() - h0.ry_end() - 1;
    // nothing to re-align where the two alignments meet and neither shows an error within ten columns of the junction
    if (y_distance == 0 && !h0.dev_tail() && !h1.dev_head()) return;
    const fsv_wtask t1 = A.tasks[ti + 1];
    if (t1.ovl != t0.ovl) return;                           // the overlap's last window
    int y_start = h0.ry_end(), x_start = t0.x_start + (int)t0.x_len - 1;
    const int leftLen = min(min(x_start - t0.x_start, y_start), FSV_BC_SIDE);
    const int rightLen = min(min(t1.x_start + (int)t1.x_len - x_start, t0.y_len - y_start), FSV_BC_SIDE);
    const int xLen = leftLen + rightLen;
    if (xLen <= 0) return;
    x_start -= leftLen; y_start -= leftLen;
    const int thr = double_thr(A.thr_tab[xLen], xLen, A.k_cap);
    if (thr > FSV_K_MAX) return;
    const uint32_t slot = atomicAdd(A.n_tasks2, 1u);
    fsv_wtask w;
    w.x_word = t0.x_word; w.y_word = t0.y_word; w.x_start = x_start; w.y_start = y_start; w.y_len = t0.y_len;
    w.x_len = (uint16_t)xLen; w.k = (uint8_t)thr; w.y_rev = t0.y_rev; w.ovl = t0.ovl; w.win = ti;
    A.tasks2[slot] = w;
    A.bc_idx[ti] = (int32_t)slot;
}

// one thread per junction task: is its cigar used?  Not when it has clearly more errors in its inner columns than the two window
// cigars have there; and not when it shows, column for column, what the window cigars show (then nothing changes and the windows
// beside it need no second look by k_snp_sites -- most of them: the re-alignment usually finds the two window alignments again)
__global__ __launch_bounds__(256) void k_bcig_accept(BcigArgs A)
{
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= *A.n_tasks2) return;
    A.bc_rec[slot] = make_uint4(0, 0, 0, 0);
    const fsv_wtask w = A.tasks2[slot];
    const fsv_wres r = A.res2[slot];
    const uint32_t ti = w.win;
    const fsv_wpath *PB = A.paths2 + slot, *P0 = A.paths + ti, *P1 = A.paths + ti + 1;
    if (r.err < 0) return;      // (before the record is asked for: K6 left none)
    const PathHead hb = PathHead::load(PB);
    if (!hb.present()) return;
    const int xLen = w.x_len, thr = w.k;
    if (xLen + 2 * thr - r.extra_begin - r.extra_end < xLen) return;      // o_len < xLen
    const fsv_wtask t0 = A.tasks[ti], t1 = A.tasks[ti + 1];
    const PathHead h0 = PathHead::load(P0), h1 = PathHead::load(P1);
    const int x_end0 = t0.x_start + (int)t0.x_len - 1, leftLen = x_end0 - w.x_start, rightLen = xLen - leftLen;
    int y_distance = h1.ry_start() - h0.ry_end() - 1;
    if (y_distance < 0) y_distance = -y_distance;
    int L = FSV_BC_USELESS, R = FSV_BC_USELESS;
    const uint32_t first_ti = ti - t0.win;                  // (window tasks carry their index inside the overlap)
    if (t0.win == 0 && w.x_start == t0.x_start) L = 0;
    {
        // the overlap's last window: the next task belongs to another overlap (or there is none)
        const bool last_junction = ti + 2 >= *A.n_tasks || A.tasks[ti + 2].ovl != t0.ovl;
        if (last_junction && w.x_start + xLen - 1 == t1.x_start + (int)t1.x_len - 1) R = 0;
    }
    (void)first_ti;
    if (leftLen <= L || rightLen <= R) return;
    const int plb = hb.len(), eb = hb.err();
    const int pl0 = h0.len(), e0 = h0.err(), pl1 = h1.len(), e1 = h1.err();
    const int m_err = scan_ops_interval(PB, plb, eb, L, xLen - R - 1);
    const int b_err = scan_ops(P0, pl0, e0, leftLen - L, 1), f_err = scan_ops(P1, pl1, e1, rightLen - R, 0);
    if (f_err + b_err + y_distance + 1 < m_err) return;
    // Does it show anything the window cigars do not?  Column by column over the columns it would be used for: the same op, and
    // for a column with a partner the same base of y (its position).
    bool differs = false, mm0 = false, mm1 = false;
    int lo0 = 0x7fffffff, hi0d = -1, lo1 = 0x7fffffff, hi1d = -1;      // first / last differing junction column on either side
    {
        // columns of the junction cigar that stand for window 0: [L, leftLen] (its last column included); for window 1:
        // [leftLen + 1, leftLen + 1 + (rightLen - 1 - R) - 1] (markSNP_advance's intervals, restated in snp_sites_window)
        OpReader RB(PB), R0(P0), R1(P1);
        int pb = 0, xb = 0, yb = hb.ry_start();
        // window 0 from its column x0c on: skip its ops in front of that column
        const int x0c = (w.x_start + L) - t0.x_start;
        int p0 = 0, x0 = 0, y0 = h0.ry_start();
        if (e0 != 0) { while (p0 < pl0 && x0 < x0c) { const uint32_t op = R0.get(p0++); if (op == 2u) y0++; else { x0++; if (op != 3u) y0++; } } }
        else { x0 = x0c; y0 += x0c; p0 = x0c; }
        if (eb != 0) { while (pb < plb && xb < L) { const uint32_t op = RB.get(pb++); if (op == 2u) yb++; else { xb++; if (op != 3u) yb++; } } }
        else { xb = L; yb += L; pb = L; }
        auto next = [](OpReader &Rd, int &p, int pl, int e, int &y, uint32_t &op_out, int &y_out) {
            // the next op that consumes a column of x: its code and the position of its partner in y
            if (e == 0) { op_out = 0u; y_out = y; y++; p++; return; }
            while (p < pl) { const uint32_t op = Rd.get(p++); if (op == 2u) { y++; continue; } op_out = op; y_out = y; if (op != 3u) y++; return; }
            op_out = 0u; y_out = y;
        };
        const int hi0 = leftLen;                                   // last junction column read for window 0
        for (; xb <= hi0; xb++) {
            uint32_t ob, ow; int ybp, ywp;
            next(RB, pb, plb, eb, yb, ob, ybp);
            next(R0, p0, pl0, e0, y0, ow, ywp);
            if (ob != ow || (ob != 3u && ybp != ywp)) { if (lo0 > xb) lo0 = xb; hi0d = xb; }
            if (ob == 1u || ow == 1u) mm0 = true;
        }
        // window 1: junction columns leftLen + 1 .. leftLen + (rightLen - 1 - R)
        int p1 = 0, y1 = h1.ry_start();
        const int hi1 = leftLen + (rightLen - 1 - R);
        for (; xb <= hi1; xb++) {
            uint32_t ob, ow; int ybp, ywp;
            next(RB, pb, plb, eb, yb, ob, ybp);
            next(R1, p1, pl1, e1, y1, ow, ywp);
            if (ob != ow || (ob != 3u && ybp != ywp)) { if (lo1 > xb) lo1 = xb; hi1d = xb; }
            if (ob == 1u || ow == 1u) mm1 = true;
        }
        differs = lo0 <= hi0d || lo1 <= hi1d;
    }
    if (!differs) { atomicAdd(A.n_same, 1u); return; }
    atomicAdd(A.n_used, 1u);
    A.bc_rec[slot] = make_uint4(1u, (uint32_t)w.x_start, (uint32_t)xLen | ((uint32_t)L << 16) | ((uint32_t)R << 24), 0u);
    // what k_consensus needs to know about the two windows: the columns where the partition's tallies can differ from its own
    const uint32_t rd = A.pair_read[t0.ovl], g0 = A.gwin_off[rd] + (uint32_t)(t0.x_start / FSV_WINDOW);
    const int gs0 = (t0.x_start / FSV_WINDOW) * FSV_WINDOW;
    if (lo0 <= hi0d) {
        if (mm0) A.bc_win[3 * (size_t)g0] = 1;
        atomicMin(&A.bc_win[3 * (size_t)g0 + 1], w.x_start + lo0 - gs0); atomicMax(&A.bc_win[3 * (size_t)g0 + 2], w.x_start + hi0d - gs0);
    }
    if (lo1 <= hi1d) {
        if (mm1) A.bc_win[3 * (size_t)(g0 + 1)] = 1;
        atomicMin(&A.bc_win[3 * (size_t)(g0 + 1) + 1], w.x_start + lo1 - gs0 - FSV_WINDOW); atomicMax(&A.bc_win[3 * (size_t)(g0 + 1) + 2], w.x_start + hi1d - gs0 - FSV_WINDOW);
    }
}

// ------------------------------------------------------------------------------------------------ k_snp_sites / k_hap_partition
// partition_overlaps_advance (Correct.cpp:7127-7206), for every read of every set as hifiasm runs it (it has no notion of a phased
// input: in a phased set the "heterozygous" columns are coincident read errors, and the few overlaps set aside by them are
// what makes the last corrected reads equal hifiasm's).  Two kernels:
//   k_snp_sites     one wavefront per 375-bp grid window: columns where at least two overlaps show a mismatch are candidate
//                   sites (cluster_advance :5585, markSNP_detail :4998); split_sub_list :5804 keeps a site when one alternative
//                   base dominates; every overlap covering a kept site leaves 0 (backbone's base), 1 (that base) or 2 (else) in
//                   the site's vector (InsertSNPVector, Correct.h:630).  Window cigars only: calculate_boundary_cigars :2310
//                   is not restated.
//   k_hap_partition one wavefront per read: generate_haplotypes_DP :6677 -- sites beside another site dropped, overlaps that are
//                   informative / not / informative again set aside (is_match 4), longest chains of mutually compatible sites
//                   enumerated (Preorder_Merge_Advance_Repeat :6233), a chain with support for both alleles
//                   (if_snp_vector_useful :6356) makes the overlaps with the other allele trans (is_match 2).
// oracle/asm.c:partition_read is the same algorithm, statement by statement.
#define FSV_SITE_WIN_CAP 255       // kept sites per grid window (their index in the window is a byte)
#define FSV_SITE_RAW_CAP 1024      // kept sites per read before the sites beside another site are dropped
#define FSV_SITE_READ_CAP 512      // ... and after (the chain DP's predecessor sets are 512-bit)
#define FSV_K7_GROUP_CAP 10000     // chains enumerated per read (the enumeration is exponential in ties; hifiasm has no bound)
struct SiteArgs {
    uint32_t *site_cnt;            // per grid window
    uint2 *site_rec;               // site records, handed out from a pool: {position in the read | homopolymer << 31, byte offset of the vector}
    uint32_t *site_off;            // per grid window: its first record
    uint32_t *rec_cursor; uint32_t rec_cap;
    int8_t *vec;                   // vector pool: one byte per overlap of the read, -1 = does not cover the site
    uint32_t *vec_cursor;          // bytes handed out
    uint32_t vec_cap;
    uint32_t *read_sites;          // per read: some window of it kept a site
    // the re-aligned junction cigars (k_bcig_tasks / k_bcig_accept); nullptr: the window cigars everywhere
    const int32_t *bc_idx;         // per window task: the junction task between it and the next window of its overlap, or -1
    const uint4 *bc_rec;           // per junction task: {bit 0: used, first column in x, columns | L << 16 | R << 24, -}
    const fsv_wpath *bc_paths;     // per junction task: its path
};

__device__ __forceinline__ void snp_sites_window(const ConsArgs &A, const uint32_t gw, const SiteArgs &S)
{
    __shared__ TallyCols T;                        // cnt: A C | G T mismatch votes | x base without partner, -
    __shared__ uint8_t s_alt[FSV_WINDOW + 1];      // 0, or 1 + the dominating other base of a kept site
    __shared__ uint8_t s_sidx[FSV_WINDOW + 1];     // kept site -> its index in the window
    __shared__ uint32_t s_nsite, s_vbase, s_rbase;
    __shared__ uint32_t s_scan[64];
    const int lane = threadIdx.x;
    const uint4 gt = A.gwin_tab[gw];
    const uint32_t r = gt.x, pbase = gt.y, n_ovl = gt.z;
    const int g = (int)gt.w;
    const int xlen = A.read_len[r];
    const int gs = g * FSV_WINDOW, glen = min(FSV_WINDOW, xlen - gs);
    if (lane == 0) S.site_cnt[gw] = 0;
    T.stage_backbone(lane, A.store + A.word_off[r], gs, xlen);
    T.reset(lane);
    for (int i = lane; i < FSV_WINDOW + 1; i += 64) s_alt[i] = 0;
    if (lane == 0) s_nsite = 0;
    __syncthreads();
    const uint32_t vstride = (n_ovl + 3u) & ~3u;
    for (int pass = 0; pass < 2; pass++) {
        for (uint32_t oi = lane; oi < n_ovl; oi += 64) {
            const OvlC oc = OvlC::load(&A.ovl_c[pbase + oi]);
            const int o_x_s = oc.x_s(), o_n_win = oc.n_win();
            const int j = g - o_x_s / FSV_WINDOW;
            if (!oc.accepted() || j < 0 || j >= o_n_win) continue;
            const uint32_t ti = oc.first_task() + (uint32_t)j;
            const fsv_wpath *P = A.paths + ti;
            if (!PathHead::load(P).present()) continue;
            const int xs = max(gs, o_x_s) - gs;
            if (pass == 0) atomicAdd(&T.cover, 1u);
            // What the overlap shows at the columns [lo, hi] (counted from the cigar's first column, which is column x0 of the read)
            // of one cigar.  pass 0: mismatches and x bases without a partner are tallied (markSNP_detail, Correct.cpp:4998);
            // pass 1: the kept sites get their evidence (addSNPtohaplotype_details :5247).  Returns the cigar's x columns.
            auto walk = [&](const fsv_wpath *Q, int x0, int lo, int hi) -> int {
                const PathHead q0 = PathHead::load(Q);
                const int plen = q0.len(), ry0 = q0.ry_start(), col0 = x0 - gs;
                if (q0.err() == 0) {          // distance 0: all matches, the record carries no ops
                    if (pass == 1) for (int xi = max(lo, -col0); xi <= min(hi, plen - 1) && col0 + xi < glen; xi++) if (s_alt[col0 + xi]) S.vec[s_vbase + (uint32_t)s_sidx[col0 + xi] * vstride + oi] = 0;
                    return plen;
                }
                const PathY q1 = PathY::load(Q);
                const uint32_t y_word = q1.y_word(); const int y_len = q1.y_len(), y_rev = q0.y_rev();
                uint2 pv[13];
                load_path_ops(Q, pv);
                T.stage_path(lane, pv);
                int n2 = 0, n3 = 0;
                for (int p = 0; p < plen; p++) {
                    const uint32_t rest = T.path[lane][p >> 4] >> ((p & 15) << 1);
                    if (pass == 0 && rest == 0u) { p = (((p >> 4) + 1) << 4) - 1; continue; }    // the rest of the word: matches
                    const uint32_t op = rest & 3u;
                    if (op == 2u) { n2++; continue; }
                    const int xi = p - n2, c = col0 + xi;
                    if (xi >= lo && xi <= hi && c >= 0 && c < glen) {
                        if (pass == 0) {
                            if (op == 3u) T.cnt_add(c, 4u);
                            else if (op == 1u) T.cnt_add(c, fsv_base_at(A.store, y_word, y_len, y_rev, ry0 + p - n3));
                        } else {
                            const uint32_t alt = s_alt[c];
                            if (alt) {
                                int8_t v = 0;
                                if (op == 3u) v = 2;
                                else if (op == 1u) v = fsv_base_at(A.store, y_word, y_len, y_rev, ry0 + p - n3) + 1u == alt ? 1 : 2;
                                S.vec[s_vbase + (uint32_t)s_sidx[c] * vstride + oi] = v;
                            }
                        }
                    }
                    if (op == 3u) n3++;
                }
                return plen - n2;
            };
            // the window cigar in the middle; beside a junction whose re-aligned cigar is in use, that cigar (markSNP_advance :5054)
            int cur_beg = 0, cur_end = 0x7fffffff;
            if (S.bc_idx) {
                const int32_t sb = j >= 1 ? S.bc_idx[ti - 1] : -1, se = j + 1 < o_n_win ? S.bc_idx[ti] : -1;
                const uint4 rb = sb >= 0 ? S.bc_rec[sb] : make_uint4(0, 0, 0, 0), re = se >= 0 ? S.bc_rec[se] : make_uint4(0, 0, 0, 0);
                if ((rb.x | re.x) & 1u) {
                    const fsv_wtask t = A.tasks[ti];
                    const int x_total_start = t.x_start, x_length = t.x_len, x_total_end = x_total_start + x_length - 1;
                    if (rb.x & 1u) {
                        const int bx = (int)rb.y, blen = (int)(rb.z & 0xffffu), bL = (int)((rb.z >> 16) & 0xffu), bR = (int)(rb.z >> 24);
                        const int xleft = x_total_start - bx, xright = bx + blen - 1 - x_total_start + 1;
                        if (xleft > bL && xright > bR) { cur_beg = xright - bR; walk(S.bc_paths + sb, bx, xleft, xleft + (xright - bR) - 1); }
                    }
                    if (re.x & 1u) {
                        const int bx = (int)re.y, blen = (int)(re.z & 0xffffu), bL = (int)((re.z >> 16) & 0xffu), bR = (int)(re.z >> 24);
                        const int xleft = x_total_end - bx, xright = bx + blen - 1 - x_total_end + 1;
                        if (xleft > bL && xright > bR) { cur_end = (x_length - 1) - ((xleft + 1) - bL); walk(S.bc_paths + se, bx, bL, xleft); }
                    }
                }
            }
            const int xcols = walk(P, gs + xs, cur_beg, cur_end);
            if (pass == 0) {
                atomicAdd(&T.cov[xs], 1);
                atomicAdd(&T.cov[xs + xcols], -1);
            }
        }
        __syncthreads();
        if (pass == 1 || T.cover == 0u) break;
        // arrived[c] = prefix sum of the difference array
        int c0, c1, run = 0;
        lane_columns(lane, glen, c0, c1);
        for (int c = c0; c < c1; c++) run += T.cov[c];
        s_scan[lane] = (uint32_t)run;
        __syncthreads();
        int arrived = 0, mine = 0;
        for (int i = 0; i < lane; i++) arrived += (int)s_scan[i];
        for (int c = c0; c < c1; c++) {
            arrived += T.cov[c];
            int oa[4], alt;
#pragma unroll
            for (int b = 0; b < 4; b++) oa[b] = (int)T.cnt_get(c, (uint32_t)b);
            if (!split_sub_site(oa, (int)T.cnt_get(c, 4u), arrived, alt)) continue;
            s_alt[c] = (uint8_t)(alt + 1);
            mine++;
        }
        s_scan[lane] = (uint32_t)mine;
        __syncthreads();
        int first = 0, all = 0;
        for (int i = 0; i < 64; i++) { if (i < lane) first += (int)s_scan[i]; all += (int)s_scan[i]; }
        if (all == 0) break;
        if (all > FSV_SITE_WIN_CAP) { if (lane == 0) atomicOr(&A.warn[r], (uint32_t)FSV_W_SITES); break; }
        if (lane == 0) {
            const uint32_t off = atomicAdd(S.vec_cursor, (uint32_t)all * vstride), roff = atomicAdd(S.rec_cursor, (uint32_t)all);
            s_vbase = off; s_rbase = roff;
            s_nsite = (off + (uint32_t)all * vstride <= S.vec_cap && roff + (uint32_t)all <= S.rec_cap) ? (uint32_t)all : 0u;
            if (!s_nsite) atomicOr(&A.warn[r], (uint32_t)FSV_W_SITES);
        }
        __syncthreads();
        if (!s_nsite) break;
        for (uint32_t i = lane; i < (uint32_t)all * vstride; i += 64) S.vec[s_vbase + i] = -1;
        for (int c = c0, k = first; c < c1; c++) {
            if (!s_alt[c]) continue;
            s_sidx[c] = (uint8_t)k;
            const int p = gs + c;
            const bool homo = homo_strict([&](int pp) { return T.xb(gs, pp); }, p, xlen);
            S.site_rec[(size_t)s_rbase + k] = make_uint2((uint32_t)p | (homo ? 0x80000000u : 0u), s_vbase + (uint32_t)k * vstride);
            k++;
        }
        if (lane == 0) { S.site_cnt[gw] = (uint32_t)all; S.site_off[gw] = s_rbase; S.read_sites[r] = 1u; }
        __threadfence_block();
        __syncthreads();
    }
}

// the windows k_consensus<., 1> marked (a fixed grid walks the list)
__global__ __launch_bounds__(64) void k_snp_sites(ConsArgs A, SiteArgs S, SiteLists L)
{
    const uint32_t n = L.win_n[0];
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        snp_sites_window(A, L.win_list[i], S);
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void k_hap_partition(ConsArgs A, SiteArgs S, fsv_ovl *__restrict__ ovl, uint4 *__restrict__ ovl_c, SiteLists L)
{
    __shared__ int32_t s_pos[FSV_SITE_RAW_CAP];
    __shared__ uint32_t s_voff[FSV_SITE_RAW_CAP];
    __shared__ uint16_t s_max[FSV_SITE_READ_CAP], s_order[FSV_SITE_READ_CAP];
    __shared__ uint32_t s_bt[FSV_SITE_READ_CAP][FSV_SITE_READ_CAP / 32];   // predecessors on a longest chain, as a bit set
    __shared__ uint16_t s_buf[FSV_SITE_READ_CAP], s_cur[FSV_SITE_READ_CAP]; // the chain being walked; per depth, the next predecessor to try
    __shared__ uint8_t s_visit[FSV_SITE_READ_CAP], s_keep[FSV_SITE_RAW_CAP];
    __shared__ uint32_t s_n;
    const int lane = threadIdx.x;
    __shared__ uint32_t s_redo;
    const uint32_t r = blockIdx.x;
    if (r >= A.n_reads || !S.read_sites[r]) return;
    const uint32_t g0 = A.gwin_off[r], g1 = A.gwin_off[r + 1];
    if (g0 == g1) return;
    if (lane == 0) s_redo = 0;
    const uint4 gt = A.gwin_tab[g0];
    const uint32_t pbase = gt.y, n_ovl = gt.z;
    // the read's kept sites in position order
    if (lane == 0) s_n = 0;
    __syncthreads();
    for (uint32_t gb = g0; gb < g1; gb += 64) {
        const uint32_t gw = gb + lane;
        const uint32_t c = gw < g1 ? S.site_cnt[gw] : 0u;
        uint32_t incl = c;
        for (int d = 1; d < 64; d <<= 1) { const uint32_t v = __shfl_up(incl, d); if (lane >= d) incl += v; }   // (wave_incl_sum: written out, the call reorders this kernel's code)
        const uint32_t base = s_n + incl - c;
        for (uint32_t k = 0; k < c; k++)
            if (base + k < FSV_SITE_RAW_CAP) { const uint2 rec = S.site_rec[(size_t)S.site_off[gw] + k]; s_pos[base + k] = (int32_t)rec.x; s_voff[base + k] = rec.y; }
        __syncthreads();
        if (lane == 63) s_n = base + c;
        __syncthreads();
    }
    int nS = (int)s_n;
    if (nS == 0) return;
    if (nS > FSV_SITE_RAW_CAP) { if (lane == 0) atomicOr(&A.warn[r], (uint32_t)FSV_W_SITES); return; }
    // a site directly beside another one is dropped
    if (nS > 1) {
        for (int j = lane; j < nS; j += 64) {
            const int p = s_pos[j] & 0x7fffffff;
            const bool left = j > 0 && p == (s_pos[j - 1] & 0x7fffffff) + 1, right = j + 1 < nS && p + 1 == (s_pos[j + 1] & 0x7fffffff);
            s_keep[j] = !(left || right);
        }
        __syncthreads();
        if (lane == 0) {
            int m = 0;
            for (int j = 0; j < nS; j++) if (s_keep[j]) { s_pos[m] = s_pos[j]; s_voff[m] = s_voff[j]; m++; }
            s_n = (uint32_t)m;
        }
        __syncthreads();
        nS = (int)s_n;
        if (nS == 0) return;
    }
    if (nS > FSV_SITE_READ_CAP) { if (lane == 0) atomicOr(&A.warn[r], (uint32_t)FSV_W_SITES); return; }
    // informative, not informative, informative again: the overlap is set aside
    for (uint32_t i = lane; i < n_ovl; i += 64) {
        if (!OvlC::load(&ovl_c[pbase + i]).accepted()) continue;
        int st = -1;
        for (int j = 0; j < nS; j++) {
            const int8_t v = S.vec[s_voff[j] + i];
            const bool inf = v == 0 || v == 1;
            if (st == -1) { if (inf) st = 0; }
            else if (st == 0) { if (!inf) st = 2; }
            else if (inf) { st = 3; break; }
        }
        if (st == 3) {
            for (int j = 0; j < nS; j++) S.vec[s_voff[j] + i] = 2;
            ovl[pbase + i].is_match = 4;
            OvlC::clear_accepted(&ovl_c[pbase + i]);
            s_redo = 1u;
        }
    }
    __threadfence_block();
    __syncthreads();
    // longest chains of mutually compatible sites
    for (int i = 0; i < nS; i++) {
        if (lane < FSV_SITE_READ_CAP / 32) s_bt[i][lane] = 0;
        int best = 1;
        for (int j = 0; j < i; j++) {
            bool bad = false;
            for (uint32_t o = lane; o < n_ovl; o += 64) {
                const int8_t a = S.vec[s_voff[i] + o], b = S.vec[s_voff[j] + o];
                if (a != b && (a == 0 || a == 1) && (b == 0 || b == 1)) bad = true;
            }
            if (__ballot(bad)) continue;
            const int cand = (int)s_max[j] + 1;
            if (cand > best) {
                best = cand;
                if (lane < FSV_SITE_READ_CAP / 32) s_bt[i][lane] = 0;
            }
            if (cand == best && lane == 0) s_bt[i][j >> 5] |= 1u << (j & 31);
            __syncthreads();
        }
        if (lane == 0) { s_max[i] = (uint16_t)best; s_visit[i] = 0; }
        __syncthreads();
    }
    // longest first, ties in site order (a stable sort, as glibc's qsort is for arrays this small)
    for (int i = lane; i < nS; i += 64) {
        int rank = 0;
        for (int j = 0; j < nS; j++) rank += (s_max[j] > s_max[i]) || (s_max[j] == s_max[i] && j < i);
        s_order[rank] = (uint16_t)i;
    }
    __syncthreads();
    uint32_t n_groups = 0;
    for (int oi = 0; oi < nS; oi++) {
        const int root = s_order[oi];
        if (s_visit[root]) continue;          // uniform: s_visit is only written between barriers
        // depth-first over the predecessor sets, ascending site index (Preorder_Merge_Advance_Repeat)
        int depth = 0;
        if (lane == 0) { s_buf[0] = (uint16_t)root; s_cur[0] = 0; s_visit[root] = 1; }
        __syncthreads();
        while (depth >= 0) {
            const int id = s_buf[depth];
            bool leaf = true;
            for (int w = 0; w < FSV_SITE_READ_CAP / 32; w++) if (s_bt[id][w]) leaf = false;
            if (leaf) {
                if (n_groups <= FSV_K7_GROUP_CAP) {
                    // process_repeat_snps for the chain s_buf[0 .. depth]: first informative entry of every overlap
                    const int plen = depth + 1;
                    int occ0 = 0, occ1 = 0;
                    for (uint32_t ob = 0; ob < n_ovl; ob += 64) {
                        const uint32_t o = ob + lane;
                        int8_t rv = -1;
                        if (o < n_ovl) for (int k = 0; k < plen && rv == -1; k++) { const int8_t v = S.vec[s_voff[s_buf[k]] + o]; if (v == 0 || v == 1) rv = v; }
                        occ0 += __popcll(__ballot(rv == 0));
                        occ1 += __popcll(__ballot(rv == 1));
                    }
                    bool useful = false;
                    if (occ0 && occ1) {
                        const double low = (double)(occ0 + occ1) * 0.3;
                        if ((double)occ1 >= low && (double)occ0 >= low) useful = true;
                        else if (occ1 >= 5 && occ0 >= 5) useful = true;
                        else if (occ1 >= 3 && occ0 >= 3 && plen >= 2) {
                            int far = 0;
                            for (int k = 0; k < plen; k++) {
                                const int cur = s_pos[s_buf[k]] & 0x7fffffff;
                                bool nearby = false;
                                if (k > 0 && (s_pos[s_buf[k - 1]] & 0x7fffffff) - cur < 10) nearby = true;
                                if (k + 1 < plen && cur - (s_pos[s_buf[k + 1]] & 0x7fffffff) < 10) nearby = true;
                                if (!nearby) far++;
                            }
                            useful = far > 0;
                        }
                    }
                    if (useful)
                        for (uint32_t o = lane; o < n_ovl; o += 64) {
                            int8_t rv = -1;
                            for (int k = 0; k < plen && rv == -1; k++) { const int8_t v = S.vec[s_voff[s_buf[k]] + o]; if (v == 0 || v == 1) rv = v; }
                            if (rv == 1 && OvlC::load(&ovl_c[pbase + o]).accepted()) { ovl[pbase + o].is_match = 2; OvlC::clear_accepted(&ovl_c[pbase + o]); s_redo = 1u; }
                        }
                    n_groups++;
                }
                depth--;
                continue;
            }
            // next predecessor of id at or after s_cur[depth]
            int nxt = -1;
            for (int j = s_cur[depth]; j < id; j++) if (s_bt[id][j >> 5] >> (j & 31) & 1u) { nxt = j; break; }
            __syncthreads();
            if (nxt < 0 || n_groups > FSV_K7_GROUP_CAP) { depth--; continue; }
            if (lane == 0) { s_cur[depth] = (uint16_t)(nxt + 1); s_buf[depth + 1] = (uint16_t)nxt; s_cur[depth + 1] = 0; s_visit[nxt] = 1; }
            __syncthreads();
            depth++;
        }
        __syncthreads();
    }
    // a read that lost an overlap: its windows get their consensus again
    if (s_redo) {
        uint32_t base = lane == 0 ? atomicAdd(&L.win_n[1], g1 - g0) : 0u;
        base = __shfl(base, 0);
        for (uint32_t i = lane; i < g1 - g0; i += 64) L.redo_list[base + i] = g0 + i;
    }
}

// ------------------------------------------------------------------------------------------------ second consensus pass
// process_boundary (Correct.cpp:4453-4728) + merge_cigars (:4267): after the grid windows, every junction between two windows of a
// read once more.  Backbone = the 375 bases of the FIRST pass's result centred on the junction (read from a 2-bit copy of that
// result placed behind the round's read store, so K5 / K6 run on it as on any window task); every overlap that covers the start
// of the later window is re-aligned to it, threshold doubled once on failure; the inner bases (25 off either end) are replaced
// by the consensus of those alignments, from the first to the last column that keeps a base.  The replacement is handed to the
// two windows it touches as patches (k_bnd_apply) so that k_newlen / k_repack work on the windows as before.
// oracle/asm.c:correct_read (second_round) is the same, statement for statement.
#define FSV_BND_HALF 187
#define FSV_BND_SIDE 25
struct BndArgs {
    const fsv_wtask *tasks; const fsv_wpath *paths; const uint32_t *n_tasks;     // the round's window tasks and their paths
    const uint4 *ovl_c; const uint32_t *pair_base, *set_start; uint32_t n_sets; const uint32_t *pair_read;   // pair slot -> its query read
    const uint32_t *gwin_off, *lb; const uint16_t *cwin_len; const uint8_t *cov3; const uint32_t *read_dirty;
    const uint32_t *brel_off; uint32_t b_base;      // first-pass result of read r in the second-pass store: word b_base + brel_off[r]
    const uint8_t *thr_tab;
    fsv_wtask *tasks2; int32_t *idx2; uint32_t *n_tasks2;      // junction tasks; idx2[window task] = its junction task or -1
    uint32_t *bnd_flag, *bnd_list, *n_bnd;                    // per junction: bit 0 = has a task (and is in the list), the rest = alignments that match base for base
    const uint32_t *store2;                                   // the second-pass store: the round's reads, then the first pass's result
    uint2 *deep_list; uint32_t *deep_n; uint32_t deep_cap;    // deep_sets = 1 (nullptr: off): junctions set aside for k_bnd_consensus_deep, as ConsArgs::deep_list
};

__global__ __launch_bounds__(256) void k_bnd_tasks(BndArgs A)
{
    const uint32_t n_tasks = min(*A.n_tasks, gridDim.x * blockDim.x);   // the grid covers the task bound
    uint32_t blk;
    if (!xcd_block((n_tasks + 255u) >> 8, blk)) return;
    const uint32_t ti = blk * blockDim.x + threadIdx.x;
    if (ti >= n_tasks) return;
    A.idx2[ti] = -1;
    const fsv_wtask t = A.tasks[ti];
    if (t.x_start % FSV_WINDOW != 0 || t.x_start == 0) return;    // only an overlap that covers the window's first base takes part
    // the tests are grouped so that the loads they need are in flight together: one test per load is one memory round trip per test
    const uint32_t p = t.ovl;
    const uint32_t r = A.pair_read[p];
    const uint32_t dirty = A.read_dirty[r], gwo = A.gwin_off[r];
    // a clean read: every overlap matches it base for base, every junction alignment has distance 0 -- its overlap record and its path
    // header (a 128-byte line for 16 bytes) are not asked for
    if (!dirty) return;
    const OvlC oc = OvlC::load(&A.ovl_c[p]);
    const PathHead h0 = PathHead::load(A.paths + ti);
    if (!(oc.accepted() && h0.present())) return;
    const uint32_t gw = gwo + (uint32_t)(t.x_start / FSV_WINDOW);
    const uint32_t cov = A.cov3[gw], cwl = A.cwin_len[gw];
    const int LB = (int)A.lb[gw];
    if (!cov || LB == 0) return;
    const int len_now = LB + (int)cwl;
    const int cws = max(0, LB - FSV_BND_HALF), cwe = min(len_now - 1, LB + FSV_BND_HALF - 1), blen = cwe - cws + 1;
    const int y_start = h0.ry_start() - FSV_BND_HALF;
    if (y_start < 0 || blen < 1) return;
    // about half of the partner reads match the first pass's result base for base on the predicted diagonal (K5 would report distance 0
    // ending on that diagonal, K6 an all-match path): such an alignment only counts towards the junction's coverage
    const uint32_t xw2 = A.b_base + A.brel_off[r];
    if (y_start + blen <= t.y_len) {
        // (all six 64-base fetches of either read in flight: with an early exit per 16 bases an exact alignment -- the common case --
        // paid 24 dependent round trips)
        uint32_t acc = 0;
#pragma unroll
        for (int c = 0; c < 6; c++) {
            if (c * 64 < blen) {
                uint32_t xb[4], yb[4], yv[4];
                fetch64_x(A.store2, xw2, cws + c * 64, xb);
                fetch64(A.store2, t.y_word, t.y_len, t.y_rev, y_start + c * 64, yb, yv);
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int b = c * 64 + j * 16;
                    if (b < blen) {
                        const int lim = min(16, blen - b);
                        acc |= (xb[j] ^ yb[j]) & (lim < 16 ? (1u << (2 * lim)) - 1u : 0xffffffffu);
                    }
                }
            }
        }
        const bool same = acc == 0u;
        if (same) { A.idx2[ti] = -2; atomicAdd(&A.bnd_flag[gw], 2u); return; }
    }
    const uint32_t slot = atomicAdd(A.n_tasks2, 1u);
    fsv_wtask w;
    w.x_word = xw2; w.y_word = t.y_word; w.x_start = cws; w.y_start = y_start; w.y_len = t.y_len;
    w.x_len = (uint16_t)blen; w.k = A.thr_tab[blen]; w.y_rev = t.y_rev; w.ovl = p; w.win = ti;
    A.tasks2[slot] = w;
    A.idx2[ti] = (int32_t)slot;
    if (!(atomicOr(&A.bnd_flag[gw], 1u) & 1u)) A.bnd_list[atomicAdd(A.n_bnd, 1u)] = gw;
}

// junction tasks K5 found no alignment for get the doubled threshold (Correct.cpp:4585-4626) and go round once more
__global__ __launch_bounds__(256) void k_bnd_retry(fsv_wtask *__restrict__ tasks2, const fsv_wres *__restrict__ res2, const uint32_t *__restrict__ n_tasks2,
                                                   fsv_wtask *__restrict__ tasks3, uint32_t *__restrict__ src3, uint32_t *__restrict__ n3, int k_cap)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= *n_tasks2 || res2[i].err >= 0) return;
    fsv_wtask t = tasks2[i];
    t.k = (uint8_t)double_thr(t.k, t.x_len, k_cap);
    tasks2[i].k = t.k;
    const uint32_t j = atomicAdd(n3, 1u);
    tasks3[j] = t; src3[j] = i;
}

__global__ __launch_bounds__(256) void k_bnd_scatter(fsv_wres *__restrict__ res2, const fsv_wres *__restrict__ res3, const uint32_t *__restrict__ src3,
                                                     const uint32_t *__restrict__ n3)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < *n3) res2[src3[j]] = res3[j];
}

// what a junction hands to the two windows it touches: in window gw-1 the bases [ts, ts + told) become tnew bytes, in window
// gw the bases [hs, hs + hold) become hnew bytes (the tail bytes first in the junction's byte slot)
struct BndPatch { uint16_t ts, told, tnew, hs, hold, hnew, valid, pad; };

template <class EV>
struct BndLds : Tally<EV> {
    uint32_t terr;
    uint16_t off[FSV_WINDOW + 2];   // where a column's output starts in the consensus
    uint8_t own[FSV_WINDOW + 1];    // the column keeps a base (its own or another one)
};
// the junction in front of grid window gw: its patch, or patch[gw].valid = 0.  SPILL: deep_sets = 1 (B.deep_list is there)
template <class EV, bool SPILL>
__device__ __forceinline__ void bnd_junction(const ConsArgs &A, const BndArgs &B, const fsv_wpath *__restrict__ paths2, const uint32_t *__restrict__ store2,
                                             BndPatch *__restrict__ patch, uint8_t *__restrict__ patch_bytes, const uint32_t gw, const EvSlab *slab = nullptr)
{
    static_assert(2 * FSV_BND_HALF + 1 <= FSV_WINDOW, "a junction's backbone fits the tally of a window");
    __shared__ BndLds<EV> S;
    const int lane = threadIdx.x;
    const uint4 gt = A.gwin_tab[gw];
    const uint32_t r = gt.x, pbase = gt.y, n_ovl = gt.z;
    const int g = (int)gt.w;
    const int gs = g * FSV_WINDOW;
    const int LB = (int)B.lb[gw], len_now = LB + (int)B.cwin_len[gw];
    const int cws = max(0, LB - FSV_BND_HALF), cwe = min(len_now - 1, LB + FSV_BND_HALF - 1), blen = cwe - cws + 1;
    if (lane == 0) { patch[gw].valid = 0; S.terr = 0; }
    S.stage_backbone(lane, store2 + B.b_base + B.brel_off[r], cws, len_now);
    S.reset(lane);
    if constexpr (EV::deep) { if (lane == 0) S.ev = *slab; }
    __syncthreads();
    for (uint32_t oi = lane; oi < n_ovl; oi += 64) {
        const OvlC oc = OvlC::load(&A.ovl_c[pbase + oi]);
        const int o_x_s = oc.x_s(), o_n_win = oc.n_win();
        const int j = g - o_x_s / FSV_WINDOW;
        if (!oc.accepted() || j < 0 || j >= o_n_win || o_x_s > gs) continue;
        const int32_t slot = B.idx2[oc.first_task() + (uint32_t)j];
        if (slot == -2) { atomicAdd(&S.cover, 1u); atomicAdd(&S.cov[0], 1); atomicAdd(&S.cov[blen], -1); continue; }   // matches base for base
        if (slot < 0) continue;
        const fsv_wpath *P = paths2 + slot;
        const PathHead h0 = PathHead::load(P);
        if (!h0.present()) continue;
        const PathY h1 = PathY::load(P);
        const int perr = h0.err();
        atomicAdd(&S.cover, 1u);
        const int ry_start = h0.ry_start(), plen = h0.len();
        int n2 = 0;
        if (perr != 0) {
            atomicAdd(&S.terr, (uint32_t)perr);
            uint2 pv[13];
            load_path_ops(P, pv);
            const uint32_t nz = S.stage_path(lane, pv);
            n2 = cons_walk(S, S.path[lane], nz, plen, 0, blen, false, A.store, h1.y_word(), h1.y_len(), h0.y_rev(), ry_start);
        }
        atomicAdd(&S.cov[0], 1);
        atomicAdd(&S.cov[plen - n2], -1);
    }
    __syncthreads();
    if (S.cover < 3u || S.terr == 0u) return;         // MIN_COVERAGE_THRESHOLD; "if there are no error, we do not need correction"
    // as in consensus_window: flagged, or with deep_sets listed for k_bnd_consensus_deep and the patch below provisional.  (SPILL is a
    // template parameter here: as a run-time test of B.deep_list the branch cost the kernel a VGPR)
    if constexpr (!EV::deep) {
        if (lane == 0 && (S.evn > S.ev.cap() || (SPILL && S.cover > 255u))) {
            if (!SPILL) atomicOr(&A.warn[r], (uint32_t)FSV_W_INS_EVENTS);
            else deep_push(B.deep_list, B.deep_n, B.deep_cap, gw, S.evn);
        }
    }
    int c0, c1;
    lane_columns(lane, blen, c0, c1);
    for (int c = c0; c < c1; c++) S.own[c] = 1;
    const bool differs = S.decide_columns(lane, c0, c1, cws, blen, len_now, false, A.ins_dag, [&](int c, int, bool kept) { S.own[c] = kept; });
    uint8_t (*s_out)[14] = S.out();
    int mine = 0;
    for (int c = c0; c < c1; c++) mine += s_out[c][0];
    if (__ballot(differs) == 0ull) return;            // the new cigar is one run of matches
    int off = wave_incl_sum(mine, lane) - mine;
    for (int c = c0; c < c1; c++) { S.off[c] = (uint16_t)off; off += s_out[c][0]; }
    // the first and the last column to replace: the first kept column at or after 25 / at or after blen - 1 - 25
    const int sb = FSV_BND_SIDE, eb = blen - 1 - FSV_BND_SIDE;
    int fs = 0x7fffffff, fe = 0x7fffffff;
    for (int c = c0; c < c1; c++) { if (S.own[c] && c >= sb && c < fs) fs = c; if (S.own[c] && c >= eb && c < fe) fe = c; }
    for (int d = 32; d >= 1; d >>= 1) { fs = min(fs, __shfl_xor(fs, d)); fe = min(fe, __shfl_xor(fe, d)); }
    __syncthreads();
    if (eb <= sb || fs == 0x7fffffff || fe == 0x7fffffff) return;     // "if there are some gap at the end of x, it very likely miscorrection"
    const int o0 = (int)S.off[fs] + s_out[fs][0] - 1, o1 = (int)S.off[fe] + s_out[fe][0] - 1;   // the two kept bases in the consensus
    const int R0 = cws + fs, R1 = cws + fe, sc = LB - cws;    // first-pass coordinates of the stretch; sc: the later window's first column
    const int o_split = sc <= fs ? o0 : (sc > fe ? o1 + 1 : (int)S.off[sc]);
    const int lb_prev = (int)B.lb[gw - 1];
    BndPatch bp;
    bp.valid = 1; bp.pad = 0;
    bp.ts = (uint16_t)max(0, R0 - lb_prev); bp.told = (uint16_t)max(0, min(R1, LB - 1) - R0 + 1); bp.tnew = (uint16_t)(o_split - o0);
    bp.hs = (uint16_t)(max(R0, LB) - LB); bp.hold = (uint16_t)max(0, R1 - max(R0, LB) + 1); bp.hnew = (uint16_t)(o1 + 1 - o_split);
    if (R0 < lb_prev || o1 + 1 - o0 > FSV_CW_STRIDE) {     // the stretch would reach a third window / outgrow its slot: left as the first pass had it
        if (lane == 0) atomicOr(&A.warn[r], (uint32_t)FSV_W_WINDOW_KEPT);
        return;
    }
    uint8_t *dst = patch_bytes + (size_t)gw * FSV_CW_STRIDE;
    for (int c = c0; c < c1; c++)
        for (int b = 0; b < s_out[c][0]; b++) { const int pos = (int)S.off[c] + b; if (pos >= o0 && pos <= o1) dst[pos - o0] = s_out[c][1 + b]; }
    if (lane == 0) patch[gw] = bp;
}

template <int EVC, bool SPILL>
__global__ __launch_bounds__(64) void k_bnd_consensus(ConsArgs A, BndArgs B, const fsv_wpath *__restrict__ paths2, const uint32_t *__restrict__ store2,
                                                      BndPatch *__restrict__ patch, uint8_t *__restrict__ patch_bytes)
{
    const uint32_t n_list = *B.n_bnd;
    for (uint32_t li = blockIdx.x; li < n_list; li += gridDim.x) {
        __syncthreads();
        bnd_junction<EvLds<EVC>, SPILL>(A, B, paths2, store2, patch, patch_bytes, B.bnd_list[li]);
    }
}

// deep_sets = 1, before k_bnd_apply: the junctions k_bnd_consensus listed get their patch again from a tally that drops nothing (see
// k_consensus_deep)
__global__ __launch_bounds__(64) void k_bnd_consensus_deep(ConsArgs A, BndArgs B, const fsv_wpath *__restrict__ paths2, const uint32_t *__restrict__ store2,
                                                           BndPatch *__restrict__ patch, uint8_t *__restrict__ patch_bytes, DeepSlabs D)
{
    const uint32_t n = min(*B.deep_n, B.deep_cap);
    const EvSlab ev = D.of_block(blockIdx.x);
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        __syncthreads();
        const uint2 e = B.deep_list[i];
        if (threadIdx.x == 0) atomicMax(D.max_events, e.y);
        bnd_junction<EvSlab, false>(A, B, paths2, store2, patch, patch_bytes, e.x, &ev);
    }
}

// one wavefront per grid window: the window with the patches of its two junctions applied, in place
__global__ __launch_bounds__(64) void k_bnd_apply(const uint32_t *__restrict__ gwin_read, const uint32_t *__restrict__ gwin_off, const BndPatch *__restrict__ patch,
                                                  const uint8_t *__restrict__ patch_bytes, const uint32_t *__restrict__ bnd_flag, uint32_t n_gwin,
                                                  uint8_t *__restrict__ cwin, uint16_t *__restrict__ cwin_len, uint32_t *__restrict__ changed, uint32_t *__restrict__ warn)
{
    __shared__ uint8_t s_old[FSV_CW_STRIDE];
    const uint32_t gw = blockIdx.x;
    if (gw >= n_gwin) return;
    const uint32_t r = gwin_read[gw];
    const bool has_h = gw > gwin_off[r] && (bnd_flag[gw] & 1u) && patch[gw].valid;
    const bool has_t = gw + 1 < gwin_off[r + 1] && (bnd_flag[gw + 1] & 1u) && patch[gw + 1].valid;
    if (!has_h && !has_t) return;
    const int lane = threadIdx.x;
    const int len = cwin_len[gw];
    uint8_t *w = cwin + (size_t)gw * FSV_CW_STRIDE;
    for (int i = lane; i < len; i += 64) s_old[i] = w[i];
    __syncthreads();
    int hs = 0, hold = 0, hnew = 0, ts = len, told = 0, tnew = 0;
    const uint8_t *hb = nullptr, *tb = nullptr;
    if (has_h) { const BndPatch p = patch[gw]; hs = p.hs; hold = p.hold; hnew = p.hnew; hb = patch_bytes + (size_t)gw * FSV_CW_STRIDE + p.tnew; }
    if (has_t) { const BndPatch p = patch[gw + 1]; ts = p.ts; told = p.told; tnew = p.tnew; tb = patch_bytes + (size_t)(gw + 1) * FSV_CW_STRIDE; }
    if (told == 0 && tnew == 0) ts = len;
    const int new_len = len - hold + hnew - told + tnew;
    if (hs + hold > ts || ts + told > len || new_len > FSV_CW_STRIDE || new_len < 0) {   // cannot happen with windows of ~375 bases: keep the first pass
        if (lane == 0) atomicOr(&warn[r], (uint32_t)FSV_W_WINDOW_KEPT);
        return;
    }
    // [0, hs) | head patch | [hs + hold, ts) | tail patch | [ts + told, len)
    const int a1 = hs, a2 = a1 + hnew, a3 = a2 + (ts - hs - hold), a4 = a3 + tnew;
    for (int i = lane; i < new_len; i += 64) {
        uint8_t v;
        if (i < a1) v = s_old[i];
        else if (i < a2) v = hb[i - a1];
        else if (i < a3) v = s_old[hs + hold + (i - a2)];
        else if (i < a4) v = tb[i - a3];
        else v = s_old[ts + told + (i - a4)];
        w[i] = v;
    }
    if (lane == 0) { cwin_len[gw] = (uint16_t)new_len; changed[r] = 1u; }
}

} // namespace
