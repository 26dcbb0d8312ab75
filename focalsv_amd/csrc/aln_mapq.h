// aln_mapq.h -- host path of the chromosome index and of fsv_contig_mapq (the kernels: k_place.h).  Included once, at the end of
// aln.hip: it packs and sketches through that file's pack_pairs / launch_sketch, each piece of work in an AlnWs of its own, and reads
// the sequences fsv_align_batch left on the device.  Opt-in: nothing here runs, and nothing is allocated, unless one of its calls is made.
#pragma once
#include <cmath>

namespace {

constexpr uint32_t REF_CHUNK_TILES = 32;    // tiles sketched together: their minimizer slots (one per base at worst) stay at 34 MB

struct RefIndex {
    AlnWs chrom;                    // the chromosome as one sequence: store and N mask
    std::unique_ptr<AlnWs> tile;    // a chunk of tiles while the index is built
    AlnWs q;                        // fsv_contig_mapq: the contigs' sketch (and their store, when the caller passes sequences)
    Dev<unsigned long long> keys, ent_hash, lk_hash;
    Dev<uint32_t> cnt, off, fill, occ, ent_pos, counters, src_word, tile_lo, own_lo, lk_cnt, lk_src, lk_out;
    Dev<uint64_t> lk_dst;
    Dev<PlaceTask> tasks;
    Dev<PlaceOut> placed;
    int k = 0, w = 0, max_occ = 0;
    uint64_t len = 0, slots = 0;
    fsv_ref_stats stats = {};
    RefTable table() const { return RefTable{keys.p, cnt.p, off.p, occ.p, slots, max_occ}; }
};

// slots of the table: a power of two, at least twice the entries
inline uint64_t ref_table_slots(uint64_t entries)
{
    uint64_t n = 1024;
    while (n < 2 * entries) n <<= 1;
    return n;
}

void ref_ws_free(fsv_ctx *ctx)
{
    delete (RefIndex *)ctx->ref_ws;
    ctx->ref_ws = nullptr;
}

// room for n elements, the first `keep` of them kept (ensure() loses what the buffer held)
template <class T> int grow_keep(fsv_ctx *ctx, Dev<T> &b, size_t keep, size_t n)
{
    if (n * sizeof(T) <= b.cap && b.p) return FSV_OK;
    Dev<T> bigger;
    TRY(ensure(ctx, bigger, n + n / 2));
    if (keep) FSV_HIP(ctx, hipMemcpyAsync(bigger.p, b.p, keep * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream));
    FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    b.swap(bigger);
    return FSV_OK;
}
template <class T> int release(fsv_ctx *ctx, Dev<T> &b)
{
    FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    Dev<T> none;
    b.swap(none);
    return FSV_OK;
}

int ref_counters(fsv_ctx *ctx, RefIndex &R, uint32_t (&c)[REF_C_COUNT])
{
    TRY(download(ctx, &c[0], R.counters, REF_C_COUNT));
    FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (c[REF_C_ERR]) return fsv_fail(ctx, FSV_EINTERNAL, "the chromosome index overran a buffer it had sized itself");
    return FSV_OK;
}

// tiles [t0, t1) sketched and their owned, N-free minimizers appended to the entry list
int ref_chunk(fsv_ctx *ctx, RefIndex &R, uint32_t t0, uint32_t t1, double &ms)
{
    AlnWs &T = *R.tile;
    const uint32_t n = t1 - t0;
    std::vector<int32_t> len(n);
    std::vector<uint32_t> src_word(n), tile_lo(n), own_lo(n), word_off, mz_off;
    uint64_t owned_bases = 0;
    for (uint32_t j = 0; j < n; j++) {
        const uint64_t first = (uint64_t)(t0 + j) * REF_TILE;
        const uint64_t lo = first >= REF_HALO ? first - REF_HALO : 0, hi = std::min<uint64_t>(R.len, first + REF_TILE + REF_HALO);
        len[j] = (int32_t)(hi - lo); src_word[j] = (uint32_t)(lo / 16); tile_lo[j] = (uint32_t)lo; own_lo[j] = (uint32_t)first;
        owned_bases += std::min<uint64_t>(R.len, first + REF_TILE) - first;
    }
    TRY(lay_out(ctx, len, store_words, STORE_SLACK, word_off));
    TRY(lay_out(ctx, len, [](uint64_t l) { return l + 64; }, 0, mz_off));
    const uint32_t words = word_off[n];
    TRY(upload(ctx, T.word_off, word_off));
    TRY(upload(ctx, T.len, len));
    TRY(upload(ctx, T.mz_off, mz_off));
    TRY(upload(ctx, R.src_word, src_word));
    TRY(upload(ctx, R.tile_lo, tile_lo));
    TRY(upload(ctx, R.own_lo, own_lo));
    TRY(ensure(ctx, T.mz, mz_off[n]));
    TRY(ensure(ctx, T.mz_cnt, n));
    TRY(ensure(ctx, T.warn, n));
    TRY(zero(ctx, T.warn, n));
    TRY(store_room(ctx, T, words, false));
    uint32_t c[REF_C_COUNT];
    TRY(ref_counters(ctx, R, c));
    const size_t room = (size_t)c[REF_C_ENT] + owned_bases;      // one minimizer per owned base at worst
    TRY(grow_keep(ctx, R.ent_hash, c[REF_C_ENT], room));
    TRY(grow_keep(ctx, R.ent_pos, c[REF_C_ENT], room));
    Timer t(ctx);
    FSV_LAUNCH(ctx, ctx->stream, k_ref_tiles, dim3(fsv_grid_for(words, 256)), dim3(256), 0, R.chrom.store.p, R.src_word.p, T.word_off.p, n, words, T.store.p);
    TRY(launch_sketch(ctx, T, SketchJob{T.store.p, n, words, 1, R.w, R.k, 0, nullptr, R.w, false, nullptr}));
    FSV_LAUNCH(ctx, ctx->stream, k_ref_keep, dim3(n), dim3(256), 0, T.mz.p, T.mz_off.p, T.mz_cnt.p, R.tile_lo.p, R.own_lo.p, R.chrom.nm(), R.k, R.ent_hash.p,
               R.ent_pos.p, (uint32_t)std::min<size_t>(room, 0xffffffffu), R.counters.p);
    ms += t.stop();
    return FSV_OK;
}

int ref_index_build_impl(fsv_ctx *ctx, const char *seq, uint64_t len, int32_t k, int32_t w, int32_t max_occ)
{
    if (!ctx || !seq) return FSV_EINVAL;
    if (len == 0 || len >= (1ull << 31)) return fsv_fail(ctx, FSV_EINVAL, "chromosome empty, or of 2^31 bases or more");
    if (k < 1 || k > 31 || !(k & 1)) return fsv_fail(ctx, FSV_EINVAL, "k must be odd and at most 31 (the position-parallel sketch kernel)");
    if (w < 1 || w > REF_W_MAX || max_occ < 1 || max_occ > REF_MAX_OCC) return fsv_fail(ctx, FSV_EINVAL, "w outside 1 .. 32 or max_occ outside 1 .. 64");
    FSV_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->ref_ws) { FSV_HIP(ctx, hipStreamSynchronize(ctx->stream)); ref_ws_free(ctx); }
    std::unique_ptr<RefIndex> Rp(new RefIndex());
    RefIndex &R = *Rp;
    R.k = k; R.w = w; R.max_occ = max_occ; R.len = len;
    R.tile.reset(new AlnWs());
    {
        std::vector<uint32_t> word_off; std::vector<int32_t> lens;
        TRY(pack_pairs(ctx, R.chrom, {seq}, {len}, word_off, lens));
        TRY(release(ctx, R.chrom.ascii));
    }
    TRY(ensure(ctx, R.counters, REF_C_COUNT));
    TRY(zero(ctx, R.counters, REF_C_COUNT));
    const uint32_t n_tiles = (uint32_t)((len + REF_TILE - 1) / REF_TILE);
    double ms = 0;
    for (uint32_t t0 = 0; t0 < n_tiles; t0 += REF_CHUNK_TILES) TRY(ref_chunk(ctx, R, t0, std::min(n_tiles, t0 + REF_CHUNK_TILES), ms));
    R.tile.reset();
    uint32_t c[REF_C_COUNT];
    TRY(ref_counters(ctx, R, c));
    const uint32_t n_ent = c[REF_C_ENT];
    R.slots = ref_table_slots(n_ent);
    TRY(ensure(ctx, R.keys, R.slots));
    TRY(ensure_each(ctx, R.slots, R.cnt, R.off, R.fill));
    FSV_HIP(ctx, hipMemsetAsync(R.keys.p, 0xff, R.slots * 8, ctx->stream));
    TRY(zero(ctx, R.cnt, R.slots));
    TRY(zero(ctx, R.fill, R.slots));
    {
        Timer t(ctx);
        if (n_ent) FSV_LAUNCH(ctx, ctx->stream, k_ref_count, dim3(fsv_grid_for(n_ent, 256)), dim3(256), 0, R.ent_hash.p, n_ent, R.keys.p, R.slots, R.cnt.p, R.counters.p);
        FSV_LAUNCH(ctx, ctx->stream, k_ref_offsets, dim3(1), dim3(256), 0, R.keys.p, R.cnt.p, R.slots, max_occ, R.off.p, R.counters.p);
        ms += t.stop();
    }
    TRY(ref_counters(ctx, R, c));
    TRY(ensure(ctx, R.occ, (size_t)c[REF_C_STORED] + 1));
    if (n_ent) {
        Timer t(ctx);
        FSV_LAUNCH(ctx, ctx->stream, k_ref_scatter, dim3(fsv_grid_for(n_ent, 256)), dim3(256), 0, R.ent_hash.p, R.ent_pos.p, n_ent, R.table(), R.fill.p, R.occ.p, R.counters.p);
        FSV_LAUNCH(ctx, ctx->stream, k_ref_sort, dim3(fsv_grid_for(R.slots, 256)), dim3(256), 0, R.table(), R.occ.p);
        ms += t.stop();
        TRY(ref_counters(ctx, R, c));
    }
    TRY(release(ctx, R.ent_hash));
    TRY(release(ctx, R.ent_pos));
    TRY(release(ctx, R.fill));
    R.stats.tiles = n_tiles; R.stats.owned = c[REF_C_OWNED]; R.stats.dropped_n = c[REF_C_DROP_N]; R.stats.keys = c[REF_C_KEYS];
    R.stats.keys_above = c[REF_C_ABOVE]; R.stats.stored = c[REF_C_STORED]; R.stats.slots = R.slots; R.stats.max_count = c[REF_C_MAXCNT]; R.stats.ms = ms;
    ctx->ref_ws = Rp.release();
    ctx->ref_ws_free = ref_ws_free;
    return FSV_OK;
}

int ref_index_lookup_impl(fsv_ctx *ctx, const uint64_t *hashes, uint32_t n, uint32_t *count_out, uint64_t *off_out, uint32_t *occ_out, uint64_t cap)
{
    if (!ctx || !off_out || (n && (!hashes || !count_out))) return FSV_EINVAL;
    if (!ctx->ref_ws) return fsv_fail(ctx, FSV_EINVAL, "no chromosome index on this context");
    RefIndex &R = *(RefIndex *)ctx->ref_ws;
    off_out[0] = 0;
    if (n == 0) return FSV_OK;
    FSV_HIP(ctx, hipSetDevice(ctx->device));
    TRY(upload(ctx, R.lk_hash, std::vector<unsigned long long>(hashes, hashes + n)));
    TRY(ensure_each(ctx, n, R.lk_cnt, R.lk_src));
    FSV_LAUNCH(ctx, ctx->stream, k_ref_lookup, dim3(fsv_grid_for(n, 256)), dim3(256), 0, R.lk_hash.p, n, R.table(), R.lk_cnt.p, R.lk_src.p);
    TRY(download(ctx, count_out, R.lk_cnt, n));
    FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<uint64_t> dst((size_t)n + 1, 0);
    for (uint32_t i = 0; i < n; i++) dst[i + 1] = dst[i] + (count_out[i] <= (uint32_t)R.max_occ ? count_out[i] : 0);
    memcpy(off_out, dst.data(), ((size_t)n + 1) * 8);
    if (dst[n] > cap) return fsv_fail(ctx, FSV_ECAP, "occurrence buffer too small (off_out[n] says how many are needed)");
    if (dst[n] == 0) return FSV_OK;
    if (!occ_out) return FSV_EINVAL;
    TRY(upload(ctx, R.lk_dst, dst));
    TRY(ensure(ctx, R.lk_out, dst[n]));
    FSV_LAUNCH(ctx, ctx->stream, k_ref_gather, dim3(fsv_grid_for(n, 256)), dim3(256), 0, n, R.table(), R.lk_cnt.p, R.lk_src.p, R.lk_dst.p, R.lk_out.p);
    TRY(download(ctx, occ_out, R.lk_out, dst[n]));
    FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return FSV_OK;
}

// one record against its contig and the chromosome (what fsv_aln_tags checks, the chromosome in the window's place)
bool mapq_rec_fits(const fsv_aln_rec &r, const fsv_alns *alns, uint32_t n_contigs, const int32_t *contig_len, const uint32_t *contig_ref, const int64_t *ref_origin,
                   uint64_t chrom_len)
{
    if (r.cigar_off > alns->n_cigar || r.n_cigar > alns->n_cigar - r.cigar_off || r.contig >= n_contigs) return false;
    const uint32_t *c = alns->cigar + r.cigar_off;
    int64_t qsum = 0, tsum = 0;
    for (uint32_t k = 0; k < r.n_cigar; k++) {
        const uint32_t op = c[k] & 0xf; const int64_t l = c[k] >> 4;
        if (op != 0 && op != 1 && op != 2 && op != 4 && op != 5) return false;
        if (op != 2) qsum += l;
        if (op == 0 || op == 2) tsum += l;
    }
    const int64_t L = contig_len[r.contig], origin = ref_origin[contig_ref[r.contig]];
    if (qsum != L || r.ref_start < 0 || (int64_t)r.ref_start + tsum != (int64_t)r.ref_end) return false;
    if (origin < 0 || origin + (int64_t)r.ref_end > (int64_t)chrom_len) return false;
    return r.q_start >= 0 && r.q_start <= r.q_end && (int64_t)r.q_end <= L && r.rev <= 1;
}

int contig_mapq_impl(fsv_ctx *ctx, const char *contig_seq, const uint64_t *contig_off, uint32_t n_contigs, const uint32_t *contig_ref,
                     const int64_t *ref_origin, uint32_t n_refs, fsv_alns *alns, const fsv_aln_params *params, struct fsv_contig_mapq *out)
{
    if (!ctx || !alns || !out || !ref_origin || !out->f1 || !out->f2 || !out->m || !out->cutoff || !out->thin || !out->flags || !out->rec_status ||
        (alns->n_rec && (!alns->rec || !alns->cigar)))
        return FSV_EINVAL;
    if (!ctx->ref_ws) return fsv_fail(ctx, FSV_EINVAL, "no chromosome index on this context");
    RefIndex &R = *(RefIndex *)ctx->ref_ws;
    out->ms = 0;
    fsv_aln_params P;
    if (params) P = *params; else fsv_aln_default_params(&P);
    TRY(check_aln_params(ctx, P));
    const bool resident = contig_seq == nullptr;
    AlnWs *Wp = (AlnWs *)ctx->aln_ws;
    std::vector<int32_t> len(n_contigs);
    std::vector<uint32_t> cref(n_contigs);
    std::vector<const char *> seq(n_contigs); std::vector<uint64_t> slen(n_contigs);
    if (resident) {
        if (!Wp || Wp->resident.n_contigs == 0 || Wp->resident.n_contigs != n_contigs || Wp->resident.n_refs != n_refs)
            return fsv_fail(ctx, FSV_EINVAL, "no sequences of an fsv_align_batch with these counts on this context");
        for (uint32_t p = 0; p < n_contigs; p++) { len[p] = Wp->resident.len[n_refs + p]; cref[p] = Wp->resident.pair_t[p]; }
    } else {
        if (!contig_off || !contig_ref || n_contigs == 0 || n_refs == 0) return FSV_EINVAL;
        for (uint32_t p = 0; p < n_contigs; p++) {
            if (contig_ref[p] >= n_refs) return fsv_fail(ctx, FSV_EINVAL, "contig_ref out of range");
            seq[p] = contig_seq + contig_off[p]; slen[p] = contig_off[p + 1] - contig_off[p]; cref[p] = contig_ref[p];
            if (slen[p] == 0 || slen[p] >= (1ull << 31)) return fsv_fail(ctx, FSV_EINVAL, "empty contig, or one of 2^31 bases or more");
            len[p] = (int32_t)slen[p];
        }
    }
    // every record is checked before anything is launched; a record that does not fit never reaches a kernel
    const uint32_t n_rec = alns->n_rec;
    std::vector<PlaceTask> tasks;
    for (uint32_t i = 0; i < n_rec; i++) {
        fsv_aln_rec &r = alns->rec[i];
        out->f1[i] = out->f2[i] = out->m[i] = out->cutoff[i] = out->thin[i] = out->flags[i] = 0;
        r.mapq = 0;
        const bool fits = mapq_rec_fits(r, alns, n_contigs, len.data(), cref.data(), ref_origin, R.len);
        out->rec_status[i] = fits ? FSV_OK : FSV_EINVAL;
        if (!fits) continue;
        const int32_t L = len[r.contig];
        const uint32_t origin = (uint32_t)ref_origin[cref[r.contig]];
        tasks.push_back(PlaceTask{r.contig, L, r.rev ? L - r.q_end : r.q_start, r.rev ? L - r.q_start : r.q_end, (int32_t)r.rev, origin + (uint32_t)r.ref_start,
                                  origin + (uint32_t)r.ref_end, i});
    }
    if (tasks.empty()) return FSV_OK;
    FSV_HIP(ctx, hipSetDevice(ctx->device));
    AlnWs &Q = R.q;
    const uint32_t *store = nullptr; size_t total_words = 0;
    if (resident) {
        std::vector<uint32_t> all_off;
        TRY(lay_out(ctx, Wp->resident.len, store_words, STORE_SLACK, all_off));
        TRY(upload(ctx, Q.word_off, std::vector<uint32_t>(all_off.begin() + n_refs, all_off.end())));
        TRY(upload(ctx, Q.len, len));
        store = Wp->store.p; total_words = all_off.back();
    } else {
        std::vector<uint32_t> word_off; std::vector<int32_t> l2;
        TRY(pack_pairs(ctx, Q, seq, slen, word_off, l2));
        store = Q.store.p; total_words = word_off[n_contigs];
    }
    std::vector<uint32_t> mz_off;
    TRY(lay_out(ctx, len, [](uint64_t l) { return l + 64; }, 0, mz_off));
    TRY(upload(ctx, Q.mz_off, mz_off));
    TRY(ensure(ctx, Q.mz, mz_off[n_contigs]));
    TRY(ensure(ctx, Q.mz_cnt, n_contigs));
    TRY(ensure(ctx, Q.warn, n_contigs));
    TRY(zero(ctx, Q.warn, n_contigs));
    TRY(upload(ctx, R.tasks, tasks));
    TRY(ensure(ctx, R.placed, n_rec));
    Timer t(ctx);
    TRY(launch_sketch(ctx, Q, SketchJob{store, n_contigs, total_words, 1, R.w, R.k, 0, nullptr, R.w, false, nullptr}));
    FSV_LAUNCH(ctx, ctx->stream, k_place, dim3((uint32_t)tasks.size()), dim3(64), 0, R.tasks.p, Q.mz.p, Q.mz_off.p, Q.mz_cnt.p, R.table(), R.placed.p, P);
    out->ms = t.stop();
    std::vector<PlaceOut> placed(n_rec);
    TRY(download(ctx, placed.data(), R.placed, n_rec));
    FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (const PlaceTask &T : tasks) {
        const PlaceOut &o = placed[T.out];
        out->f1[T.out] = o.f1; out->f2[T.out] = o.f2; out->m[T.out] = o.m; out->cutoff[T.out] = o.cutoff; out->thin[T.out] = o.thin; out->flags[T.out] = o.flags;
        alns->rec[T.out].mapq = (uint8_t)fsv_mapq_of(o.f1, o.f2, o.m);
    }
    return FSV_OK;
}

} // namespace

extern "C" int32_t fsv_mapq_of(int32_t f1, int32_t f2, int32_t m)
{
    if (f1 <= 0 || m <= 0 || f2 >= f1) return 0;
    const double v = 40.0 * (1.0 - (double)f2 / (double)f1) * std::min(1.0, (double)m / 10.0) * std::log((double)f1);
    return v >= 60.0 ? 60 : v <= 0.0 ? 0 : (int32_t)v;
}

extern "C" int fsv_ref_index_build(fsv_ctx *ctx, const char *seq, uint64_t len, int32_t k, int32_t w, int32_t max_occ)
{
    FSV_GUARD(ctx, ref_index_build_impl(ctx, seq, len, k, w, max_occ));
}

extern "C" int fsv_ref_index_stats(const fsv_ctx *ctx, fsv_ref_stats *out)
{
    if (!ctx || !out || !ctx->ref_ws) return FSV_EINVAL;
    *out = ((const RefIndex *)ctx->ref_ws)->stats;
    return FSV_OK;
}

extern "C" int fsv_ref_index_drop(fsv_ctx *ctx)
{
    if (!ctx) return FSV_EINVAL;
    if (!ctx->ref_ws) return FSV_OK;
    FSV_HIP(ctx, hipSetDevice(ctx->device));
    FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ref_ws_free(ctx);
    return FSV_OK;
}

extern "C" int fsv_ref_index_lookup(fsv_ctx *ctx, const uint64_t *hashes, uint32_t n, uint32_t *count_out, uint64_t *off_out, uint32_t *occ_out, uint64_t cap)
{
    FSV_GUARD(ctx, ref_index_lookup_impl(ctx, hashes, n, count_out, off_out, occ_out, cap));
}

extern "C" int fsv_contig_mapq(fsv_ctx *ctx, const char *contig_seq, const uint64_t *contig_off, uint32_t n_contigs, const uint32_t *contig_ref,
                               const int64_t *ref_origin, uint32_t n_refs, fsv_alns *alns, const fsv_aln_params *params, struct fsv_contig_mapq *out)
{
    FSV_GUARD(ctx, contig_mapq_impl(ctx, contig_seq, contig_off, n_contigs, contig_ref, ref_origin, n_refs, alns, params, out));
}
