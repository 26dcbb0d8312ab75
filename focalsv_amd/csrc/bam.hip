// bam.hip -- BAM records of one reference sequence without pysam / samtools.
//
// What the reference does with pysam at this boundary: `samfile.fetch(chr_name)` and, per record, reference_name / pos /
// reference_end / cigar / qname / is_reverse / mapq (extract_reads_signature.py:68-105, 160-209), and `samtools view bam region`
// to crop reads (1_crop_bam.py:74).  Here: BGZF blocks inflated with zlib on the host, records decoded into flat arrays
// (structure of arrays, CIGARs back to back in BAM encoding), region start through the .bai linear index when there is one; the
// CIGAR scan for read-level DEL / INS signatures (extract_sig_from_cigar of extract_reads_signature.py:11-44) runs as a kernel,
// one thread per record.  Format: SAM/BAM specification v1, sections 4.1 (BGZF), 4.2 (BAM), 5.2 (BAI).
//
// In file order: what the reader and the writer share (the base alphabet and its tables, the CIGAR ops that consume the reference,
// the thread fan-out, the guard of the C entry points); the BGZF stream; the header and the .bai; the aux walk; fsv_bam_fetch
// in stages (seek_to_query, view_record, judge, append_record); fsv_read_signatures; fsv_bam_write in stages (check_records,
// stable_order, encode_stream, deflate_blocks, build_bai, write_files).
#include "fsv_internal.h"
#include <zlib.h>
#include <cstdio>
#include <cstring>
#include <string>
#include <memory>
#include <new>
#include <vector>
#include <thread>
#include <atomic>
#include <future>
#include <algorithm>
#include <map>
#include <numeric>
#include <unistd.h>
#include <sys/stat.h>

namespace {

// ---- shared by the reader and the writer ------------------------------------------------------------------------------------------
// the 4-bit base codes of a BAM record, and the tables over them: a packed byte (two bases) -> 4 bits of the read store (A C G T,
// the rest A) and -> its two letters; a letter -> its code (an unknown one: N)
constexpr char BAM_BASES[17] = "=ACMGRSVTWYHKDBN";
struct BaseTabs {
    uint8_t pair2[256], nib[256];
    uint16_t pairc[256];
    BaseTabs()
    {
        static const uint8_t code[16] = {0, 0, 1, 0, 2, 0, 0, 0, 3, 0, 0, 0, 0, 0, 0, 0};
        memset(nib, 15, sizeof(nib));
        for (int c = 0; c < 16; c++) nib[(uint8_t)BAM_BASES[c]] = (uint8_t)c;
        for (int v = 0; v < 256; v++) {
            pair2[v] = (uint8_t)(code[v >> 4] | code[v & 15] << 2);
            pairc[v] = (uint16_t)((uint8_t)BAM_BASES[v >> 4] | (uint16_t)(uint8_t)BAM_BASES[v & 15] << 8);
        }
    }
};
const BaseTabs base_tabs;

// M, D, N, = and X advance the reference (mapq_rec_fits of aln_mapq.h has a narrower set of its own: what the aligner writes)
inline bool cigar_consumes_ref(uint32_t op) { return op == 0 || op == 2 || op == 3 || op == 7 || op == 8; }

// fn(i) for every i in [0, n) on up to nt threads, the caller's included; false when a call answered false or threw (a worker
// keeps what it throws to itself: an exception that leaves a thread function ends the process).  When a thread cannot start,
// those already running are joined before the error goes on to the caller.
template <class F> bool fan_out(size_t n, unsigned nt, F fn)
{
    std::atomic<bool> ok{true};
    auto work = [&](unsigned t) {
        try { for (size_t i = t; i < n; i += nt) if (!fn(i)) ok = false; }
        catch (...) { ok = false; }
    };
    if (nt <= 1) { work(0); return ok; }
    std::vector<std::thread> th;
    try { for (unsigned t = 1; t < nt; t++) th.emplace_back(work, t); }
    catch (...) { for (auto &t : th) t.join(); throw; }
    work(0);
    for (auto &t : th) t.join();
    return ok;
}

// no C++ exception crosses the C ABI (a caller through ctypes would see std::terminate).  Not FSV_GUARD: there is no context
// here, and the reader answers FSV_EINVAL for what it cannot name where the writer answers FSV_EINTERNAL.
#define BAM_GUARD(fallback, call)                                   \
    try { return (call); }                                          \
    catch (const std::bad_alloc &) { return FSV_ENOMEM; }           \
    catch (...) { return (fallback); }

struct BgzfBlock {
    std::vector<uint8_t> comp, data;
    uint32_t clen = 0, isize = 0;
    int64_t addr = 0;
    int bsize = 0;
};

struct BgzfWindow {
    std::vector<BgzfBlock> blk;
    int64_t next_addr = 0;           // file offset following the run
    std::string err;
};

struct BamCache {
    bool valid = false;
    int ref_id = 0, want = 0;
    int64_t beg = 0, end = 0;
    std::vector<int32_t> pos, ref_end, l_seq, ref, ps, hp;
    std::vector<uint16_t> flag;
    std::vector<uint8_t> mapq;
    std::vector<uint64_t> cigar_off, qname_off, seq_word_off, seq_ascii_off, sa_off;
    std::vector<uint32_t> n_cigar_op, cigar, seq_words;
    std::vector<char> qname, seq_ascii, sa;
    void clear() { *this = BamCache(); }
};

struct FileCloser { void operator()(FILE *f) const { fclose(f); } };

} // namespace

struct fsv_bam {
    std::unique_ptr<FILE, FileCloser> f;
    std::string path, err;
    std::vector<std::string> ref_name;
    std::vector<int32_t> ref_len;
    uint64_t first_record_voff = 0;  // virtual offset behind the header: where a scan without an index starts
    // BGZF stream state
    std::vector<uint8_t> block;      // inflated data of the current block
    size_t block_pos = 0;
    int64_t block_addr = 0;          // file offset of the current block
    int64_t next_addr = 0;           // file offset of the next block
    bool eof = false;
    BgzfWindow win;                  // blocks read ahead and inflated in parallel; win_i = the next one to hand out
    size_t win_i = 0, run_blocks = 16;
    std::future<BgzfWindow> pending; // the run after `win`, being read and inflated in the background (valid() while there is one)
    int n_threads = 1;
    BamCache cache;                  // the records of the last sizing call, until the caller has taken them
    // .bai: per reference the smallest virtual offset of its chunks (where a scan of that reference starts), and the linear index
    bool have_index = false;
    std::vector<uint64_t> ref_first_voff;
    std::vector<std::vector<uint64_t>> linear;

    // wait for the read-ahead and let go of its blocks; what it stored as an error is thrown here
    void drop_pending() { if (pending.valid()) (void)pending.get(); }
    // (an error the read-ahead stored concerns blocks nobody asked for: it ends with the handle; the file closes after the read-ahead is done with it)
    ~fsv_bam() { try { drop_pending(); } catch (...) {} }
};

namespace {

// ---- the BGZF stream ----------------------------------------------------------------------------------------------------------------
// one BGZF block: header parsed and compressed bytes read by the (serial) file scan, inflated by whichever thread takes it
bool inflate_block(BgzfBlock &k)
{
    k.data.resize(k.isize);
    if (!k.isize) return true;
    z_stream zs;
    memset(&zs, 0, sizeof(zs));
    if (inflateInit2(&zs, -15) != Z_OK) return false;
    zs.next_in = k.comp.data(); zs.avail_in = (uInt)k.clen;
    zs.next_out = k.data.data(); zs.avail_out = k.isize;
    const int rc = inflate(&zs, Z_FINISH);
    inflateEnd(&zs);
    return rc == Z_STREAM_END && zs.total_out == k.isize;
}

// the next block of the file, header and compressed bytes, into k: nullptr when it is whole (or, with *at_end, when nothing is left),
// else what is wrong with it
const char *read_raw_block(FILE *f, BgzfBlock &k, bool *at_end)
{
    uint8_t hdr[18];
    const size_t got = fread(hdr, 1, 18, f);
    *at_end = got == 0;
    if (got == 0) return nullptr;
    if (got != 18 || hdr[0] != 31 || hdr[1] != 139 || hdr[2] != 8 || !(hdr[3] & 4)) return "not a BGZF block";
    const unsigned xlen = hdr[10] | hdr[11] << 8;
    // the BC subfield is the first extra subfield in every BGZF writer; tolerate others in front of it
    std::vector<uint8_t> extra(xlen);
    if (xlen) memcpy(extra.data(), hdr + 12, std::min<size_t>(6, xlen));
    if (xlen > 6 && fread(extra.data() + 6, 1, xlen - 6, f) != xlen - 6) return "truncated BGZF header";
    int bsize = -1;
    for (size_t p = 0; p + 4 <= extra.size();) {
        const unsigned slen = extra[p + 2] | extra[p + 3] << 8;
        if (extra[p] == 'B' && extra[p + 1] == 'C' && slen == 2 && p + 6 <= extra.size()) bsize = (extra[p + 4] | extra[p + 5] << 8) + 1;
        p += 4 + slen;
    }
    const int clen = bsize - 12 - (int)xlen - 8;   // block = 12-byte header + extra + deflate data + crc32 + isize
    if (bsize < 0) return "BGZF block without BC subfield";
    if (clen < 0) return "bad BGZF block size";
    k.comp.resize((size_t)clen + 8);
    if (fread(k.comp.data(), 1, k.comp.size(), f) != k.comp.size()) return "truncated BGZF block";
    k.clen = (uint32_t)clen;
    k.isize = k.comp[clen + 4] | k.comp[clen + 5] << 8 | k.comp[clen + 6] << 16 | (uint32_t)k.comp[clen + 7] << 24;
    if (k.isize > 65536) return "bad BGZF block size";
    k.bsize = bsize;
    return nullptr;
}

// read a run of up to `want` blocks starting at file offset addr and inflate them on the reader's threads.  A malformed block behind
// at least one good one ends the run: the next run starts at it and reports it.
BgzfWindow load_window(fsv_bam *b, int64_t addr, size_t want)
{
    BgzfWindow w;
    w.next_addr = addr;
    if (fseeko(b->f.get(), (off_t)addr, SEEK_SET) != 0) { w.err = "seek failed"; return w; }
    while (w.blk.size() < want) {
        BgzfBlock k;
        bool at_end = false;
        const char *bad = read_raw_block(b->f.get(), k, &at_end);
        if (at_end) break;
        if (bad) { if (w.blk.empty()) w.err = bad; break; }
        k.addr = w.next_addr;
        w.next_addr += k.bsize;
        w.blk.push_back(std::move(k));
    }
    const size_t n = w.blk.size();
    const unsigned nt = (unsigned)std::min<size_t>((size_t)std::max(1, b->n_threads), (n + 7) / 8);
    if (!fan_out(n, nt, [&](size_t i) { return inflate_block(w.blk[i]); })) { w.blk.clear(); w.err = "inflate failed"; }
    return w;
}

// The run grows from 16 to 512 blocks as a scan goes on, so a region query touches little beyond its blocks while a chromosome scan
// keeps every thread busy; from 64 blocks on the next run is read and inflated in the background while this one is parsed.
bool bgzf_read_block(fsv_bam *b)
{
    if (b->win_i == b->win.blk.size()) {
        if (b->pending.valid()) b->win = b->pending.get();
        else b->win = load_window(b, b->win.next_addr, b->run_blocks);
        b->win_i = 0;
        if (!b->win.err.empty()) { b->err = b->win.err; return false; }
        if (b->win.blk.empty()) { b->eof = true; b->block.clear(); b->block_pos = 0; return true; }
        b->run_blocks = std::min<size_t>(512, b->run_blocks * 2);
        if (b->run_blocks >= 64 && b->n_threads > 1) {
            const int64_t at = b->win.next_addr;
            const size_t want = b->run_blocks;
            b->pending = std::async(std::launch::async, [b, at, want] { return load_window(b, at, want); });
        }
    }
    BgzfBlock &k = b->win.blk[b->win_i++];
    b->block.swap(k.data);
    b->block_addr = k.addr;
    b->next_addr = k.addr + k.bsize;
    b->block_pos = 0;
    return true;
}

// read n bytes of the uncompressed stream; false at a clean end of file before the first byte (err empty) or on an error
bool bgzf_read(fsv_bam *b, void *dst, size_t n)
{
    uint8_t *o = (uint8_t *)dst;
    while (n) {
        if (b->block_pos == b->block.size()) {
            if (b->eof) return false;
            if (!bgzf_read_block(b)) return false;
            if (b->eof) return false;
            continue;
        }
        const size_t k = std::min(n, b->block.size() - b->block_pos);
        memcpy(o, b->block.data() + b->block_pos, k);
        o += k; n -= k; b->block_pos += k;
    }
    return true;
}

bool bgzf_seek(fsv_bam *b, uint64_t voff)
{
    b->drop_pending();
    b->win = BgzfWindow();
    b->win.next_addr = (int64_t)(voff >> 16);
    b->win_i = 0; b->run_blocks = 16;
    b->eof = false;
    if (!bgzf_read_block(b)) return false;
    if (b->eof) { b->block_pos = 0; return (voff & 0xffff) == 0; }
    if ((voff & 0xffff) > b->block.size()) { b->err = "virtual offset past the block"; return false; }
    b->block_pos = (size_t)(voff & 0xffff);
    return true;
}

// (at a block's end: the start of the next block, which is also right at the end of the file)
inline uint64_t bgzf_tell(const fsv_bam *b)
{
    return b->block_pos == b->block.size() && !b->block.empty() ? (uint64_t)b->next_addr << 16 : ((uint64_t)b->block_addr << 16 | (uint64_t)b->block_pos);
}

// ---- the header and the index ---------------------------------------------------------------------------------------------------------
// magic, text, reference names and lengths, from the start of the stream; read once, at open
bool read_header(fsv_bam *b)
{
    char magic[4]; int32_t l_text = 0, n_ref = 0;
    bool ok = bgzf_read(b, magic, 4) && !memcmp(magic, "BAM\1", 4) && bgzf_read(b, &l_text, 4) && l_text >= 0;
    if (ok) { std::vector<char> text((size_t)l_text); ok = l_text == 0 || bgzf_read(b, text.data(), (size_t)l_text); }
    ok = ok && bgzf_read(b, &n_ref, 4) && n_ref >= 0;
    for (int32_t r = 0; ok && r < n_ref; r++) {
        int32_t l_name = 0, l_ref = 0;
        ok = bgzf_read(b, &l_name, 4) && l_name > 0 && l_name < (1 << 16);
        std::vector<char> nm((size_t)std::max(1, l_name));
        ok = ok && bgzf_read(b, nm.data(), (size_t)l_name) && bgzf_read(b, &l_ref, 4);
        if (ok) { b->ref_name.emplace_back(nm.data(), strnlen(nm.data(), (size_t)l_name)); b->ref_len.push_back(l_ref); }   // the name may lack its NUL
    }
    return ok;
}

void load_bai(fsv_bam *b)
{
    for (const std::string &p : {b->path + ".bai", b->path.size() > 4 ? b->path.substr(0, b->path.size() - 4) + ".bai" : std::string()}) {
        if (p.empty()) continue;
        const std::unique_ptr<FILE, FileCloser> f(fopen(p.c_str(), "rb"));
        if (!f) continue;
        auto rd = [&](void *d, size_t n) { return fread(d, 1, n, f.get()) == n; };
        char magic[4]; int32_t n_ref = 0;
        bool ok = rd(magic, 4) && !memcmp(magic, "BAI\1", 4) && rd(&n_ref, 4) && n_ref == (int32_t)b->ref_name.size();
        std::vector<uint64_t> first((size_t)std::max(0, n_ref), ~0ull);
        std::vector<std::vector<uint64_t>> lin((size_t)std::max(0, n_ref));
        for (int32_t r = 0; ok && r < n_ref; r++) {
            int32_t n_bin = 0;
            ok = rd(&n_bin, 4) && n_bin >= 0;      // a damaged index is "no index" (whole-file scan), never a huge resize
            for (int32_t i = 0; ok && i < n_bin; i++) {
                uint32_t bin = 0; int32_t n_chunk = 0;
                ok = rd(&bin, 4) && rd(&n_chunk, 4) && n_chunk >= 0;
                for (int32_t c = 0; ok && c < n_chunk; c++) {
                    uint64_t beg = 0, end = 0;
                    ok = rd(&beg, 8) && rd(&end, 8);
                    if (ok && bin != 37450 && beg < first[r]) first[r] = beg;   // bin 37450 is the metadata pseudo-bin
                }
            }
            int32_t n_intv = 0;
            ok = ok && rd(&n_intv, 4) && n_intv >= 0 && n_intv <= (1 << 24);   // 2^24 x 16 kb windows = 2^38 bases
            if (ok) { lin[r].resize((size_t)n_intv); ok = n_intv == 0 || rd(lin[r].data(), (size_t)n_intv * 8); }
        }
        if (ok) { b->have_index = true; b->ref_first_voff = first; b->linear = lin; return; }
    }
}

// ---- aux tags -------------------------------------------------------------------------------------------------------------------------
struct AuxField { char type = 0; const uint8_t *val = nullptr; size_t size = 0; };   // type 0: absent

// The two-letter tag (t0, t1) in the aux block [p, end): its type byte, where its value starts and the bytes the value takes (a
// string's NUL, a B array's sub-type and count included).  Absent: no such tag, a field of unknown type in front of it or as its own
// (the rest cannot be walked), or a value -- its own or one in front -- that runs past end.
AuxField aux_find(const uint8_t *p, const uint8_t *end, char t0, char t1)
{
    while (end - p >= 3) {
        const char a = (char)p[0], b = (char)p[1], ty = (char)p[2];
        p += 3;
        const size_t left = (size_t)(end - p);
        size_t sz = 0;
        switch (ty) {
        case 'A': case 'c': case 'C': sz = 1; break;
        case 's': case 'S': sz = 2; break;
        case 'i': case 'I': case 'f': sz = 4; break;
        case 'Z': case 'H': { const uint8_t *q = p; while (q < end && *q) q++; sz = (size_t)(q - p) + 1; break; }
        case 'B': {
            if (left < 5) return {};
            uint32_t cnt; memcpy(&cnt, p + 1, 4);
            const char st = (char)p[0];
            sz = 5 + (size_t)cnt * ((st == 'c' || st == 'C') ? 1 : (st == 's' || st == 'S') ? 2 : 4);
            break;
        }
        default: return {};
        }
        if (sz > left) return {};
        if (a == t0 && b == t1) return {ty, p, sz};
        p += sz;
    }
    return {};
}

// integer value of a tag; false when the tag is absent or not an integer
bool aux_int(const uint8_t *p, const uint8_t *end, char t0, char t1, int32_t *out)
{
    const AuxField f = aux_find(p, end, t0, t1);
    switch (f.type) {
    case 'c': *out = (int8_t)f.val[0]; return true;
    case 'C': *out = f.val[0]; return true;
    case 's': { int16_t x; memcpy(&x, f.val, 2); *out = x; return true; }
    case 'S': { uint16_t x; memcpy(&x, f.val, 2); *out = x; return true; }
    case 'i': case 'I': memcpy(out, f.val, 4); return true;   // (an I above 2^31 wraps, as a cast does)
    default: return false;
    }
}

// value of a string (Z) tag: pointer into the record and its length; false when the tag is absent or not a string
bool aux_str(const uint8_t *p, const uint8_t *end, char t0, char t1, const char **out, size_t *len)
{
    const AuxField f = aux_find(p, end, t0, t1);
    if (f.type != 'Z') return false;
    *out = (const char *)f.val; *len = f.size - 1;
    return true;
}

// ---- fsv_bam_fetch in stages ------------------------------------------------------------------------------------------------------
// counts to the caller; with buffers (pos != NULL) also the arrays, after which the reader lets go of them
int copy_out(fsv_bam *b, fsv_bam_records *out, int want_seq)
{
    BamCache &c = b->cache;
    const size_t n = c.pos.size();
    out->n_rec = n; out->n_cigar = c.cigar.size(); out->qname_bytes = c.qname.size(); out->seq_words = c.seq_words.size();
    out->seq_ascii_bytes = c.seq_ascii.size(); out->sa_bytes = c.sa.size();
    if (!out->pos) return FSV_OK;
    if (n > out->rec_cap || c.cigar.size() > out->cigar_cap || c.qname.size() > out->qname_cap) return FSV_ECAP;
    auto put = [](void *dst, const void *src, size_t bytes) { if (dst && bytes) memcpy(dst, src, bytes); };
    put(out->pos, c.pos.data(), n * 4); put(out->ref_end, c.ref_end.data(), n * 4); put(out->flag, c.flag.data(), n * 2); put(out->mapq, c.mapq.data(), n);
    put(out->cigar_off, c.cigar_off.data(), n * 8); put(out->n_cigar_op, c.n_cigar_op.data(), n * 4); put(out->qname_off, c.qname_off.data(), n * 8);
    put(out->l_seq, c.l_seq.data(), n * 4); put(out->cigar, c.cigar.data(), c.cigar.size() * 4); put(out->qname, c.qname.data(), c.qname.size());
    put(out->ref_id, c.ref.data(), n * 4);
    if (out->ps && out->hp) { put(out->ps, c.ps.data(), n * 4); put(out->hp, c.hp.data(), n * 4); }
    if ((want_seq & 1) && out->seq_word_off) {
        if (c.seq_words.size() > out->seq_cap) return FSV_ECAP;
        put(out->seq_word_off, c.seq_word_off.data(), n * 8); put(out->seq_words_buf, c.seq_words.data(), c.seq_words.size() * 4);
    }
    if ((want_seq & 2) && out->seq_ascii_off) {
        if (c.seq_ascii.size() > out->seq_ascii_cap) return FSV_ECAP;
        put(out->seq_ascii_off, c.seq_ascii_off.data(), n * 8); put(out->seq_ascii, c.seq_ascii.data(), c.seq_ascii.size());
    }
    if ((want_seq & 4) && out->sa_off) {
        if (c.sa.size() > out->sa_cap) return FSV_ECAP;
        put(out->sa_off, c.sa_off.data(), n * 8); put(out->sa, c.sa.data(), c.sa.size());
    }
    c.clear();
    return FSV_OK;
}

// what a fetch asks for, normalised: reference ref_id over [beg, end), or (all) every record of the file, unmapped ones included
struct Query { int ref_id; int64_t beg, end; bool all; };

// Put the stream where the query's scan starts: with an index, the linear-index entry of the window that holds beg (or the
// reference's first chunk); without one, or for the whole file, the first record.
enum class Seek { ok, no_records, failed };
Seek seek_to_query(fsv_bam *b, const Query &q)
{
    uint64_t v = b->first_record_voff;
    if (b->have_index && !q.all) {
        v = b->ref_first_voff[(size_t)q.ref_id];
        const auto &lin = b->linear[(size_t)q.ref_id];
        const size_t w = (size_t)(q.beg >> 14);
        if (w < lin.size() && lin[w] != 0 && (v == ~0ull || lin[w] > v)) v = lin[w];
        if (v == ~0ull) return Seek::no_records;   // no records on this reference
    }
    return bgzf_seek(b, v) ? Seek::ok : Seek::failed;
}

// one record (block_size bytes behind the length word): the fixed 32 bytes, and where its parts lie
struct RecView {
    int32_t ref_id, pos, l_seq;
    uint8_t l_name, mapq;
    uint16_t n_cigar_op, flag;
    bool fits;                       // name + CIGAR + packed bases lie inside the record (and l_seq >= 0): only then are the pointers set
    const char *qname;
    const uint8_t *cigar, *seq, *aux, *rend;   // (aux: nullptr when the qualities are cut short, a record without tags)
    int64_t ref_end() const
    {
        int64_t e = pos;
        for (uint32_t k = 0; k < n_cigar_op; k++) { uint32_t v; memcpy(&v, cigar + 4 * k, 4); if (cigar_consumes_ref(v & 0xf)) e += v >> 4; }
        return e;
    }
};

RecView view_record(const uint8_t *rec, int32_t block_size)
{
    RecView v{};
    memcpy(&v.ref_id, rec, 4); memcpy(&v.pos, rec + 4, 4);
    v.l_name = rec[8]; v.mapq = rec[9];
    memcpy(&v.n_cigar_op, rec + 12, 2); memcpy(&v.flag, rec + 14, 2); memcpy(&v.l_seq, rec + 16, 4);
    v.rend = rec + block_size;
    const size_t nb = v.l_seq >= 0 ? ((size_t)v.l_seq + 1) / 2 : 0, seq_at = (size_t)32 + v.l_name + (size_t)v.n_cigar_op * 4;
    v.fits = v.l_seq >= 0 && seq_at + nb <= (size_t)block_size;
    if (!v.fits) return v;
    v.qname = (const char *)rec + 32;
    v.cigar = rec + 32 + v.l_name;
    v.seq = rec + seq_at;
    if (seq_at + nb + (size_t)v.l_seq <= (size_t)block_size) v.aux = v.seq + nb + (size_t)v.l_seq;
    return v;
}

// Whether the query takes the record, in this order (`samtools view` overlap semantics): a sorted file is past the query at a later
// reference, at an unmapped record (they come last) or at pos >= end; a record that does not fit its block is an error wherever the
// scan gets to it; one that ends at or before beg is skipped, unless it has no CIGAR and starts inside; so is a placed unmapped one.
enum class Verdict { take, skip, stop, bad };
Verdict judge(const RecView &v, const Query &q, int64_t *ref_end)
{
    if (!q.all) {
        if (v.ref_id != q.ref_id) return (v.ref_id > q.ref_id || v.ref_id < 0) ? Verdict::stop : Verdict::skip;
        if (v.pos >= q.end) return Verdict::stop;
    }
    if (!v.fits) return Verdict::bad;
    *ref_end = v.ref_end();
    if (!q.all) {
        if (*ref_end <= q.beg && !(v.n_cigar_op == 0 && v.pos >= q.beg)) return Verdict::skip;   // ends before the window
        if (v.flag & 4) return Verdict::skip;                                                      // unmapped but placed: fetch() skips it too
    }
    return Verdict::take;
}

// l_seq bases, two per byte -> 2 bits each, 16 per word; the padding nibble of an odd-length read is not a base
void unpack_words(const uint8_t *sq, int32_t l_seq, std::vector<uint32_t> &out)
{
    const size_t nb = (size_t)(l_seq + 1) / 2, w0 = out.size(), nw = (size_t)(l_seq + 15) / 16;
    out.resize(w0 + nw);
    uint32_t *w = out.data() + w0;
    for (size_t i = 0; i < nw; i++) {
        uint32_t x = 0;
        const size_t k1 = std::min<size_t>(8, nb - i * 8);
        for (size_t k = 0; k < k1; k++) x |= (uint32_t)base_tabs.pair2[sq[i * 8 + k]] << (4 * k);
        w[i] = x;
    }
    if (l_seq & 1) w[nw - 1] &= ~(3u << ((l_seq & 15) << 1));
}

// l_seq bases, two per byte -> text (what pysam's read.seq gives)
void unpack_text(const uint8_t *sq, int32_t l_seq, std::vector<char> &out)
{
    const size_t nb = (size_t)(l_seq + 1) / 2, a0 = out.size();
    out.resize(a0 + nb * 2);
    char *w = out.data() + a0;
    for (size_t i = 0; i < nb; i++) memcpy(w + 2 * i, &base_tabs.pairc[sq[i]], 2);
    out.resize(a0 + (size_t)l_seq);
}

void append_record(BamCache &c, const RecView &v, int64_t ref_end, int want_seq)
{
    c.pos.push_back(v.pos); c.ref_end.push_back((int32_t)ref_end); c.flag.push_back(v.flag); c.mapq.push_back(v.mapq); c.ref.push_back(v.ref_id);
    c.cigar_off.push_back(c.cigar.size()); c.n_cigar_op.push_back(v.n_cigar_op); c.qname_off.push_back(c.qname.size()); c.l_seq.push_back(v.l_seq);
    const bool has_aux = v.aux != nullptr;
    int32_t t;
    c.ps.push_back(has_aux && aux_int(v.aux, v.rend, 'P', 'S', &t) ? t : FSV_BAM_NO_TAG);
    c.hp.push_back(has_aux && aux_int(v.aux, v.rend, 'H', 'P', &t) ? t : FSV_BAM_NO_TAG);
    const size_t c0 = c.cigar.size();
    c.cigar.resize(c0 + v.n_cigar_op);
    if (v.n_cigar_op) memcpy(c.cigar.data() + c0, v.cigar, (size_t)v.n_cigar_op * 4);
    c.qname.insert(c.qname.end(), v.qname, v.qname + v.l_name);
    if (want_seq & 4) {   // the SA tag's text + NUL; a record without one takes the NUL alone
        const char *sv = nullptr; size_t sl = 0;
        c.sa_off.push_back(c.sa.size());
        if (has_aux && aux_str(v.aux, v.rend, 'S', 'A', &sv, &sl)) c.sa.insert(c.sa.end(), sv, sv + sl);
        c.sa.push_back(0);
    }
    if (want_seq & 2) { c.seq_ascii_off.push_back(c.seq_ascii.size()); unpack_text(v.seq, v.l_seq, c.seq_ascii); }
    if (want_seq & 1) { c.seq_word_off.push_back(c.seq_words.size()); unpack_words(v.seq, v.l_seq, c.seq_words); }
}

// the records from where the stream stands to the end of the query (or of the file) into the cache
int scan_records(fsv_bam *b, const Query &q, int want_seq)
{
    std::vector<uint8_t> rec;
    for (;;) {
        int32_t bs = 0;
        if (!bgzf_read(b, &bs, 4)) return b->err.empty() ? FSV_OK : FSV_EINVAL;   // (err empty: a clean end of file)
        if (bs < 32) return FSV_EINVAL;
        rec.resize((size_t)bs + 8);
        if (!bgzf_read(b, rec.data(), (size_t)bs)) return FSV_EINVAL;
        const RecView v = view_record(rec.data(), bs);
        int64_t ref_end = 0;
        switch (judge(v, q, &ref_end)) {
        case Verdict::bad: return FSV_EINVAL;
        case Verdict::stop: return FSV_OK;
        case Verdict::skip: break;
        case Verdict::take: append_record(b->cache, v, ref_end, want_seq); break;
        }
    }
}

int bam_open_impl(const char *path, fsv_bam **out)
{
    if (!path || !out) return FSV_EINVAL;
    std::unique_ptr<fsv_bam> b(new fsv_bam());
    b->path = path;
    b->f.reset(fopen(path, "rb"));
    if (!b->f) return FSV_EINVAL;
    b->n_threads = (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    if (!read_header(b.get())) return FSV_EINVAL;
    b->first_record_voff = bgzf_tell(b.get());
    load_bai(b.get());
    *out = b.release();
    return FSV_OK;
}

// Records of reference ref_id overlapping [beg, end) (end <= 0: to the end of the reference), in file order -- the iteration
// pysam's fetch() gives.  Two calls: with rec == NULL the counts come back (n_rec, n_cigar, qname_bytes, seq_bases), then the
// caller allocates and calls again.  want_seq bit 0: also the bases, 2 bits each as in the read store (N -> A), read r at word
// seq_word_off[r]; bit 1: the bases as text (what pysam's read.seq gives), read r at seq_ascii + seq_ascii_off[r].  ref_id -1: every
// record of the file, unmapped ones included -- fetch(until_eof=True) of output_fas.py:26.
int bam_fetch_impl(fsv_bam *b, int ref_id, int64_t beg, int64_t end, fsv_bam_records *out, int want_seq)
{
    if (!b || !out || ref_id < -1 || ref_id >= (int)b->ref_name.size()) return FSV_EINVAL;
    Query q{ref_id, beg, end, ref_id == -1};
    if (q.all) { q.beg = 0; q.end = INT64_MAX; }
    else if (q.end <= 0) q.end = b->ref_len[(size_t)ref_id];
    if (q.beg < 0) q.beg = 0;
    // one parse per query: the sizing call (pos == NULL) decodes into the reader's own arrays, the call with buffers copies them out
    BamCache &c = b->cache;
    if (c.valid && c.ref_id == ref_id && c.beg == q.beg && c.end == q.end && c.want == want_seq) return copy_out(b, out, want_seq);
    switch (seek_to_query(b, q)) {
    case Seek::failed: return FSV_EINVAL;
    case Seek::no_records: c.clear(); return copy_out(b, out, want_seq);
    case Seek::ok: break;
    }
    c.clear();
    TRY(scan_records(b, q, want_seq));
    c.valid = true; c.ref_id = ref_id; c.beg = q.beg; c.end = q.end; c.want = want_seq;
    return copy_out(b, out, want_seq);
}

} // namespace

extern "C" int fsv_bam_open(const char *path, fsv_bam **out) { BAM_GUARD(FSV_EINVAL, bam_open_impl(path, out)) }
extern "C" int fsv_bam_fetch(fsv_bam *b, int ref_id, int64_t beg, int64_t end, fsv_bam_records *out, int want_seq)
{
    BAM_GUARD(FSV_EINVAL, bam_fetch_impl(b, ref_id, beg, end, out, want_seq))
}
extern "C" void fsv_bam_close(fsv_bam *b) { delete b; }   // (~fsv_bam lets nothing through)

extern "C" int fsv_bam_ref_id(const fsv_bam *b, const char *name)
{
    if (!b || !name) return -1;
    for (size_t i = 0; i < b->ref_name.size(); i++) if (b->ref_name[i] == name) return (int)i;
    return -1;
}

extern "C" int fsv_bam_n_refs(const fsv_bam *b) { return b ? (int)b->ref_name.size() : 0; }
extern "C" const char *fsv_bam_ref_name(const fsv_bam *b, int id) { return b && id >= 0 && id < (int)b->ref_name.size() ? b->ref_name[(size_t)id].c_str() : nullptr; }
extern "C" void fsv_bam_set_threads(fsv_bam *b, int n) { if (b) b->n_threads = n < 1 ? 1 : n; }
extern "C" int64_t fsv_bam_ref_length(const fsv_bam *b, int id) { return b && id >= 0 && id < (int)b->ref_len.size() ? (int64_t)b->ref_len[(size_t)id] : -1; }
extern "C" int fsv_bam_has_index(const fsv_bam *b) { return b && b->have_index ? 1 : 0; }

// ---------------------------------------------------------------------------------------------------------------------
// read-level signatures from CIGARs (extract_reads_signature.py:11-44): one thread per record
namespace {
__global__ void k_cigar_sigs(const int32_t *__restrict__ pos, const uint8_t *__restrict__ mapq, const uint64_t *__restrict__ cigar_off,
                             const uint32_t *__restrict__ n_op, const uint32_t *__restrict__ cigar, uint32_t n_rec, int min_mapq, int min_svlen,
                             fsv_read_sig *__restrict__ out, uint32_t cap, uint32_t *__restrict__ n_out)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rec || mapq[r] < min_mapq || n_op[r] == 0) return;
    const uint32_t *c = cigar + cigar_off[r];
    const uint32_t n = n_op[r];
    const int32_t head = (c[0] & 0xf) == 5 ? (int32_t)(c[0] >> 4) : 0;   // a leading hard clip shifts the read offsets
    int32_t ref = pos[r], ctg = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t op = c[i] & 0xf, len = c[i] >> 4;
        if (op == 0) { ref += (int32_t)len; ctg += (int32_t)len; }
        else if (op == 4) ctg += (int32_t)len;
        else if (op == 2 || op == 1) {
            if ((int)len >= min_svlen) {
                const uint32_t at = atomicAdd(n_out, 1u);
                if (at < cap) { fsv_read_sig s; s.rec = r; s.type = op == 2 ? 0u : 1u; s.ref_pos = ref; s.len = (int32_t)len; s.read_off = ctg + head; s.pad = 0; out[at] = s; }
            }
            if (op == 2) ref += (int32_t)len; else ctg += (int32_t)len;
        }
    }
}

// the device buffers live for the call (a buffer kept on the context would change what the caller sees in free memory)
int read_signatures_impl(fsv_ctx *ctx, const fsv_bam_records *rec, int min_mapq, int min_svlen, fsv_read_sig *out, uint32_t cap, uint32_t *n_out)
{
    if (!ctx || !rec || !out || !n_out) return FSV_EINVAL;
    *n_out = 0;
    if (rec->n_rec == 0) return FSV_OK;
    FSV_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)rec->n_rec;
    Dev<int32_t> d_pos; Dev<uint8_t> d_mq; Dev<uint64_t> d_off; Dev<uint32_t> d_nop, d_cig, d_n; Dev<fsv_read_sig> d_out;
    TRY(upload(ctx, d_pos, rec->pos, n)); TRY(upload(ctx, d_mq, rec->mapq, n)); TRY(upload(ctx, d_off, rec->cigar_off, n));
    TRY(upload(ctx, d_nop, rec->n_cigar_op, n)); TRY(upload(ctx, d_cig, rec->cigar, (size_t)rec->n_cigar));
    TRY(ensure(ctx, d_out, cap)); TRY(ensure(ctx, d_n, 1)); TRY(zero(ctx, d_n, 1));
    FSV_LAUNCH(ctx, ctx->stream, k_cigar_sigs, dim3(fsv_grid_for(rec->n_rec, 256)), dim3(256), 0, d_pos.p, d_mq.p, d_off.p, d_nop.p, d_cig.p, (uint32_t)n,
               min_mapq, min_svlen, d_out.p, cap, d_n.p);
    uint32_t cnt = 0;
    TRY(download(ctx, &cnt, d_n, 1));
    FSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *n_out = cnt;
    if (cnt > cap) return FSV_ECAP;
    if (cnt) { TRY(download(ctx, out, d_out, cnt)); FSV_HIP(ctx, hipStreamSynchronize(ctx->stream)); }
    return FSV_OK;
}
} // namespace

extern "C" int fsv_read_signatures(fsv_ctx *ctx, const fsv_bam_records *rec, int min_mapq, int min_svlen, fsv_read_sig *out, uint32_t cap, uint32_t *n_out)
{
    BAM_GUARD(FSV_EINVAL, read_signatures_impl(ctx, rec, min_mapq, min_svlen, out, cap, n_out))
}

// ---------------------------------------------------------------------------------------------------------------------
// fsv_bam_write: a coordinate-sorted BAM and its .bai from flat arrays (SAM/BAM specification v1, sections 4.1, 4.2, 5.2, 5.3)
namespace {

constexpr size_t BGZF_PAYLOAD = 0xff00;

int reg2bin(int64_t beg, int64_t end)
{
    --end;
    if (beg >> 14 == end >> 14) return (int)(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (int)(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (int)(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (int)(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (int)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}

template <class T> void put_le(std::vector<uint8_t> &v, T x) { const size_t at = v.size(); v.resize(at + sizeof(T)); memcpy(v.data() + at, &x, sizeof(T)); }

// one BGZF block of n payload bytes (n <= BGZF_PAYLOAD; n = 0: the end-of-file marker): header, raw deflate, crc32, isize
bool bgzf_block(const uint8_t *src, size_t n, std::vector<uint8_t> &out)
{
    for (int level : {6, 0}) {   // (a payload that deflate cannot fit into a 64 KiB block goes in stored: 0xff00 bytes always fit)
        out.assign(18 + compressBound((uLong)n) + 8, 0);
        z_stream zs;
        memset(&zs, 0, sizeof(zs));
        if (deflateInit2(&zs, level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) return false;
        zs.next_in = const_cast<Bytef *>(src); zs.avail_in = (uInt)n;
        zs.next_out = out.data() + 18; zs.avail_out = (uInt)(out.size() - 18 - 8);
        const int rc = deflate(&zs, Z_FINISH);
        const size_t clen = zs.total_out;
        deflateEnd(&zs);
        if (rc != Z_STREAM_END) return false;
        const size_t bsize = 18 + clen + 8;
        if (bsize > 65536) continue;
        static const uint8_t head[16] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 'B', 'C', 2, 0};
        memcpy(out.data(), head, 16);
        const uint16_t bs = (uint16_t)(bsize - 1);
        memcpy(out.data() + 16, &bs, 2);
        const uint32_t crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), src, (uInt)n), isize = (uint32_t)n;
        memcpy(out.data() + 18 + clen, &crc, 4);
        memcpy(out.data() + 18 + clen + 4, &isize, 4);
        out.resize(bsize);
        return true;
    }
    return false;
}

// a file under a temporary name next to its final one: written whole, renamed by commit(), removed if that never happens
struct TempFile {
    std::string tmp, final_path; FILE *f = nullptr;
    explicit TempFile(const std::string &path) : tmp(path + ".tmpXXXXXX"), final_path(path)
    {
        const int fd = mkstemp(&tmp[0]);
        if (fd >= 0) { f = fdopen(fd, "wb"); if (!f) { close(fd); unlink(tmp.c_str()); } }
    }
    TempFile(const TempFile &) = delete;
    TempFile &operator=(const TempFile &) = delete;
    bool write(const void *p, size_t n) { return f && (n == 0 || fwrite(p, 1, n, f) == n); }
    bool flush() { if (!f) return false; const bool ok = fclose(f) == 0; f = nullptr; if (ok) { const mode_t m = umask(0); umask(m); (void)chmod(tmp.c_str(), 0666 & ~m); } return ok; }   // (mkstemp makes it 0600)
    bool commit() { if (tmp.empty() || rename(tmp.c_str(), final_path.c_str()) != 0) return false; tmp.clear(); return true; }
    ~TempFile() { if (f) fclose(f); if (!tmp.empty()) unlink(tmp.c_str()); }
};

// the arguments and every record, in the order that decides which error a doubly wrong input gets; ref_span[i]: the reference bases of record i
int check_records(const char *path, const fsv_bam_out *in, std::vector<int64_t> &ref_span)
{
    if (!path || !in || (in->n_refs && (!in->ref_name || !in->ref_len))) return FSV_EINVAL;
    const uint64_t n = in->n_rec;
    if (n && (!in->ref_id || !in->pos || !in->flag || !in->mapq || !in->qname_off || !in->qname || !in->cigar_off || !in->n_cigar_op || !in->seq_off)) return FSV_EINVAL;
    if ((in->cs_off == nullptr) != (in->cs == nullptr) || (in->sa_off == nullptr) != (in->sa == nullptr)) return FSV_EINVAL;
    for (uint32_t r = 0; r < in->n_refs; r++) if (!in->ref_name[r] || in->ref_len[r] < 0) return FSV_EINVAL;
    ref_span.assign(n, 0);
    for (uint64_t i = 0; i < n; i++) {
        const int32_t rid = in->ref_id[i];
        if (strlen(in->qname + in->qname_off[i]) > 254 || in->seq_off[i + 1] < in->seq_off[i] || in->seq_off[i + 1] - in->seq_off[i] > 0x7fffffffull) return FSV_EINVAL;
        if (in->n_cigar_op[i] > 65535) return FSV_EUNSUP;
        if (in->n_cigar_op[i] && !in->cigar) return FSV_EINVAL;
        if (rid == -1) { if (in->pos[i] != -1 || !(in->flag[i] & 4) || in->n_cigar_op[i]) return FSV_EINVAL; continue; }
        if (rid < 0 || (uint32_t)rid >= in->n_refs || in->pos[i] < 0 || (in->flag[i] & 4)) return FSV_EINVAL;
        for (uint32_t k = 0; k < in->n_cigar_op[i]; k++) {
            const uint32_t c = in->cigar[in->cigar_off[i] + k], op = c & 0xf;
            if (op > 8) return FSV_EINVAL;
            if (cigar_consumes_ref(op)) ref_span[i] += c >> 4;
        }
        if (ref_span[i] == 0) return FSV_EINVAL;
        if ((int64_t)in->pos[i] + ref_span[i] > (1ll << 29)) return FSV_EUNSUP;     // beyond what a .bai can index
    }
    return FSV_OK;
}

// the records by (reference, position), equal ones in input order, unmapped ones (-1) last
std::vector<uint64_t> stable_order(const fsv_bam_out *in)
{
    std::vector<uint64_t> order(in->n_rec);
    std::iota(order.begin(), order.end(), 0ull);
    std::stable_sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) {
        const uint32_t ra = (uint32_t)in->ref_id[a], rb = (uint32_t)in->ref_id[b];     // -1 sorts last
        return ra != rb ? ra < rb : (ra != 0xffffffffu && in->pos[a] < in->pos[b]);
    });
    return order;
}

void encode_header(const fsv_bam_out *in, std::vector<uint8_t> &st)
{
    const char *text = in->header_text ? in->header_text : "";
    st.insert(st.end(), {'B', 'A', 'M', 1});
    put_le<int32_t>(st, (int32_t)strlen(text));
    st.insert(st.end(), text, text + strlen(text));
    put_le<int32_t>(st, (int32_t)in->n_refs);
    for (uint32_t r = 0; r < in->n_refs; r++) {
        const size_t l = strlen(in->ref_name[r]) + 1;
        put_le<int32_t>(st, (int32_t)l);
        st.insert(st.end(), in->ref_name[r], in->ref_name[r] + l);
        put_le<int32_t>(st, in->ref_len[r]);
    }
}

// record i behind what st holds; FSV_EUNSUP when it is longer than a block_size can say
int encode_record(const fsv_bam_out *in, uint64_t i, int64_t ref_span, std::vector<uint8_t> &st)
{
    const size_t at0 = st.size();
    const char *name = in->qname + in->qname_off[i];
    const size_t l_name = strlen(name) + 1;
    const int32_t l_seq = (int32_t)(in->seq_off[i + 1] - in->seq_off[i]);
    const int64_t end = (int64_t)in->pos[i] + std::max<int64_t>(1, ref_span);
    put_le<int32_t>(st, 0);     // block_size, set below
    put_le<int32_t>(st, in->ref_id[i]); put_le<int32_t>(st, in->pos[i]);
    st.push_back((uint8_t)l_name); st.push_back(in->mapq[i]);
    put_le<uint16_t>(st, (uint16_t)reg2bin(in->pos[i], end)); put_le<uint16_t>(st, (uint16_t)in->n_cigar_op[i]); put_le<uint16_t>(st, in->flag[i]);
    put_le<int32_t>(st, l_seq); put_le<int32_t>(st, -1); put_le<int32_t>(st, -1); put_le<int32_t>(st, 0);
    st.insert(st.end(), name, name + l_name);
    if (in->n_cigar_op[i]) { const uint8_t *c = (const uint8_t *)(in->cigar + in->cigar_off[i]); st.insert(st.end(), c, c + (size_t)in->n_cigar_op[i] * 4); }
    const uint8_t *sq = (const uint8_t *)(in->seq ? in->seq + in->seq_off[i] : nullptr);
    const size_t at = st.size();
    st.resize(at + (size_t)(l_seq + 1) / 2, 0);
    for (int32_t j = 0; j < l_seq; j++) st[at + (size_t)(j >> 1)] |= (uint8_t)(base_tabs.nib[sq[j]] << ((j & 1) ? 0 : 4));
    st.insert(st.end(), (size_t)l_seq, 0xff);
    if (in->nm && in->nm[i] != FSV_BAM_NO_TAG) { st.insert(st.end(), {'N', 'M', 'i'}); put_le<int32_t>(st, in->nm[i]); }
    if (in->cs && in->cs_off[i + 1] > in->cs_off[i]) {
        st.insert(st.end(), {'c', 's', 'Z'});
        st.insert(st.end(), in->cs + in->cs_off[i], in->cs + in->cs_off[i + 1]);
        st.push_back(0);
    }
    if (in->sa && in->sa[in->sa_off[i]]) {
        const char *sa = in->sa + in->sa_off[i];
        st.insert(st.end(), {'S', 'A', 'Z'});
        st.insert(st.end(), sa, sa + strlen(sa) + 1);
    }
    const uint64_t body = st.size() - at0 - 4;
    if (body > 0x7fffffffull) return FSV_EUNSUP;
    const int32_t bs = (int32_t)body;
    memcpy(st.data() + at0, &bs, 4);
    return FSV_OK;
}

// the uncompressed stream: header, then the records; start[k]: where record order[k] begins, start[n]: the end
int encode_stream(const fsv_bam_out *in, const std::vector<uint64_t> &order, const std::vector<int64_t> &ref_span, std::vector<uint8_t> &st,
                  std::vector<uint64_t> &start)
{
    encode_header(in, st);
    start.resize(order.size() + 1);
    for (size_t k = 0; k < order.size(); k++) {
        start[k] = st.size();
        TRY(encode_record(in, order[k], ref_span[order[k]], st));
    }
    start[order.size()] = st.size();
    return FSV_OK;
}

// BGZF: blocks of BGZF_PAYLOAD bytes, deflated side by side, then the end-of-file marker
bool deflate_blocks(const std::vector<uint8_t> &st, int n_threads, std::vector<std::vector<uint8_t>> &blk)
{
    const size_t nb = (st.size() + BGZF_PAYLOAD - 1) / BGZF_PAYLOAD;
    blk.resize(nb + 1);
    const unsigned nt = (unsigned)std::min<size_t>((size_t)std::min(16, std::max(1, n_threads)), std::max<size_t>(1, nb / 4));
    const bool ok = fan_out(nb, nt, [&](size_t b) { return bgzf_block(st.data() + b * BGZF_PAYLOAD, std::min(BGZF_PAYLOAD, st.size() - b * BGZF_PAYLOAD), blk[b]); });
    return ok && bgzf_block(nullptr, 0, blk[nb]);
}

// the index: per reference the bins' chunks (neighbours in file order joined) and the linear index
std::vector<uint8_t> build_bai(const fsv_bam_out *in, const std::vector<uint64_t> &order, const std::vector<int64_t> &ref_span,
                               const std::vector<uint64_t> &start, const std::vector<std::vector<uint8_t>> &blk)
{
    std::vector<uint64_t> caddr(blk.size() + 1, 0);
    for (size_t b = 0; b < blk.size(); b++) caddr[b + 1] = caddr[b] + blk[b].size();
    auto voff = [&](uint64_t u) { return caddr[u / BGZF_PAYLOAD] << 16 | (u % BGZF_PAYLOAD); };
    const uint64_t n = in->n_rec;
    std::vector<uint8_t> bai;
    bai.insert(bai.end(), {'B', 'A', 'I', 1});
    put_le<int32_t>(bai, (int32_t)in->n_refs);
    uint64_t k = 0;
    for (uint32_t r = 0; r < in->n_refs; r++) {
        std::map<uint32_t, std::vector<std::pair<uint64_t, uint64_t>>> bins;
        std::vector<uint64_t> lin;
        for (; k < n && in->ref_id[order[k]] == (int32_t)r; k++) {
            const uint64_t i = order[k];
            const int64_t beg = in->pos[i], end = beg + ref_span[i];
            const uint64_t v0 = voff(start[k]), v1 = voff(start[k + 1]);
            auto &ch = bins[(uint32_t)reg2bin(beg, end)];
            if (!ch.empty() && ch.back().second == v0) ch.back().second = v1; else ch.emplace_back(v0, v1);
            const size_t w1 = (size_t)((end - 1) >> 14);
            if (lin.size() <= w1) lin.resize(w1 + 1, ~0ull);
            for (size_t w = (size_t)(beg >> 14); w <= w1; w++) lin[w] = std::min(lin[w], v0);
        }
        put_le<int32_t>(bai, (int32_t)bins.size());
        for (const auto &b : bins) {
            put_le<uint32_t>(bai, b.first); put_le<int32_t>(bai, (int32_t)b.second.size());
            for (const auto &c : b.second) { put_le<uint64_t>(bai, c.first); put_le<uint64_t>(bai, c.second); }
        }
        put_le<int32_t>(bai, (int32_t)lin.size());
        uint64_t last = 0;
        for (uint64_t v : lin) { if (v != ~0ull) last = v; put_le<uint64_t>(bai, last); }     // an empty window carries the previous offset forward
    }
    put_le<uint64_t>(bai, n - k);     // the records without a coordinate
    return bai;
}

// both files whole under temporary names, then renamed
int write_files(const char *path, const std::vector<std::vector<uint8_t>> &blk, const std::vector<uint8_t> &bai)
{
    TempFile fb(path), fi(std::string(path) + ".bai");
    bool w = fb.f && fi.f;
    for (size_t b = 0; w && b < blk.size(); b++) w = fb.write(blk[b].data(), blk[b].size());
    w = w && fi.write(bai.data(), bai.size());
    w = w && fb.flush() && fi.flush();
    if (!w || !fb.commit()) return FSV_EINTERNAL;
    if (!fi.commit()) { unlink(path); return FSV_EINTERNAL; }
    return FSV_OK;
}

int bam_write_impl(const char *path, const fsv_bam_out *in, int n_threads)
{
    std::vector<int64_t> ref_span;
    TRY(check_records(path, in, ref_span));
    const std::vector<uint64_t> order = stable_order(in);
    std::vector<uint8_t> st;
    std::vector<uint64_t> start;
    TRY(encode_stream(in, order, ref_span, st, start));
    std::vector<std::vector<uint8_t>> blk;
    if (!deflate_blocks(st, n_threads, blk)) return FSV_EINTERNAL;
    return write_files(path, blk, build_bai(in, order, ref_span, start, blk));
}

} // namespace

extern "C" int fsv_bam_write(const char *path, const fsv_bam_out *in, int n_threads) { BAM_GUARD(FSV_EINTERNAL, bam_write_impl(path, in, n_threads)) }
