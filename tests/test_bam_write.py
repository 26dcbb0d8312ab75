"""fsv_bam_write (focalsv_amd/csrc/bam.hip, host only: runs without a GPU): the stream against tests/bam_writer.py's encoder, the
records back through the library's reader, the .bai parsed here, the error returns."""
import os
import random
import struct
import zlib

import pytest

from focalsv_amd import _lib, bam as B
from tests import bam_writer as W

REFS = [("chr1", 9000000), ("chr2", 600000), ("chrEmpty", 1000), ("chr3", 200000)]
HEADER = "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chr1\tLN:9000000\n@PG\tID:test\n"
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def _seq(rng, n):
    return "".join(rng.choices("ACGT", k=n))


def _rec(rng, ref, pos, cigar, name, tags="all", seq=None):
    ql = sum(n for op, n in cigar if op in (0, 1, 4))
    r = {"ref": ref, "pos": pos, "mapq": rng.choice([0, 37, 60]), "flag": rng.choice([0, 16, 2048, 2064]), "qname": name, "cigar": cigar,
         "seq": _seq(rng, ql) if seq is None else seq}
    if tags in ("all", "nm", "nm+sa"):
        r["nm"] = rng.randrange(0, 5000)
    if tags in ("all", "cs"):
        r["cs"] = ":%d*ag+ttt-c:7" % rng.randrange(1, 100000)
    if tags in ("all", "sa", "nm+sa"):
        r["sa"] = "chr2,%d,+,100M20S,60,3;chr1,5,-,20S100M,0,11;" % rng.randrange(1, 500000)
    return r


def make_records(seed=11):
    rng = random.Random(seed)
    recs = []
    kinds = ["all", "nm", "cs", "sa", "nm+sa", "none"]
    for k in range(160):      # scattered records, many sharing a position
        ref = rng.choice([0, 0, 1, 3])
        pos = rng.choice([100, 16000, 16383, 16384, 40000]) if k % 4 == 0 else rng.randrange(0, REFS[ref][1] - 5000)
        m = rng.randrange(1, 1500)
        cigar = [(4, rng.randrange(1, 30))] * (k % 3 == 0) + [(0, m), (1, rng.randrange(1, 40)), (0, rng.randrange(1, 900)), (2, rng.randrange(1, 3000)), (0, 5)]
        recs.append(_rec(rng, ref, pos, cigar, "ctg_%d" % k, kinds[k % 6]))
    # across 16 kb windows and across the boundaries of every bin level (2^14, 2^17, 2^20, 2^23)
    for j, (pos, ln) in enumerate([(16380, 10), (16383, 1), (16384, 1), (16000, 40000), ((1 << 17) - 3, 10), ((1 << 20) - 50, 100), ((1 << 23) - 1, 2),
                                   (100, 8500000), (500000, 20000)]):
        recs.append(_rec(rng, 0, pos, [(0, ln)], "span_%d" % j, kinds[j % 6], seq="" if ln > 100000 else None))
    recs.append(_rec(rng, 1, 70000, [(0, 150000)], "multi_block", "all"))                                        # a record of several BGZF blocks
    recs.append(_rec(rng, 3, 1234, [(0, 3), (1, 2)] * 499 + [(0, 7), (2, 1)], "ops_1000", "nm"))               # 1 000 ops
    recs.append(_rec(rng, 3, 1234, [(0, 50)], "n" * 254, "none"))                                               # the longest name a BAM holds
    recs.append(_rec(rng, 1, 599990, [(0, 10)], "q" * 200, "cs"))
    recs.append(_rec(rng, 3, 50, [(0, 20)], "no_seq", "sa", seq=""))
    for j in range(3):
        recs.append({"ref": -1, "pos": -1, "mapq": 0, "flag": 4, "qname": "unmapped_%d" % j, "cigar": [], "seq": _seq(rng, 300 + j)})
    rng.shuffle(recs)
    return recs


def sorted_records(recs):
    return sorted(recs, key=lambda r: (r["ref"] if r["ref"] >= 0 else 1 << 40, r["pos"]))     # (Python's sort is stable)


def tags_of(r):
    t = []
    if r.get("nm") is not None:
        t.append(("NM", "i", r["nm"]))
    if r.get("cs"):
        t.append(("cs", "Z", r["cs"]))
    if r.get("sa"):
        t.append(("SA", "Z", r["sa"]))
    return t


def bgzf_members(raw):
    """[(file offset, payload)] of every BGZF block of the file"""
    out, at = [], 0
    while at < len(raw):
        assert raw[at:at + 4] == b"\x1f\x8b\x08\x04" and raw[at + 12:at + 16] == b"BC\x02\x00"
        bsize = struct.unpack_from("<H", raw, at + 16)[0] + 1
        data = zlib.decompress(raw[at + 18:at + bsize - 8], -15)
        crc, isize = struct.unpack_from("<II", raw, at + bsize - 8)
        assert isize == len(data) <= 0xff00 and crc == zlib.crc32(data) & 0xffffffff
        out.append((at, data))
        at += bsize
    return out


def parse_bai(path, n_refs):
    raw = open(path, "rb").read()
    assert raw[:4] == b"BAI\1" and struct.unpack_from("<i", raw, 4)[0] == n_refs
    at, out = 8, []
    for _ in range(n_refs):
        bins = {}
        (n_bin,), at = struct.unpack_from("<i", raw, at), at + 4
        for _ in range(n_bin):
            (b, n_chunk), at = struct.unpack_from("<Ii", raw, at), at + 8
            assert b not in bins
            bins[b] = [struct.unpack_from("<QQ", raw, at + 16 * c) for c in range(n_chunk)]
            at += 16 * n_chunk
        (n_intv,), at = struct.unpack_from("<i", raw, at), at + 4
        lin = list(struct.unpack_from("<%dQ" % n_intv, raw, at))
        at += 8 * n_intv
        out.append((bins, lin))
    assert len(raw) - at in (0, 8)      # the optional count of unplaced reads
    return out


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    d = tmp_path_factory.mktemp("bamw")
    recs = make_records()
    path = _lib.bam_write(str(d / "w.bam"), REFS, recs, header_text=HEADER, threads=4)
    srt = sorted_records(recs)
    text = HEADER.encode()
    head = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(REFS))
    for name, ln in REFS:
        head += struct.pack("<i", len(name) + 1) + name.encode() + b"\0" + struct.pack("<i", ln)
    enc = [W.encode_record(r["ref"], r["pos"], r["mapq"], r["flag"], r["qname"], r["cigar"], r["seq"], tags_of(r)) for r in srt]
    starts, u = [], len(head)
    for e in enc:
        starts.append(u)
        u += len(e)
    return {"path": path, "recs": recs, "sorted": srt, "stream": head + b"".join(enc), "starts": starts, "raw": open(path, "rb").read()}


def test_stream_is_the_reference_encoding(written):
    mem = bgzf_members(written["raw"])
    assert len(mem) >= 4 and mem[-1][1] == b"" and written["raw"][-28:] == EOF_BLOCK
    assert all(len(d) > 0 for _, d in mem[:-1])
    got = b"".join(d for _, d in mem)
    assert len(got) == len(written["stream"]) and got == written["stream"]
    assert sorted(os.listdir(os.path.dirname(written["path"]))) == ["w.bam", "w.bam.bai"]       # no temporary file left


def test_thread_count_does_not_change_the_bytes(written, tmp_path):
    for t in (1, 16, 1000, 0):
        p = _lib.bam_write(str(tmp_path / ("t%d.bam" % t)), REFS, written["recs"], header_text=HEADER, threads=t)
        assert open(p, "rb").read() == written["raw"]
        assert open(p + ".bai", "rb").read() == open(written["path"] + ".bai", "rb").read()


def _check_records(got, exp):
    assert len(got) == len(exp) and got.names == [r["qname"] for r in exp]
    for k, r in enumerate(exp):
        c = got.cigar[int(got.cigar_off[k]): int(got.cigar_off[k]) + int(got.n_cigar_op[k])]
        assert [(int(x) & 0xf, int(x) >> 4) for x in c] == r["cigar"]
        assert (int(got.ref_id[k]), int(got.pos[k]), int(got.flag[k]), int(got.mapq[k])) == (r["ref"], r["pos"], r["flag"], r["mapq"])
        assert got.seq_text(k) == r["seq"] and got.sa_tag(k) == (r.get("sa") or "")


def _overlap(srt, ri, beg, end):
    return [r for r in srt if r["ref"] == ri and r["pos"] < end and r["pos"] + W._ref_len(r["cigar"]) > beg]


REGIONS = [(0, b + d0, b + d1) for b in (16384, 32768, 1 << 17, 1 << 20, 1 << 23) for d0, d1 in ((-5, 5), (0, 1), (-1, 0), (-1, 1), (3, 20000))] + \
          [(0, 0, 1), (0, 8999999, 9000000), (1, 0, 600000), (1, 219999, 220001), (2, 0, 1000), (3, 1234, 1235), (3, 150000, 200000)]


def test_reader_round_trip_and_region_fetches(written, tmp_path):
    srt = written["sorted"]
    with B.BamFile(written["path"]) as bam:
        assert bam.has_index and bam.references == [n for n, _ in REFS] and bam.reference_lengths == [ln for _, ln in REFS]
        _check_records(bam.fetch(until_eof=True, want_seq=6), srt)
        for ri, beg, end in REGIONS:
            _check_records(bam.fetch(REFS[ri][0], beg, end, want_seq=6), _overlap(srt, ri, beg, end))
    bare = tmp_path / "bare.bam"
    bare.write_bytes(written["raw"])                    # the same file without its .bai: every fetch scans
    with B.BamFile(str(bare)) as bam:
        assert not bam.has_index
        for ri, beg, end in REGIONS:
            _check_records(bam.fetch(REFS[ri][0], beg, end, want_seq=6), _overlap(srt, ri, beg, end))


def test_index(written):
    mem = bgzf_members(written["raw"])
    srt, starts = written["sorted"], written["starts"]
    ubase, u = [], 0
    for _, d in mem:
        ubase.append(u)
        u += len(d)

    def voff(upos):
        b = max(i for i in range(len(mem)) if ubase[i] <= upos and len(mem[i][1]) > 0)
        return mem[b][0] << 16 | (upos - ubase[b])

    start_voff = [voff(s) for s in starts]
    by_addr = dict(mem)
    bai = parse_bai(written["path"] + ".bai", len(REFS))
    for ri, (bins, lin) in enumerate(bai):
        mine = [(r, v) for r, v in zip(srt, start_voff) if r["ref"] == ri]
        if not mine:
            assert not bins and not lin
            continue
        wins = {}
        for r, v in mine:
            beg, end = r["pos"], r["pos"] + W._ref_len(r["cigar"])
            chunks = bins[W.reg2bin(beg, end)]
            assert any(a <= v < b for a, b in chunks), (r["qname"], hex(v), chunks)
            for w in range(beg >> 14, ((end - 1) >> 14) + 1):
                wins[w] = min(wins.get(w, 1 << 63), v)
        assert set(bins) == {W.reg2bin(r["pos"], r["pos"] + W._ref_len(r["cigar"])) for r, _ in mine}
        assert len(lin) == max(wins) + 1
        last = 0
        for w, got in enumerate(lin):
            last = wins.get(w, last)
            assert got == last, (ri, w)
        at_voff = {v: r for r, v in mine}
        for chunks in bins.values():
            assert all(a < b for a, b in chunks) and all(chunks[i][1] <= chunks[i + 1][0] for i in range(len(chunks) - 1))
            for a, _ in chunks:         # a chunk starts on a record header of this reference
                data = by_addr[a >> 16]
                tail = data[a & 0xffff:] + b"".join(d for o, d in mem if o > a >> 16)[:64]
                bs, ref_id, pos, l_name = struct.unpack_from("<iiiB", tail, 0)
                r = at_voff[a]
                assert (ref_id, pos, l_name) == (ri, r["pos"], len(r["qname"]) + 1) and bs >= 32


def test_errors(tmp_path):
    ok = {"ref": 0, "pos": 5, "mapq": 60, "flag": 0, "qname": "a", "cigar": [(0, 4)], "seq": "ACGT"}
    for bad in ({"ref": len(REFS)}, {"ref": -2}, {"cigar": [(4, 4)]}, {"cigar": []}, {"pos": -1}, {"qname": "x" * 255}, {"flag": 4},
                {"ref": -1, "pos": -1, "flag": 0, "cigar": []}, {"ref": -1, "pos": -1, "flag": 4}):
        p = tmp_path / "bad.bam"
        with pytest.raises(_lib.FsvError) as e:
            _lib.bam_write(str(p), REFS, [ok, dict(ok, **bad)])
        assert e.value.code == _lib.EINVAL, bad
        assert os.listdir(tmp_path) == []
    with pytest.raises(_lib.FsvError):
        _lib.bam_write(str(tmp_path / "no_such_dir" / "x.bam"), REFS, [ok])
    assert os.listdir(tmp_path) == []
    p = _lib.bam_write(str(tmp_path / "empty.bam"), REFS, [])         # no records at all is a valid file
    with B.BamFile(p) as bam:
        assert bam.has_index and len(bam.fetch(until_eof=True)) == 0 and len(bam.fetch("chr2")) == 0
