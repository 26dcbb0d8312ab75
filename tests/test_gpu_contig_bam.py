"""dippav_variant_call(..., contig_bam=True): assemblies.sorted.bam + .bai beside outputs that stay byte for byte, the records the
calls were made from inside it, NM / cs equal to tests/cs_model.py on the chromosome text, SA tags on the split contigs."""
import gzip
import os
import struct

import numpy as np
import pytest

from focalsv_amd import _lib, bam as B, fasta, synth
from focalsv_amd.dippav import variant_call as VC, vcf
from .cs_model import cs_nm

pytestmark = pytest.mark.gpu

CHR_LEN = 200000


def _rnd(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=n))


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = tmp_path_factory.mktemp("contig_bam")
    rng = np.random.default_rng(77)
    chrom = bytearray(_rnd(rng, CHR_LEN))
    hp = ([], [])
    for k, i in enumerate((1, 4, 6)):                     # planted DEL / INS (region 4: also a private INS on haplotype 2)
        r = synth.make_region(i, width=16000, depth_per_hap=0.3, start=10000 + 40000 * k)
        chrom[r.start:r.start + 16000] = r.ref
        for h in (0, 1):
            hp[h].append(("Region_chr21_S%d_E%d" % (r.start, r.start + 16000), r.haps[h]))
    s, ref = 130000, _rnd(rng, 30000)                     # a region whose haplotype 2 carries an inverted piece: three records, SA tags
    chrom[s:s + 30000] = ref
    tag = "Region_chr21_S%d_E%d" % (s, s + 30000)
    hp[0].append((tag, ref[:9000] + ref[9100:]))
    hp[1].append((tag, ref[:12000] + synth.revcomp(ref[12000:14000]) + ref[14000:]))
    hp[1].append((tag, _rnd(rng, 3000)))                  # matches nothing in its window: unaligned
    hp[0].append((tag, b"ACGTACGT"))                      # shorter than a seed: unaligned
    paths = []
    for h in (0, 1):
        paths.append(str(d / ("in_hp%d.fa" % (h + 1))))
        with open(paths[-1], "w") as f:
            for name, seq in hp[h]:
                f.write(">" + name + "\n" + fasta.fold(seq.decode()) + "\n")
    ref_fa = str(d / "ref.fa")
    with open(ref_fa, "w") as f:
        f.write(">chr20\n" + fasta.fold(_rnd(rng, 4000).decode(), 60) + "\n>chr21 the one\n" + fasta.fold(bytes(chrom).decode(), 60) + "\n")
    captured = []
    real = VC.records_from_alignment

    def spy(*a, **kw):
        captured.append(real(*a, **kw))
        return captured[-1]
    VC.records_from_alignment = spy
    try:
        with _lib.Context(0) as ctx:
            for sub, on in (("off", False), ("on", True)):
                VC.dippav_variant_call("CCS", None, ref_fa, paths[0], paths[1], str(d / sub), 21, read_records=[], ctx=ctx, contig_bam=on)
    finally:
        VC.records_from_alignment = real
    assert len(captured) == 2 and captured[0] == captured[1]
    return {"off": str(d / "off"), "on": str(d / "on"), "records": captured[1], "chrom": bytes(chrom).decode(),
            "contigs": {"contig_hp%d_%d" % (h + 1, k): seq.decode() for h in (0, 1) for k, (_, seq) in enumerate(hp[h])}}


def _files(root):
    out = {}
    for base, _, names in os.walk(root):
        for n in names:
            p = os.path.join(base, n)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def test_files_and_everything_else_unchanged(case):
    off, on = _files(case["off"]), _files(case["on"])
    assert set(on) - set(off) == {"assemblies.sorted.bam", "assemblies.sorted.bam.bai"}
    assert "assemblies.sorted.bam" not in off
    for name, data in off.items():
        assert on[name] == data, name


def bam_records(path):
    """every record of a BAM, parsed here: dicts with the fixed fields, SEQ text and the aux tags NM / cs / SA"""
    raw = gzip.open(path, "rb").read()
    assert raw[:4] == b"BAM\1"
    l_text, = struct.unpack_from("<i", raw, 4)
    text = raw[8:8 + l_text].decode()
    at = 8 + l_text
    n_ref, = struct.unpack_from("<i", raw, at)
    at += 4
    refs = []
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", raw, at)
        refs.append((raw[at + 4:at + 4 + l_name - 1].decode(), struct.unpack_from("<i", raw, at + 4 + l_name)[0]))
        at += 8 + l_name
    out = []
    while at < len(raw):
        bs, ref_id, pos, l_name, mapq, _bin, n_cig, flag, l_seq = struct.unpack_from("<iiiBBHHHi", raw, at)
        p = at + 36
        name = raw[p:p + l_name - 1].decode()
        p += l_name
        cig = [(c & 0xf, c >> 4) for c in struct.unpack_from("<%dI" % n_cig, raw, p)]
        p += 4 * n_cig
        seq = "".join("=ACMGRSVTWYHKDBN"[(raw[p + (j >> 1)] >> (0 if j & 1 else 4)) & 15] for j in range(l_seq))
        p += (l_seq + 1) // 2 + l_seq
        tags, order = {}, []
        while p < at + 4 + bs:
            t, ty = raw[p:p + 2].decode(), chr(raw[p + 2])
            order.append(t)
            if ty == "i":
                tags[t] = struct.unpack_from("<i", raw, p + 3)[0]
                p += 7
            else:
                assert ty == "Z"
                e = raw.index(b"\0", p + 3)
                tags[t] = raw[p + 3:e].decode()
                p = e + 1
        assert p == at + 4 + bs and order == [t for t in ("NM", "cs", "SA") if t in tags]
        out.append({"ref": ref_id, "pos": pos, "mapq": mapq, "flag": flag, "qname": name, "cigar": cig, "seq": seq, "tags": tags})
        at += 4 + bs
    return text, refs, out


def test_records_are_the_ones_the_calls_were_made_from(case):
    path = os.path.join(case["on"], "assemblies.sorted.bam")
    with B.BamFile(path) as bam:
        assert bam.has_index and bam.references == ["chr20", "chr21"] and bam.reference_lengths == [4000, CHR_LEN]
        got = bam.fetch(until_eof=True, want_seq=6)
        mapped = [k for k in range(len(got)) if got.ref_id[k] >= 0]
        segs = [got.segment(k) for k in mapped]
        assert segs == case["records"] and len(segs) >= 10
        assert [got.names[k] for k in range(len(got)) if got.ref_id[k] < 0] == ["contig_hp1_4", "contig_hp2_4"]     # the unaligned contigs, last
        assert all(int(got.flag[k]) == 4 and got.seq_text(k) == case["contigs"][got.names[k]] for k in range(len(got)) if got.ref_id[k] < 0)
        by_region = bam.fetch("chr21", 130000, 160000)
        assert [by_region.segment(k) for k in range(len(by_region))] == [r for r in case["records"] if r.reference_end > 130000 and r.pos < 160000]
    body = VC.call_chromosome(segs, "chr21", case["chrom"], case["contigs"])[1]
    lines = open(os.path.join(case["on"], "dippav_variant_chr21.vcf")).readlines()
    assert lines[:len(vcf.HEADER_LINES)] == vcf.HEADER_LINES and lines[len(vcf.HEADER_LINES):] == body and len(body) >= 3


def test_tags(case):
    text, refs, recs = bam_records(os.path.join(case["on"], "assemblies.sorted.bam"))
    assert text.split("\n")[:3] == ["@HD\tVN:1.6\tSO:coordinate", "@SQ\tSN:chr20\tLN:4000", "@SQ\tSN:chr21\tLN:%d" % CHR_LEN]
    assert text.split("\n")[3].startswith("@PG\tID:focalsv_amd") and refs == [("chr20", 4000), ("chr21", CHR_LEN)]
    mapped = [r for r in recs if r["ref"] >= 0]
    by_name = {}
    for r in mapped:
        by_name.setdefault(r["qname"], []).append(r)
        oriented = case["contigs"][r["qname"]]
        if r["flag"] & 16:
            oriented = synth.revcomp(oriented.encode()).decode()
        assert r["seq"] == oriented                                                     # the full contig on the record's strand, clips kept
        assert (r["tags"]["NM"], r["tags"]["cs"]) == cs_nm(r["cigar"], r["seq"], case["chrom"], r["pos"]), r["qname"]
    assert any(r["tags"]["NM"] > 0 for r in mapped)
    split = {n: rs for n, rs in by_name.items() if len(rs) > 1}
    assert "contig_hp2_3" in split and len(split["contig_hp2_3"]) == 3                  # the inverted piece and what it cuts apart
    assert {bool(r["flag"] & 16) for r in split["contig_hp2_3"]} == {False, True}
    for r in mapped:
        assert ("SA" in r["tags"]) == (r["qname"] in split)
    for rs in split.values():
        primary = [r for r in rs if not r["flag"] & 2048]
        assert len(primary) == 1

        def entry(r):
            return "chr21,%d,%s,%s,%d,%d" % (r["pos"] + 1, "-" if r["flag"] & 16 else "+", B.cigar_string(r["cigar"]), r["mapq"], r["tags"]["NM"])
        for r in rs:
            assert r["tags"]["SA"].endswith(";")
            ents = r["tags"]["SA"][:-1].split(";")
            assert sorted(ents) == sorted(entry(o) for o in rs if o is not r)
            if r is not primary[0]:
                assert ents[0] == entry(primary[0])
    for r in recs:
        if r["ref"] < 0:
            assert (r["pos"], r["flag"], r["cigar"], r["tags"]) == (-1, 4, [], {})
