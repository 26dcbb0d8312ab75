"""dippav_variant_call(..., chrom_mapq=True) end to end: a contig of a unique region keeps its call and TIG_MAPQ=60; a contig of one copy of a
25 kb duplication, 0.5 % off the other copy, gets the model's mapping quality -- below 50 -- in signature/chr*_cigar.txt and in the contig
BAM, and loses its call as it does behind minimap2 in the reference pipeline.  With the option off every file is what it is today.

The divergence is chosen with the model on the CPU: at 25 kb ln f1 is 10.1, so 40 (1 - f2 / f1) ln f1 falls below 50 only while f2 / f1 stays
above 0.876.  With substitutions at 1 % of the positions the model gives f2 / f1 = 0.853 ... 0.876 and mapq 50, 52, 56, 58 over four random
draws (59 and 60 with every 100th base changed): at or above the threshold.  At 0.5 % it gives f1 = 24 972, f2 = 23 659, mapq 21."""
import os

import numpy as np
import pytest

from focalsv_amd import _lib, bam as B, fasta
from focalsv_amd.dippav import variant_call as VC
from tests import mapq_model as MQ
from tests.test_gpu_contig_mapq import mutate, rnd

pytestmark = pytest.mark.gpu

CHR_LEN = 400_000
A, B_LOCUS, B_COPY, DUP = 50_000, 150_000, 300_000, 25_000


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = tmp_path_factory.mktemp("chrom_mapq")
    rng = np.random.default_rng(5)
    chrom = bytearray(rnd(rng, CHR_LEN))
    chrom[B_COPY:B_COPY + DUP] = mutate(rng, bytes(chrom[B_LOCUS:B_LOCUS + DUP]), 0.005)
    chrom = bytes(chrom)
    a = chrom[A:A + 16_000]
    b = chrom[B_LOCUS:B_LOCUS + DUP]
    contigs = [("Region_chr21_S%d_E%d" % (A, A + 16_000), a[:8000] + a[8300:]),                    # a 300 bp deletion at A + 8000
               ("Region_chr21_S%d_E%d" % (B_LOCUS, B_LOCUS + DUP), b[:12_000] + rnd(rng, 300) + b[12_000:])]   # a 300 bp insertion at B + 12000
    paths = []
    for h in (1, 2):                                            # both haplotypes carry both contigs
        paths.append(str(d / ("in_hp%d.fa" % h)))
        with open(paths[-1], "w") as f:
            for name, seq in contigs:
                f.write(">" + name + "\n" + fasta.fold(seq.decode()) + "\n")
    ref_fa = str(d / "ref.fa")
    with open(ref_fa, "w") as f:
        f.write(">chr21\n" + fasta.fold(chrom.decode(), 60) + "\n")
    captured, real = [], VC.records_from_alignment

    def spy(*a, **kw):
        captured.append(real(*a, **kw))
        return captured[-1]
    VC.records_from_alignment = spy
    try:
        with _lib.Context(0) as ctx:
            for sub, kw in (("off", {}), ("on", {"chrom_mapq": True}), ("on_bam", {"chrom_mapq": True, "contig_bam": True})):
                VC.dippav_variant_call("CCS", None, ref_fa, paths[0], paths[1], str(d / sub), 21, read_records=[], ctx=ctx, **kw)
            with pytest.raises(_lib.FsvError):                  # the call drops its index: the context is left as it found it
                ctx.ref_index_stats()
    finally:
        VC.records_from_alignment = real
    # what the model says of the records the calls were made from
    index = MQ.Index(chrom)
    seqs = {"contig_hp%d_%d" % (h, k): contigs[k][1] for h in (1, 2) for k in (0, 1)}
    want = {}
    for r in captured[1]:
        assert len([x for x in captured[1] if x.qname == r.qname]) == 1 and not r.is_reverse
        L = len(seqs[r.qname])
        clip = lambda op: op[1] if op[0] == 4 else 0
        rec = {"q_start": clip(r.cigar[0]), "q_end": L - clip(r.cigar[-1]), "ref_start": r.pos, "ref_end": r.reference_end, "rev": 0}
        want[r.qname] = MQ.place(index, seqs[r.qname], rec, 0)["mapq"]
    return {"dir": {s: str(d / s) for s in ("off", "on", "on_bam")}, "records": captured, "want": want}


def vcf_body(root):
    return [ln for ln in open(os.path.join(root, "dippav_variant_chr21.vcf")) if not ln.startswith("#")]


def cigar_txt(root):
    return {f[0]: int(f[1]) for f in (ln.split("\t") for ln in open(os.path.join(root, "signature", "chr21_cigar.txt")))}


def calls_near(body, pos, svtype):
    return [ln for ln in body if abs(int(ln.split("\t")[1]) - pos) < 50 and "SVTYPE=" + svtype in ln]


def test_the_model_puts_the_duplicated_contig_below_50(case):
    assert case["want"]["contig_hp1_0"] == case["want"]["contig_hp2_0"] == 60
    assert 0 < case["want"]["contig_hp1_1"] < 50 and case["want"]["contig_hp2_1"] == case["want"]["contig_hp1_1"]


def test_option_off_calls_both_with_60(case):
    body = vcf_body(case["dir"]["off"])
    for pos, svtype in ((A + 8000, "DEL"), (B_LOCUS + 12_000, "INS")):
        hit = calls_near(body, pos, svtype)
        assert len(hit) == 1 and "TIG_MAPQ=60" in hit[0] and "SVLEN=300" in hit[0].replace("SVLEN=-", "SVLEN="), (pos, body)
    assert set(cigar_txt(case["dir"]["off"]).values()) == {60}
    assert all(r.mapq == 60 for r in case["records"][0])


def test_option_on_keeps_the_unique_call_and_drops_the_duplicated_one(case):
    body = vcf_body(case["dir"]["on"])
    hit = calls_near(body, A + 8000, "DEL")
    assert len(hit) == 1 and "TIG_MAPQ=60" in hit[0]
    assert hit == calls_near(vcf_body(case["dir"]["off"]), A + 8000, "DEL")
    assert calls_near(body, B_LOCUS + 12_000, "INS") == [] and len(body) == 1
    assert cigar_txt(case["dir"]["on"]) == case["want"]
    assert {r.qname: r.mapq for r in case["records"][1]} == case["want"]


def test_contig_bam_shows_the_value(case):
    assert vcf_body(case["dir"]["on_bam"]) == vcf_body(case["dir"]["on"])
    with B.BamFile(os.path.join(case["dir"]["on_bam"], "assemblies.sorted.bam")) as bam:
        got = bam.fetch(until_eof=True)
        assert {got.names[k]: int(got.mapq[k]) for k in range(len(got))} == case["want"]
