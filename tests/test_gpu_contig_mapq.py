"""fsv_contig_mapq on the GPU (k_place, focalsv_amd/csrc/k_place.h) against tests/mapq_model.place: f1, f2, m, cutoff, thin, flags and
mapq of every record equal, on two chromosomes of under 600 kb with planted paralogs.  Records come from align_batch, two are hand-built."""
import numpy as np
import pytest

from focalsv_amd import _lib
from tests import mapq_model as MQ

pytestmark = pytest.mark.gpu
FIELDS = ("f1", "f2", "m", "cutoff", "thin", "flags")
COMP = bytes.maketrans(b"ACGT", b"TGCA")
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def rnd(rng, n):
    return rng.choice(ACGT, size=n).tobytes()


def revcomp(s):
    return s.translate(COMP)[::-1]


def mutate(rng, s, rate):
    """substitutions at `rate` of the positions"""
    a = np.frombuffer(s, dtype=np.uint8).copy()
    at = np.nonzero(rng.random(len(a)) < rate)[0]
    a[at] = ACGT[(np.searchsorted(ACGT, a[at]) + rng.integers(1, 4, len(at))) % 4]
    return a.tobytes()


class Scene:
    """a chromosome and the contigs cut from it: contig i belongs to the window [lo - 1000, hi + 1000) around its locus"""

    def __init__(self, chrom):
        self.chrom, self.names, self.contigs, self.refs, self.origin = chrom, [], [], [], []

    def add(self, name, contig, lo, hi, pad=1000):
        lo, hi = max(0, lo - pad), min(len(self.chrom), hi + pad)
        self.names.append(name)
        self.contigs.append(contig)
        self.refs.append(self.chrom[lo:hi])
        self.origin.append(lo)
        return len(self.contigs) - 1

    def hand_record(self, rec, cigar, name, ops, ref_start, q_start, q_end, rev=0):
        """a record of contig `name` appended to (rec, cigar); ref_start in the contig's window"""
        ci = self.names.index(name)
        r = np.zeros(1, dtype=_lib.ALN_REC_DTYPE)
        r["ref_start"], r["ref_end"] = ref_start, ref_start + sum(n for op, n in ops if op in (0, 2))
        r["q_start"], r["q_end"], r["n_cigar"], r["cigar_off"], r["contig"], r["rev"], r["mapq"] = q_start, q_end, len(ops), len(cigar), ci, rev, 60
        return np.concatenate([rec, r]), np.concatenate([cigar, np.array([n << 4 | op for op, n in ops], dtype=np.uint32)])

    def model(self, index, rec):
        return [MQ.place(index, self.contigs[int(r["contig"])], r, self.origin[int(r["contig"])]) for r in rec]

    def of(self, rec, name):
        return [i for i, r in enumerate(rec) if self.names[int(r["contig"])] == name]


def main_scene():
    rng = np.random.default_rng(2024)
    c = bytearray(rnd(rng, 480_000))
    S = None

    def paste(at, s):
        c[at:at + len(s)] = s
    loci = {"unique": (20_000, 30_000), "exact_same": (40_000, 50_000), "exact_rev": (60_000, 68_000), "div1": (80_000, 88_000), "div3": (90_000, 98_000),
            "div8": (100_000, 108_000), "div15": (110_000, 118_000), "copy_a": (130_000, 140_000), "del3k": (150_000, 162_000), "revrec": (260_000, 268_000)}
    seg = lambda name: bytes(c[loci[name][0]:loci[name][1]])
    paste(300_000, seg("exact_same"))
    paste(320_000, revcomp(seg("exact_rev")))
    for name, at, rate in (("div1", 340_000, 0.01), ("div3", 350_000, 0.03), ("div8", 360_000, 0.08), ("div15", 370_000, 0.15)):
        paste(at, mutate(rng, seg(name), rate))
    copy_b = mutate(rng, seg("copy_a"), 0.03)
    paste(380_000, copy_b)
    # a contig of two pieces 60 kb apart (a deletion beyond max_gap): only the second piece has a paralog
    a0 = 170_000
    paste(400_000, bytes(c[a0 + 70_000:a0 + 80_000]))
    S = Scene(bytes(c))
    for name in ("unique", "exact_same", "exact_rev", "div1", "div3", "div8", "div15"):
        S.add(name, seg(name), *loci[name])
    S.add("b_on_a", copy_b, *loci["copy_a"])                     # cut from copy B, aligned to copy A's window
    d = seg("del3k")
    S.add("del3k", d[:5000] + d[8000:], *loci["del3k"])
    S.add("split", S.chrom[a0:a0 + 10_000] + S.chrom[a0 + 70_000:a0 + 80_000], a0, a0 + 80_000)
    S.add("revrec", revcomp(seg("revrec")), *loci["revrec"])
    S.add("long60k", S.chrom[a0 + 5000:a0 + 65_000], a0 + 5000, a0 + 65_000)
    S.add("short", S.chrom[25_000:25_048], 25_000, 25_048)
    return S


def family_scene():
    """12 copies of a 20 kb unit, each 1 % off the master, 2 kb apart: the contig is copy 5"""
    rng = np.random.default_rng(77)
    master = rnd(rng, 20_000)
    parts, at, where = [rnd(rng, 3000)], 3000, []
    for i in range(12):
        parts.append(mutate(rng, master, 0.01))
        where.append(at)
        parts.append(rnd(rng, 2000))
        at += 22_000
    S = Scene(b"".join(parts))
    S.add("family", S.chrom[where[5]:where[5] + 20_000], where[5], where[5] + 20_000)
    return S


@pytest.fixture(scope="module")
def ctx():
    with _lib.Context(0) as c:
        yield c


class Run:
    """a scene aligned and placed once: records, what the library said of them three ways, and what the model says"""

    def __init__(self, ctx, S, hand=()):
        self.S = S
        self.index = MQ.Index(S.chrom)
        ctx.ref_index(S.chrom)
        cref = list(range(len(S.contigs)))
        rec, cigar, status = ctx.align_batch(S.contigs, cref, S.refs)
        assert (rec["mapq"] == 60).all()
        for name, ops, ref_start, q_start, q_end in hand:
            rec, cigar = S.hand_record(rec, cigar, name, ops, ref_start, q_start, q_end)
        self.rec_in, self.cigar, self.cref = rec, cigar, cref
        self.resident = ctx.contig_mapq(rec, cigar, S.origin, n_contigs=len(S.contigs))     # the contigs align_batch left on the device
        self.rec, self.out = ctx.contig_mapq(rec, cigar, S.origin, S.contigs, cref)
        self.again = ctx.contig_mapq(rec, cigar, S.origin, S.contigs, cref)
        self.want = S.model(self.index, rec)

    def rows(self, name):
        return self.S.of(self.rec, name)

    def got(self, i):
        return {**{f: int(self.out[f][i]) for f in FIELDS}, "mapq": int(self.rec["mapq"][i])}


@pytest.fixture(scope="module")
def main(ctx):
    S = main_scene()
    return Run(ctx, S, hand=[("long60k", [(0, 60_000)], 1000, 0, 60_000), ("short", [(0, 48)], 1000, 0, 48)])


@pytest.fixture(scope="module")
def family(ctx, main):       # (after main: one index per context)
    return Run(ctx, family_scene())


def test_every_record_equals_the_model(main):
    assert not main.out["rec_status"].any()
    assert len(main.rec) >= len(main.S.contigs)
    bad = [(main.S.names[int(main.rec["contig"][i])], main.got(i), main.want[i]) for i in range(len(main.rec)) if main.got(i) != main.want[i]]
    assert not bad, bad[:4]


def one(run, name):
    rows = run.rows(name)
    assert len(rows) == 1, (name, len(rows))
    return run.got(rows[0])


def test_unique_contig(main):
    g = one(main, "unique")
    assert g["f2"] == 0 and g["mapq"] == 60 and g["m"] > 500 and g["thin"] == 1 and g["flags"] == 0 and g["cutoff"] == 50


def test_exact_copies_elsewhere(main):
    for name in ("exact_same", "exact_rev"):
        g = one(main, name)
        assert g["f2"] >= g["f1"] > 0 and g["mapq"] == 0, (name, g)


def test_mapq_does_not_decrease_as_the_copy_diverges(main):
    q = [one(main, n)["mapq"] for n in ("exact_same", "div1", "div3", "div8", "div15")]
    assert q == sorted(q) and q[0] == 0 and q[-1] == 60, q
    assert 0 < one(main, "div1")["f2"] < one(main, "div1")["f1"]


def test_contig_of_the_other_copy(main):
    g = one(main, "b_on_a")
    assert g["f2"] > g["f1"] > 0 and g["mapq"] == 0


def test_deletion_inside_the_own_locus(main):
    g = one(main, "del3k")
    assert g["mapq"] == 60 and g["f2"] == 0


def test_fewer_than_ten_own_anchors(main):
    g = main.got(main.rows("short")[-1])      # the hand-built record
    assert 1 <= g["m"] < 10 and g["f2"] == 0
    assert g["mapq"] == MQ.mapq_of(g["f1"], 0, g["m"]) < MQ.mapq_of(g["f1"], 0, 10) == 60


def test_primary_keeps_60_and_the_supplementary_with_a_paralog_drops(main):
    rows = main.rows("split")
    assert len(rows) == 2
    by_q = sorted(rows, key=lambda i: int(main.rec["q_start"][i]))
    first, second = main.got(by_q[0]), main.got(by_q[1])
    assert first["mapq"] == 60 and first["f2"] == 0
    assert second["mapq"] == 0 and second["f2"] >= second["f1"]


def test_reverse_strand_record(main):
    rows = main.rows("revrec")
    assert len(rows) == 1 and int(main.rec["rev"][rows[0]]) == 1
    g = main.got(rows[0])
    assert g["mapq"] == 60 and g["f2"] == 0 and g["m"] > 400


def test_thinning_beyond_4096_seeds(main):
    i = main.rows("long60k")[-1]      # the hand-built record
    g = main.got(i)
    assert g["thin"] == 2 and g["mapq"] == 60 and 2000 < g["m"] < MQ.QMAX


def test_resident_contigs_and_a_second_call(main):
    for rec, out in (main.resident, main.again):
        assert rec.tobytes() == main.rec.tobytes()
        assert all(out[f].tobytes() == main.out[f].tobytes() for f in FIELDS + ("rec_status",))


def test_bad_cigar_fails_alone(ctx, main):
    rec, cigar = main.rec_in.copy(), main.cigar.copy()
    i = main.rows("div3")[0]
    cigar[int(rec["cigar_off"][i])] += 7 << 4          # the record's ops no longer sum to its contig
    j = main.rows("unique")[0]
    rec["ref_end"][j] = len(main.S.chrom)              # beyond the chromosome from this window
    got, out = ctx.contig_mapq(rec, cigar, main.S.origin, main.S.contigs, main.cref)
    assert out["rec_status"][i] == -2 and out["rec_status"][j] == -2 and got["mapq"][i] == 0 and got["mapq"][j] == 0
    others = [r for r in range(len(rec)) if r not in (i, j)]
    assert not out["rec_status"][others].any()
    assert got["mapq"][others].tolist() == main.rec["mapq"][others].tolist()
    assert all(out[f][others].tolist() == main.out[f][others].tolist() for f in FIELDS)
    with pytest.raises(_lib.FsvError) as e:            # the device-resident path needs the counts of the last align_batch
        ctx.contig_mapq(rec, cigar, main.S.origin[:-1], n_contigs=len(main.S.contigs) - 1)
    assert e.value.code == -2


def test_repeat_family_truncates_the_cutoff(family):
    assert not family.out["rec_status"].any()
    for i in range(len(family.rec)):
        assert family.got(i) == family.want[i]
    g = one(family, "family")
    assert g["cutoff"] < 50 and g["flags"] & _lib.MQ_TRUNC
    assert family.rec.tobytes() == family.again[0].tobytes() == family.resident[0].tobytes()
