"""Contig / reference-window pairs with SVs the aligner used to refuse or miscall: duplication-type
INS / DEL of 6-30 kb (both copies fall between two unique seeds: an event of more than max_cells cells), a dispersed repeat,
a tandem array of short units, a replacement, inversions.  Shared by the oracle tests (CPU) and the -m gpu tests."""
import numpy as np

from focalsv_amd import synth

_A = np.frombuffer(b"ACGT", dtype=np.uint8)


def rnd(rng, n):
    return _A[rng.integers(0, 4, n)].tobytes()


def mutate(rng, s, rate):
    b = bytearray(s)
    for i in np.nonzero(rng.random(len(b)) < rate)[0]:
        b[i] = b"ACGT"[(b"ACGT".index(b[i]) + 1 + int(rng.integers(0, 3))) % 4]
    return bytes(b)


def left_del(ref, pos, n):
    """leftmost position of the deletion ref[pos : pos + n]"""
    while pos > 0 and ref[pos - 1] == ref[pos + n - 1]:
        pos -= 1
    return pos


def left_ins(hap, hpos, n, rpos):
    """leftmost reference position of the insertion hap[hpos : hpos + n] that sits in front of reference base rpos"""
    while hpos > 0 and hap[hpos - 1] == hap[hpos + n - 1]:
        hpos -= 1
        rpos -= 1
    return rpos


def events(rec):
    """(type, ref pos, length) of the I / D runs of at least 30 bases of one record (dict with ref_start and cigar [(op, len)])"""
    pos, out = rec["ref_start"], []
    for op, n in rec["cigar"]:
        if op == 0:
            pos += n
        elif op == 2:
            if n >= 30:
                out.append(("DEL", pos, n))
            pos += n
        elif op == 1 and n >= 30:
            out.append(("INS", pos, n))
    return out


class Case:
    def __init__(self, name, ref, hap, truth, n_rec=1, strands=None):
        self.name, self.ref, self.hap, self.truth, self.n_rec, self.strands = name, ref, hap, truth, n_rec, strands


def _with_small_del(L):
    """a 120 bp deletion at 5 000 in the left flank: the other SV of the contig that must still be called"""
    return L[:5000] + L[5120:]


def duplication_cases(sizes=(6000, 8000, 12000, 30000), divs=(0.0, 0.02)):
    out = []
    for size in sizes:
        for div in divs:
            rng = np.random.default_rng(size + int(div * 1000))
            L, R, C = rnd(rng, 12000), rnd(rng, 12000), rnd(rng, size)
            C2 = mutate(rng, C, div)
            small = ("DEL", left_del(L, 5000, 120), 120)
            # tandem duplication as an insertion: the second copy is new
            ref, hap = L + C + R, _with_small_del(L) + C + C2 + R
            at = len(L) - 120 + size
            out.append(Case("dup-INS-%d-%g" % (size, div), ref, hap, [small, ("INS", left_ins(hap, at, size, len(L) + size), size)]))
            # and the matching deletion: the reference has both copies
            ref, hap = L + C + C2 + R, _with_small_del(L) + C + R
            out.append(Case("dup-DEL-%d-%g" % (size, div), ref, hap, [small, ("DEL", left_del(ref, len(L) + size, size), size)]))
    return out


def other_cases():
    out = []
    rng = np.random.default_rng(77)
    # a dispersed two-copy repeat of 12 kb (2 % diverged) with variation inside the first copy: SNPs every 700 bases and a 300 bp
    # deletion -- the copy has no unique seeds, so its 12 k x 12 k box used to be refused
    L, M, R, C = rnd(rng, 9000), rnd(rng, 7000), rnd(rng, 9000), rnd(rng, 12000)
    C2 = mutate(rng, C, 0.02)
    ref = L + C + M + C2 + R
    hc = bytearray(C)
    for i in range(350, len(hc), 700):
        hc[i] = b"ACGT"[(b"ACGT".index(hc[i]) + 1) % 4]
    hc = bytes(hc)
    hap = _with_small_del(L) + hc[:6000] + hc[6300:] + M + C2 + R
    out.append(Case("dispersed-repeat", ref, hap, [("DEL", left_del(L, 5000, 120), 120), ("DEL", left_del(ref, len(L) + 6000, 300), 300)]))
    # a dispersed duplication: a second copy of C inserted 7 kb downstream
    ref = L + C[:8000] + M + R
    hap = _with_small_del(L) + C[:8000] + M + C[:8000] + R
    at = len(L) - 120 + 8000 + len(M)
    out.append(Case("dispersed-dup-INS", ref, hap, [("DEL", left_del(L, 5000, 120), 120), ("INS", left_ins(hap, at, 8000, len(L) + 8000 + len(M)), 8000)]))
    # a tandem array of 50-base units, 130 copies against 260: nothing in it can be seeded, the box is closed from its corners
    unit = rnd(rng, 50)
    ref = L + unit * 130 + R
    hap = _with_small_del(L) + unit * 260 + R
    out.append(Case("array-INS", ref, hap, [("DEL", left_del(L, 5000, 120), 120), ("INS", left_ins(hap, len(L) - 120 + 6500, 6500, len(L) + 6500), 6500)]))
    # 8 kb replaced by 10 kb of unrelated sequence
    X, Y = rnd(rng, 8000), rnd(rng, 10000)
    ref = L + X + R
    hap = _with_small_del(L) + Y + R
    out.append(Case("replacement", ref, hap, [("DEL", left_del(L, 5000, 120), 120), ("INS", len(L), 10000), ("DEL", len(L), 8000)]))
    return out


def inversion_cases(sizes=(2000, 5000)):
    out = []
    for size in sizes:
        for rc in (0, 1):
            rng = np.random.default_rng(size)
            L, M, R = rnd(rng, 12000), rnd(rng, size), rnd(rng, 15000)
            ref = L + M + R
            hap = _with_small_del(L) + synth.revcomp(M) + R
            if rc:
                hap = synth.revcomp(hap)
            out.append(Case("inversion-%d-%s" % (size, "-+"[1 - rc]), ref, hap, [("DEL", left_del(L, 5000, 120), 120)], n_rec=3,
                            strands=[rc, rc, 1 - rc]))
    return out


def n_window_cases():
    """reference windows that hold runs of N (they used to be stored -- and to seed and match -- as poly-A).
    The contig carries real sequence where the reference has N; minimap2 scores an N against anything as -1 and skips k-mers with
    an N: the alignment runs through a short run as 'M', nothing is called there, and the contig's real SVs still are."""
    out = []
    rng = np.random.default_rng(4242)
    L, M, R = rnd(rng, 12000), rnd(rng, 9000), rnd(rng, 12000)
    small = ("DEL", left_del(L, 5000, 120), 120)
    hap = _with_small_del(L) + M + R
    for name, runs in (("N-run-3", [(3000, 3)]), ("N-run-200", [(3000, 200)]), ("N-run-1500", [(3000, 1500)]),
                       ("N-runs-many", [(500, 1), (1200, 40), (4000, 300), (7000, 17)])):
        m = bytearray(M)
        for at, n in runs:
            m[at:at + n] = b"N" * n
        out.append(Case(name, L + bytes(m) + R, hap, [small]))
    # an N run of 60 next to a real 400 bp deletion (30 bases apart) and one inside a 500 bp insertion's flank
    m = bytearray(M)
    m[2970:3030 - 30] = b"N" * 30
    ref = L + bytes(m) + R
    hap2 = _with_small_del(L) + M[:3100] + M[3500:] + R
    out.append(Case("N-run-beside-DEL", ref, hap2, [small, ("DEL", left_del(L + M + R, len(L) + 3100, 400), 400)]))
    ins = rnd(rng, 500)
    m = bytearray(M)
    m[5050:5090] = b"N" * 40
    ref = L + bytes(m) + R
    hap3 = _with_small_del(L) + M[:5000] + ins + M[5000:] + R
    out.append(Case("N-run-beside-INS", ref, hap3, [small, ("INS", left_ins(hap3, len(L) - 120 + 5000, 500, len(L) + 5000), 500)]))
    # a window that starts and ends in N, and poly-A in the contig opposite an N run (what "N stored as A" made an exact match)
    m = bytearray(M)
    m[3000:3300] = b"N" * 300
    hm = bytearray(M)
    hm[3000:3300] = b"A" * 300
    out.append(Case("N-run-vs-polyA", b"N" * 700 + L[700:] + bytes(m) + R[:-900] + b"N" * 900, _with_small_del(L) + bytes(hm) + R, [small]))
    return out


def cigar_head_cases():
    """nine contigs of one 6 kb reference, contig n (1 ... 9) without the n single bases at 3000, 3010, ..., 3000 + 10 (n - 1).  No
    19-mer fits between two deletions, so they share one DP event of 2n - 1 ... 2n + 1 runs (the padding M at either end): in one
    batch the events fall on both sides of the 8 runs per event that the host reads back in its one strided copy"""
    ref = rnd(np.random.default_rng(11), 6000)
    out = []
    for n in range(1, 10):
        cut = [3000 + 10 * i for i in range(n)]
        hap = b"".join(ref[a + 1:b] for a, b in zip([-1] + cut, cut + [len(ref)]))
        out.append(Case("single-DEL-x%d" % n, ref, hap, [], n_rec=1))
    return out


# the planted blocks of dp_class_cases as (reference bases, contig bases): what each event's DP covers at the least
DP_CLASS_BLOCKS = ((100, 0), (1000, 1200), (5000, 600), (3300, 3500), (0, 2000))


def _unlike(rng, n, x):
    """n random bases to replace the block x with nothing to pair at the junctions.  The alignment is the new bases as an insertion,
    then x as a deletion; a first or last base like x's, or a tail that is a head of x, would pair there for free and shorten both."""
    while True:
        y = rnd(rng, n)
        if y[0] != x[0] and y[-1] != x[-1] and not any(y[-k:] == x[:k] for k in range(1, 33)):
            return y


def dp_class_cases():
    """one contig, forward and reverse-complemented, whose five events between unique flanks of 6-8 kb take the four kernels of the
    event DP (aln.hip: nw_class) in one batch: a 100-base deletion (class 0: a short query), 1 000 reference bases replaced by 1 200
    unrelated ones (class 1), 5 000 replaced by 600 (class 1 with more than 4 096 target bases: its ring wraps), 3 300 replaced by
    3 500 (class 2: a query above 3 072, about 12 M cells, below max_cells) and a 2 000-base insertion (class 3: a short target
    side).  A replacement comes out as an insertion next to a deletion; the new bases are drawn so that nothing pairs at its junctions, so
    both have the planted lengths."""
    rng = np.random.default_rng(49)
    F = [rnd(rng, n) for n in (6000, 7000, 8000, 6500, 7500, 6700)]
    X = [rnd(rng, n) for n, _ in DP_CLASS_BLOCKS[:4]]
    Y = [b""] + [_unlike(rng, m, x) for (_, m), x in zip(DP_CLASS_BLOCKS[1:4], X[1:])]
    ins = rnd(rng, DP_CLASS_BLOCKS[4][1])
    ref = F[0] + X[0] + F[1] + X[1] + F[2] + X[2] + F[3] + X[3] + F[4] + F[5]
    hap = F[0] + F[1] + Y[1] + F[2] + Y[2] + F[3] + Y[3] + F[4] + ins + F[5]
    truth, rpos, hpos = [], 0, 0
    for k in range(4):
        rpos += len(F[k])
        hpos += len(F[k])
        if Y[k]:
            truth.append(("INS", left_ins(hap, hpos, len(Y[k]), rpos), len(Y[k])))
        # a deletion behind its insertion has no M run in front to move through: it stays at the block's first base
        truth.append(("DEL", rpos if Y[k] else left_del(ref, rpos, len(X[k])), len(X[k])))
        rpos += len(X[k])
        hpos += len(Y[k])
    rpos += len(F[4])
    hpos += len(F[4])
    truth.append(("INS", left_ins(hap, hpos, len(ins), rpos), len(ins)))
    return [Case("dp-classes-+", ref, hap, truth, strands=[0]), Case("dp-classes--", ref, synth.revcomp(hap), truth, strands=[1])]


# ---- small boxes: the oversize-event path (k_extract_boxes, k_chain_aln<true>, k_aln_events<true>, k_corner) at a few hundred bases
SMALL_BOX_MAX_CELLS = 1 << 16   # 256 x 256 cells: an event of 300 bases a side is oversize, the 400-base insertion found inside a re-seeded
                                # box (about 470 x 70 cells with its padding) still goes to the DP
CORNER_RUNS = (0, 1, 63, 64, 65, 127, 128, 129)


def _array(unit, n):
    """n bases of a tandem array of a 7-base unit: identical on both sides, so a corner's gap-free run crosses it, and nothing in it
    seeds -- each of its k-mers occurs every 7 bases, more often than a seed may at either depth"""
    return (unit * (n // len(unit) + 1))[:n]


class BoxCase(Case):
    """kind 'seeded': the box has anchors of its own, the planted gap comes out of the DP (truth as in Case); kind 'corner': nothing
    in it seeds, it is closed from its corners: an insertion run next to a deletion run"""
    def __init__(self, name, ref, hap, truth, kind, strands):
        Case.__init__(self, name, ref, hap, truth, strands=strands)
        self.kind = kind


def small_box_cases():
    """contigs of 3.3-3.9 kb, each forward and reverse-complemented, with one event that exceeds SMALL_BOX_MAX_CELLS between unique
    flanks of 1 500 bases:
      a tandem duplication of a 400-base unit as an insertion and as a deletion: the box seeds again (minimizers that occur twice);
      300 bases replaced by 330 unrelated ones: nothing seeds, the box is closed from its corners; the same with a reference N ten
      bases in front of the fill -- no seed covers the N, so it lies inside the left corner's run;
      such fills behind a shared head, in front of a shared tail, or both, of CORNER_RUNS bases of a tandem array: the corner runs
      cross them, in steps of 64 positions"""
    out = []

    def both_strands(name, ref, hap, truth, kind):
        out.append(BoxCase(name + "-+", ref, hap, truth, kind, [0]))
        out.append(BoxCase(name + "--", ref, synth.revcomp(hap), truth, kind, [1]))

    rng = np.random.default_rng(2025)
    L, R, C = rnd(rng, 1500), rnd(rng, 1500), rnd(rng, 400)
    ref, hap = L + C + R, L + C + C + R
    both_strands("box-dup-INS", ref, hap, [("INS", left_ins(hap, len(L) + 400, 400, len(L) + 400), 400)], "seeded")
    ref, hap = L + C + C + R, L + C + R
    both_strands("box-dup-DEL", ref, hap, [("DEL", left_del(ref, len(L) + 400, 400), 400)], "seeded")
    X = rnd(rng, 300)
    Y = _unlike(rng, 330, X)
    both_strands("box-unrelated", L + X + R, L + Y + R, None, "corner")
    both_strands("box-unrelated-N", L[:-10] + b"N" + L[-9:] + X + R, L + Y + R, None, "corner")
    unit = b"ACCTGAT"
    for n in CORNER_RUNS:
        for name, head, tail in (("head", n, 0), ("tail", 0, n), ("both", n, n)):
            rng = np.random.default_rng(7000 + n)
            L, R, X = rnd(rng, 1500), rnd(rng, 1500), rnd(rng, 300)
            Y = _unlike(rng, 330, X)
            H, T = _array(unit, head), _array(unit, tail)
            both_strands("box-corner-%s-%d" % (name, n), L + H + X + T + R, L + H + Y + T + R, None, "corner")
    return out


def small_box_params(p):
    p.max_cells = SMALL_BOX_MAX_CELLS
    return p


_small_box_oracle = []


def small_box_oracle():
    """the cases and the oracle's records of each, computed once per process"""
    if not _small_box_oracle:
        from tests import oracle_lib as O
        cases = small_box_cases()
        po = small_box_params(O.aln_default_params())
        _small_box_oracle.append((cases, [O.align_contig_multi(c.hap, c.ref, po) for c in cases]))
    return _small_box_oracle[0]


def check_box_case(case, recs):
    """what the oracle (or the GPU) must make of a small box case: one record on the planted strand that covers the contig; 'seeded':
    the planted gap with its length, left-aligned, and nothing else; 'corner': exactly one insertion run next to one deletion run,
    both of at least the lengths that the two fills differ by construction, and no other gap"""
    assert len(recs) == 1 and [r["rev"] for r in recs] == case.strands, (case.name, len(recs))
    cg = recs[0]["cigar"]
    assert sum(n for op, n in cg if op in (0, 1, 4)) == len(case.hap), case.name
    if case.kind == "seeded":
        check_case(case, recs)
        return
    gaps = [(i, op, n) for i, (op, n) in enumerate(cg) if op in (1, 2)]
    assert len(gaps) == 2 and gaps[1][0] == gaps[0][0] + 1 and (gaps[0][1], gaps[1][1]) == (1, 2), (case.name, cg)     # I, then D
    ins, dele = gaps[0][2], gaps[1][2]
    assert ins - dele == 30 and dele >= 200, (case.name, cg)


def check_case(case, recs):
    """recs: the records of the contig (dicts with ref_start, rev, cigar): every planted SV within 1 bp with its exact length,
    nothing else; the expected number of records and their strands"""
    assert len(recs) == case.n_rec, (case.name, len(recs))
    if case.strands is not None:
        assert [r["rev"] for r in recs] == case.strands, (case.name, [r["rev"] for r in recs])
    ev = [e for r in recs for e in events(r)]
    miss = [t for t in case.truth if not any(k == t[0] and n == t[2] and abs(p - t[1]) <= 1 for k, p, n in ev)]
    assert not miss and len(ev) == len(case.truth), (case.name, ev, case.truth)
    for r in recs:
        assert sum(n for op, n in r["cigar"] if op in (0, 1, 4)) == len(case.hap), case.name


def split_calls(recs):
    """what DipPAV's split rule makes of consecutive records (sorted by position, as in the BAM)"""
    from focalsv_amd.dippav import signatures as S
    segs = [S.AlignedSegment("chr21", r["ref_start"], r["ref_end"], r["cigar"], "contig_hp1_0", bool(r["rev"]), 60, None) for r in recs]
    segs.sort(key=lambda x: x.pos)
    out = []
    for a, b in zip(segs, segs[1:]):
        d, i = S.extract_sig_from_split(a, b)
        out += d + i
    return out


def mixed_window_cases(sizes, seed=31):
    """reference groups of very different lengths for ONE fsv_align_batch call: the seed window of a group is max(w, L / 3000 + 1),
    L = its longest sequence, so groups of 30 kb, 150 kb and 400 kb are sketched with w = 19, 51 and 134 in one launch.  Per group
    three contigs, none longer than the window (the oracle takes L per pair): the window with a deletion and an insertion, forward;
    an inner part with a deletion, reverse strand; an inner part with an insertion, forward.  -> (refs, [(Case, group)])"""
    rng = np.random.default_rng(seed)
    refs, out = [], []
    for gi, L in enumerate(sizes):
        ref = rnd(rng, L)
        refs.append(ref)
        a, b = L // 3, 2 * L // 3
        ins = rnd(rng, 200)
        hap = ref[:a] + ref[a + 500:b] + ins + ref[b:]
        out.append((Case("mixed-%d-both" % L, ref, hap, [("DEL", left_del(ref, a, 500), 500), ("INS", left_ins(hap, b - 500, 200, b), 200)]), gi))
        lo, hi, c = 2000, L - 1000, L // 2
        hap = ref[lo:c] + ref[c + 1000:hi]
        out.append((Case("mixed-%d-del-rev" % L, ref, synth.revcomp(hap), [("DEL", left_del(ref, c, 1000), 1000)], strands=[1]), gi))
        lo, hi, c = L // 4, 3 * L // 4, L // 2 + 77
        ins = rnd(rng, 400)
        hap = ref[lo:c] + ins + ref[c:hi]
        out.append((Case("mixed-%d-ins" % L, ref, hap, [("INS", left_ins(hap, c - lo, 400, c), 400)]), gi))
    return refs, out
