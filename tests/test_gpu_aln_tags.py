"""fsv_aln_tags on the GPU (k_aln_tags, focalsv_amd/csrc/k_aln.h) against tests/cs_model.py: NM and the cs bytes equal, on sequences
that are mutated copies with the CIGAR known by construction."""
import ctypes as C
import random

import numpy as np
import pytest

from focalsv_amd import _lib
from .cs_model import D, H, I, M, S, cs_nm, revcomp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with _lib.Context(0) as c:
        yield c


def rnd(rng, n):
    return "".join(rng.choices("ACGT", k=n))


def other(rng, c):
    return rng.choice([x for x in "ACGT" if x != c.upper()])


def pair(rng, ops, ref_start=0, mism=(), tail=7):
    """(query, window) for a CIGAR: M columns are copies but for the columns listed in mism (counted over all M columns of the record),
    I / S / H bases exist in the query only, D bases in the window only; the window has ref_start bases in front and `tail` behind"""
    q, r, col = [], [rnd(rng, ref_start)], 0
    mism = set(mism)
    for op, n in ops:
        if op == M:
            seg = rnd(rng, n)
            r.append(seg)
            q.append("".join(other(rng, c) if col + k in mism else c for k, c in enumerate(seg)) if mism else seg)
            col += n
        elif op == D:
            r.append(rnd(rng, n))
        else:
            q.append(rnd(rng, n))
    return "".join(q), "".join(r) + rnd(rng, tail)


class Batch:
    """contigs with their windows and records -> the arrays fsv_aln_tags takes, and what the model says of every record"""

    def __init__(self):
        self.contigs, self.cref, self.refs, self.rec, self.cigar, self.want = [], [], [], [], [], []

    def add(self, contig, ref, records, ref_index=None):
        """records: [(ops, ref_start, rev)] of this contig; contig: its text as the caller holds it (the forward strand)"""
        if ref_index is None:
            ref_index = len(self.refs)
            self.refs.append(ref)
        ci = len(self.contigs)
        self.contigs.append(contig)
        self.cref.append(ref_index)
        for ops, rs, rev in records:
            self.rec.append((rs, rs + sum(n for op, n in ops if op in (M, D)), 0, 0, len(ops), 0, len(self.cigar), ci, rev, 60, (0, 0)))
            self.cigar += [n << 4 | op for op, n in ops]
            self.want.append(cs_nm(ops, revcomp(contig) if rev else contig, self.refs[ref_index], rs))
        return ref_index

    def arrays(self):
        return np.array(self.rec, dtype=_lib.ALN_REC_DTYPE), np.array(self.cigar, dtype=np.uint32)

    def run(self, ctx):
        rec, cigar = self.arrays()
        return ctx.aln_tags(rec, cigar, [c.encode() for c in self.contigs], self.cref, [r.encode() for r in self.refs])

    def check(self, ctx):
        nm, cs, status, ms = self.run(ctx)
        assert not status.any()
        bad = [k for k in range(len(self.want)) if (int(nm[k]), cs[k].decode()) != self.want[k]]
        assert not bad, (len(bad), bad[:5], [(int(nm[k]), cs[k][:80], self.want[k][0], self.want[k][1][:80]) for k in bad[:2]])
        return nm, cs


def test_m_run_lengths_at_every_word_misalignment(ctx):
    rng = random.Random(1)
    b = Batch()
    for n in (1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025):
        for qs in range(18):
            for rs in range(18):
                ops = [(S, qs)] * (qs > 0) + [(M, n)]
                q, r = pair(rng, ops, rs, mism=rng.sample(range(n), rng.choice([0, 1, 2])) if n > 1 else ([0] if rng.random() < 0.3 else []))
                b.add(q, r, [(ops, rs, 0)])
    b.check(ctx)


def test_mismatch_positions(ctx):
    rng = random.Random(2)
    b = Batch()
    for mism in ([0], [199], [0, 199], [15], [16], [15, 16], [63], [64], [63, 64], [127, 128], [30, 31], range(100, 170), range(0, 200), [5, 64, 65, 66, 130]):
        for rs in (0, 3):
            q, r = pair(rng, [(M, 200)], rs, mism=mism)
            b.add(q, r, [([(M, 200)], rs, 0)])
    b.check(ctx)


def test_digit_count_edges(ctx):
    rng = random.Random(3)
    runs = (9, 10, 99, 100, 999, 1000, 9999, 10000, 99999, 100000)
    mism, at = [], 0
    for n in runs[:-1]:
        at += n
        mism.append(at)
        at += 1
    total = at + runs[-1]
    q, r = pair(rng, [(M, total)], 5, mism=mism)
    b = Batch()
    b.add(q, r, [([(M, total)], 5, 0)])
    _, cs = b.check(ctx)
    assert [int(t.split("*")[0]) for t in cs[0].decode().split(":")[1:]] == list(runs)


def test_indels(ctx):
    rng = random.Random(4)
    b = Batch()
    for n in (1, 16, 17, 64, 65, 300):
        for op in (I, D):
            for ops in ([(M, 40), (op, n), (M, 33)], [(M, 16), (op, n), (M, 64)]):
                q, r = pair(rng, ops, 2, mism=[3, 45])
                b.add(q, r, [(ops, 2, 0)])
    for ops in ([(M, 20), (I, 5), (D, 7), (M, 20)], [(M, 20), (D, 70), (I, 66), (M, 20)], [(S, 9), (I, 4), (M, 30)], [(S, 9), (D, 4), (M, 30)],
                [(H, 3), (I, 65), (M, 30), (D, 2), (S, 4)], [(M, 10), (I, 3), (I, 4), (M, 10), (M, 7), (D, 1), (D, 2), (M, 3)]):
        q, r = pair(rng, ops, 11, mism=[1])
        b.add(q, r, [(ops, 11, 0)])
    b.check(ctx)


def test_strands_and_clips(ctx):
    rng = random.Random(5)
    b = Batch()
    for ops in ([(S, 5), (M, 90)], [(M, 90), (S, 6)], [(S, 17), (M, 90), (S, 31)], [(H, 5), (M, 90), (H, 6)], [(H, 2), (S, 3), (M, 70), (I, 2), (M, 9), (S, 1), (H, 1)]):
        for rev in (0, 1):
            q, r = pair(rng, ops, 4, mism=[0, 40, 69])
            b.add(revcomp(q) if rev else q, r, [(ops, 4, rev)])      # the caller holds the forward strand; rev = 1 reads its reverse complement
    # three records of one contig: two parts on the forward strand, the piece between them on the other
    A, Bm, Cc = rnd(rng, 300), rnd(rng, 130), rnd(rng, 250)
    window = "GG" + A + revcomp(Bm) + Cc + "TT"
    contig = A[:100] + other(rng, A[100]) + A[101:] + Bm + Cc
    b.add(contig, window, [([(M, 300), (S, 380)], 2, 0), ([(S, 430), (M, 250)], 2 + 430, 0), ([(S, 250), (M, 130), (S, 300)], 2 + 300, 1)])
    nm, _ = b.check(ctx)
    assert list(nm[-3:]) == [1, 0, 0]


def test_reference_n_and_case(ctx):
    rng = random.Random(6)
    b = Batch()
    for n_at in ([50], range(10, 41), range(60, 70), [0, 15, 16, 31, 32, 119]):
        q, r = pair(rng, [(M, 120)], 3, mism=[70])
        r = "".join("N" if k - 3 in set(n_at) else c for k, c in enumerate(r))
        b.add(q, r, [([(M, 120)], 3, 0)])
    ops = [(M, 30), (D, 20), (M, 30), (I, 3), (M, 10)]
    q, r = pair(rng, ops, 0, mism=[2])
    r = r[:35] + "NNNNNRYK" + r[43:]                      # N (and other IUPAC letters) inside a deletion
    b.add(q, r, [(ops, 0, 0)])
    q, r = pair(rng, [(M, 100)], 6, mism=[10, 11])
    b.add(q, r.lower(), [([(M, 100)], 6, 0)])            # lower-case reference
    q, r = pair(rng, [(M, 100)], 0)
    b.add(q[:40] + "N" + q[41:], r[:40].lower() + r[40:], [([(M, 100)], 0, 0)])      # an N in the contig pairs with nothing either
    nm, cs = b.check(ctx)
    assert b"*n" in cs[0] and nm[0] == 2
    nn = Batch()                                          # a batch without any N: the kernels drop the mask
    q, r = pair(rng, [(M, 100)], 1, mism=[7])
    nn.add(q, r, [([(M, 100)], 1, 0)])
    nn.check(ctx)


def test_batch_shapes(ctx):
    rng = random.Random(7)
    one = Batch()
    q, r = pair(rng, [(M, 50)], 0, mism=[9])
    one.add(q, r, [([(M, 50)], 0, 0)])
    one.check(ctx)
    many = Batch()                                        # 200 short records on one window (and 200 is no multiple of 64 or 256)
    window = rnd(rng, 4000)
    for k in range(200):
        a, n = rng.randrange(0, 3500), rng.randrange(20, 400)
        seg = list(window[a:a + n])
        for p in rng.sample(range(n), 2):
            seg[p] = other(rng, seg[p])
        ri = many.add("".join(seg), window, [([(M, n)], a, 0)], ref_index=0 if k else None)
        assert ri == 0
    many.check(ctx)
    mixed = Batch()                                       # a long record (cut into several tasks) among short ones
    ops = [(S, 13), (M, 20000), (I, 5000), (M, 20000), (D, 8000), (M, 25000), (S, 8)]
    for k in range(3):
        q, r = pair(rng, [(M, 300)], k, mism=[k])
        mixed.add(q, r, [([(M, 300)], k, 0)])
    q, r = pair(rng, ops, 77, mism=[0, 32768, 64999])
    assert len(q) > 70000
    mixed.add(q, r, [(ops, 77, 0)])
    mixed.add(revcomp(q), r, [(ops, 77, 1)])
    for k in range(3):
        q, r = pair(rng, [(M, 300)], k, mism=[299])
        mixed.add(q, r, [([(M, 300)], k, 0)])
    nm, _ = mixed.check(ctx)
    assert nm[3] == 3 + 5000 + 8000


def raw_tags(ctx, b, cs_cap, rec=None, cigar=None):
    """one fsv_aln_tags call with explicit sequences -> (return code, cs_bytes, nm, cs_off, cs buffer or None, rec_status)"""
    if rec is None:
        rec, cigar = b.arrays()
    n = len(rec)
    rseq, roff = _lib.join_refs([r.encode() for r in b.refs])
    coff = np.zeros(len(b.contigs) + 1, dtype=np.uint64)
    np.cumsum([len(c) for c in b.contigs], out=coff[1:])
    cseq = np.frombuffer("".join(b.contigs).encode() + b"\0", dtype=np.uint8)
    cref = np.asarray(b.cref, dtype=np.uint32)
    alns = _lib.Alns(rec.ctypes.data, n, n, cigar.ctypes.data, len(cigar), len(cigar), None)
    nm, off, st = np.full(n, 77, np.int32), np.zeros(n + 1, np.uint64), np.full(n, 77, np.int32)
    cs = None if cs_cap is None else np.zeros(max(1, cs_cap), np.uint8)
    out = _lib.AlnTags(nm.ctypes.data, off.ctypes.data, None if cs is None else cs.ctypes.data, 0 if cs is None else cs_cap, 0, st.ctypes.data, 0.0)
    rc = ctx._lib.fsv_aln_tags(ctx._h, cseq.ctypes.data, coff.ctypes.data, len(b.contigs), cref.ctypes.data, rseq.ctypes.data, roff.ctypes.data,
                               len(b.refs), C.byref(alns), C.byref(out))
    return rc, int(out.cs_bytes), nm, off, cs, st


def small_batch(seed, n):
    rng = random.Random(seed)
    b = Batch()
    for k in range(n):
        ops = [(S, k)] * (k > 0) + [(M, 80 + k), (I, 2), (M, 40), (D, 3), (M, 9)]
        q, r = pair(rng, ops, k, mism=[5, 100])
        b.add(q, r, [(ops, k, 0)])
    return b


def test_context_reuse_and_capacity(ctx):
    small_batch(8, 40).check(ctx)
    b = small_batch(9, 7)                                 # a second, smaller call on the same context
    b.check(ctx)
    total = sum(len(w[1]) for w in b.want)
    rc, need, nm, off, _, st = raw_tags(ctx, b, None)     # the count-only call
    assert rc == 0 and need == total and list(nm) == [w[0] for w in b.want] and not st.any()
    assert list(np.diff(off.astype(np.int64))) == [len(w[1]) for w in b.want]
    rc, need, _, _, _, _ = raw_tags(ctx, b, total - 1)
    assert rc == _lib.ECAP and need == total
    rc, need, nm, off, cs, _ = raw_tags(ctx, b, total)
    assert rc == 0 and need == total and cs.tobytes().decode() == "".join(w[1] for w in b.want)


def test_bad_records_fail_alone(ctx):
    b = small_batch(10, 6)
    rec, cigar = b.arrays()
    cigar = cigar.copy()
    cigar[int(rec[1]["cigar_off"])] += 1 << 4             # record 1: its query length is off by one
    rec[4]["ref_start"] += 10                             # record 4: ref_end no longer ref_start + its reference bases
    end = len(b.refs[2]) + 1                              # record 2: consistent in itself, but it ends beyond its window
    rec[2]["ref_start"], rec[2]["ref_end"] = end - (b.rec[2][1] - b.rec[2][0]), end
    rc, need, nm, off, cs, st = raw_tags(ctx, b, 1 << 16, rec, cigar)
    assert rc == 0
    assert list(st) == [0, _lib.EINVAL, _lib.EINVAL, 0, _lib.EINVAL, 0]
    for k in range(6):
        got = cs[int(off[k]):int(off[k + 1])].tobytes().decode()
        assert (int(nm[k]), got) == ((-1, "") if st[k] else b.want[k]), k


def test_unsupported_op(ctx):
    b = small_batch(11, 3)
    for op in (3, 6, 7, 8):
        rec, cigar = b.arrays()
        cigar[int(rec[1]["cigar_off"]) + 2] = 5 << 4 | op
        rc = raw_tags(ctx, b, 1 << 16, rec, cigar)[0]
        assert rc == _lib.EUNSUP, op


def random_pair(rng, n, rate):
    """a window of n bases and a copy with substitutions and short indels at `rate` per base -> (ops, query, window)"""
    ref = rnd(rng, n)
    q, ops = [], []

    def push(op, k=1):
        if ops and ops[-1][0] == op:
            ops[-1] = (op, ops[-1][1] + k)
        else:
            ops.append((op, k))
    i = 0
    while i < n:
        x = rng.random()
        if x < rate / 3:
            k = min(rng.randrange(1, 6), n - i); push(D, k); i += k
        elif x < 2 * rate / 3:
            k = rng.randrange(1, 6); q.append(rnd(rng, k)); push(I, k)
        else:
            q.append(other(rng, ref[i]) if x < rate else ref[i]); push(M); i += 1
    return ops, "".join(q), ref


def test_random_pairs(ctx):
    rng = random.Random(12)
    b = Batch()
    for k in range(300):
        ops, q, r = random_pair(rng, rng.randrange(1, 2001), 10 ** rng.uniform(-3, -1))
        if not q:
            continue
        rev = k % 3 == 0
        b.add(revcomp(q) if rev else q, r, [(ops, 0, int(rev))])
    assert len(b.contigs) >= 295
    b.check(ctx)


def test_hand_off_from_align_batch(ctx):
    rng = random.Random(13)
    window = rnd(rng, 9000)
    body = window[1000:8000]
    contigs = [body, body[:3000] + rnd(rng, 200) + body[3000:], body[:4000] + body[4150:], revcomp(body[:2500] + other(rng, body[2500]) + body[2501:])]
    for k in range(4):
        seg = list(body[200 * k: 6000 + 100 * k])
        for p in rng.sample(range(len(seg)), 5):
            seg[p] = other(rng, seg[p])
        contigs.append("".join(seg))
    enc, refs = [c.encode() for c in contigs], [window.encode(), rnd(rng, 500).encode()]
    rec, cigar, status = ctx.align_batch(enc, [0] * 8, refs)
    assert not status.any() and len(rec) == 8 and rec[3]["rev"] == 1
    with pytest.raises(_lib.FsvError) as e:
        ctx.aln_tags(rec, cigar, n_contigs=7, n_refs=2)
    assert e.value.code == _lib.EINVAL
    with pytest.raises(_lib.FsvError) as e:
        ctx.aln_tags(rec, cigar, n_contigs=8, n_refs=1)
    assert e.value.code == _lib.EINVAL
    nm0, cs0, st0, _ = ctx.aln_tags(rec, cigar, n_contigs=8, n_refs=2)          # the sequences the aligner left on the device
    nm1, cs1, st1, _ = ctx.aln_tags(rec, cigar, enc, [0] * 8, refs)
    assert list(nm0) == list(nm1) and cs0 == cs1 and not st0.any() and not st1.any()
    for k, r in enumerate(rec):
        ops = [(int(c) & 0xf, int(c) >> 4) for c in cigar[int(r["cigar_off"]): int(r["cigar_off"]) + int(r["n_cigar"])]]
        c = contigs[int(r["contig"])]
        assert (int(nm0[k]), cs0[k].decode()) == cs_nm(ops, revcomp(c) if r["rev"] else c, window, int(r["ref_start"]))
    assert b"+" in cs0[1] and b"-" in cs0[2] and nm0[1] == 200 and nm0[2] == 150
    with pytest.raises(_lib.FsvError) as e:                                     # an explicit call replaced the aligner's sequences
        ctx.aln_tags(rec, cigar, n_contigs=8, n_refs=2)
    assert e.value.code == _lib.EINVAL
