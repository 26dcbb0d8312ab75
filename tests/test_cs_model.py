"""tests/cs_model.py pinned on hand-written answers (each token kind, the N rule) and on its own arithmetic: the columns and bases
its tokens stand for must add up to the CIGAR's M / I / D totals and to NM.  Host only."""
import random
import re

import pytest

from .cs_model import D, H, I, M, S, cs_nm, revcomp

KNOWN = [
    # (cigar, query, ref, ref_start, nm, cs)
    ([(M, 8)], "ACGTACGT", "ACGTACGT", 0, 0, ":8"),
    ([(M, 8)], "ACGTACGT", "ACGAACGT", 0, 1, ":3*at:4"),
    ([(M, 4)], "TCGA", "ACGT", 0, 2, "*at:2*ta"),                                     # first and last column
    ([(M, 4)], "AGTA", "ACGA", 0, 2, ":1*cg*gt:1"),                                   # two adjacent
    ([(M, 3), (I, 2), (M, 3)], "ACGTTACG", "ACGACG", 0, 2, ":3+tt:3"),
    ([(M, 3), (D, 2), (M, 3)], "ACGACG", "ACGTTACG", 0, 2, ":3-tt:3"),
    ([(M, 2), (I, 1), (D, 2), (M, 2)], "ACGTT", "ACCCTT", 0, 3, ":2+g-cc:2"),         # I directly followed by D
    ([(S, 2), (M, 4), (S, 3)], "GGACGTCCC", "TTACGTTT", 2, 0, ":4"),                  # clips are not represented; ref_start
    ([(H, 2), (I, 1), (M, 3)], "GGAACG", "ACG", 0, 1, "+a:3"),                        # an indel as the first op after a clip
    ([(M, 3), (M, 2)], "ACGTA", "ACGTA", 0, 0, ":3:2"),                               # a run ends with its M op
    ([(M, 5)], "ACGTA", "ACNTA", 0, 1, ":2*ng:2"),                                    # a reference N pairs with nothing
    ([(M, 3)], "ANG", "ANG", 0, 1, ":1*nn:1"),                                        # ... not even with an N
    ([(M, 4)], "ACGT", "acgt", 0, 0, ":4"),                                           # case does not matter
    ([(M, 2), (D, 3), (M, 2)], "ACGT", "ACNRYGT", 0, 3, ":2-nnn:2"),                  # deleted N (any other letter is one)
    ([(M, 12)], "ACGTACGTACGT", "ACGTACGTACGT", 0, 0, ":12"),
]


@pytest.mark.parametrize("case", KNOWN, ids=[c[5] for c in KNOWN])
def test_known_answers(case):
    cigar, q, r, rs, nm, cs = case
    assert cs_nm(cigar, q, r, rs) == (nm, cs)


def test_reverse_strand_is_the_oriented_contig():
    contig, ref = "AAACGT", "ACGTTT"          # its reverse complement ACGTTT matches the window
    assert cs_nm([(M, 6)], revcomp(contig), ref) == (0, ":6")
    assert revcomp("ACGTNacgtn") == "nacgtNACGT"


TOKEN = re.compile(r":(\d+)|\*([acgtn])([acgtn])|\+([acgtn]+)|-([acgtn]+)")


def totals_of(cs):
    """(M columns, inserted bases, deleted bases, nm) the tokens of a cs string stand for; the string must be tokens end to end"""
    m = i = d = nm = 0
    at = 0
    for t in TOKEN.finditer(cs):
        assert t.start() == at, cs
        at = t.end()
        if t.group(1) is not None:
            assert t.group(1)[0] != "0"
            m += int(t.group(1))
        elif t.group(2) is not None:
            m, nm = m + 1, nm + 1
        elif t.group(4) is not None:
            i, nm = i + len(t.group(4)), nm + len(t.group(4))
        else:
            d, nm = d + len(t.group(5)), nm + len(t.group(5))
    assert at == len(cs), cs
    return m, i, d, nm


def test_token_arithmetic_reproduces_the_cigar():
    rng = random.Random(5)
    for _ in range(200):
        cigar, q, r = [], [], []
        if rng.random() < 0.5:
            n = rng.randint(1, 9); cigar.append((rng.choice((S, H)), n)); q += rng.choices("ACGT", k=n)
        for _ in range(rng.randint(1, 12)):
            op, n = rng.choice((M, M, I, D)), rng.randint(1, 40)
            cigar.append((op, n))
            if op == M:
                seg = rng.choices("ACGT", k=n)
                q += seg
                r += [c if rng.random() > 0.1 else rng.choice("ACGTN") for c in seg]
            elif op == I:
                q += rng.choices("ACGT", k=n)
            else:
                r += rng.choices("ACGTN", k=n)
        lead = rng.randint(0, 5)
        nm, cs = cs_nm(cigar, "".join(q), "T" * lead + "".join(r), lead)
        want = tuple(sum(n for op, n in cigar if op == o) for o in (M, I, D))
        m, i, d, nm_tok = totals_of(cs)
        assert (m, i, d) == want and nm_tok == nm
