"""The model of the chromosome-level mapping quality (tests/mapq_model.py) on hand answers, and fsv_mapq_of (host only, no device)
against it.  No GPU."""
import random

import pytest

from focalsv_amd import _lib
from tests import mapq_model as MQ

HAND = [((1000, 0, 20), 60), ((1000, 900, 20), 27), ((1000, 880, 20), 33), ((1000, 900, 5), 13), ((30, 0, 3), 40), ((1000, 1000, 20), 0),
        ((1000, 1200, 20), 0), ((0, 0, 0), 0)]


@pytest.mark.parametrize("args,want", HAND)
def test_mapq_of_hand_answers(args, want):
    assert MQ.mapq_of(*args) == want
    assert _lib.mapq_of(*args) == want


def test_library_mapq_of_equals_model_on_a_grid():
    f1s = sorted({0, 1, 2, 3, 7, 19, 20, 38, 57, 100, 199, 200, 201, 1000, 4999, 12345, 99999, 10 ** 6} | {int(1.9 ** e) for e in range(1, 22)})
    bad = []
    for f1 in f1s:
        f2s = {0, 1, f1 // 10, f1 // 3, f1 // 2, (f1 * 7) // 8, (f1 * 9) // 10, (f1 * 99) // 100, f1 - 1, f1, f1 + 1}
        for f2 in sorted(x for x in f2s if x >= 0):
            for m in range(0, 13):
                if _lib.mapq_of(f1, f2, m) != MQ.mapq_of(f1, f2, m):
                    bad.append((f1, f2, m))
    assert not bad, bad[:10]
    assert _lib.mapq_of(-5, 0, 3) == 0 and _lib.mapq_of(100, 0, -1) == 0


# ---- classes, c*, the reference-major DP on hand-built hits: (count, relative strand, chromosome position, contig coordinate)
def colinear(c, rel, p0, q0, n, step=100):
    return [(c, rel, p0 + i * step, q0 + i * step) for i in range(n)]


def test_class_split():
    hits = colinear(1, 0, 10_000, 50, 20) + colinear(2, 0, 300_000, 50, 8) + colinear(2, 1, 200_000, 50, 5) + [(1, 1, 10_500, 700)]
    cut, (own, fwd, rev) = MQ.classify(hits, rev=0, own_lo=10_000, own_hi=13_000, max_occ=50)
    assert cut == 50
    assert len(own) == 20 and len(fwd) == 8 and len(rev) == 6      # a hit of the other strand inside the own interval is elsewhere
    f1, f2, m = MQ.score((own, fwd, rev))
    assert (f1, m) == (20 * 19, 20) and f2 == 8 * 19
    # the same hits seen by a rev = 1 record over the reverse-strand locus
    cut, (own, fwd, rev) = MQ.classify(hits, rev=1, own_lo=200_000, own_hi=200_500, max_occ=50)
    assert len(own) == 5 and len(fwd) == 28 and len(rev) == 1


def test_cutoff_is_the_largest_count_every_class_can_hold():
    base = colinear(1, 0, 1000, 0, 100)
    many = [(7, 0, 500_000 + i, i) for i in range(MQ.AMAX - 10)]      # elsewhere forward: fits with the count-1 and count-3 hits of its class
    more = [(9, 0, 900_000 + i, i) for i in range(20)]                # ... and overflows with these
    few = [(3, 0, 400_000 + i, i) for i in range(10)] + [(12, 1, 100 + i, i) for i in range(5)]
    cut, classes = MQ.classify(base + many + more + few, 0, 1000, 20_000, 50)
    assert cut == 8
    assert len(classes[0]) == 100 and len(classes[1]) == MQ.AMAX and len(classes[2]) == 0      # count 12 is above c* in every class
    cut, _ = MQ.classify(base + few, 0, 1000, 20_000, 50)
    assert cut == 50
    # c* never falls below 1
    cut, _ = MQ.classify([(1, 0, 500_000 + i, i) for i in range(MQ.AMAX + 5)], 0, 0, 10, 50)
    assert cut == 1


def test_two_loci_interleaved_in_contig_order_score_each_on_its_own():
    """two copies of a 30-seed stretch elsewhere on the chromosome: in contig order their hits alternate, and beyond 64 seeds a contig-major
    DP with a look-back of 64 sees only a few of its own locus; reference-major each locus is one run"""
    n = 200
    a = [(2, 0, 100_000 + 100 * i, 100 * i) for i in range(n)]
    b = [(2, 0, 300_000 + 100 * i, 100 * i) for i in range(n)]
    hits = [h for pair in zip(a, b) for h in pair]
    cut, classes = MQ.classify(hits, 0, 0, 10, 50)
    anchors = classes[1]
    assert anchors == sorted(anchors) and anchors[:n] == [(p, q) for _, _, p, q in a]
    f, pre, best = MQ.chain_dp(anchors)
    assert f[best] == n * 19 and best == n - 1                      # the first best end wins: locus a
    assert f[2 * n - 1] == n * 19 and pre[n] == -1                  # locus b starts a chain of its own
    # a 150 bp insertion inside a locus costs the gap penalty once
    g = [(p, q + (150 if i >= 100 else 0)) for i, (p, q) in enumerate(anchors[:n])]
    f, pre, best = MQ.chain_dp(g)
    assert f[best] == n * 19 - ((150 >> 7) + (7 >> 1) + 1)
    # ties: the nearer predecessor
    f, pre, best = MQ.chain_dp([(0, 0), (19, 19), (38, 38), (57, 57)])
    assert pre == [-1, 0, 1, 2] and f == [19, 38, 57, 76]


def test_tiling_reproduces_the_sketch_in_one_piece():
    rng = random.Random(11)
    seq = "".join(rng.choices("ACGT", k=200_000))
    seq = seq[:70_000] + "N" * 30 + seq[70_030:131_060] + "N" + seq[131_061:]      # an N run inside a tile, one N next to a tile boundary
    tiled, whole = MQ.Index(seq), MQ.Index(seq, tiled=False)
    assert tiled.stats["tiles"] == 4 and whole.stats["tiles"] == 4
    assert tiled.table == whole.table
    assert tiled.stats == whole.stats
    assert tiled.stats["dropped_n"] > 0


def test_n_substitute_matches_the_oracle():
    from tests import oracle_lib as O
    ref = "ACGT" * 20 + "N" * 40 + "".join(random.Random(3).choices("ACGT", k=300))
    text, mask = MQ.seed_text(ref)
    assert mask.sum() == 40 and text[:80] == ref[:80] and text[120:] == ref[120:]
    # oracle/aln.c seeds a window with an N through the same substitution: a contig equal to the substituted text aligns across the run as 'M'
    a = O.align_contig(text.encode(), ref.encode())
    assert a is not None and a["cigar"] == [(0, len(ref))]
