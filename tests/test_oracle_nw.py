"""oracle/aln.c:orc_nw on tests/nw_cases.py against two things it shares no code with: its CIGAR re-scored (cigar_score) gives its
score, and its score is the optimum of a plain score-only DP under the piecewise gap cost (plain_score).  The GPU kernels are
compared with orc_nw bit for bit (tests/test_gpu_nw.py), so this is what stands behind that comparison."""
import pytest

from tests import nw_cases as N
from tests import oracle_lib as O


@pytest.mark.parametrize("cls", (0, 1, 2, 3))
def test_oracle_score_is_its_cigars_and_the_optimum(cls):
    cs = N.by_class()[cls]
    assert len(cs) >= 20
    for name, t, q, params in cs:
        sc, cg = O.nw(t, q, N.set_params(O.aln_default_params(), params))
        assert N.cigar_score(t, q, cg, params) == sc, (name, len(t), len(q), sc)
        assert N.plain_score(t, q, params) == sc, (name, len(t), len(q), sc)


def test_cap_cases_sit_on_both_sides_of_the_cap():
    """the named cap cases: exactly ALN_CG_CAP runs, and more (1027 for the class-2 pair, whatever the merges leave for class 1)"""
    by_name = {c[0]: c for c in N.cases()}
    for name, want in N.CAP_RUNS.items():
        _, t, q, params = by_name[name]
        sc, cg = O.nw(t, q, N.set_params(O.aln_default_params(), params))
        assert len(cg) == want if want is not None else len(cg) > N.CG_CAP, (name, len(cg))
    assert sorted(v for v in N.CAP_RUNS.values() if v is not None) == [N.CG_CAP, N.CG_CAP, 1027]


def test_every_class_has_its_cases_and_parameter_sets():
    counts = N.check_floors()
    assert sum(counts.values()) == len(N.cases()) and min(counts.values()) >= 20
    for name, t, q, params in N.cases():
        assert len(t) * len(q) <= N.MAX_CELLS and params in N.PARAM_SETS and set(q) <= set(b"ACGT"), name


def test_nw_class_mirror_at_its_boundaries():
    assert [N.nw_class(ql, tl) for ql, tl in ((256, 99999), (257, 256), (257, 257), (3072, 257), (3073, 257), (3073, 256), (99999, 1))] == [0, 3, 1, 1, 2, 3, 3]


def test_plain_score_and_cigar_score_by_hand():
    """small pairs worked out by hand, so that the two checkers are pinned to something too"""
    # three matches; one mismatch; a target N costs 1 whatever it faces
    assert N.plain_score(b"ACG", b"ACG", N.ASM5) == 3 and N.plain_score(b"ACG", b"ATG", N.SINGLE) == 2 + 2 - 4
    assert N.plain_score(b"ANG", b"ACG", N.ASM5) == 1 and N.cigar_score(b"ANG", b"ACG", [3 << 4], N.ASM5) == 1
    # a gap of 100 under asm5 takes the second piece: 81 + 100, not 39 + 300; of 10 the first: 39 + 30
    t = b"ACGTTGCA" * 4
    assert N.plain_score(t, t[:16] + b"G" * 100 + t[16:], N.ASM5) == 32 - 181
    assert N.plain_score(t[:16] + b"C" * 10 + t[16:], t, N.ASM5) == 32 - 69
    assert N.gap_cost(21, N.ASM5) == 102 and N.gap_cost(22, N.ASM5) == 103 and N.gap_cost(100, N.SINGLE) == 204
    assert N.cigar_score(t, t[:16] + b"G" * 100 + t[16:], [16 << 4, 100 << 4 | 1, 16 << 4], N.ASM5) == 32 - 181
    # boundaries: a one-base target against 50 query bases is a match and two gaps, or a match at one end and one gap
    assert N.plain_score(b"A", b"C" * 49 + b"A", N.ASM5) == 1 - (81 + 49)
    with pytest.raises(AssertionError):
        N.cigar_score(b"ACG", b"ACG", [2 << 4], N.ASM5)


def test_tie_order_by_hand():
    """Two sequences with no base in common align as one insertion and one deletion, and either order scores the same: the last
    cell sees E (E2) and F (F2) tie, the deletion wins (diagonal > E > F > E2 > F2), so the walk from the end takes the target
    first and the CIGAR reads insertion, then deletion.  Every other check here is blind to a tie taken the other way."""
    p = N.set_params(O.aln_default_params(), N.ASM5)
    sc, cg = O.nw(b"A" * 100, b"C" * 100, p)
    assert (sc, O.cigar_str(cg)) == (-2 * 181, "100I100D")
    sc, cg = O.nw(b"A" * 10, b"C" * 10, p)                 # the first gap piece: 39 + 30 below 81 + 10
    assert (sc, O.cigar_str(cg)) == (-2 * 69, "10I10D")
    p = N.set_params(O.aln_default_params(), (1, 19, 39, 3, -1, -1))
    sc, cg = O.nw(b"A" * 10, b"C" * 10, p)
    assert (sc, O.cigar_str(cg)) == (-2 * 69, "10I10D")
