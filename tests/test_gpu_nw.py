"""fsv_nw on tests/nw_cases.py: every size class of run_nw on its boundaries and past its ring wraps, four scoring sets, ties,
reference N, both sides of the CIGAR cap -- score and CIGAR bit-identical to oracle/aln.c:orc_nw, which tests/test_oracle_nw.py
holds against a plain DP on the same list."""
import pytest

from focalsv_amd import _lib
from tests import nw_cases as N
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with _lib.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def oracle():
    """name -> (score, CIGAR words) of orc_nw, once for the module"""
    return {name: O.nw(t, q, N.set_params(O.aln_default_params(), params)) for name, t, q, params in N.cases()}


def _over_cap(name):
    return name in N.CAP_RUNS and N.CAP_RUNS[name] != N.CG_CAP


def _same_as_oracle(ctx, oracle, case):
    name, t, q, params = case
    sc, cg = ctx.nw(t, q, N.set_params(ctx.default_aln_params(), params))
    osc, ocg = oracle[name]
    what = (name, N.nw_class(len(q), len(t)), len(q), len(t))
    assert sc == osc, what + (sc, osc)
    if list(cg) != list(ocg):
        at = next((i for i, (x, y) in enumerate(zip(cg, ocg)) if x != y), min(len(cg), len(ocg)))
        assert False, what + ("first differing run", at, O.cigar_str(cg[at:at + 4]), O.cigar_str(ocg[at:at + 4]), len(cg), len(ocg))
    assert N.cigar_score(t, q, cg, params) == sc, what


@pytest.mark.parametrize("cls", (0, 1, 2, 3))
def test_class_matches_oracle(ctx, oracle, cls):
    cs = [c for c in N.by_class()[cls] if not _over_cap(c[0])]
    assert len(cs) >= 20 and {c[3] for c in cs} == set(N.PARAM_SETS)
    for case in cs:
        _same_as_oracle(ctx, oracle, case)


def test_cigar_cap_is_an_error_return(ctx, oracle):
    """exactly ALN_CG_CAP runs come back, all of them; one run more is FSV_ECAP -- an ordinary error: the next call on the same
    context gives the oracle's answer again.  A class-2 and a class-1 pair on either side."""
    by_name = {c[0]: c for c in N.cases()}
    small = by_name["grid-q65-t257"]
    for name, want in N.CAP_RUNS.items():
        case = by_name[name]
        if want == N.CG_CAP:
            assert len(oracle[name][1]) == N.CG_CAP
            _same_as_oracle(ctx, oracle, case)
        else:
            assert len(oracle[name][1]) > N.CG_CAP
            with pytest.raises(_lib.FsvError) as e:
                ctx.nw(case[1], case[2], N.set_params(ctx.default_aln_params(), case[3]))
            assert e.value.code == _lib.ECAP
        _same_as_oracle(ctx, oracle, small)


def test_every_class_has_its_cases_and_parameter_sets(oracle):
    counts = N.check_floors()
    assert min(counts.values()) >= 20 and len(oracle) == len(N.cases()) == sum(counts.values())
