"""The verdict kernels between K5 and the consensus (k_rescue_accept, k_left_rescue, and with partial_charge = 1 their DEFER forms and the
charge kernels) at their smallest: the five sets of tests/left_rescue_cases.py, on which the left-extension pass decides a read.
Corrected reads after 1 and 3 rounds and the contigs against oracle/asm.c, each set alone, all five in one batch in both orders between
two ordinary sets, and with the partial charge on."""
import pytest

from focalsv_amd import _lib
from focalsv_amd.readsets import pack_sets
from tests import left_rescue_cases as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with _lib.Context(0) as c:
        yield c


def check(ctx, sets, rounds, partial_charge=0):
    """one fsv_assemble_batch call over `sets`: every set's corrected reads and contigs equal the oracle's"""
    p = ctx.default_asm_params()
    p.n_rounds, p.partial_charge = rounds, partial_charge
    b = pack_sets([list(s) for s in sets])
    d = ctx.upload(b.words)
    try:
        contigs, cset, cnr, status = ctx.assemble_batch(d, b.word_off, b.read_len, b.set_start, p, None)
        reads = ctx.fetch_reads(b.n_reads, int(b.read_len.sum()) * 2 + 1024)
    finally:
        ctx.dev_free(d)
    k = 0
    for si, s in enumerate(sets):
        want_contigs, want_reads = L.oracle(s, rounds, partial_charge)
        bad = [j for j in range(len(s)) if reads[k + j] != want_reads[j]]
        assert not bad, (rounds, partial_charge, si, bad)
        k += len(s)
        mine = [c for c, cs in zip(contigs, cset) if cs == si]
        assert mine == list(want_contigs), (rounds, partial_charge, si, [len(c) for c in mine], [len(c) for c in want_contigs])


@pytest.mark.parametrize("region", L.REGIONS)
def test_each_set_alone(ctx, region):
    for rounds in (1, 3):
        check(ctx, [L.read_set(region)], rounds)


@pytest.mark.parametrize("order", ["forward", "backward"])
def test_five_sets_in_one_batch_between_ordinary_sets(ctx, order):
    first, last = L.ordinary_sets()
    five = [L.read_set(r) for r in (L.REGIONS if order == "forward" else L.REGIONS[::-1])]
    for rounds in (1, 3):
        check(ctx, [first] + five + [last], rounds)


def test_with_the_partial_charge(ctx):
    """the DEFER instantiations of the rescue kernels, k_charge_tasks and k_charge_accept, against the oracle's partial_charge = 1"""
    first, last = L.ordinary_sets()
    for rounds in (1, 3):
        check(ctx, [first] + [L.read_set(r) for r in L.REGIONS] + [last], rounds, partial_charge=1)
