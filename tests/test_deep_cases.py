"""The read sets of tests/deep_cases.py are what they are meant to be: the same bytes every time, sets the oracle alone corrects, and small
enough for the oracle to answer each in seconds.  These conditions say the cases are sane; they are not measurements."""
import pytest

from tests import deep_cases as D

CASES = [("locus", 1, None), ("locus", 3, None), ("locus", 3, D.N_JUNCTION_READS), ("tiling", 3, None), ("ont", 3, None), ("wide", 3, None),
         ("shallow11", 3, None), ("shallow12", 3, None)]


def test_every_builder_is_deterministic():
    for f, args in ((D.hifi_locus, ()), (D.hifi_locus, (D.N_JUNCTION_READS,)), (D.hifi_tiling, ()), (D.ont_locus, ()), (D.wide_counters, ()), (D.shallow, (11,))):
        a = f(*args)
        f.cache_clear()
        b = f(*args)
        assert a == b and a is not b, f.__name__
        truths, reads = a
        assert len(truths) == len(reads)


def test_half_of_the_reads_are_reverse_complemented():
    from focalsv_amd import synth
    truths, _ = D.hifi_locus()
    assert all(truths[i] == (synth.revcomp(truths[0]) if i & 1 else truths[0]) for i in range(len(truths)))


def test_the_oracle_alone_corrects_the_locus():
    truths, reads = D.hifi_locus()
    assert len(reads) == 48 and all(1400 < len(r) < 1600 for r in reads)
    for rounds in (1, 3):
        _, corrected, _ = D.oracle("locus", rounds)
        assert sum(c == t for c, t in zip(corrected, truths)) >= 44, rounds


def test_the_oracle_alone_corrects_the_read_with_the_deletion():
    truths, reads = D.wide_counters()
    assert len(reads) == 301 and reads[0] != truths[0] and len(reads[0]) == 799 and reads[1:] == truths[1:]
    _, corrected, _ = D.oracle("wide")
    assert corrected[0] == truths[0]


def test_the_tiling_gives_one_contig():
    contigs, _, _ = D.oracle("tiling")
    assert len(contigs) == 1 and abs(len(contigs[0]) - 9000) < 200


@pytest.mark.parametrize("case,rounds,n_reads", CASES)
def test_every_oracle_run_stays_under_ten_seconds(case, rounds, n_reads):
    assert D.oracle(case, rounds, n_reads)[2] < 10.0
