"""tests/left_rescue_cases.py without a GPU: the five sets are as small as promised and the left-extension pass decides a read on each."""
import pytest

from tests import left_rescue_cases as L


@pytest.mark.parametrize("region", L.REGIONS)
def test_left_pass_changes_a_round1_read(region):
    reads = L.read_set(region)
    assert 8 <= len(reads) <= 12 and sum(len(r) for r in reads) <= 40000, (len(reads), sum(len(r) for r in reads))
    _, on = L.oracle(reads, 1, left_rescue=1)
    _, off = L.oracle(reads, 1, left_rescue=0)
    changed = [j for j in range(len(reads)) if on[j] != off[j]]
    print("region", region, len(reads), "reads,", sum(len(r) for r in reads), "bases; reads the left pass changes:", changed)
    assert changed, "the synthetic generator drifted: the left-extension pass no longer decides a read of this set"
