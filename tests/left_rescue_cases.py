"""The smallest read sets on which the left-extension pass (k_left_rescue: recalcate_window_advance's left pass, Correct.cpp:2745-2905)
decides a corrected read: hap 1 of five synthetic regions at width 8 000 and 4x per haplotype -- 8 to 12 reads, at most 40 kb a set.
On each of them the oracle's round-1 reads with left_rescue = 0 differ from those with left_rescue = 1 (tests/test_left_rescue_cases.py
asserts exactly that, without a GPU), so a verdict or a retry written wrongly in the rescue kernels shows in the result
(tests/test_gpu_left_rescue.py)."""
from functools import lru_cache

from focalsv_amd import synth
from tests import oracle_lib as O

REGIONS = (69, 78, 114, 183, 280)


@lru_cache(maxsize=None)
def read_set(region):
    return tuple(synth.make_region(region, width=8000, depth_per_hap=4).reads[0])


@lru_cache(maxsize=None)
def ordinary_sets():
    """two sets no rescue pass decides anything on, to stand beside the five in a batch"""
    r = synth.make_region(2, width=16000, depth_per_hap=10.0)
    return tuple(r.reads[0]), tuple(r.reads[1])


@lru_cache(maxsize=None)
def oracle(reads, rounds, partial_charge=0, left_rescue=1):
    """(contigs, corrected reads) of oracle/asm.c, computed once per (set, parameters)"""
    p = O.default_params()
    p.n_rounds, p.partial_charge, p.left_rescue = rounds, partial_charge, left_rescue
    contigs, corrected = O.assemble(list(reads), p)
    return tuple(contigs), tuple(corrected)
