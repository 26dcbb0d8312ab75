"""The whole assembly with full_lists = 1 on noisy reads beyond the default caps: the ONT profile on reads of 36-48 kb (lists up to
~5 900 minimizers) and on a set with reads of 66-75 kb (the chain kernels' long layout) -- corrected reads and contigs equal the
oracle's, which has no cap, and the status carries no truncation bit; with the option off the same call is flagged FSV_W_MZ_TRUNC.  On
HiFi sets, where no list reaches a cap, the option changes nothing."""
import hashlib
import json
import os

import pytest

from focalsv_amd import _lib
from tests import long_list_cases as L
from tests import oracle_lib as O
from tests.test_gpu_asm import gpu_assemble

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    with _lib.Context(0) as c:
        yield c


def ont(ctx, full_lists):
    p = ctx.ont_asm_params()
    p.full_lists = full_lists
    return p


def check_against_oracle(ctx, reads, w_later=None):
    reads = list(reads)
    p, po = ont(ctx, 1), O.ont_params()
    if w_later is not None:
        p.w_later = po.w_later = w_later
    contigs, cset, status, got, b = gpu_assemble(ctx, [reads], p)
    assert int(status[0]) == 0, int(status[0])
    want_contigs, want_reads = O.assemble(reads, po)
    differ = [j for j in range(len(reads)) if got[j] != want_reads[j]]
    assert not differ, (differ, [(len(got[j]), len(want_reads[j])) for j in differ])
    assert [bytes(c) for c in contigs] == want_contigs, ([len(c) for c in contigs], [len(c) for c in want_contigs])
    return want_contigs


def test_reads_of_36_to_48_kb_equal_the_oracle(ctx):
    hap, reads = L.noisy_main_set()
    want = check_against_oracle(ctx, reads)
    assert len(want) == 1 and abs(len(want[0]) - len(hap)) < 200
    # the control: without the option the long reads' lists are cut and the set says so
    contigs, cset, status, got, b = gpu_assemble(ctx, [list(reads)], ont(ctx, 0))
    assert int(status[0]) & _lib.W_MZ_TRUNC


def test_long_lists_in_every_round_equal_the_oracle(ctx):
    """w_later = 0: the dense seeds stay for every round and the final pass, so the corrected reads' lists stay above 4 096, corrected
    pairs share more minimizers than a tile holds (k_chain_spill in the later rounds), and the final pass keeps the lists of the reads
    the last round left unchanged (k_uniq_long's only_changed skip on lists of its own class).  The set with the two reads of 66-75 kb:
    corrected, they share ~5 900 minimizers, more than the 4 096 tile of these rounds.  The kernels' own counters say that both took work"""
    check_against_oracle(ctx, L.noisy_long_set()[1], w_later=0)
    st = ctx.asm_stats()
    assert st["n_long_list_reads"] >= 4 and st["n_spilled_pairs"] >= 1, (st["n_long_list_reads"], st["n_spilled_pairs"])
    assert st["kernels"]["k_uniq_long"]["launches"] >= 1 and st["kernels"]["k_chain_spill"]["launches"] >= 1


def test_reads_of_66_kb_and_more_equal_the_oracle(ctx):
    hap, reads = L.noisy_long_set()
    assert max(len(r) for r in reads) >= 65536
    check_against_oracle(ctx, reads)


def test_hifi_sets_are_untouched_by_the_option(ctx):
    """two sets of tests/golden/hifiasm_contigs.json (their reads are synth.make_region's, checked by md5): no list reaches a cap, so
    neither new kernel may change a byte; and the result is still hifiasm's"""
    from focalsv_amd import synth
    from tests.test_gpu_asm import canon
    gold = [g for g in json.load(open(os.path.join(ROOT, "tests", "golden", "hifiasm_contigs.json")))["sets"] if g["region"] == 2][:2]
    assert len(gold) == 2
    sets = [synth.make_region(g["region"], width=g["width"], depth_per_hap=g["depth"]).reads[g["hap"] - 1] for g in gold]
    for s, g in zip(sets, gold):
        assert hashlib.md5(b"\n".join(s)).hexdigest() == g["reads_md5"]
    p1 = ctx.default_asm_params()
    p1.full_lists = 1
    c0, s0, st0, r0, _ = gpu_assemble(ctx, sets, ctx.default_asm_params())
    c1, s1, st1, r1, _ = gpu_assemble(ctx, sets, p1)
    st = ctx.asm_stats()
    assert st["n_long_list_reads"] == 0 and st["n_spilled_pairs"] == 0
    assert r0 == r1 and [bytes(c) for c in c0] == [bytes(c) for c in c1] and list(s0) == list(s1) and list(st0) == list(st1)
    for si, g in enumerate(gold):
        got = sorted((len(c), hashlib.md5(canon(c)).hexdigest()) for c, cs in zip(c1, s1) if cs == si)
        assert got == sorted((c["len"], c["md5"]) for c in g["contigs"])
