"""fsv_asm_params.deep_sets = 1 on the read sets of tests/deep_cases.py: windows and junctions with more inserted-base events than the LDS
buffer holds (256; 2 048 with the wide-band profiles), and a column with more than 255 votes "after an insertion".  With the option the
corrected reads (fsv_assemble_batch + fsv_asm_fetch_reads) and the contigs equal O.assemble, which has no cap, and FSV_W_INS_EVENTS is
never raised; without it the same sets carry the bit, which pins that the input is beyond the cap without asking the code under test."""
import hashlib
import json
import os

import pytest

from focalsv_amd import _lib
from tests import deep_cases as D
from tests import oracle_lib as O
from tests.test_gpu_asm import gpu_assemble

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W_INS_EVENTS = 8


@pytest.fixture(scope="module")
def ctx():
    with _lib.Context(0) as c:
        yield c


def params(ctx, deep, profile="hifi", **kw):
    p = ctx.ont_asm_params() if profile == "ont" else ctx.default_asm_params()
    p.deep_sets = deep
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def check_against_oracle(ctx, case, p, n_rounds=3, n_reads=None, contigs_too=True):
    reads = list(D.reads_of(case, n_reads))
    contigs, cset, status, got, b = gpu_assemble(ctx, [reads], p)
    st = ctx.deep_windows()
    print(case, n_rounds, n_reads, "status", int(status[0]), st)
    assert not int(status[0]) & W_INS_EVENTS, int(status[0])
    want_contigs, want_reads, _ = D.oracle(case, n_rounds, n_reads)
    differ = [j for j in range(len(reads)) if got[j] != want_reads[j]]
    assert not differ, (differ, [(len(got[j]), len(want_reads[j])) for j in differ])
    if contigs_too:
        assert [bytes(c) for c in contigs] == want_contigs, ([len(c) for c in contigs], [len(c) for c in want_contigs])
    return st


@pytest.mark.parametrize("rounds", [1, 3])
def test_one_locus_hifi(ctx, rounds):
    """case 1: 48 reads x 1 500, 1.2 % indels"""
    reads = list(D.reads_of("locus"))
    _, _, status, _, _ = gpu_assemble(ctx, [reads], params(ctx, 0, n_rounds=rounds))
    assert int(status[0]) & W_INS_EVENTS, int(status[0])      # the input exceeds the cap
    assert ctx.deep_windows() == {"n_deep_windows": 0, "n_deep_junctions": 0, "max_events": 0}
    st = check_against_oracle(ctx, "locus", params(ctx, 1, n_rounds=rounds), rounds)
    assert st["n_deep_windows"] > 0 and st["max_events"] > 256, st
    assert ctx.asm_stats()["kernels"]["k_consensus_deep"]["launches"] >= 1


def test_junctions(ctx):
    """case 2: the locus at N_JUNCTION_READS = 120 reads with the second consensus pass (second_round = 1): junctions spill as well.  A
    junction's backbone is the first pass's result, so only the partners' own insertions are events there -- 375 x 0.6 % = 2.25 per overlap,
    not the 9 of a window, whose backbone is a raw read.  At 72 reads (the windows' fullest: 695 events, 198 listed) that is ~160 per junction
    and none is listed; at 120, the most the case may take, ~270"""
    p = params(ctx, 1, second_round=1)
    st = check_against_oracle(ctx, "locus", p, 3, D.N_JUNCTION_READS)
    assert st["n_deep_windows"] > 0 and st["n_deep_junctions"] > 0 and st["max_events"] > 256, st
    assert ctx.asm_stats()["kernels"]["k_bnd_consensus_deep"]["launches"] >= 1


def test_a_contig(ctx):
    """case 3: 150 reads x 3 000 tiling 9 kb"""
    st = check_against_oracle(ctx, "tiling", params(ctx, 1))
    assert st["n_deep_windows"] > 0 and st["max_events"] > 256, st
    assert len(D.oracle("tiling")[0]) == 1


def test_wide_band(ctx):
    """case 4: the ONT profile, 100 reads x 1 500 at 10 % error: beyond the wide cap too"""
    st = check_against_oracle(ctx, "ont", params(ctx, 1, "ont"))
    assert st["max_events"] > 2048, st


def test_wide_counters(ctx):
    """case 5: 301 reads x 800, 300 votes "after an insertion" for one base at one column"""
    truths, _ = D.wide_counters()
    st = check_against_oracle(ctx, "wide", params(ctx, 1))
    assert st["n_deep_windows"] > 0, st
    assert D.oracle("wide")[1][0] == truths[0]


def run_batch(ctx, order, deep):
    sets = [list(D.reads_of(c)) for c in order]
    contigs, cset, status, got, b = gpu_assemble(ctx, sets, params(ctx, deep))
    per_set, k = [], 0
    for si, s in enumerate(sets):
        per_set.append((got[k:k + len(s)], [bytes(c) for c, cs in zip(contigs, cset) if cs == si], int(status[si])))
        k += len(s)
    return dict(zip(order, per_set)), ctx.deep_windows()


def test_batch_shapes(ctx):
    """a deep set between two shallow ones, first, last; the context reused with the option 1, 0, 1; two runs with 1 give the same bytes"""
    alone, st_alone = run_batch(ctx, ["locus"], 1)
    assert st_alone["n_deep_windows"] > 0
    want = {c: D.oracle(c) for c in ("shallow11", "locus", "shallow12")}
    mid1, st1 = run_batch(ctx, ["shallow11", "locus", "shallow12"], 1)
    mid0, st0 = run_batch(ctx, ["shallow11", "locus", "shallow12"], 0)
    again, st2 = run_batch(ctx, ["shallow11", "locus", "shallow12"], 1)
    assert st0 == {"n_deep_windows": 0, "n_deep_junctions": 0, "max_events": 0}
    assert mid0["locus"][2] & W_INS_EVENTS
    assert st1 == st_alone == st2      # only the deep set's windows are counted
    assert mid1 == again                # nothing depends on the order the events arrive in
    for c in ("shallow11", "shallow12"):
        assert mid0[c] == mid1[c] and not mid1[c][2] & W_INS_EVENTS      # (status 4: one locus lays out no contig, as in the oracle)
    for c in want:
        assert mid1[c][0] == want[c][1] and mid1[c][1] == want[c][0] and not mid1[c][2] & W_INS_EVENTS, c
    assert mid1["locus"] == alone["locus"]
    for order in (["locus", "shallow11", "shallow12"], ["shallow11", "shallow12", "locus"]):
        res, st = run_batch(ctx, order, 1)
        assert st == st_alone and all(res[c] == mid1[c] for c in order), order


def test_no_work(ctx):
    """set 0 of tests/golden/hifiasm_contigs.json: nothing reaches a cap, so the option changes no byte, the result is still hifiasm's and
    the statistics are all zero"""
    from focalsv_amd import synth
    from tests.test_gpu_asm import canon
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "hifiasm_contigs.json")))["sets"][0]
    s = synth.make_region(g["region"], width=g["width"], depth_per_hap=g["depth"]).reads[g["hap"] - 1]
    assert hashlib.md5(b"\n".join(s)).hexdigest() == g["reads_md5"]
    c0, s0, st0, r0, _ = gpu_assemble(ctx, [s], params(ctx, 0))
    c1, s1, st1, r1, _ = gpu_assemble(ctx, [s], params(ctx, 1))
    assert ctx.deep_windows() == {"n_deep_windows": 0, "n_deep_junctions": 0, "max_events": 0}
    assert r0 == r1 and [bytes(c) for c in c0] == [bytes(c) for c in c1] and list(st0) == list(st1)
    assert sorted((len(c), hashlib.md5(canon(c)).hexdigest()) for c in c1) == sorted((c["len"], c["md5"]) for c in g["contigs"])
