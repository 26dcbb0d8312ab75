"""The k-mer count table stage on the GPU (fsv_kmer_table; fsv_assemble_batch with kmer_table = 1) against tests/kmer_model.py --
the oracle's sketch counted with numpy, which tests/test_kmer_peaks.py pins to hifiasm-0.14's own log -- field by field, all 4 096
histogram bins and the sorted filter list; and the assembly's low-coverage verdict against a kmer_table = 0 call."""
import json
import os
import random

import numpy as np
import pytest

from focalsv_amd import _lib, synth
from focalsv_amd.readsets import pack_sets
from tests import kmer_model as M

pytestmark = pytest.mark.gpu

FIELDS = ("peak_hom", "peak_het", "cutoff", "low_i", "max_i", "n_entries", "n_distinct", "n_filtered", "n_indexed")


@pytest.fixture(scope="module")
def ctx():
    with _lib.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def region700():
    r = synth.make_region(700, width=26000, depth_per_hap=6.0)
    return [r.reads[0], r.reads[1]]


@pytest.fixture(scope="module")
def lowcov(golden_dir):
    gold = json.load(open(os.path.join(golden_dir, "hifiasm_lowcov.json")))["sets"]
    return gold, [synth.make_region(g["region"], width=g["width"], depth_per_hap=g["depth"]).reads[g["hap"] - 1] for g in gold]


def gpu_table(ctx, sets, w=1, k=51, hpc=1):
    b = pack_sets(sets)
    d = ctx.upload(b.words)
    try:
        return ctx.kmer_table(d, b.word_off, b.read_len, b.set_start, w, k, hpc)
    finally:
        ctx.dev_free(d)


def assert_equals_model(rec, hist, flt, model, what):
    for f in FIELDS:
        assert int(rec[f]) == int(model[f]), (what, f, int(rec[f]), int(model[f]))
    assert np.array_equal(hist.astype(np.int64), model["hist"]), (what, "hist", np.flatnonzero(hist.astype(np.int64) != model["hist"])[:8])
    assert np.array_equal(flt, model["filter"]), (what, "filter", len(flt), len(model["filter"]))


@pytest.mark.parametrize("w", [1, 51])
def test_two_haplotypes_of_one_region_as_two_sets(ctx, region700, w):
    """region 700 at 6x: haplotype 1 (14 reads) has no coverage peak -- every k-mer is filtered --, haplotype 2 (13 reads) peaks at 7:
    the smallest shape where the sets' tables could leak into each other"""
    out, hist, flt = gpu_table(ctx, region700, w=w)
    models = [M.kmer_table(s, w) for s in region700]
    for s in (0, 1):
        assert_equals_model(out[s], hist[s], flt[s], models[s], (w, s))
    if w == 1:
        assert [int(x) for x in out["peak_hom"]] == [-1, 7] and int(out[0]["cutoff"]) == -5 and int(out[1]["cutoff"]) == 35
        assert int(out[0]["n_filtered"]) == int(out[0]["n_distinct"]) == 31162 and int(out[1]["n_filtered"]) == 0
    else:
        assert (int(out[1]["n_distinct"]), int(out[1]["n_indexed"]), int(hist[1][5]), int(hist[1][7])) == (1242, 4275, 116, 161)   # hifiasm's first ha_pt_gen


def test_repeat_regions_have_a_filter(ctx, golden_dir):
    """make_repeat_region(2) and (9): 357 and 2 656 k-mers reach 5 x the homozygous peak -- as the model says and as hifiasm logged"""
    gold = {g["index"]: g for g in json.load(open(os.path.join(golden_dir, "hifiasm_kmer_table.json")))["sets"] if g["kind"] == "repeat"}
    sets = [synth.make_repeat_region(i).reads[0] for i in (2, 9)]
    out, hist, flt = gpu_table(ctx, sets)
    for s, i in enumerate((2, 9)):
        assert_equals_model(out[s], hist[s], flt[s], M.kmer_table(sets[s]), i)
        ft = gold[i]["ft"]
        assert (int(out[s]["n_filtered"]), int(out[s]["cutoff"]), int(out[s]["peak_hom"]), int(out[s]["peak_het"])) == (ft["filtered"], ft["cutoff"], ft["peak_hom"], ft["peak_het"])
    assert [int(x) for x in out["n_filtered"]] == [357, 2656] and [int(x) for x in out["cutoff"]] == [65, 75]


def assemble(ctx, sets, kmer_table, fetch=True):
    b = pack_sets(sets)
    d = ctx.upload(b.words)
    try:
        p = ctx.default_asm_params()
        assert p.kmer_table == 0
        p.kmer_table = kmer_table
        contigs, cset, cnr, status = ctx.assemble_batch(d, b.word_off, b.read_len, b.set_start, p)
        reads = ctx.fetch_reads(b.n_reads, int(b.read_len.sum()) * 2 + 1024) if fetch else None
        verdicts = ctx.last_kmer_table(b.n_sets) if kmer_table else None
        table = ctx.kmer_table(d, b.word_off, b.read_len, b.set_start, 1, p.k, p.hpc, want_hist=False, want_filter=False)[0] if kmer_table else None
    finally:
        ctx.dev_free(d)
    per_set = [[c for c, cs in zip(contigs, cset) if cs == s] for s in range(len(sets))]
    start = np.concatenate([[0], np.cumsum([len(s) for s in sets])])
    per_set_reads = None if reads is None else [reads[start[s]:start[s + 1]] for s in range(len(sets))]
    return per_set, status, per_set_reads, verdicts, table


def test_assembly_leaves_sets_without_a_peak_alone(ctx, lowcov):
    """the 30 low-coverage sets in one call: with kmer_table = 1 the four sets where hifiasm filters every k-mer
    (reference_left_reads_uncorrected in the golden) come back uncorrected, without a contig, flagged; the other 26 are bit-identical
    to the kmer_table = 0 call"""
    gold, sets = lowcov
    contigs1, status1, reads1, (verdicts, ms), table = assemble(ctx, sets, 1)
    contigs0, status0, reads0, _, _ = assemble(ctx, sets, 0)
    low = [s for s in range(len(sets)) if status1[s] & _lib.W_LOW_COV]
    assert low == [s for s, g in enumerate(gold) if g["reference_left_reads_uncorrected"]] and len(low) == 4
    assert not any(st & _lib.W_LOW_COV for st in status0)
    for s in range(len(sets)):
        if s in low:
            assert status1[s] & _lib.W_NO_LAYOUT and contigs1[s] == [] and reads1[s] == list(sets[s]), s
            assert reads0[s] != list(sets[s])       # (the default path does correct these reads)
        else:
            assert (contigs1[s], reads1[s], int(status1[s])) == (contigs0[s], reads0[s], int(status0[s])), s
    assert [int(v["peak_hom"]) < 0 for v in verdicts] == [s in low for s in range(len(sets))]
    assert verdicts.tobytes() == table.tobytes()
    assert ms > 0.0


def test_verdicts_of_a_call_cut_into_chunks_come_in_set_order(ctx, lowcov, monkeypatch):
    """a workspace budget of 30 MB puts each of these six sets (~20 MB of workspace each) into a chunk of its own"""
    gold, all_sets = lowcov
    pick = [0, 1, 10, 11, 20, 21]          # regions 700, 705, 710: sets 0, 10, 20 and 21 have no peak
    sets = [all_sets[i] for i in pick]
    whole, status_w, _, (verdicts_w, _), table = assemble(ctx, sets, 1)
    monkeypatch.setenv("FSV_ASM_BUDGET_GB", "0.03")
    with pytest.raises(_lib.FsvError) as e:     # fsv_asm_fetch_reads serves single-pass batches only: the call was cut
        assemble(ctx, sets, 1)
    assert e.value.code == _lib.EINVAL and "fsv_asm_fetch_reads" in str(e.value)
    cut, status_c, _, (verdicts_c, ms), _ = assemble(ctx, sets, 1, fetch=False)
    assert verdicts_c.tobytes() == verdicts_w.tobytes() == table.tobytes()
    assert [int(v["peak_hom"]) < 0 for v in verdicts_c] == [True, False, True, False, True, True]
    assert [bool(st & _lib.W_LOW_COV) for st in status_c] == [True, False, True, False, True, True]
    assert cut == whole and list(status_c) == list(status_w)
    assert ms > 0.0


def assemble_all_stages(ctx, sets, on):
    """assemble_batch with kmer_table = kmer_filter = partial_charge = on -> (contigs per set, statuses, what the three getters say: the
    records and the time of each, or the FsvError of a getter that refuses)"""
    b = pack_sets(sets)
    d = ctx.upload(b.words)
    try:
        p = ctx.default_asm_params()
        p.kmer_table = p.kmer_filter = p.partial_charge = on
        contigs, cset, _, status = ctx.assemble_batch(d, b.word_off, b.read_len, b.set_start, p)
    finally:
        ctx.dev_free(d)
    left = []
    for getter in (lambda: ctx.last_kmer_table(b.n_sets), lambda: ctx.last_kmer_index(b.n_sets), ctx.last_charge):
        try:
            left.append(getter())
        except _lib.FsvError as e:
            left.append(e)
    return [[c for c, cs in zip(contigs, cset) if cs == s] for s in range(len(sets))], [int(x) for x in status], left


def test_three_stages_of_a_call_cut_into_chunks(ctx, lowcov, monkeypatch):
    """kmer_table, kmer_filter and partial_charge together on the six sets of the test above, whole and with every set in a chunk of its own
    (fsv_asm_fetch_reads refusing proves the cut): the chunk loop with the filter sets, the appended filter list and the charge clock alive
    at once leaves what the single pass leaves; a call with the three options off then leaves every getter refusing"""
    _, all_sets = lowcov
    sets = [all_sets[i] for i in (0, 1, 10, 11, 20, 21)]
    n_reads = sum(len(s) for s in sets)
    counters = ("n_overlaps", "n_windows", "n_ext", "n_accepted", "n_flipped")
    whole, status_w, (table_w, index_w, charge_w) = assemble_all_stages(ctx, sets, 1)
    ctx.fetch_reads(n_reads, sum(len(r) for s in sets for r in s) * 2 + 1024)       # (one pass: its reads are there)
    monkeypatch.setenv("FSV_ASM_BUDGET_GB", "0.03")
    cut, status_c, (table_c, index_c, charge_c) = assemble_all_stages(ctx, sets, 1)
    with pytest.raises(_lib.FsvError) as e:
        ctx.fetch_reads(n_reads, sum(len(r) for s in sets for r in s) * 2 + 1024)
    assert e.value.code == _lib.EINVAL and "fsv_asm_fetch_reads" in str(e.value)
    print("whole:", table_w[1], index_w[1], charge_w, "cut:", table_c[1], index_c[1], charge_c)
    assert cut == whole and status_c == status_w
    assert table_c[0].tobytes() == table_w[0].tobytes() and index_c[0].tobytes() == index_w[0].tobytes()
    assert [charge_c[n] for n in counters] == [charge_w[n] for n in counters]
    for ms in (table_w[1], index_w[1], charge_w["ms"], table_c[1], index_c[1], charge_c["ms"]):
        assert ms > 0.0
    _, _, left = assemble_all_stages(ctx, sets, 0)
    assert [isinstance(x, _lib.FsvError) and x.code for x in left] == [_lib.EINVAL] * 3


def edge_sets():
    rng = random.Random(5)
    rand = lambda n: "".join(rng.choice("ACGT") for _ in range(n)).encode()
    sets = [[rand(30), rand(50), rand(12)]]                     # every read shorter than k = 51: no entry, no peak
    sets.append([rand(5000)])                                   # one read: every count is 1 (a few 2 with k = 15)
    sets += [[rand(2000) for _ in range(3)] for _ in range(64)]  # every key distinct: one slot per entry, many tiny tables
    # a 7-base unit without a homopolymer, in reads of 1.5-2.5 kb at every phase: seven canonical k-mers, each seen > 4095 times
    unit = "ACGTCAG"
    sets.append([(unit * 400)[i % 7:i % 7 + 1500 + 25 * i].encode() for i in range(40)])
    # table sizes at the power of two: 4 095 and 4 096 entries with k = 15 and no compression (2 x 4 096 = the 8 192 slots exactly)
    sets.append([rand(1379), rand(1379), rand(1379)])
    sets.append([rand(1379), rand(1379), rand(1380)])
    return sets


@pytest.mark.parametrize("k,w,hpc", [(51, 1, 1), (15, 1, 0), (20, 3, 1)])
def test_edge_shapes_equal_model(ctx, k, w, hpc):
    """all in one call: no entry at all, a single read, 64 sets of three random 2 kb reads, a tandem array that saturates the count, tables
    filled to exactly one half -- under hifiasm's scheme, the ONT profile's k = 15 without compression, and an even k (replay kernel)"""
    sets = edge_sets()
    out, hist, flt = gpu_table(ctx, sets, w=w, k=k, hpc=hpc)
    models = [M.kmer_table(s, w, k, hpc) for s in sets]
    for s in range(len(sets)):
        assert_equals_model(out[s], hist[s], flt[s], models[s], (k, w, hpc, s))
    tandem = models[66]
    assert tandem["hist"][M.MAX_COUNT] > 0 and max(np.unique(M.set_hashes(sets[66], w, k, hpc), return_counts=True)[1]) > M.MAX_COUNT
    if k == 51:
        assert models[0]["n_entries"] == 0 and int(out[0]["peak_hom"]) == -1 and int(out[0]["n_filtered"]) == 0
        assert all(models[s]["n_distinct"] == models[s]["n_entries"] > 3000 for s in range(2, 66))
    if (k, hpc) == (15, 0):
        assert [models[s]["n_entries"] for s in (67, 68)] == [4095, 4096]


def test_scheme_outside_the_sketch_range_is_refused(ctx, region700):
    for w, k in ((0, 51), (256, 51), (65, 50), (1, 64), (1, 0)):
        with pytest.raises(_lib.FsvError) as e:
            gpu_table(ctx, region700[:1], w=w, k=k)
        assert e.value.code == _lib.EINVAL
