"""fsv_asm_params.partial_charge = 1 through fsv_assemble_batch: non_trim_error_rate's charge for unmatched windows (Correct.cpp:725-845)
on the HIP path -- k_charge_tasks, k_bpm_ext, k_charge_accept after K6 -- against hifiasm-0.14's corrected reads and against
oracle/asm.c with partial_charge = 1.  The five mixed sets whose first round the full-length charge gets wrong in one read each
(KNOWN_MIXED_READ_DEVIATIONS) are what the option is for; every other golden set must not move."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

from focalsv_amd import _lib, synth
from focalsv_amd.readsets import pack_sets
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu

FIVE = (104, 107, 115, 131, 140)


@pytest.fixture(scope="module")
def ctx():
    with _lib.Context(0) as c:
        yield c


def canon(s):
    return min(s, synth.revcomp(s))


def reads_md5(reads):
    return hashlib.md5(b"\n".join(canon(c) for c in reads)).hexdigest()


def contig_keys(contigs):
    return sorted((len(c), hashlib.md5(canon(c)).hexdigest()) for c in contigs)


def assemble(ctx, sets, flags=None, rounds=None, partial_charge=1, params=None):
    """one fsv_assemble_batch call -> (corrected reads per set, contigs per set, status)"""
    p = params if params is not None else ctx.default_asm_params()
    if rounds is not None:
        p.n_rounds = rounds
    p.partial_charge = partial_charge
    b = pack_sets(sets)
    d = ctx.upload(b.words)
    try:
        contigs, cset, cnr, status = ctx.assemble_batch(d, b.word_off, b.read_len, b.set_start, p, flags)
        reads = ctx.fetch_reads(b.n_reads, int(b.read_len.sum()) * 2 + 1024)
    finally:
        ctx.dev_free(d)
    per_set, k = [], 0
    for s in sets:
        per_set.append(reads[k:k + len(s)])
        k += len(s)
    return per_set, [[c for c, cs in zip(contigs, cset) if cs == si] for si in range(len(sets))], status


@pytest.fixture(scope="module")
def mixed(golden_dir):
    """the 48 mixed sets: (golden record, reads)"""
    out = []
    for g in json.load(open(os.path.join(golden_dir, "hifiasm_mixed_reads.json")))["sets"]:
        r = synth.make_region(g["region"])
        out.append((g, r.reads[0] + r.reads[1]))
        assert hashlib.md5(b"\n".join(out[-1][1])).hexdigest() == g["reads_md5"], "synthetic generator drifted"
    assert len(out) == 48
    return out


@pytest.fixture(scope="module")
def five(mixed):
    return [(g, s) for g, s in mixed if g["region"] in FIVE]


@pytest.fixture(scope="module")
def five_round1(ctx, five):
    """round 1 of the five sets in one call with the option on -> (reads per set, the call's charge counters)"""
    reads, _, status = assemble(ctx, [s for _, s in five], [1] * 5, rounds=1)
    return reads, ctx.last_charge()


@pytest.fixture(scope="module")
def phased(golden_dir):
    """phased sets of four goldens: (name, golden record, reads)"""
    def gold(name):
        return json.load(open(os.path.join(golden_dir, name)))["sets"]
    out = []
    for g in gold("hifiasm_contigs.json"):
        if g["region"] in (1, 2, 39):
            out.append(("contigs", g, synth.make_region(g["region"], width=g["width"], depth_per_hap=g["depth"]).reads[g["hap"] - 1]))
    g = next(g for g in gold("hifiasm_repeats.json") if g["index"] == 35)
    out.append(("repeat", g, synth.make_repeat_region(35).reads[0]))
    g = next(g for g in gold("hifiasm_lowcov.json") if g["depth"] == 6.0 and not g["reference_left_reads_uncorrected"])
    out.append(("lowcov", g, synth.make_region(g["region"], width=g["width"], depth_per_hap=g["depth"]).reads[g["hap"] - 1]))
    g = next(g for g in gold("hifiasm_fresh.json") if (g["region"], g["hap"]) == (8011, 1))
    out.append(("fresh", g, synth.make_region(g["region"], width=g["width"], depth_per_hap=g["depth"]).reads[g["hap"] - 1]))
    for _, g, s in out:
        if "reads_md5" in g:
            assert hashlib.md5(b"\n".join(s)).hexdigest() == g["reads_md5"], "synthetic generator drifted"
    return out


def test_five_sets_round1_equals_hifiasm(ctx, five, five_round1):
    reads, st = five_round1
    assert [g["region"] for g, _ in five] == list(FIVE)
    for (g, _), r in zip(five, reads):
        assert reads_md5(r) == g["round_md5"][0], g["region"]
    off, _, _ = assemble(ctx, [s for _, s in five], [1] * 5, rounds=1, partial_charge=0)
    for (g, _), r in zip(five, off):
        assert reads_md5(r) != g["round_md5"][0], ("the full-length charge already gives hifiasm's reads", g["region"])
    # one read changes in each set
    assert [sum(a != b for a, b in zip(x, y)) for x, y in zip(reads, off)] == [1] * 5


def test_five_sets_counters(five_round1):
    _, st = five_round1
    print("fsv_charge_stats, round 1 of the five sets:", st)
    assert st["n_flipped"] >= 1
    assert st["n_ext"] <= 2 * st["n_windows"]
    assert st["n_accepted"] <= st["n_overlaps"]
    assert st["n_flipped"] <= st["n_accepted"]
    assert 0 < st["n_overlaps"] <= st["n_windows"]
    assert st["ms"] > 0.0


@pytest.mark.parametrize("region", [131, 104])
def test_reads_equal_the_oracle_read_for_read(five, five_round1, region):
    i = FIVE.index(region)
    p = O.default_params()
    p.n_rounds, p.graph_layout, p.partial_charge = 1, 0, 1
    _, want = O.assemble(five[i][1], p)
    got = five_round1[0][i]
    bad = [j for j in range(len(want)) if got[j] != want[j]]
    assert not bad, (region, bad[:8])


@pytest.mark.parametrize("rounds", [1, 2, 3])
def test_all_mixed_sets_equal_hifiasm_without_deviations(ctx, mixed, rounds):
    reads, _, status = assemble(ctx, [s for _, s in mixed], [1] * len(mixed), rounds=rounds)
    bad = [g["region"] for (g, _), r in zip(mixed, reads) if reads_md5(r) != g["round_md5"][rounds - 1]]
    assert not bad, (rounds, bad)


def test_phased_sets_do_not_move(ctx, phased):
    from tests.test_oracle_asm import check_repeat_set
    reads, contigs, status = assemble(ctx, [s for _, _, s in phased])
    for (name, g, s), r, c in zip(phased, reads, contigs):
        if name == "repeat":
            check_repeat_set(g, c, r, synth.make_repeat_region(35).haps[0])
            continue
        want_reads = g["round_md5"][2] if name == "fresh" else g["corrected_reads_md5"]
        want_contigs = sorted((n, m) for n, m in g["contigs"]) if name == "fresh" else sorted((x["len"], x["md5"]) for x in g["contigs"])
        assert reads_md5(r) == want_reads, (name, g["region"], g["hap"])
        assert contig_keys(c) == want_contigs, (name, g["region"], g["hap"])
    assert ctx.last_charge()["n_ext"] <= 2 * ctx.last_charge()["n_windows"]


def test_order_and_neighbours(ctx, five, five_round1, phased):
    """the five sets alone, and interleaved with four phased sets in another order: the same reads per set"""
    alone = five_round1[0]
    others = [s for _, _, s in phased[:4]]
    order = [3, 0, 4, 2, 1]
    sets, flags, where = [], [], {}
    for n, i in enumerate(order):
        where[i] = len(sets)
        sets.append(five[i][1]); flags.append(1)
        if n < len(others):
            sets.append(others[n]); flags.append(0)
    reads, _, _ = assemble(ctx, sets, flags, rounds=1)
    for i in range(5):
        assert reads[where[i]] == alone[i], FIVE[i]


def test_wide_band_profiles_refuse_the_option(ctx, five):
    for make in (ctx.ont_asm_params, ctx.clr_asm_params):
        with pytest.raises(_lib.FsvError) as e:
            assemble(ctx, [five[3][1][:6]], params=make())
        assert e.value.code == _lib.EINVAL and "31" in str(e.value)


def _assemble_raw(ctx, sets, params_ptr):
    """fsv_assemble_batch with the params pointer as given (None: NULL) -> (reads, contigs)"""
    b = pack_sets(sets)
    word_off = np.ascontiguousarray(b.word_off, dtype=np.uint64)
    read_len = np.ascontiguousarray(b.read_len, dtype=np.int32)
    set_start = np.ascontiguousarray(b.set_start, dtype=np.uint32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    d = ctx.upload(b.words)
    try:
        rs = _lib.ReadSets(C.c_void_p(d), ptr(word_off).value, ptr(read_len).value, ptr(set_start).value, len(read_len), len(set_start) - 1, None)
        cap, ccap = C.c_uint64(), C.c_uint32()
        ctx.check(ctx._lib.fsv_assemble_batch_bound(C.byref(rs), C.byref(cap), C.byref(ccap)), "fsv_assemble_batch_bound")
        seq = np.empty(cap.value, dtype=np.uint8)
        off = np.zeros(ccap.value + 1, dtype=np.uint64)
        cset, cnr, status = np.zeros(ccap.value, dtype=np.uint32), np.zeros(ccap.value, dtype=np.uint32), np.zeros(rs.n_sets, dtype=np.int32)
        out = _lib.Contigs(ptr(seq).value, cap.value, ptr(off).value, ptr(cset).value, ptr(cnr).value, ccap.value, 0, ptr(status).value)
        ctx.check(ctx._lib.fsv_assemble_batch(ctx._h, C.byref(rs), params_ptr, C.byref(out)), "fsv_assemble_batch")
        reads = ctx.fetch_reads(b.n_reads, int(b.read_len.sum()) * 2 + 1024)
    finally:
        ctx.dev_free(d)
    return reads, [seq[int(off[i]):int(off[i + 1])].tobytes() for i in range(out.n_contigs)]


def test_default_is_off(ctx, five):
    s131 = five[FIVE.index(131)][1]
    null = _assemble_raw(ctx, [s131], None)
    with pytest.raises(_lib.FsvError) as e:
        ctx.last_charge()
    assert e.value.code == _lib.EINVAL
    p = ctx.default_asm_params()
    assert p.partial_charge == 0
    explicit = _assemble_raw(ctx, [s131], C.byref(p))
    with pytest.raises(_lib.FsvError) as e:
        ctx.last_charge()
    assert e.value.code == _lib.EINVAL
    assert null == explicit
