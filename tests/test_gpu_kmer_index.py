"""fsv_kmer_index on the GPU -- hifiasm's first ha_pt_gen per read set (htab.cpp:952-998): the count table at w = 1, its filter list, the
filter sets, the FILTERED sketch at w = 51, counted -- against tests/sketch_filter_model.py and against what hifiasm-0.14 itself logs
(tests/golden/hifiasm_kmer_table.json: distinct minimizers counted, positions indexed, the histogram's lowest and highest points, peak_hom,
peak_het).  The sample: all 26 golden sets with a peak and a non-empty filter (1 to 4 057 keys), four with an empty filter, two without a
peak (every k-mer filtered: the index of nothing) -- in ONE call, so a set's filter could leak into its neighbours'.  Then
fsv_asm_last_kmer_index after fsv_assemble_batch with kmer_table = 1, kmer_filter = 1."""
import json
import os

import numpy as np
import pytest

from focalsv_amd import _lib
from focalsv_amd.readsets import pack_sets
from tests import kmer_model as KM
from tests import sketch_filter_model as FM

pytestmark = pytest.mark.gpu

TABLE_FIELDS = ("peak_hom", "peak_het", "cutoff", "low_i", "max_i", "n_entries", "n_distinct", "n_filtered", "n_indexed")
INDEX_FIELDS = ("n_entries", "n_distinct", "n_indexed", "low_i", "max_i", "peak_hom", "peak_het")


def _sample(gold):
    flt = [i for i, g in enumerate(gold) if g["ft"]["filtered"] > 0 and g["ft"]["cutoff"] > 0]
    empty = [i for i, g in enumerate(gold) if g["ft"]["filtered"] == 0]
    none = [i for i, g in enumerate(gold) if g["ft"]["cutoff"] < 0]
    assert len(flt) == 26 and len(none) == 4
    # (the sets without a peak go between sets with a filter)
    return flt[:5] + none[:1] + flt[5:20] + empty[:2] + none[3:] + flt[20:] + [empty[len(empty) // 2], empty[-1]]


@pytest.fixture(scope="module")
def ctx():
    with _lib.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def sample(golden_dir, ctx):
    """(golden records, read sets, the one fsv_kmer_index call's result) for the sampled sets"""
    gold = json.load(open(os.path.join(golden_dir, "hifiasm_kmer_table.json")))["sets"]
    pick = _sample(gold)
    assert len(pick) == 32 and len(set(pick)) == 32
    recs = [gold[i] for i in pick]
    sets = [KM.reads_of(g) for g in recs]
    b = pack_sets(sets)
    d = ctx.upload(b.words)
    try:
        tab, idx, hist = ctx.kmer_index(d, b.word_off, b.read_len, b.set_start, 51, 51, 1)
    finally:
        ctx.dev_free(d)
    return recs, sets, (tab, idx, hist)


@pytest.mark.parametrize("n", range(32))
def test_index_equals_model_and_hifiasm(sample, n):
    recs, sets, (tab, idx, hist) = sample
    g = recs[n]
    mtab, midx = FM.kmer_index(sets[n], 51, 51, 1)
    what = (g["kind"], g.get("index"), g.get("region"), g.get("hap"))
    for f in TABLE_FIELDS:
        assert int(tab[n][f]) == int(mtab[f]), (what, "table", f, int(tab[n][f]), int(mtab[f]))
    for f in INDEX_FIELDS:
        assert int(idx[n][f]) == int(midx[f]), (what, "index", f, int(idx[n][f]), int(midx[f]))
    assert np.array_equal(hist[n].astype(np.int64), midx["hist"]), (what, "hist", np.flatnonzero(hist[n].astype(np.int64) != midx["hist"])[:8])
    # hifiasm's own lines
    pt = g["pt"]
    h = hist[n]
    pair = lambda i: None if i < 0 else [int(i), int(h[i])]
    assert (int(idx[n]["n_distinct"]), int(idx[n]["n_indexed"])) == (pt["counted"], pt["indexed"]), what
    assert pair(int(idx[n]["low_i"])) == pt["lowest"] and pair(int(idx[n]["max_i"])) == pt["highest"], what
    assert int(idx[n]["peak_hom"]) == pt["peak_hom"], what
    if pt["peak_hom"] >= 0:
        assert int(idx[n]["peak_het"]) == pt["peak_het"], what
    if g["ft"]["cutoff"] < 0:       # every k-mer filtered: counted 0, indexed 0
        assert int(idx[n]["n_entries"]) == 0 and not h.any()


def test_the_sample_is_what_it_says(sample):
    recs, _, (tab, idx, _) = sample
    kinds = [("none" if g["ft"]["cutoff"] < 0 else "filter" if g["ft"]["filtered"] else "empty") for g in recs]
    assert (kinds.count("filter"), kinds.count("empty"), kinds.count("none")) == (26, 4, 2)
    assert sorted(int(t["n_filtered"]) for t, kd in zip(tab, kinds) if kd == "filter")[:2] == [1, 6] and max(int(t["n_filtered"]) for t, kd in zip(tab, kinds) if kd == "filter") == 4057
    # the filter moves the index: on repeat sets 9 and 16 the unfiltered w = 51 sketch has fewer distinct minimizers at more positions
    for g, i in zip(recs, idx):
        if g["kind"] == "repeat" and g["index"] in (9, 16):
            plain = KM.kmer_table(KM.reads_of(g), 51)
            assert plain["n_distinct"] < int(i["n_distinct"]) and plain["n_indexed"] > int(i["n_indexed"])


def test_assembly_keeps_the_index_of_round_0(ctx, sample):
    """fsv_assemble_batch with both options on, four sets in one call: a filter of one key, a set without a peak, a filter of 37, none --
    fsv_asm_last_kmer_index returns what fsv_kmer_index computes for the same sets, and a call without the option returns FSV_EINVAL"""
    recs, sets, (tab, idx, _) = sample
    by_keys = {int(t["n_filtered"]): n for n, t in enumerate(tab) if int(t["peak_hom"]) >= 0}
    none = next(n for n, t in enumerate(tab) if int(t["peak_hom"]) < 0)
    pick = [by_keys[1], none, by_keys[37], by_keys[0]]
    b = pack_sets([sets[n] for n in pick])
    d = ctx.upload(b.words)
    try:
        p = ctx.default_asm_params()
        assert p.kmer_filter == 0
        p.kmer_table, p.kmer_filter, p.n_rounds = 1, 1, 1
        _, _, _, status = ctx.assemble_batch(d, b.word_off, b.read_len, b.set_start, p)
        got, ms = ctx.last_kmer_index(len(pick))
        verdicts, _ = ctx.last_kmer_table(len(pick))
        p.kmer_filter = 0
        ctx.assemble_batch(d, b.word_off, b.read_len, b.set_start, p)
        with pytest.raises(_lib.FsvError) as e:
            ctx.last_kmer_index(len(pick))
        assert e.value.code == _lib.EINVAL
    finally:
        ctx.dev_free(d)
    assert ms > 0.0
    assert [bool(st & _lib.W_LOW_COV) for st in status] == [False, True, False, False]
    for j, n in enumerate(pick):
        assert got[j].tobytes() == idx[n].tobytes(), (j, got[j], idx[n])
        assert verdicts[j].tobytes() == tab[n].tobytes(), j
    assert int(got[1]["n_entries"]) == 0 and int(got[1]["peak_hom"]) == -1
