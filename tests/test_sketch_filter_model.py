"""tests/sketch_filter_model.py (ha_sketch with hifiasm's high-count k-mer filter, sketch.cpp:39-137), no device:
 (a) with an empty filter both forms of the model equal oracle.sketch entry for entry, on a sample of tests/sketch_cases.py over every
     (w, k, hpc) class -- w = 1 / small / large, odd and even k (palindromes take no slot), with and without compression -- and every
     length edge; with filters the numpy form equals the line-by-line one;
 (b) on the golden read sets of tests/golden/hifiasm_kmer_table.json the FILTERED w = 51 sketch, counted, gives what hifiasm-0.14 itself
     logs from its first ha_pt_gen -- distinct minimizers counted, positions indexed, the histogram's lowest / highest / left / right
     points, peak_hom, peak_het -- on all 26 sets with a peak and a non-empty filter, and on the other 48 as before;
 (c) the unfiltered sketch does not give those figures on repeat sets 9 and 16, so (b) can tell the difference."""
import json
import os
import random

import numpy as np
import pytest

from tests import kmer_model as KM
from tests import oracle_lib as O
from tests import sketch_cases as SC
from tests import sketch_filter_model as FM

FIELDS = ("hash", "pos", "rev", "span")
# one grid point per class: (w = 1 | 1 < w < k | w = k | w > k | w = 255) x (k odd | even | 1 | 63) x hpc
SAMPLE = ((1, 51, 1), (1, 20, 0), (1, 1, 1), (2, 2, 0), (3, 15, 0), (16, 20, 1), (15, 19, 0), (51, 51, 1), (51, 50, 1), (64, 32, 1), (64, 63, 0),
          (17, 2, 1), (100, 3, 1), (255, 19, 0), (255, 62, 1), (33, 1, 0), (10, 16, 0), (19, 15, 0), (255, 21, 1))


def _rows(a):
    return [tuple(int(m[f]) for f in FIELDS) for m in a]


@pytest.mark.parametrize("gp", SAMPLE, ids=lambda gp: "w%d-k%d-hpc%d" % gp)
def test_empty_filter_equals_the_oracle(gp):
    """(a): every edge length, and of the other kinds the tandem / homopolymer / end-run cases, at the sampled grid points"""
    w, k, hpc = gp
    cases = SC.cases_for(w, k, hpc) if gp in [(g[0], g[1], g[2]) for g in SC.GRID] else []
    if not cases:       # a grid point of the GPU tests that tests/sketch_cases.py does not list: the same generators
        rng = random.Random("filter-model/%d/%d/%d" % gp)
        cases = [{"kind": "edge", "tag": str(n), "seq": SC._entries_seq(rng, n, hpc, k)} for n in SC.edge_lengths(w, k)]
        cases.append({"kind": "homopolymer", "tag": "dense", "seq": SC._homopolymer_rich(rng, 64, SC.HP_RUNS)})
        cases.append({"kind": "tandem", "tag": "AT", "seq": "AT" * (w + k + 40)})
        cases.append({"kind": "tandem", "tag": "ACGT", "seq": "ACGT" * (w + k + 40)})
    kinds = set()
    for n, c in enumerate(cases):
        want = _rows(O.sketch(c["seq"], w, k, hpc))
        got = _rows(FM.sketch(c["seq"], w, k, hpc))
        assert got == want, (gp, c["kind"], c["tag"])
        if len(c["seq"]) <= 1500 or n % 7 == 0:
            assert [tuple(r) for r in FM.sketch_literal(c["seq"], w, k, hpc)] == want, (gp, c["kind"], c["tag"], "literal")
        kinds.add(c["kind"])
    assert {"edge", "tandem", "homopolymer"} <= kinds


def test_slots_hold_the_dummies_and_skip_the_palindromes():
    """what takes a slot: the first k - 1 entries and the spans of 256 and more are dummies in a slot; a palindrome takes none"""
    rng = random.Random(5)
    s = "".join(rng.choices("ACGT", k=400))
    sl = FM.slots(s, 21, 0)
    assert len(sl) == 400 and (sl["hash"][:20] == np.uint64(FM.MAX)).all() and (sl["hash"][20:] != np.uint64(FM.MAX)).all()
    assert list(sl["pos"][20:]) == list(range(20, 400)) and (sl["span"][20:] == 21).all()
    # even k: ACGT repeated -- every other 4-mer is its own reverse complement in the high plane
    sl = FM.slots("ACGT" * 20, 4, 0)
    assert len(sl) < 80 and len(sl) == O.sketch_info("ACGT" * 20, 1, 4, 0)[1]
    # compression: a run of 300 inside makes the 5 k-mers that hold it dummies, each in a slot
    s = "ACGTCAGTCA" + "G" * 300 + "TCAGCTAGCATCG"
    sl = FM.slots(s, 5, 1)
    assert len(sl) == 10 + 1 + 13
    assert [int(h != FM.MAX) for h in sl["hash"]] == [0] * 4 + [1] * 6 + [0] * 5 + [1] * 9
    assert _rows(sl[sl["hash"] != np.uint64(FM.MAX)]) == _rows(O.sketch(s, 1, 5, 1))


@pytest.mark.parametrize("gp", ((51, 51, 1), (1, 51, 1), (19, 15, 0), (255, 21, 1), (10, 16, 0), (64, 32, 1)), ids=lambda gp: "w%d-k%d-hpc%d" % gp)
def test_filtered_numpy_form_equals_the_literal_one(gp):
    w, k, hpc = gp
    rng = random.Random("filtered/%d/%d/%d" % gp)
    n_flt = 0
    for n in (w + k + 30, 3 * w + k + 200):
        seq = SC._entries_seq(rng, n, hpc, k)
        if hpc:
            seq = seq[:len(seq) // 2] + seq[len(seq) // 2] * 300 + seq[len(seq) // 2:]
        sl = FM.slots(seq, k, hpc)
        real = [int(h) for h in sl["hash"] if int(h) != FM.MAX]
        plain = FM.sketch(seq, w, k, hpc)
        for flt in ([int(plain["hash"][0])] if len(plain) else [], [int(h) for h in plain["hash"]], rng.sample(real, len(real) // 3), real[w:2 * w + 1], real,
                    [12345, 2 ** 63 + 7]):
            got = FM.sketch(seq, w, k, hpc, flt)
            assert _rows(got) == [tuple(r) for r in FM.sketch_literal(seq, w, k, hpc, flt)], (gp, n, len(flt))
            assert not set(int(h) for h in got["hash"]) & set(flt)
            if flt == real:
                assert len(got) == 0
            if flt == [12345, 2 ** 63 + 7]:
                assert _rows(got) == _rows(plain)
            n_flt += 1
    assert n_flt == 12


# ---- (b), (c): hifiasm's own figures ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden_indexes(golden_dir):
    """per golden set: (record, table model, index model) -- computed once"""
    gold = json.load(open(os.path.join(golden_dir, "hifiasm_kmer_table.json")))["sets"]
    return [(g,) + FM.kmer_index(KM.reads_of(g), 51, 51, 1) for g in gold]


def _pt_figures(idx):
    fig = KM.log_figures(idx)
    fig.update(counted=idx["n_distinct"], indexed=idx["n_indexed"])
    return fig


def test_filtered_sketch_gives_hifiasm_index_figures(golden_indexes):
    """(b): nothing skipped, no known deviation"""
    n_flt = n_none = n_empty = 0
    for g, tab, idx in golden_indexes:
        assert (tab["n_filtered"], tab["cutoff"]) == (g["ft"]["filtered"], g["ft"]["cutoff"]), g
        fig = _pt_figures(idx)
        assert fig == {k: g["pt"][k] for k in fig}, (g["kind"], g.get("index"), g.get("region"), fig, g["pt"])
        if g["ft"]["cutoff"] < 0:
            n_none += 1
            assert idx["n_entries"] == 0 and idx["n_distinct"] == 0
        elif g["ft"]["filtered"]:
            n_flt += 1
        else:
            n_empty += 1
    assert (n_flt, n_none, n_empty) == (26, 4, 44)


def test_unfiltered_sketch_does_not(golden_indexes):
    """(c): repeat sets 9 and 16 -- the figures of the unfiltered w = 51 sketch are far from hifiasm's"""
    for g, _, idx in golden_indexes:
        if g["kind"] == "repeat" and g["index"] in (9, 16):
            plain = KM.kmer_table(KM.reads_of(g), 51)
            assert (plain["n_distinct"], plain["n_indexed"]) != (g["pt"]["counted"], g["pt"]["indexed"])
            assert plain["n_distinct"] < g["pt"]["counted"] and plain["n_indexed"] > g["pt"]["indexed"]
            assert (idx["n_distinct"], idx["n_indexed"]) == (g["pt"]["counted"], g["pt"]["indexed"])
