"""fsv_kmer_peaks (the host half of the k-mer count table stage: ha_analyze_count, hist.cpp:15-96) through ctypes, no device --
against tests/kmer_model.py, and that model against what hifiasm-0.14 itself logs (tests/golden/hifiasm_kmer_table.json:
tools/make_golden_kmer_table.py) on 74 read sets: 30 at low coverage, 36 repeat-rich, 8 unphased.

Branches of ha_analyze_count the GOLDEN histograms reach (test_branches_the_golden_reaches asserts the list): no peak (4 sets),
a single peak, a left peak kept, a left peak dropped by the 0.05 rule and by the 0.95 rule, a right peak kept (the right-peak return
path), a right peak dropped by the 0.05 rule and by the 0.95 rule, plateau ties among the local maxima.  Not reached by the golden,
covered by the synthetic histograms below: a right peak dropped by the 2.5 x rule, and hist[1] = 0."""
import json
import os

import numpy as np
import pytest

from focalsv_amd import _lib
from tests import kmer_model as M

N = M.N_COUNTS


@pytest.fixture(scope="module")
def golden_tables(golden_dir):
    """per golden set: (record, model at w = 1, model at w = 51 or None where ha_ft_gen's filter is not empty)"""
    gold = json.load(open(os.path.join(golden_dir, "hifiasm_kmer_table.json")))["sets"]
    out = []
    for g in gold:
        reads = M.reads_of(g)
        out.append((g, M.kmer_table(reads, 1), M.kmer_table(reads, 51) if g["ft"]["filtered"] == 0 else None))
    return out


def lib_peaks(hist, start_cnt=M.START_CNT):
    return _lib.kmer_peaks(hist, start_cnt)


def model_peaks(hist, start_cnt=M.START_CNT):
    r = M.analyze_count(hist, start_cnt=start_cnt)
    return r["peak_hom"], r["peak_het"], r["low_i"], r["max_i"]


def branches(hist):
    """which ways through ha_analyze_count a histogram takes (labels), worked out apart from the model's code"""
    h = [int(x) for x in hist]
    r = M.analyze_count(h)
    out = set()
    if h[1] == 0:
        out.add("hist[1] = 0")
    if r["peak_hom"] < 0:
        return out | {"no peak"}
    lo, top = r["low_i"], r["max_i"]
    for side, rng in (("left", range(top - 1, lo, -1)), ("right", range(top + 1, N - 1))):
        cand = [i for i in rng if h[i] >= h[i - 1] and h[i] >= h[i + 1]]
        if not cand:
            continue
        best = max(h[i] for i in cand)
        p = [i for i in cand if h[i] == best][0]
        if any(h[i] == h[i - 1] or h[i] == h[i + 1] for i in cand if h[i] > 0):
            out.add("plateau tie")
        between = h[p + 1:top] if side == "left" else h[top + 1:p]
        valley = min([h[top]] + between)
        if h[p] < h[top] * 0.05:
            out.add(side + " dropped: 0.05")
        elif valley > h[p] * 0.95:
            out.add(side + " dropped: 0.95")
        elif side == "right" and p > top * 2.5:
            out.add("right dropped: 2.5 x")
        else:
            out.add(side + " kept")
            assert r[side] == p
    if "left kept" not in out and "right kept" not in out:
        out.add("single peak")
    return out


def test_library_equals_model_on_golden_histograms(golden_tables):
    for g, t1, t51 in golden_tables:
        for t in (t1, t51):
            if t is not None:
                assert lib_peaks(t["hist"]) == (t["peak_hom"], t["peak_het"], t["low_i"], t["max_i"]), g


def test_model_equals_hifiasm_on_every_kmer(golden_tables):
    """ha_ft_gen's lines (w = 1): lowest, highest, left, right, peak_hom, peak_het, filtered N k-mers occurring C or more times"""
    no_peak = []
    for g, t1, _ in golden_tables:
        ft = g["ft"]
        fig = M.log_figures(t1)
        assert fig == {k: ft[k] for k in fig}, g
        assert (t1["n_filtered"], t1["cutoff"]) == (ft["filtered"], ft["cutoff"]), g
        if t1["peak_hom"] < 0:
            no_peak.append(g)
            assert t1["cutoff"] == -5 and t1["n_filtered"] == t1["n_distinct"]
    # without a peak hifiasm filters every k-mer and corrects nothing: exactly the sets hifiasm_lowcov.json marks
    assert [(g["region"], g["hap"]) for g in no_peak] == [(700, 1), (705, 1), (710, 1), (710, 2)]
    assert [g for g, _, _ in golden_tables if g.get("reference_left_reads_uncorrected")] == no_peak


def test_model_equals_hifiasm_on_minimizers(golden_tables):
    """the first ha_pt_gen's lines (w = 51) on the sets whose filter is empty (with a filter the minimizers differ: not restated)"""
    n = 0
    for g, _, t51 in golden_tables:
        if t51 is None:
            continue
        n += 1
        pt = g["pt"]
        fig = M.log_figures(t51)
        assert fig == {k: pt[k] for k in fig}, g
        assert (t51["n_distinct"], t51["n_indexed"]) == (pt["counted"], pt["indexed"]), g
    assert n >= 40


def test_branches_the_golden_reaches(golden_tables):
    seen = set()
    for g, t1, t51 in golden_tables:
        seen |= branches(t1["hist"])
        if t51 is not None:
            seen |= branches(t51["hist"])
    assert seen == {"no peak", "single peak", "left kept", "left dropped: 0.05", "left dropped: 0.95", "right kept", "right dropped: 0.05",
                    "right dropped: 0.95", "plateau tie"}, sorted(seen)


def H(*vals, **at):
    """a 4096-bin histogram: vals go to bins 1, 2, ...; at: {"b23": 300} puts 300 into bin 23"""
    h = np.zeros(N, dtype=np.int64)
    h[1:1 + len(vals)] = vals
    for k, v in at.items():
        h[int(k[1:])] = v
    return h


# name -> (histogram, (peak_hom, peak_het, low_i, max_i) worked out by hand from hist.cpp's rules, labels branches() must report).
# Every histogram starts with an error tail 900 400 200 100 50 20 in bins 1-6, so the lowest point is bin 6 unless said otherwise.
TAIL = (900, 400, 200, 100, 50, 20)
SYNTHETIC = {
    "monotone fall": (H(900, 800, 700, 600, 500, 400, 300, 200, 100), (-1, -1, 4095, -1), {"no peak"}),
    # bins 7-15: 10 30 80 150 200 150 80 30 10 -- the walk goes on to bin 7
    "single peak": (H(*TAIL, 10, 30, 80, 150, 200, 150, 80, 30, 10), (11, -1, 7, 11), {"single peak"}),
    # a left peak of 120 at bin 8 under a peak of 600 at bin 13, valley 30
    "left kept": (H(*TAIL, 60, 120, 60, 30, 100, 300, 600, 300, 100, 20), (13, 8, 6, 13), {"left kept"}),
    # the left peak is 25 < 5 % of 600
    "left dropped: 0.05": (H(*TAIL, 22, 25, 22, 21, 100, 300, 600, 300, 100, 20), (13, -1, 6, 13), {"left dropped: 0.05"}),
    # the valley behind the left peak of 120 stays at 117 > 114
    "left dropped: 0.95": (H(*TAIL, 100, 120, 118, 117, 200, 300, 600, 300, 100, 20), (13, -1, 6, 13), {"left dropped: 0.95"}),
    # peak 600 at bin 9, a right peak of 300 at bin 14, valley 50: the right peak is the homozygous one
    "right kept": (H(*TAIL, 100, 300, 600, 300, 100, 50, 150, 300, 150, 50), (14, 9, 6, 9), {"right kept"}),
    "right dropped: 0.05": (H(*TAIL, 100, 300, 600, 300, 100, 20, 22, 25, 22, 10), (9, -1, 6, 9), {"right dropped: 0.05"}),
    # the valley in front of the right peak of 300 stays at 288 > 285
    "right dropped: 0.95": (H(*TAIL, 100, 300, 600, 300, 290, 288, 289, 300, 150, 50), (9, -1, 6, 9), {"right dropped: 0.95"}),
    # the highest peak is at bin 9: a right peak at bin 22 <= 22.5 stays, one at bin 23 goes
    "right kept below 2.5 x": (H(*TAIL, 100, 300, 600, 300, 100, 50, b21=150, b22=300, b23=150), (22, 9, 6, 9), {"right kept"}),
    "right dropped: 2.5 x": (H(*TAIL, 100, 300, 600, 300, 100, 50, b22=150, b23=300, b24=150), (9, -1, 6, 9), {"right dropped: 2.5 x"}),
    # a flat bottom 20 20 20 in bins 5-7: the lowest point is its END; a flat top 200 200 in bins 9-10: the highest peak is the FIRST,
    # the second is a right peak with no valley in between (the valley then counts as the top itself: dropped by the 0.95 rule)
    "plateau: bottom and top": (H(500, 300, 100, 50, 20, 20, 20, 60, 200, 200, 90, 40), (9, -1, 7, 9), {"single peak", "plateau tie", "right dropped: 0.95"}),
    # two left peaks of 300 at bins 7 and 9: the one nearer the highest peak (bin 12)
    "plateau: equal left peaks": (H(*TAIL, 300, 100, 300, 100, 500, 1000, 500, 100), (12, 9, 6, 12), {"left kept"}),
    # and two right peaks of 300 at bins 15 and 17: the nearer one again, and it is then the homozygous peak
    "plateau: equal right peaks": (H(*TAIL, 300, 100, 300, 100, 500, 1000, 500, 100, 300, 100, 300, 100), (15, 12, 6, 12), {"left kept", "right kept"}),
    "hist[1] = 0": (H(0, 700, 300, 100, 30, 10, 40, 200, 40), (8, -1, 6, 8), {"single peak", "hist[1] = 0"}),
    # a peak at bin 3 lies below min_hist_kmer_cnt: the walk starts at bin 5 and only falls
    "peak below the start": (H(100, 300, 900, 300, 100, 30, 10), (-1, -1, 4095, -1), {"no peak"}),
    # the last two bins: bin 4094 rises over 4093 (the lowest point), bin 4095 is the peak; no bin is read beyond the array
    "rise into the last bins": (H(100, b4094=3, b4095=7), (4095, -1, 4093, 4095), None),
    "only the last bin": (H(b4095=7), (4095, -1, 4094, 4095), None),
    "empty": (H(), (-1, -1, 4095, -1), {"no peak", "hist[1] = 0"}),
}


@pytest.mark.parametrize("name", sorted(SYNTHETIC))
def test_synthetic_histograms(name):
    hist, want, labels = SYNTHETIC[name]
    assert model_peaks(hist) == want, (name, model_peaks(hist))
    assert lib_peaks(hist) == want, (name, lib_peaks(hist))
    if labels is not None:
        got = branches(hist)
        assert labels <= got, (name, sorted(got))


def test_random_histograms_equal_model():
    """bumpy random shapes: a falling error tail and up to three peaks with noise -- plateaus and near-threshold ratios come up by chance"""
    rng = np.random.default_rng(11)
    seen = set()
    for _ in range(400):
        h = np.zeros(N, dtype=np.int64)
        tail = int(rng.integers(2, 12))
        h[1:tail + 1] = np.sort(rng.integers(0, 5000, tail))[::-1]
        for _p in range(int(rng.integers(0, 4))):
            at, ht, wd = int(rng.integers(6, 120)), int(rng.integers(1, 3000)), int(rng.integers(1, 12))
            for d in range(-wd, wd + 1):
                if 1 <= at + d < N:
                    h[at + d] += ht * (wd + 1 - abs(d)) // (wd + 1)
        h[1:200] += rng.integers(0, int(rng.integers(1, 40)), 199)
        if rng.random() < 0.3:
            h[1] = 0
        assert lib_peaks(h) == model_peaks(h)
        seen |= branches(h)
    assert {"no peak", "single peak", "left kept", "right kept", "left dropped: 0.95", "right dropped: 0.95", "right dropped: 2.5 x"} <= seen, sorted(seen)


def test_other_bin_counts_and_bad_arguments():
    h = H(900, 100, 10, b18=100, b19=300, b20=500, b21=300, b22=100)[:64]
    assert _lib.kmer_peaks(h, 5) == model_peaks(h, 5) == (20, -1, 17, 20)
    assert _lib.kmer_peaks(h, 30) == model_peaks(h, 30) == (-1, -1, 63, -1)      # the walk starts behind the peak
    # hist[1] = 0 moves the first bin looked at from 1 to 2: from bin 1 the walk would stop at once (5 > 0)
    h = H(0, 5, 1, 4)[:16]
    assert _lib.kmer_peaks(h, 1) == model_peaks(h, 1) == (4, -1, 3, 4)
    assert _lib.kmer_peaks(h, 0) == model_peaks(h, 0) == (4, -1, 3, 4)
    lib = _lib.load()
    import ctypes as C
    a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
    hp = h.ctypes.data_as(C.c_void_p)
    assert lib.fsv_kmer_peaks(hp, 2, 0, C.byref(a), C.byref(b), C.byref(c)) == _lib.EINVAL
    assert lib.fsv_kmer_peaks(hp, 64, 64, C.byref(a), C.byref(b), C.byref(c)) == _lib.EINVAL
    assert lib.fsv_kmer_peaks(None, 64, 5, C.byref(a), C.byref(b), C.byref(c)) == _lib.EINVAL
