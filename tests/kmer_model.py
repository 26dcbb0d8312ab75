"""A Python model of hifiasm-0.14's k-mer count table per read set (ha_ft_gen / ha_pt_gen / ha_analyze_count: htab.cpp:917-998,
hist.cpp:15-96), built on the oracle's sketch: the reference for fsv_kmer_peaks and fsv_kmer_table.  TEST INFRASTRUCTURE.

The keys are the hashes of the entries oracle.sketch emits for (w, k, hpc); a count saturates at 4095; hist[c] = distinct keys seen c
times.  tests/test_kmer_peaks.py pins this model to what hifiasm itself logs (tests/golden/hifiasm_kmer_table.json)."""
import numpy as np

from tests import oracle_lib as O

N_COUNTS = 4096      # YAK_N_COUNTS
MAX_COUNT = 4095     # YAK_MAX_COUNT
START_CNT = 5        # min_hist_kmer_cnt
HIGH_FACTOR = 5.0    # high_factor


def analyze_count(hist, n_cnt=None, start_cnt=START_CNT):
    """ha_analyze_count -> dict(peak_hom, peak_het, low_i, max_i, left, right): `left` / `right` are the secondary peaks that survive
    their rules (-1: none); max_i, left and right are -1 when the histogram never rises behind its lowest point (peak_hom -1)"""
    cnt = [int(x) for x in hist]
    n = len(cnt) if n_cnt is None else n_cnt
    res = {"peak_hom": -1, "peak_het": -1, "low_i": -1, "max_i": -1, "left": -1, "right": -1}
    start = 1 if cnt[1] > 0 else 2
    i = max(start, start_cnt) + 1
    while i < n and not cnt[i] > cnt[i - 1]:
        i += 1
    low_i = res["low_i"] = i - 1
    if low_i == n - 1:
        return res
    max_i = max(range(low_i + 1, n), key=lambda j: (cnt[j], -j))       # the first of the largest
    res["max_i"] = max_i
    top = cnt[max_i]

    def local_maxima(rng):
        return [j for j in rng if cnt[j] >= cnt[j - 1] and cnt[j] >= cnt[j + 1]]

    def survives(p, lo, hi):
        """a secondary peak at p; [lo, hi): the bins between it and the highest peak"""
        valley = min([top] + cnt[lo:hi])
        return not (cnt[p] < top * 0.05 or valley > cnt[p] * 0.95)

    left = local_maxima(range(max_i - 1, low_i, -1))          # scanned downwards: the first of the largest is the one nearest max_i
    if left:
        p = max(left, key=lambda j: (cnt[j], j))
        if survives(p, p + 1, max_i):
            res["left"] = p
    right = local_maxima(range(max_i + 1, n - 1))
    if right:
        p = max(right, key=lambda j: (cnt[j], -j))
        if survives(p, max_i + 1, p) and not p > max_i * 2.5:
            res["right"] = p
    if res["right"] > 0:
        res["peak_hom"], res["peak_het"] = res["right"], max_i
    else:
        res["peak_hom"], res["peak_het"] = max_i, res["left"]
    return res


def set_hashes(reads, w=1, k=51, hpc=1):
    """the hashes of every sketch entry of every read of the set, in read order"""
    parts = [O.sketch(r.decode() if isinstance(r, bytes) else r, w, k, hpc)["hash"] for r in reads]
    return np.concatenate(parts) if parts else np.zeros(0, np.uint64)


def count_table(hashes):
    """-> (keys ascending, counts saturated at 4095, hist int64[4096])"""
    keys, counts = np.unique(np.asarray(hashes, dtype=np.uint64), return_counts=True)
    counts = np.minimum(counts, MAX_COUNT).astype(np.int64)
    return keys, counts, np.bincount(counts, minlength=N_COUNTS).astype(np.int64)


def kmer_table(reads, w=1, k=51, hpc=1):
    """the whole stage on one read set -> dict with the fields of fsv_kmer_set, `hist`, `filter` (ascending hashes with
    count >= cutoff) and the two secondary peaks"""
    hashes = set_hashes(reads, w, k, hpc)
    keys, counts, hist = count_table(hashes)
    res = analyze_count(hist)
    hom = res["peak_hom"]
    cutoff = min(int(hom * HIGH_FACTOR), MAX_COUNT - 1)
    flt = keys[counts >= cutoff]
    res.update(cutoff=cutoff, n_entries=int(len(hashes)), n_distinct=int(len(keys)), n_filtered=int(len(flt)),
               n_indexed=int(sum(c * int(hist[c]) for c in range(2, MAX_COUNT))), hist=hist, filter=flt)
    return res


def log_figures(res):
    """the figures hifiasm logs for a histogram, as tests/golden/hifiasm_kmer_table.json records them: [index, value] pairs or None"""
    h = res["hist"]
    pair = lambda i: None if i < 0 else [int(i), int(h[i])]
    out = {"lowest": pair(res["low_i"]), "highest": pair(res["max_i"]), "left": pair(res["left"]), "right": pair(res["right"]),
           "peak_hom": res["peak_hom"], "peak_het": res["peak_het"]}
    if res["peak_hom"] < 0:
        out["peak_het"] = -1
    return out


def reads_of(g):
    """the read set of one record of tests/golden/hifiasm_kmer_table.json (list of bytes)"""
    from focalsv_amd import synth
    if g["kind"] == "repeat":
        return synth.make_repeat_region(g["index"]).reads[0]
    if g["kind"] == "unphased":
        r = synth.make_region(g["region"])
        return r.reads[0] + r.reads[1]
    return synth.make_region(g["region"], width=g["width"], depth_per_hap=g["depth"]).reads[g["hap"] - 1]
