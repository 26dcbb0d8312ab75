"""Read sets deep enough to fill a consensus window's insertion-event buffer (FSV_EV_CAP = 256, FSV_EV_CAP_WIDE = 2 048) or its 8-bit
"after an insertion" counters -- the two limits fsv_asm_params.deep_sets lifts.  The events of a window grow as (overlaps on the window)
x (indel rate) x 375 x 2, so ~48 overlaps at 1.2 % indels pass 256 and ~100 at 10 % ONT error pass 2 048.  Every builder is seeded; reads
are synth._rand_seq / synth._add_errors, every other read reverse-complemented.  A builder returns (truths, reads): truths[i] is what
read i would be without errors, on its own strand."""
import functools

import numpy as np

from focalsv_amd import synth

INDELS = (0.0, 0.5, 0.5)      # substitution : insertion : deletion
HIFI_DEEP_RATE = 0.012       # 0.6 % insertions + 0.6 % deletions: a pair stays under the 3 % an overlap is accepted with
N_LOCUS_READS = 48
N_JUNCTION_READS = 120      # (72 fill the windows -- 695 events -- but no junction: see tests/test_gpu_deep_sets.py::test_junctions)


def _strand(b, i):
    return synth.revcomp(b) if i & 1 else b


def locus(n_reads, length, rate, seed, split=INDELS):
    """n_reads noisy copies of one stretch of `length` bases"""
    rng = np.random.default_rng(seed)
    ref = synth._rand_seq(rng, length)
    truth = ref.tobytes()
    reads = [_strand(synth._add_errors(rng, ref, rate, split).tobytes(), i) for i in range(n_reads)]
    return [_strand(truth, i) for i in range(n_reads)], reads


def tiling(n_reads, read_len, span, rate, seed, split=INDELS):
    """n_reads noisy reads of read_len bases starting at even steps over `span` bases"""
    rng = np.random.default_rng(seed)
    ref = synth._rand_seq(rng, span)
    starts = [round(i * (span - read_len) / (n_reads - 1)) for i in range(n_reads)]
    truths = [_strand(ref[s:s + read_len].tobytes(), i) for i, s in enumerate(starts)]
    reads = [_strand(synth._add_errors(rng, ref[s:s + read_len], rate, split).tobytes(), i) for i, s in enumerate(starts)]
    return truths, reads


@functools.lru_cache(maxsize=None)
def hifi_locus(n_reads=N_LOCUS_READS):
    """case 1 (48 reads) / case 2 (N_JUNCTION_READS): 1 500 bases, 1.2 % indels"""
    return locus(n_reads, 1500, HIFI_DEEP_RATE, 4801)


@functools.lru_cache(maxsize=None)
def hifi_tiling():
    """case 3: 150 reads x 3 000 over 9 kb (50 x), 1.2 % indels -- one contig"""
    return tiling(150, 3000, 9000, HIFI_DEEP_RATE, 4803)


@functools.lru_cache(maxsize=None)
def ont_locus():
    """case 4: 100 reads x 1 500 at 10 % error (1:1:1), for the ONT profile"""
    return locus(100, 1500, 0.10, 4804, (1 / 3, 1 / 3, 1 / 3))


@functools.lru_cache(maxsize=None)
def wide_counters():
    """case 5: 301 reads x 800.  Read 0 has one base deleted and the next one substituted, at a site outside any homopolymer; the other 300
    are error-free copies with alternating strands.  Seen from read 0 every one of them inserts a base and then shows a mismatch: 300 votes
    "after an insertion" for one base at one column, more than an 8-bit field holds"""
    rng = np.random.default_rng(4805)
    ref = synth._rand_seq(rng, 800)
    site = next(p for p in range(380, 420) if all(ref[q] != ref[q + 1] for q in range(p - 3, p + 4)))
    bad = ref.copy()
    bad[site + 1] = next(c for c in b"ACGT" if c not in (ref[site], ref[site + 1], ref[site + 2]))     # (no homopolymer made either)
    bad = np.delete(bad, site)
    truth = ref.tobytes()
    reads = [bad.tobytes()] + [_strand(truth, i) for i in range(1, 301)]
    return [truth] + [_strand(truth, i) for i in range(1, 301)], reads


@functools.lru_cache(maxsize=None)
def shallow(seed):
    """a set no window of which comes near a cap: 8 reads x 1 500, 1.2 % indels"""
    return locus(8, 1500, HIFI_DEEP_RATE, seed)


# ---- the oracle's answer for a case, computed once per process and shared by the tests that need it ------------------------------------
@functools.lru_cache(maxsize=None)
def oracle(case, n_rounds=3, n_reads=None):
    """case: "locus" (n_reads reads), "tiling", "ont", "wide", "shallow<seed>" -> (contigs, corrected reads, seconds) of O.assemble with the
    profile the case is for (the ONT case: the parameters tests/test_gpu_ont.py uses)"""
    import time
    from tests import oracle_lib as O
    reads = reads_of(case, n_reads)
    p = O.ont_params() if case == "ont" else O.default_params()
    p.n_rounds = n_rounds
    t0 = time.perf_counter()
    contigs, corrected = O.assemble(list(reads), p)
    return contigs, corrected, time.perf_counter() - t0


def build(case, n_reads=None):
    if case == "locus":
        return hifi_locus(n_reads or N_LOCUS_READS)
    if case.startswith("shallow"):
        return shallow(int(case[7:]))
    return {"tiling": hifi_tiling, "ont": ont_locus, "wide": wide_counters}[case]()


def reads_of(case, n_reads=None):
    return build(case, n_reads)[1]
