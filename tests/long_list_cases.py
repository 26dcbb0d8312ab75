"""Reads and read pairs beyond the two caps that fsv_asm_params.full_lists lifts: minimizer lists above FSV_UQ_MAX = 4 096 entries (the
per-read index, k_uniq_long) and pairs with more anchors than the chaining tile holds (4 096 in the compact layout, 2 560 in the long
one: k_chain_spill), and reads at the edges of the two small classes of the index (SMALL_LISTS).  Everything is built from seeded random strings and classified through the oracle alone, which has neither cap;
tests/test_long_list_cases.py asserts the floors on a machine without a GPU, tests/test_gpu_read_index.py and
tests/test_gpu_long_chain.py compare the kernels with the oracle on the same reads.

Schemes as (w, k, hpc): DENSE (5, 15, 0) -- one minimizer per ~3 bases, so the caps sit at reads of 8-13 kb; ONT (15, 15, 0), the
noisy-read profiles' seeds; W1 (1, 15, 0), every k-mer."""
import random
from functools import lru_cache

from tests import chain_cases as CC
from tests import oracle_lib as O
from tests.kernel_cases import _bases, revcomp

SEED = 31
UQ_MAX = 4096
TILE_COMPACT, TILE_LONG = 4096, 2560      # FSV_AMAX_WIDE, FSV_AMAX_WIDE_LONG
DENSE, ONT, W1 = (5, 15, 0), (15, 15, 0), (1, 15, 0)
EDGE_LISTS = (4095, 4096, 4097)


@lru_cache(maxsize=None)
def genome():
    """the 40 kb random string most reads are cut from"""
    return _bases(random.Random(SEED), 40000)


def lists(seq, scheme):
    """(raw sketch, unique minimizers sorted by hash) of a read, from the oracle"""
    mz = O.sketch(seq, *scheme)
    return mz, O.unique_sorted(mz)


@lru_cache(maxsize=None)
def read_with_list(want, scheme=DENSE):
    """a substring of the genome whose raw and unique lists both have exactly `want` entries"""
    g = genome()
    per = 3.0 if scheme == DENSE else 8.0
    for start in range(0, 400, 7):
        n_bases = int(want * per)
        for _ in range(200):
            mz, uq = lists(g[start:start + n_bases], scheme)
            if len(mz) == want:
                break
            n_bases += max(1, int(abs(want - len(mz)) * per * 0.7)) * (1 if len(mz) < want else -1)
        if len(mz) == want and len(uq) == want:
            return g[start:start + n_bases]
    raise AssertionError("no read with a list of %d" % want)


def straddled(hashes, step):
    """multiples of `step` inside a run of equal values of the sorted array `hashes`"""
    return [i for i in range(step, len(hashes), step) if hashes[i - 1] == hashes[i]]


@lru_cache(maxsize=None)
def tandem_read():
    """random flanks around a tandem array of 8 copies of a 1 000-base unit: the array's ~330 hashes occur 8 times each, and in the
    hash-sorted raw list a run of equal hashes lies across a multiple of 1 024 and one across 4 096"""
    rng = random.Random(SEED + 1)
    for _ in range(200):
        r = _bases(rng, 3000) + _bases(rng, 1000) * 8 + _bases(rng, 3000)
        mz, _ = lists(r, DENSE)
        h = sorted(int(x) for x in mz["hash"])
        if len(h) > UQ_MAX and [i for i in straddled(h, 1024) if i % 4096] and straddled(h, 4096):
            return r
    raise AssertionError("no tandem read with runs across the tile boundaries")


@lru_cache(maxsize=None)
def homopolymer_read():
    """5 000 x A in front of 3 000 random bases: without HPC every A-mer is reported, so the raw list takes more than half of the
    read's slot (len + 64 entries) and the merge needs a buffer outside it; one run of equal hashes thousands of entries long"""
    return "A" * 5000 + _bases(random.Random(SEED + 2), 3000)


@lru_cache(maxsize=None)
def long_read():
    """66 kb: puts a batch into the chain kernels' long layout, and has a list above 16 384"""
    return _bases(random.Random(SEED + 3), 66000)


@lru_cache(maxsize=None)
def index_batches():
    """{name: (scheme, reads)}: long and short lists mixed (the tests also run every batch in reverse order)"""
    g = genome()
    rng = random.Random(SEED + 4)
    dense = [g[13000:14200]] + [read_with_list(n) for n in EDGE_LISTS] + [g[:14000], _bases(rng, 900), g[:30000], g[2000:40000], tandem_read(),
                                                                        homopolymer_read(), g[300:3000], long_read(), g[20000:26000]]
    ont = [g[:20000], _bases(rng, 40000), g[5000:6000], _bases(rng, 45000), read_with_list(4097, ONT), read_with_list(4096, ONT)]
    w1 = [_bases(rng, 5000), _bases(rng, 1000), _bases(rng, 4300)]
    return {"dense": (DENSE, dense), "ont": (ONT, ont), "w1": (W1, w1)}


# ---- the two small size classes of the index at their edges (k_uniq<1024>: raw lists up to 1 024 entries; k_uniq_walk<4096> above)
# raw list sizes: nothing, the first few, either side of the 256 threads of a block (one entry per thread, then two; the network padded
# to the next power of two), of 512 and of the boundary between the two classes
SMALL_LISTS = (0, 1, 2, 3, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025)


@lru_cache(maxsize=None)
def read_with_raw_list(want, scheme=DENSE):
    """a substring of the genome, 14 bases (k - 1: no k-mer at all) or more, whose raw list has exactly `want` entries; found as
    read_with_list finds its reads"""
    g = genome()
    per = 3.0
    for start in range(0, 400, 7):
        n_bases = max(14, int(want * per))
        for _ in range(200):
            mz, _uq = lists(g[start:start + n_bases], scheme)
            if len(mz) == want:
                return g[start:start + n_bases]
            n_bases = max(14, n_bases + max(1, int(abs(want - len(mz)) * per * 0.7)) * (1 if len(mz) < want else -1))
    raise AssertionError("no read with a raw list of %d" % want)


@lru_cache(maxsize=None)
def small_tandem_reads():
    """(a, b): random flanks around a tandem array.  a: four copies of a 200-base unit, a raw list of at most 1 024 entries; b: six
    copies of a 500-base unit, a raw list of 1 025 to 4 096 entries in which a run of equal hashes lies across a multiple of 256 of
    the hash-sorted list (a chunk boundary of the compaction whatever the list's length).  In both the array's hashes occur several
    times, so the unique list is shorter than the raw one"""
    rng = random.Random(SEED + 6)
    for _ in range(200):
        a = _bases(rng, 300) + _bases(rng, 200) * 4 + _bases(rng, 300)
        b = _bases(rng, 1500) + _bases(rng, 500) * 6 + _bases(rng, 1500)
        (ra, ua), (rb, ub) = lists(a, DENSE), lists(b, DENSE)
        if len(ua) < len(ra) <= 1024 < len(rb) <= UQ_MAX and len(ub) < len(rb) and straddled(sorted(int(x) for x in rb["hash"]), 256):
            return a, b
    raise AssertionError("no pair of small tandem reads")


@lru_cache(maxsize=None)
def small_index_batch():
    """the reads of SMALL_LISTS, then the two tandem reads (scheme DENSE)"""
    return tuple(read_with_raw_list(n) for n in SMALL_LISTS) + small_tandem_reads()


# ---- pairs by anchor count
def _total(x, y, p):
    i = dict(zip(O.CHAIN_INFO, (int(v) for v in O.set_overlaps([x, y], p, 0)["info"][0])))
    return i["nfwd"] + i["nrev"], i


def pair_with_anchors(x, yfull, want, p):
    """(x, y) with y = yfull without its last c bases, c chosen so that x and y share exactly `want` minimizers (both strands counted:
    what the tile must hold before the minority strand is dropped); yfull reaches x's end, so the count falls as c grows"""
    lo, hi = 0, len(yfull) - 200
    while lo < hi:                       # the smallest c with at most `want`
        mid = (lo + hi) // 2
        if _total(x, yfull[:len(yfull) - mid], p)[0] > want:
            lo = mid + 1
        else:
            hi = mid
    for c in sorted(range(max(0, lo - 40), lo + 40), key=lambda v: abs(v - lo)):
        if _total(x, yfull[:len(yfull) - c], p)[0] == want:
            return x, yfull[:len(yfull) - c]
    return None      # the count steps over `want` here (a minimizer that changes takes a neighbour with it)


def _with_errors(rng, s, at, rate):
    """s with substitutions and indels at `rate`, and from `at` on 800 bases of 2-base indels in turn every 19 bases and 1 500 bases at
    4 % (there the chain DP links past anchors, several times in a row)"""
    z = CC._zigzag(rng, s, at, at + 800, 19)
    return CC._mutate(rng, z[:at + 1000], rate) + CC._mutate(rng, z[at + 1000:at + 2500], 0.04) + CC._mutate(rng, z[at + 2500:], rate)


@lru_cache(maxsize=None)
def chain_sets():
    """read sets of the dense scheme as tests/chain_cases.py shapes them (dicts with name, reads).  Names: a<count>-<clean|err><+|->:
    a pair that shares exactly <count> minimizers -- at and one past either tile -- on one diagonal (clean) or with errors in y (_with_errors),
    y on either strand; big-...: above 8 192; long-...: pairs of the 66 kb read (they carry the long layout with them)"""
    p = CC.params("dense")
    g = genome()
    rng = random.Random(SEED + 5)
    sets = []
    add = lambda name, reads: sets.append({"name": name, "reads": list(reads), "sweep": False, "tags": {}})
    x = g[3000:25000]
    full = {"clean": g[:22500], "err": _with_errors(rng, g[:22500], 3200, 0.015)}
    for want in (TILE_LONG, TILE_LONG + 1, TILE_COMPACT, TILE_COMPACT + 1):
        for kind in ("clean", "err"):
            a, b = next(pr for pr in (pair_with_anchors(x[:len(x) - 37 * j], full[kind], want, p) for j in range(12)) if pr)
            add("a%d-%s+" % (want, kind), [a, b])
            add("a%d-%s-" % (want, kind), [revcomp(b), a])
    big = {"clean": g[:36000], "err": _with_errors(rng, g[:36000], 3200, 0.012)}
    for kind in ("clean", "err"):
        add("big-%s+" % kind, [g[3000:40000], big[kind]])
        add("big-%s-" % kind, [revcomp(big[kind]), g[3000:40000]])
    lr = long_read()
    add("long-clean", [lr, lr[30000:60000], revcomp(lr[1000:27000])])
    add("long-err", [_with_errors(rng, lr[20000:52000], 300, 0.012), lr])
    return tuple(sets)


def chain_info(s):
    """per unordered pair (q < t) of a set: (shared minimizers on both strands, the oracle's CHAIN_INFO counters, the two list sizes)"""
    p = CC.params("dense")
    e = O.set_overlaps(s["reads"], p, 0)
    n, out = len(s["reads"]), {}
    for q in range(n):
        for t in range(q + 1, n):
            i = dict(zip(O.CHAIN_INFO, (int(v) for v in e["info"][CC.upair_index(n, q, t)])))
            out[q, t] = (i["nfwd"] + i["nrev"], i, int(e["nuq"][q]), int(e["nuq"][t]))
    return out


def spilling_pairs(sets, tile):
    """global indices of the unordered pairs of a batch that share more minimizers than `tile`"""
    out, base = [], 0
    for s in sets:
        n = len(s["reads"])
        out += [base + CC.upair_index(n, q, t) for (q, t), v in chain_info(s).items() if v[0] > tile]
        base += n * (n - 1) // 2
    return out


@lru_cache(maxsize=None)
def noisy_main_set():
    """(stretch, reads as bytes): a 70 kb random stretch and 28 reads of it at 10 % error, 6 of them above 33 kb -- with the ONT seeds
    their lists pass 4 096 while two such reads share few minimizers"""
    import numpy as np
    from focalsv_amd import synth
    rng = np.random.default_rng(4711)
    hap = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 70000)]
    reads = synth._sample_reads(rng, hap, 4.0, 36000, 48000, 0.10) + synth._sample_reads(rng, hap, 4.0, 10000, 30000, 0.10)
    return hap.tobytes(), tuple(reads)


@lru_cache(maxsize=None)
def noisy_long_set():
    """an 80 kb stretch, two reads of 66-75 kb among reads of 10-30 kb at 10 % error: the long layout, end to end"""
    import numpy as np
    from focalsv_amd import synth
    rng = np.random.default_rng(4712)
    hap = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 80000)]
    reads = synth._sample_reads(rng, hap, 1.8, 66000, 75000, 0.10)[:2] + synth._sample_reads(rng, hap, 3.0, 10000, 30000, 0.10)
    return hap.tobytes(), tuple(reads)
