"""K1 on the GPU (both kernels: position-parallel and deque replay) vs minimizers minted from the reference's ha_sketch
and vs the CPU oracle on synthetic reads (tandem repeats, homopolymers, read ends inside runs), and -- further down -- on the cases
of tests/sketch_cases.py over the whole (w, k, HPC) range: every case, any batch shape, a reused context, junk in the padding bits,
sequences as long as the aligner's, the output capacity."""
import json
import os
import random

import numpy as np
import pytest

from focalsv_amd import _lib, synth
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with _lib.Context(0) as c:
        yield c


def _run(ctx, seqs, w, k, hpc, variant):
    words, off, lens = _lib.pack_reads(seqs)
    d = ctx.upload(words)
    try:
        return ctx.sketch_reads(d, off, lens, w, k, hpc, variant)
    finally:
        ctx.dev_free(d)


@pytest.mark.parametrize("variant", [0, 1])
def test_sketch_matches_reference_golden(ctx, golden_dir, variant):
    cases = [c for c in json.load(open(os.path.join(golden_dir, "sketch.json")))["cases"] if "N" not in c["seq"]]
    for (w, k, hpc) in sorted({(c["w"], c["k"], c["hpc"]) for c in cases}):
        mine = [c for c in cases if (c["w"], c["k"], c["hpc"]) == (w, k, hpc)]
        got = _run(ctx, [c["seq"] for c in mine], w, k, hpc, variant)
        for c, g in zip(mine, got):
            assert [[int(m["hash"]), int(m["pos"]), int(m["rev"]), int(m["span"])] for m in g] == c["mz"], (w, k, hpc, len(c["seq"]))


@pytest.mark.parametrize("variant", [0, 1])
def test_sketch_matches_oracle_on_reads(ctx, variant):
    r = synth.make_region(7)  # tandem-repeat region
    rng = random.Random(3)
    seqs = [x.decode() for x in r.reads[0][:24]]
    seqs += ["A" * 300 + "".join(rng.choice("ACGT") for _ in range(500)) + "C" * 400 + "ACGT" * 100, "ACGTTGCA" * 40, "ACG", "A" * 2000,
             "".join(rng.choice("ACGT") for _ in range(130)), ("".join(rng.choice("ACGT") for _ in range(37))) * 120]
    for (w, k, hpc) in ((51, 51, 1), (19, 19, 0), (51, 50, 1)):
        if variant == 0 and k % 2 == 0:
            continue  # the position-parallel kernel is for odd k; even k takes the replay kernel either way
        got = _run(ctx, seqs, w, k, hpc, variant)
        for s, g in zip(seqs, got):
            want = O.sketch(s, w, k, hpc)
            assert len(g) == len(want), (w, k, hpc, len(s), len(g), len(want))
            a = [(int(m["hash"]), int(m["pos"]), int(m["rev"]), int(m["span"])) for m in g]
            b = [(int(m["hash"]), int(m["pos"]), int(m["rev"]), int(m["span"])) for m in want]
            assert a == b


# ---- the whole (w, k, HPC) range: tests/sketch_cases.py against the oracle (which tests/test_oracle_sketch.py pins on the
# ---- reference's digests over the same grid).  Exact equality on (hash, pos, rev, span) and on the count, nothing left out.
from tests import sketch_cases as SC  # noqa: E402

FIELDS = ("hash", "pos", "rev", "span")
_cases, _want = {}, {}


def _grid_cases(gp):
    if gp not in _cases:
        _cases[gp] = SC.cases_for(*gp)
    return _cases[gp]


def _oracle(gp, c):
    key = gp + (c["kind"], c["tag"])
    if key not in _want:
        _want[key] = O.sketch(c["seq"], *gp)
    return _want[key]


def _diff(g, want):
    """None when equal, else a short description of the first difference"""
    if len(g) == len(want) and all(np.array_equal(g[f], want[f]) for f in FIELDS):
        return None
    n = min(len(g), len(want))
    bad = np.zeros(n, dtype=bool)
    for f in FIELDS:
        bad |= g[f][:n] != want[f][:n]
    i = int(np.argmax(bad)) if bad.any() else n
    row = lambda a: tuple(int(a[f][i]) for f in FIELDS) if i < len(a) else None
    return "n %d vs %d, first difference at #%d: got %s want %s" % (len(g), len(want), i, row(g), row(want))


def _same_bits(a, b):
    return len(a) == len(b) and all(np.array_equal(a[f], b[f]) for f in FIELDS)


def _refused(ctx, gp, variant):
    with pytest.raises(_lib.FsvError) as e:
        _run(ctx, ["ACGT" * 100], gp[0], gp[1], gp[2], variant)
    return e.value.code == _lib.EINVAL and "w <= 64 (replay kernel" in str(e.value)


@pytest.mark.parametrize("variant", [0, 1])
def test_grid_matches_oracle(ctx, variant):
    """3a: every case of every grid point, one fsv_sketch_reads call per (w, k, hpc).  Variant 0 takes the position-parallel
    kernel for odd k (all w up to 255) and the replay kernel for even k; variant 1 the replay kernel for every k.  The grid points
    left out are exactly those the library is documented to refuse -- the replay kernel with w > 64 -- and each is shown to be
    refused with that reason."""
    skipped, bad, n_reads, n_mz = [], [], 0, 0
    for gp in SC.GRID:
        w, k, hpc = gp
        why = SC.gpu_limit(w, k, variant)
        if why:
            assert _refused(ctx, gp, variant), gp
            skipped.append(gp)
            continue
        cases = _grid_cases(gp)
        got = _run(ctx, [c["seq"] for c in cases], w, k, hpc, variant)
        assert len(got) == len(cases)
        for c, g in zip(cases, got):
            d = _diff(g, _oracle(gp, c))
            if d:
                bad.append((gp, c["kind"], c["tag"], len(c["seq"]), d))
            n_mz += len(g)
        n_reads += len(cases)
    print("sketch grid, variant %d: %d grid points, %d reads, %d minimizers; refused (replay kernel, w > 64): %d grid points: %s"
          % (variant, len(SC.GRID) - len(skipped), n_reads, n_mz, len(skipped), skipped))
    assert not bad, (len(bad), len({b[0] for b in bad}), bad[:12])
    n_wide = sum(w > 64 for w in SC.WS)
    if variant == 0:
        assert all(k % 2 == 0 and w > 64 for (w, k, hpc) in skipped) and len(skipped) == n_wide * sum(k % 2 == 0 for k in SC.KS) * 2
        cov = SC.coverage([c for gp in SC.GRID if gp not in skipped for c in _grid_cases(gp)], O.sketch_info)
        print("coverage:", {n: sum(d[n] for d in cov.values()) for n in SC.COUNTS})
    else:
        assert all(w > 64 for (w, k, hpc) in skipped) and len(skipped) == n_wide * len(SC.KS) * 2


BATCH_POINTS = ((51, 51, 1, 0), (19, 19, 0, 0), (200, 19, 0, 0), (255, 63, 1, 0), (128, 3, 1, 0), (64, 62, 1, 0), (17, 20, 0, 0), (33, 31, 1, 1), (64, 19, 0, 1))


def test_batch_shape_does_not_matter(ctx):
    """3b: a read's result does not depend on its place in the batch or on its neighbours (bit planes and run ends of all reads
    share one scratch, k-mers are cut from words past a read's own plane): the same reads shuffled; interleaved with reads of
    other content; and alone -- one read of every grid point the library accepts, a call each."""
    rng = random.Random(11)
    for (w, k, hpc, variant) in BATCH_POINTS:
        seqs = [c["seq"] for c in _grid_cases((w, k, hpc))]
        plain = _run(ctx, seqs, w, k, hpc, variant)
        perm = list(range(len(seqs)))
        rng.shuffle(perm)
        got = _run(ctx, [seqs[i] for i in perm], w, k, hpc, variant)
        for j, i in enumerate(perm):
            assert _same_bits(got[j], plain[i]), ("shuffled", w, k, hpc, variant, i)
        other = [c["seq"] for c in _grid_cases((3, 15, 0))] + ["".join(rng.choices("ACGT", k=n)) for n in (1, 17, 700, 5000, 33)] + ["T" * 2000, "G"]
        mixed, where = [], []
        for i, s in enumerate(seqs):
            for _ in range(rng.randrange(3)):
                mixed.append(rng.choice(other))
            where.append(len(mixed))
            mixed.append(s)
        mixed.append(rng.choice(other))
        got = _run(ctx, mixed, w, k, hpc, variant)
        for i, j in enumerate(where):
            assert _same_bits(got[j], plain[i]), ("interleaved", w, k, hpc, variant, i)
    n_single = 0
    for n, gp in enumerate(SC.GRID):
        w, k, hpc = gp
        for variant in (0, 1):
            if SC.gpu_limit(w, k, variant) or (variant == 1 and n % 3):
                continue
            cases = _grid_cases(gp)
            i = (n * 7 + variant) % len(cases)
            got = _run(ctx, [cases[i]["seq"]], w, k, hpc, variant)
            assert _diff(got[0], _oracle(gp, cases[i])) is None, ("single", gp, variant, cases[i]["kind"], cases[i]["tag"])
            n_single += 1
    print("single-read calls:", n_single)
    assert n_single >= 200


@pytest.mark.parametrize("variant", [0, 1])
def test_context_reuse(variant):
    """3c: a large batch, then a few short reads with other parameters, then the large batch again on one context; each result
    equals that of a context that has run nothing else (stale bit planes, counts, scratch and buffer sizes)"""
    big_gp, small_gp = ((200, 19, 0), (3, 3, 1)) if variant == 0 else ((64, 51, 1), (2, 2, 0))
    rng = random.Random(5)
    big = [c["seq"] for c in _grid_cases(big_gp)] + ["".join(rng.choices("ACGT", k=60000))]
    small = ["ACGTTGCA", "A", "AC" * 20, "".join(rng.choices("ACGT", k=63)), "GGGGGGGGGGGGGGGGGT"]

    def fresh(seqs, gp):
        with _lib.Context(0) as c:
            return _run(c, seqs, gp[0], gp[1], gp[2], variant)

    want_big, want_small = fresh(big, big_gp), fresh(small, small_gp)
    for s, g in zip(big, want_big):
        assert _diff(g, O.sketch(s, *big_gp)) is None
    for s, g in zip(small, want_small):
        assert _diff(g, O.sketch(s, *small_gp)) is None
    with _lib.Context(0) as c:
        for step, (seqs, gp, want) in enumerate(((big, big_gp, want_big), (small, small_gp, want_small), (big, big_gp, want_big),
                                                 (small, big_gp, None), (small, small_gp, want_small))):
            got = _run(c, seqs, gp[0], gp[1], gp[2], variant)
            if want is None:
                want = [O.sketch(s, *gp) for s in seqs]
            for i, (g, x) in enumerate(zip(got, want)):
                assert _same_bits(g, x), (step, gp, i)


@pytest.mark.parametrize("fill", ["ones", "random"])
@pytest.mark.parametrize("variant", [0, 1])
def test_padding_bits_are_not_bases(ctx, variant, fill):
    """3d: the 2-bit fields of a read's last word beyond its length, and the words behind the last read, hold anything"""
    nprng = np.random.default_rng(17)
    for gp in ((51, 51, 1), (19, 19, 0), (3, 1, 1), (64, 63, 1), (16, 20, 1), (2, 2, 0)) + (((255, 19, 0), (129, 3, 1)) if variant == 0 else ()):
        w, k, hpc = gp
        cases = _grid_cases(gp)
        words, off, lens = _lib.pack_reads([c["seq"] for c in cases])
        n_store = int(off[-1])
        words = np.concatenate([words[:n_store], np.zeros(16, dtype=np.uint32)])
        junk = np.full(len(words), 0xffffffff, dtype=np.uint32) if fill == "ones" else nprng.integers(0, 1 << 32, len(words), dtype=np.uint64).astype(np.uint32)
        n_filled = 0
        for r, n in enumerate(lens):
            assert int(off[r + 1]) - int(off[r]) == (int(n) + 15) // 16
            used = int(n) % 16
            if used:
                last = int(off[r + 1]) - 1
                keep = np.uint32((1 << (2 * used)) - 1)
                words[last] = (words[last] & keep) | (junk[last] & ~keep)
                n_filled += 1
        words[n_store:] = junk[n_store:]
        assert n_filled > len(cases) // 2
        d = ctx.upload(words)
        try:
            got = ctx.sketch_reads(d, off, lens, w, k, hpc, variant)
        finally:
            ctx.dev_free(d)
        for c, g in zip(cases, got):
            assert _diff(g, _oracle(gp, c)) is None, (gp, variant, fill, c["kind"], c["tag"], _diff(g, _oracle(gp, c)))


def _tandem_rich(rng, n):
    out, total = [], 0
    while total < n:
        if rng.random() < 0.5:
            s = "".join(rng.choices("ACGT", k=rng.randrange(200, 6000)))
        else:
            u = "".join(rng.choices("ACGT", k=rng.choice((1, 2, 3, 7, 37, 100, 255, 300, 1000))))
            s = u * (rng.randrange(300, 9000) // len(u) + 1)
        out.append(s)
        total += len(s)
    return "".join(out)[:n]


def test_long_sequences(ctx):
    """3e: what the aligner sketches -- windows and contigs of up to 760 kb (hundreds of tiles) with w up to 255 -- through the
    position-parallel kernel, and a read above 131 072 bases through the replay kernel, whose words then stay in HBM"""
    rng = random.Random(23)
    seqs = ["".join(rng.choices("ACGT", k=300000)), "".join(rng.choices("ACGT", k=760000)), _tandem_rich(rng, 760000)]
    for gp in ((101, 19, 0), (255, 19, 0), (51, 51, 1)):
        got = _run(ctx, seqs, gp[0], gp[1], gp[2], 0)
        for s, g in zip(seqs, got):
            d = _diff(g, O.sketch(s, *gp))
            assert d is None, (gp, len(s), d)
    s140 = _tandem_rich(rng, 70000) + "".join(rng.choices("ACGT", k=70000))
    assert (len(s140) + 15) // 16 > 8192
    for gp in ((51, 50, 1), (64, 62, 0)):
        for variant in (0, 1):
            got = _run(ctx, [s140, "ACGT" * 50], gp[0], gp[1], gp[2], variant)
            d = _diff(got[0], O.sketch(s140, *gp))
            assert d is None, (gp, variant, d)


def test_capacity_one_short_is_ecap(ctx):
    """3f: an output buffer one entry short is FSV_ECAP, and the context goes on working"""
    for (w, k, hpc, variant) in ((51, 51, 1, 0), (19, 20, 0, 0), (200, 19, 0, 0), (31, 15, 1, 1)):
        gp = (w, k, hpc)
        cases = _grid_cases(gp)
        need = sum(len(_oracle(gp, c)) for c in cases)
        words, off, lens = _lib.pack_reads([c["seq"] for c in cases])
        d = ctx.upload(words)
        try:
            with pytest.raises(_lib.FsvError) as e:
                ctx.sketch_reads(d, off, lens, w, k, hpc, variant, out_cap=need - 1)
            assert e.value.code == _lib.ECAP
            got = ctx.sketch_reads(d, off, lens, w, k, hpc, variant, out_cap=need)
        finally:
            ctx.dev_free(d)
        assert sum(len(g) for g in got) == need
        for c, g in zip(cases, got):
            assert _diff(g, _oracle(gp, c)) is None, (gp, variant, c["kind"], c["tag"])


def _raw_sketch(ctx, store_dev, word_off, lens, w, k, hpc, cap=64):
    """the C entry fsv_sketch_reads itself, the caller's word_off handed through as it is -> (rc, message, per-read minimizers)"""
    word_off = np.ascontiguousarray(word_off, dtype=np.uint64)
    ss = np.asarray([0, len(lens)], dtype=np.uint32)
    rs = _lib.ReadSets(_lib.C.c_void_p(store_dev), _lib._ptr(word_off).value, _lib._ptr(lens).value, _lib._ptr(ss).value, len(lens), 1)
    out = np.zeros(cap, dtype=_lib.MZ_DTYPE)
    off = np.zeros(len(lens) + 1, dtype=np.uint64)
    rc = ctx._lib.fsv_sketch_reads(ctx._h, _lib.C.byref(rs), w, k, hpc, 0, _lib._ptr(out), cap, _lib._ptr(off))
    return rc, ctx._lib.fsv_last_error(ctx._h).decode(), [out[int(off[i]):int(off[i + 1])].copy() for i in range(len(lens))]


def test_word_off_beyond_32_bits_is_refused(ctx):
    """one read of 16 bases whose word_off array ends at 2^32: FSV_EUNSUP before anything is launched (no large allocation is needed: no word
    is read), as fsv_assemble_batch and fsv_kmer_table answer; the same read at word_off [0, 1] afterwards, on the same context, gives the
    oracle's sketch.  (Before the read-set checks were made one function the first call returned FSV_OK: 2^32 was cut to 32 bits, 0, and the
    kernel sketched through the offsets [0, 0] -- for this one read the right words by accident.)"""
    seq, (w, k, hpc) = "ACGTTGCATGGATCCA", (3, 5, 0)
    words, off, lens = _lib.pack_reads([seq])
    assert [int(x) for x in off] == [0, 1]
    want = O.sketch(seq, w, k, hpc)
    assert len(want) > 0
    d = ctx.upload(words)
    try:
        rc, msg, got = _raw_sketch(ctx, d, [0, 1 << 32], lens, w, k, hpc)
        print("word_off [0, 2^32]: rc", rc, repr(msg), [(int(m["hash"]), int(m["pos"])) for m in got[0]])
        assert rc == _lib.EUNSUP and msg == "store larger than 2^32 words; split the batch", (rc, msg)
        rc, msg, got = _raw_sketch(ctx, d, off, lens, w, k, hpc)
        print("word_off [0, 1]: rc", rc, [(int(m["hash"]), int(m["pos"])) for m in got[0]])
        assert rc == _lib.OK
    finally:
        ctx.dev_free(d)
    assert _diff(got[0], want) is None
