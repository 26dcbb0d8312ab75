"""fsv_sketch_reads_filtered on the GPU -- both sketch kernels with hifiasm's high-count k-mer filter compiled in (k_sketch.h, template
parameter FLT) behind the filter sets k_flt_build makes of the caller's lists -- against tests/sketch_filter_model.py (ha_sketch with
hf != 0, sketch.cpp:39-137), bit for bit and entry for entry in emission order.

One call per (w, k, hpc, variant): the same read sits in one read set per filter, so one launch sees the same read under different
filters, an empty set, and a set with an empty list between two with lists.  The filters come from the read's own w = 1 entries
(the model's slots): see _filters below for the list and what each one is there for."""
import ctypes as C
import random

import numpy as np
import pytest

from focalsv_amd import _lib
from tests import sketch_cases as SC
from tests import sketch_filter_model as FM

pytestmark = pytest.mark.gpu

FIELDS = ("hash", "pos", "rev", "span")
POINTS = ((51, 51, 1), (1, 51, 1), (19, 15, 0), (255, 21, 1), (10, 16, 0), (64, 32, 1))
# variant 0: the position-parallel kernel for odd k, the replay kernel for even k; variant 1: the replay kernel for odd k too (w <= 64)
RUNS = [(gp, v) for gp in POINTS for v in (0, 1) if v == 0 or (gp[1] % 2 == 1 and gp[0] <= 64)]
TILE = SC.TILE
MAXH = np.uint64(FM.MAX)


@pytest.fixture(scope="module")
def ctx():
    with _lib.Context(0) as c:
        yield c


def _run(ctx, seqs, set_start, filters, w, k, hpc, variant):
    words, off, lens = _lib.pack_reads(seqs)
    d = ctx.upload(words)
    try:
        return ctx.sketch_reads_filtered(d, off, lens, set_start, filters, w, k, hpc, variant)
    finally:
        ctx.dev_free(d)


def _diff(g, want):
    if len(g) == len(want) and all(np.array_equal(g[f], want[f]) for f in FIELDS):
        return None
    n = min(len(g), len(want))
    bad = np.zeros(n, dtype=bool)
    for f in FIELDS:
        bad |= g[f][:n] != want[f][:n]
    i = int(np.argmax(bad)) if bad.any() else n
    row = lambda a: tuple(int(a[f][i]) for f in FIELDS) if i < len(a) else None
    return "n %d vs %d, first difference at #%d: got %s want %s" % (len(g), len(want), i, row(g), row(want))


def _read(gp):
    """one read of ~2 300 entries (two tile boundaries of the position-parallel kernel; at most ~6 kb): random sequence, then a tandem
    repeat whose unit is shorter than the window (the same k-mer twice inside one window), then -- with compression -- a run of 300 bases
    (spans of 256 and more: dummies by themselves), then random sequence again"""
    w, k, hpc = gp
    rng = random.Random("sketch-filter/%d/%d/%d" % gp)
    u = max(2, min(7, w - 1))
    unit = SC._compressed(rng, u)
    if unit[0] == unit[-1]:
        unit = unit[:-1] + next(b for b in "ACGT" if b not in (unit[0], unit[-2]))
    tandem = unit * ((k + 3 * max(w, 8)) // u + 2)
    parts = [SC._compressed(rng, max(300, 2 * TILE + w + 120 - len(tandem) - 900)), tandem, SC._compressed(rng, 500)]
    for i in (1, 2):      # no run across a joint
        while parts[i][0] == parts[i - 1][-1]:
            parts[i - 1] = parts[i - 1][:-1]
    if not hpc:
        return "".join(parts) + "".join(rng.choices("ACGT", k=400))
    head = SC._expand(rng, "".join(parts), SC.SHORT_RUNS)
    tail = SC._expand(rng, SC._compressed(rng, 400), SC.SHORT_RUNS)
    long_base = next(b for b in "ACGT" if b not in (head[-1], tail[0]))
    return head + long_base * 300 + tail


def _filters(gp, seq, sl, rng):
    """name -> list of hashes, from the read's own slots (sl: FM.slots; slot s is entry s of the position-parallel kernel for odd k)"""
    w, k, hpc = gp
    x = sl["hash"]
    real = np.flatnonzero(x != MAXH)
    plain = FM.sketch(seq, w, k, hpc, None, sl)
    mz = FM.window(x.tolist(), w, k)      # the slots of the plain sketch's minimizers
    t0 = w + k - 2
    hs = lambda idx: [int(x[i]) for i in idx if 0 <= i < len(x) and x[i] != MAXH]
    out = {
        "nothing": [],
        # the minimum of the first full window (the start anomaly: the partial window's minimum and its copies)
        "first window minimum": [int(x[k - 1:t0 + 1].min())],
        "last minimizer": [int(plain["hash"][-1])],
        # w and w + 1 slots in a row: one window, then two, with no candidate at all
        "w slots": hs(range(700, 700 + w)),
        "w + 1 slots": hs(range(900, 900 + w + 1)),
        "first w + k - 1 slots": hs(range(0, w + k - 1)),
        "every entry": hs(range(len(x))),
        "not in the read": [12345, 2 ** 63 + 11, int(x[real[5]]) ^ 1],
        "every minimizer": [int(h) for h in plain["hash"]],
        # both sides of a tile boundary of the position-parallel kernel, and the ends of its 2 (w - 1) halo
        # (with the minimizers nearest to it on either side, so that the reported entries move)
        "tile boundary": hs([TILE - 1, TILE, 2 * TILE - 1, 2 * TILE, max(m for m in mz if m < TILE), min(m for m in mz if m >= TILE),
                             max(m for m in mz if m < 2 * TILE), min(m for m in mz if m >= 2 * TILE)]),
        "tile halo": hs([TILE - (w - 1), TILE - (w - 1) + 1, TILE - 2, TILE + 1, TILE + (w - 1) - 1, TILE + (w - 1), 2 * TILE - (w - 1), 2 * TILE + (w - 2)]),
        "a third of the entries": [int(x[i]) for i in rng.sample(list(real), len(real) // 3)],
    }
    # the replay kernel's lanes start at base len * lane / 64 and warm up over the w + k + 4 runs in front: entries inside that run-up
    warm = []
    for lane in (1, 17, 40, 63):
        c0 = len(seq) * lane // 64
        s0 = int(real[min(len(real) - 1, int(np.searchsorted(sl["pos"][real], c0)))])      # the first entry that ends in the lane's slice
        warm += hs([s0 - w - k, s0 - w, s0 - 3, s0 - 1, s0, s0 + 1])
    out["replay warm-up"] = warm
    if w > 1:   # (a window of one slot holds no k-mer twice)
        twice = next(int(x[i]) for i in real if i > k and (x[i + 1:i + w] == x[i]).any())
        assert sum(int(h) == twice for h in x) >= 2
        out["twice inside a window"] = [twice]
    if hpc:     # the slots beside the dummies a run of 300 makes
        gaps = [i for i in range(k, len(x)) if x[i] == MAXH]
        assert len(gaps) >= min(k, 5), "the long run makes dummies past the first k - 1 slots"
        out["beside a long run"] = hs([gaps[0] - 2, gaps[0] - 1, gaps[-1] + 1, gaps[-1] + 2])
    return out


_cache = {}


def _case(gp):
    """the batch of one grid point, with what the model says of it: (seqs, set_start, filters, want, names)"""
    if gp in _cache:
        return _cache[gp]
    w, k, hpc = gp
    rng = random.Random("sketch-filter-lists/%d/%d/%d" % gp)
    seq = _read(gp)
    assert len(seq) <= 6500
    sl = FM.slots(seq, k, hpc)
    assert len(sl) > 2 * TILE + w
    flt = _filters(gp, seq, sl, rng)
    seqs, set_start, filters, want, names = [], [0], [], [], []
    for n, (name, f) in enumerate(flt.items()):
        if n == 3:      # an empty set, with a list of its own
            set_start.append(len(seqs)); filters.append([int(sl["hash"][k])]); names.append("(empty set)")
        lst = list(f) + list(f[:3])      # duplicates, and no order
        rng.shuffle(lst)
        seqs.append(seq)
        want.append(FM.sketch(seq, w, k, hpc, f, sl))
        set_start.append(len(seqs)); filters.append(lst); names.append(name)
    # short reads -- no full window, and exactly one -- with their last minimum filtered, two to a set
    t0 = w + k - 2
    for n in (t0, t0 + 1):
        s = SC._entries_seq(rng, n, hpc, k)
        plain = FM.sketch(s, w, k, hpc)
        f = [int(plain["hash"][-1])] if len(plain) else []
        seqs += [s, s[: max(1, len(s) // 2)]]
        want += [FM.sketch(s, w, k, hpc, f), FM.sketch(s[: max(1, len(s) // 2)], w, k, hpc, f)]
        set_start.append(len(seqs)); filters.append(f); names.append("short %d" % n)
    _cache[gp] = (seqs, set_start, filters, want, names, flt)
    return _cache[gp]


@pytest.mark.parametrize("gp,variant", RUNS, ids=["w%d-k%d-hpc%d-v%d" % (gp + (v,)) for gp, v in RUNS])
def test_filtered_sketch_equals_model(ctx, gp, variant):
    w, k, hpc = gp
    seqs, set_start, filters, want, names, flt = _case(gp)
    assert len(seqs) <= 40
    got = _run(ctx, seqs, set_start, filters, w, k, hpc, variant)
    assert len(got) == len(seqs)
    bad = []
    for r, (g, x) in enumerate(zip(got, want)):
        d = _diff(g, x)
        if d:
            s = int(np.searchsorted(set_start, r, side="right")) - 1
            bad.append((names[s], r, d))
    assert not bad, bad[:6]
    # the filters do something: the filtered sketches differ from the plain one, "every entry" leaves nothing, absent hashes leave all
    by = {names[int(np.searchsorted(set_start, r, side="right")) - 1]: got[r] for r in range(len(flt))}
    plain = by["nothing"]
    assert len(by["every entry"]) == 0 and len(plain) > 0
    assert _diff(by["not in the read"], plain) is None
    for name in ("first window minimum", "last minimizer", "w slots", "every minimizer", "tile boundary"):
        assert _diff(by[name], plain) is not None, name
    assert not set(int(h) for h in by["every minimizer"]["hash"]) & set(int(h) for h in plain["hash"])


@pytest.mark.parametrize("n_keys", [1, 1023, 1024, 1025])
def test_filter_set_sizing(ctx, n_keys):
    """lists of 1, 1 023, 1 024 and 1 025 keys: a set of 2, 2 048, 2 048 and 4 096 slots -- every key found, nothing else"""
    gp = (51, 51, 1)
    seq = _read(gp)
    sl = FM.slots(seq, 51, 1)
    rng = random.Random(n_keys)
    real = sorted({int(h) for h in sl["hash"] if h != MAXH})
    own = rng.sample(real, min(n_keys, 600))
    pad = [rng.getrandbits(64) & ~1 for _ in range(n_keys - len(own))]      # (never UINT64_MAX)
    pad = [p for p in pad if p not in real]
    keys = own + pad
    assert len(keys) == n_keys
    for variant in (0, 1):
        got = _run(ctx, [seq, seq], [0, 1, 2], [keys, list(reversed(keys))], 51, 51, 1, variant)
        want = FM.sketch(seq, 51, 51, 1, own, sl)
        assert _diff(got[0], want) is None and _diff(got[1], want) is None, (n_keys, variant)


def test_probe_wraps_past_the_last_slot(ctx):
    """eight keys, so a set of 16 slots: a real minimizer of the read and four made-up keys that all start at slot 15, three made-up
    keys that start at slots 0, 1 and 2 -- whatever the order of arrival the claims run over the end of the set (slots 15, 0 .. 6), and
    the lookup of an absent hash that starts at slots 15 .. 3 walks the wrapped run to a free slot"""
    gp = (51, 51, 1)
    seq = _read(gp)
    sl = FM.slots(seq, 51, 1)
    plain = FM.sketch(seq, 51, 51, 1, None, sl)
    real = {int(h) for h in sl["hash"] if h != MAXH}
    key = next(int(h) for h in plain["hash"] if FM.start_slot(int(h), 16) == 15)
    rng = random.Random("probe wrap")

    def made_up(slot):
        while True:
            x = rng.getrandbits(64)
            if x != FM.MAX and x not in real and x not in keys and FM.start_slot(x, 16) == slot:
                return x
    keys = [key]
    for slot in (15, 15, 15, 15, 0, 1, 2):
        keys.append(made_up(slot))
    assert len(set(keys)) == 8 and [FM.start_slot(x, 16) for x in keys] == [15] * 5 + [0, 1, 2]
    assert not (set(keys[1:]) & real) and FM.MAX not in keys
    unfiltered = real - {key}
    assert any(FM.start_slot(h, 16) == 15 for h in unfiltered) and any(FM.start_slot(h, 16) == 0 for h in unfiltered)
    want = FM.sketch(seq, 51, 51, 1, [key], sl)
    assert _diff(want, plain) is not None
    shuffled = list(keys)
    rng.shuffle(shuffled)
    for variant in (0, 1):
        for lst in (keys, shuffled):
            got = _run(ctx, [seq, seq], [0, 1, 2], [lst, []], 51, 51, 1, variant)
            assert _diff(got[0], want) is None, (variant, _diff(got[0], want))
            assert _diff(got[1], plain) is None, (variant, _diff(got[1], plain))
            assert _diff(got[0], got[1]) is not None


@pytest.mark.parametrize("variant", [0, 1])
def test_no_lists_is_the_plain_sketch_and_contexts_are_reusable(variant):
    """NULL lists, lists that are all empty, and a context that ran with lists first: the bytes of fsv_sketch_reads"""
    gp = (51, 51, 1) if variant == 0 else (10, 16, 0)
    w, k, hpc = gp
    seqs, set_start, filters, want, names, flt = _case(gp)
    words, off, lens = _lib.pack_reads(seqs)
    with _lib.Context(0) as c:
        d = c.upload(words)
        try:
            with_lists = c.sketch_reads_filtered(d, off, lens, set_start, filters, w, k, hpc, variant)
            plain = c.sketch_reads(d, off, lens, w, k, hpc, variant)
            null = c.sketch_reads_filtered(d, off, lens, set_start, None, w, k, hpc, variant)
            empty = c.sketch_reads_filtered(d, off, lens, set_start, [[] for _ in filters], w, k, hpc, variant)
            again = c.sketch_reads_filtered(d, off, lens, set_start, filters, w, k, hpc, variant)
        finally:
            c.dev_free(d)
    for r in range(len(seqs)):
        assert _diff(with_lists[r], want[r]) is None and _diff(again[r], want[r]) is None, r
        for other in (null, empty):
            assert other[r].tobytes() == plain[r].tobytes(), r
    assert any(_diff(a, b) is not None for a, b in zip(with_lists, plain))


def test_refused_arguments(ctx):
    seq = "".join(random.Random(1).choices("ACGT", k=500))
    words, off, lens = _lib.pack_reads([seq, seq])
    d = ctx.upload(words)
    try:
        def code(fn):
            with pytest.raises(_lib.FsvError) as e:
                fn()
            return e.value.code, str(e.value)
        # UINT64_MAX is the dummy hash
        c, msg = code(lambda: ctx.sketch_reads_filtered(d, off, lens, [0, 1, 2], [[5], [7, FM.MAX]], 19, 19, 0, 0))
        assert c == _lib.EINVAL and "UINT64_MAX" in msg
        # the (w, k, variant) limits of fsv_sketch_reads
        c, msg = code(lambda: ctx.sketch_reads_filtered(d, off, lens, [0, 1, 2], [[5], [7]], 65, 19, 0, 1))
        assert c == _lib.EINVAL and "w <= 64 (replay kernel" in msg
        c, msg = code(lambda: ctx.sketch_reads_filtered(d, off, lens, [0, 1, 2], [[5], [7]], 256, 19, 0, 0))
        assert c == _lib.EINVAL and "w <= 255" in msg
        assert code(lambda: ctx.sketch_reads_filtered(d, off, lens, [0, 1, 2], [[5], [7]], 19, 64, 0, 0))[0] == _lib.EINVAL
        # set_start that does not span the reads; offsets that do not start at 0 or fall
        assert code(lambda: ctx.sketch_reads_filtered(d, off, lens, [0, 1, 1], [[5], [7]], 19, 19, 0, 0))[0] == _lib.EINVAL
        lib = _lib.load()
        woff, rl, ss = np.ascontiguousarray(off, dtype=np.uint64), np.ascontiguousarray(lens, dtype=np.int32), np.asarray([0, 1, 2], dtype=np.uint32)
        rs = _lib.ReadSets(C.c_void_p(d), woff.ctypes.data, rl.ctypes.data, ss.ctypes.data, 2, 2, None)
        out, o = np.zeros(2000, dtype=_lib.MZ_DTYPE), np.zeros(3, dtype=np.uint64)
        keys = np.asarray([5, 7, 9], dtype=np.uint64)
        for offs in ([1, 2, 3], [0, 2, 1]):
            fo = np.asarray(offs, dtype=np.uint64)
            rc = lib.fsv_sketch_reads_filtered(ctx._h, C.byref(rs), 19, 19, 0, 0, out.ctypes.data_as(C.c_void_p), 2000, o.ctypes.data_as(C.c_void_p),
                                               keys.ctypes.data_as(C.c_void_p), fo.ctypes.data_as(C.c_void_p))
            assert rc == _lib.EINVAL, offs
        rc = lib.fsv_sketch_reads_filtered(ctx._h, C.byref(rs), 19, 19, 0, 0, out.ctypes.data_as(C.c_void_p), 2000, o.ctypes.data_as(C.c_void_p),
                                           keys.ctypes.data_as(C.c_void_p), None)
        assert rc == _lib.EINVAL
        # and the context goes on working
        got = ctx.sketch_reads_filtered(d, off, lens, [0, 1, 2], [[], [5]], 19, 19, 0, 0)
        assert _diff(got[0], FM.sketch(seq, 19, 19, 0)) is None
    finally:
        ctx.dev_free(d)
