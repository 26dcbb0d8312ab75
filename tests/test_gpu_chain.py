"""k_chain on the GPU, stage level: the raw overlap records of every ordered pair slot and the window tasks, as fsv_asm_overlaps
returns them after one pass's sketch + index + chaining, against the oracle's orc_set_overlaps (collect_overlaps and the window grid
of align_overlaps, which tests/test_oracle_asm.py pins on hifiasm) on the read sets of tests/chain_cases.py.  Everything is integer and
compared exactly: q, t, x_s, x_e, y_s, y_e, score, n_chain, rev, valid, n_win per slot (a slot the oracle has no overlap for: valid 0);
x_start, x_len, y_start, k, y_rev, y_len, win per task."""
import numpy as np
import pytest

from focalsv_amd import _lib
from tests import chain_cases as CC
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu

FIELDS = ("q", "t", "x_s", "x_e", "y_s", "y_e", "score", "n_chain", "rev", "valid", "n_win")
TASK_FIELDS = ("x_start", "x_len", "y_start", "k", "y_rev", "y_len", "win")


@pytest.fixture(scope="module")
def ctx():
    with _lib.Context(0) as c:
        yield c


def run(ctx, scheme, sets, pass_, rechain=()):
    """one fsv_asm_overlaps call on the sets as one batch"""
    reads = [r for s in sets for r in s["reads"]]
    words, off, lens = _lib.pack_reads(reads)
    set_start = np.cumsum([0] + [len(s["reads"]) for s in sets]).astype(np.uint32)
    d = ctx.upload(words)
    try:
        ovl, pair_base, tasks, overflow, warn = ctx.asm_overlaps(d, off, lens, set_start, CC.lib_params(ctx.default_asm_params(), scheme), pass_, rechain)
    finally:
        ctx.dev_free(d)
    want_base = np.cumsum([0] + [len(s["reads"]) * (len(s["reads"]) - 1) for s in sets])
    assert [int(b) for b in pair_base] == [int(b) for b in want_base]
    return {"ovl": ovl, "pair_base": pair_base, "tasks": tasks, "overflow": overflow, "warn": warn, "set_start": set_start, "word_off": off, "lens": lens}


_runs = {}


def suite_run(ctx, scheme, pass_):
    if (scheme, pass_) not in _runs:
        _runs[scheme, pass_] = run(ctx, scheme, CC.sets_of(scheme), pass_)
    return _runs[scheme, pass_]


def _rec(o, fields):
    return {f: int(o[f]) for f in fields if f in o.dtype.names}


def wanted(e, n, n_win=True):
    """the oracle's overlaps of one set as {(q, t): record}"""
    return {(int(o["q"]), int(o["t"])): o for o in e["ovl"]}


def check_records(scheme, sets, got, want, skip=()):
    """every ordered slot of every set against the oracle's overlaps -> list of differences (strings)"""
    bad = []
    for si, (s, e) in enumerate(zip(sets, want)):
        n, base = len(s["reads"]), int(got["pair_base"][si])
        w = wanted(e, n)
        for q in range(n):
            for t in range(n):
                if q == t or (s["name"], min(q, t), max(q, t)) in skip:
                    continue
                g = got["ovl"][base + CC.slot_index(n, q, t)]
                o = w.get((q, t))
                if o is None:
                    if int(g["valid"]) != 0:
                        bad.append("%s: the oracle has no overlap, the kernel wrote %s" % (CC.describe(scheme, s["name"], q, t), _rec(g, FIELDS)))
                    continue
                exp = _rec(o, FIELDS)
                exp["valid"] = 1
                diff = [f for f in FIELDS if int(g[f]) != exp[f]]
                if diff:
                    bad.append("%s: fields %s differ: kernel %s oracle %s" % (CC.describe(scheme, s["name"], q, t), diff, _rec(g, FIELDS), exp))
    return bad


def check_tasks(scheme, sets, got, want):
    """the window tasks of every valid slot against the oracle's window grid; the ranges tile [0, n_tasks)"""
    bad, ranges = [], []
    tasks = got["tasks"]
    for si, (s, e) in enumerate(zip(sets, want)):
        n, base, r0 = len(s["reads"]), int(got["pair_base"][si]), int(got["set_start"][si])
        w = wanted(e, n)
        for q in range(n):
            for t in range(n):
                if q == t:
                    continue
                slot = base + CC.slot_index(n, q, t)
                g = got["ovl"][slot]
                if not int(g["valid"]):
                    continue
                f, nw = int(g["first_win"]), int(g["n_win"])
                ranges.append((f, nw))
                o = w.get((q, t))
                if o is None or nw != int(o["n_win"]) or f < 0 or f + nw > len(tasks):
                    bad.append("%s: tasks [%d, %d) of %d" % (CC.describe(scheme, s["name"], q, t), f, f + nw, len(tasks)))
                    continue
                for j in range(nw):
                    tk, ow = tasks[f + j], e["win"][int(o["first_win"]) + j]
                    exp = {"x_start": int(ow["x_start"]), "x_len": int(ow["x_len"]), "y_start": int(ow["y_start"]), "k": int(ow["k"]), "y_rev": int(o["rev"]),
                           "y_len": len(s["reads"][t]), "win": j, "ovl": slot, "x_word": int(got["word_off"][r0 + q]), "y_word": int(got["word_off"][r0 + t])}
                    have = {f2: int(tk[f2]) for f2 in exp}
                    if have != exp:
                        bad.append("%s: window %d of %d: kernel %s oracle %s" % (CC.describe(scheme, s["name"], q, t), j, nw, have, exp))
    ranges.sort()
    at = 0
    for f, nw in ranges:
        if f != at:
            bad.append("task ranges do not tile: a range starts at %d, the one before ends at %d" % (f, at))
            break
        at += nw
    if at != len(tasks):
        bad.append("task ranges cover %d of %d tasks" % (at, len(tasks)))
    return bad


def report(bad):
    assert not bad, "%d differences; the first:\n%s" % (len(bad), "\n".join(bad[:8]))


@pytest.mark.parametrize("scheme", CC.SCHEMES)
@pytest.mark.parametrize("pass_", [0, 1])
def test_overlaps_match_oracle(ctx, pass_, scheme):
    """every ordered slot of every pair, both directions (the mirrored slot is the kernel's own arithmetic), in a correction-round pass
    and in the final pass"""
    got = suite_run(ctx, scheme, pass_)
    assert not (got["warn"] & _lib.W_ANCHOR_TRUNC).any() and not (got["warn"] & _lib.W_MZ_TRUNC).any()
    report(check_records(scheme, CC.sets_of(scheme), got, CC.expected(scheme, pass_)))
    if pass_ == 1:
        assert len(got["tasks"]) == 0 and not got["ovl"]["n_win"].any()


@pytest.mark.parametrize("scheme", CC.SCHEMES)
def test_window_tasks_match_oracle(ctx, scheme):
    """pass 0: the tasks of either direction of every overlap -- the window grid, the chain's diagonal at each window start (the
    mirrored side searches the chain by the target coordinate, backwards on the reverse strand), the thresholds, the store offsets"""
    got = suite_run(ctx, scheme, 0)
    assert got["overflow"] == 0
    report(check_tasks(scheme, CC.sets_of(scheme), got, CC.expected(scheme, 0)))
    assert len(got["tasks"]) == sum(len(e["win"]) for e in CC.expected(scheme, 0)) > 0


def _upairs(sets, pair_base):
    """global index of every unordered pair of the batch -> (set index, q, t)"""
    out = {}
    for si, s in enumerate(sets):
        n = len(s["reads"])
        for q in range(n):
            for t in range(q + 1, n):
                out[int(pair_base[si]) // 2 + CC.upair_index(n, q, t)] = (si, q, t)
    return out


@pytest.mark.parametrize("scheme", ["dense", "hifi", "ont"])
def test_rechain_from_both_sides(ctx, scheme):
    """pass 2: either slot of a listed pair is the oracle's chain from that slot's own side with bw_rechain; the slots of the other
    pairs keep their final-pass records bit for bit.  Lists: none, one pair, every pair."""
    sets = CC.sets_of(scheme)
    first = suite_run(ctx, scheme, 1)
    want1, want2 = CC.expected(scheme, 1), CC.expected(scheme, 2)
    up = _upairs(sets, first["pair_base"])
    assert sorted(up) == list(range(len(up)))
    # one pair: the first whose anchors leave the diagonal and that overlaps at the re-chain's bandwidth
    multi = [(pr["set"], pr["q"], pr["t"]) for pr in CC.classified(scheme) if "several diagonals, bw %d" % CC.params(scheme).bw_ec in pr["classes"]]
    one = next(i for i, v in sorted(up.items()) if v in multi and (v[1], v[2]) in wanted(want2[v[0]], 0))
    for lst in ([], [one], sorted(up, reverse=True)):
        got = run(ctx, scheme, sets, 2, lst)
        listed = {up[i] for i in lst}
        bad = []
        for si, s in enumerate(sets):
            n, base = len(s["reads"]), int(got["pair_base"][si])
            for q in range(n):
                for t in range(n):
                    if q == t:
                        continue
                    slot = base + CC.slot_index(n, q, t)
                    if (si, min(q, t), max(q, t)) not in listed and got["ovl"][slot].tobytes() != first["ovl"][slot].tobytes():
                        bad.append("%s: not listed, but its record changed: %s, was %s" % (CC.describe(scheme, s["name"], q, t), got["ovl"][slot], first["ovl"][slot]))
        mixed = [{"ovl": np.array([o for o in w2["ovl"] if (si, min(int(o["q"]), int(o["t"])), max(int(o["q"]), int(o["t"]))) in listed] +
                                  [o for o in w1["ovl"] if (si, min(int(o["q"]), int(o["t"])), max(int(o["q"]), int(o["t"]))) not in listed], dtype=O.OVL_DTYPE)}
                 for si, (w1, w2) in enumerate(zip(want1, want2))]
        report(bad + check_records(scheme, sets, got, mixed))
        assert len(got["tasks"]) == 0


def _per_set(got, si, n):
    """the records and tasks of one set of a run, free of where the set stands in its batch"""
    base, r0 = int(got["pair_base"][si]), int(got["set_start"][si])
    out = []
    for slot in range(base, base + n * (n - 1)):
        g = got["ovl"][slot]
        rec = tuple(int(g[f]) for f in FIELDS)
        tk = got["tasks"][int(g["first_win"]): int(g["first_win"]) + int(g["n_win"])] if int(g["valid"]) else got["tasks"][:0]
        out.append((rec, [tuple(int(x[f]) for f in TASK_FIELDS) + (int(x["ovl"]) - base, int(x["x_word"]) - int(got["word_off"][r0]), int(x["y_word"]) - int(got["word_off"][r0]))
                          for x in tk]))
    return out


def test_long_layout_gives_the_same_records(ctx):
    """a read of 65 536 bases in a set of its own has no pairs, but puts the whole batch into the long LDS layout (64-bit keys, 32-bit
    DP arrays, staged target records) and the wide list into the 2 560 tile: records and tasks of the other sets stay what they were"""
    sets = CC.sets_of("dense")
    filler = CC.truncation_set()[1]
    short = suite_run(ctx, "dense", 0)
    for pass_ in (0, 1):
        got = run(ctx, "dense", sets[:3] + [filler] + sets[3:], pass_)
        order = sets[:3] + [filler] + sets[3:]
        want = CC.expected("dense", pass_)
        want = want[:3] + [{"ovl": np.zeros(0, dtype=O.OVL_DTYPE), "win": np.zeros(0, dtype=O.GWIN_DTYPE)}] + want[3:]
        report(check_records("dense", order, got, want) + (check_tasks("dense", order, got, want) if pass_ == 0 else []))
        assert got["overflow"] == 0
        r_fill = int(got["set_start"][3])
        assert not np.delete(got["warn"], r_fill).any()
        if pass_ == 0:
            for si, s in enumerate(sets):
                assert _per_set(got, si if si < 3 else si + 1, len(s["reads"])) == _per_set(short, si, len(s["reads"])), s["name"]


def test_batch_shape_does_not_matter(ctx):
    """sets of 1, 2, 3, 9 and 12 reads (0, 1, 3, 36, 66 pairs: chunks of 8 pairs cross query rows and set boundaries) alone, together and in
    other orders, with batch totals of 0, 1 and 7 pairs mod 8: per set, the same records and tasks"""
    by = {n: CC.set_named("dense", n) for n in ("single", "swap0+", "ins40-0-", "clean", "locus", "regimes")}
    assert [len(by[n]["reads"]) for n in ("single", "swap0+", "ins40-0-", "clean", "locus", "regimes")] == [1, 2, 2, 3, 9, 12]
    full = CC.sets_of("dense")
    exp = {s["name"]: e for s, e in zip(full, CC.expected("dense", 0))}
    alone = {}
    for n, s in by.items():
        got = run(ctx, "dense", [s], 0)
        report(check_records("dense", [s], got, [exp[n]]) + check_tasks("dense", [s], got, [exp[n]]))
        alone[n] = _per_set(got, 0, len(s["reads"]))
    for names, mod8 in ((("regimes", "locus", "clean", "single"), 1), (("single", "swap0+", "regimes", "locus", "ins40-0-"), 0),
                        (("locus", "ins40-0-", "single", "regimes"), 7), (("clean", "single", "single", "swap0+", "locus"), 0)):
        sets = [by[n] for n in names]
        got = run(ctx, "dense", sets, 0)
        assert (len(got["ovl"]) // 2) % 8 == mod8
        assert got["overflow"] == 0 and not got["warn"].any()
        report(check_tasks("dense", sets, got, [exp[n] for n in names]))
        for si, n in enumerate(names):
            assert _per_set(got, si, len(by[n]["reads"])) == alone[n], (names, n)
    whole = suite_run(ctx, "dense", 0)
    for n in by:
        si = [s["name"] for s in full].index(n)
        assert _per_set(whole, si, len(by[n]["reads"])) == alone[n], n


def test_anchor_truncation_is_flagged(ctx):
    """long layout: a pair whose lists both lie in (2 560, 4 096] and which shares more anchors than the 2 560 tile holds sets
    FSV_W_ANCHOR_TRUNC on its query read and on no other; every other pair of the batch is what the oracle says (the truncated pair's
    record is not compared: the oracle has no tile)"""
    trunc, filler = CC.truncation_set()
    p = CC.params("dense")
    e = O.set_overlaps(trunc["reads"], p, 0)
    info = dict(zip(O.CHAIN_INFO, e["info"][0]))
    assert 2560 < e["nuq"][0] <= CC.UQ_MAX and 2560 < e["nuq"][1] <= CC.UQ_MAX and info["anchors"] > 2560 and e["nuq"][2] <= 1024
    sets = [CC.set_named("dense", "locus"), trunc, CC.set_named("dense", "clean"), filler]
    want = [CC.expected("dense", 0)[[s["name"] for s in CC.sets_of("dense")].index("locus")], e,
            CC.expected("dense", 0)[[s["name"] for s in CC.sets_of("dense")].index("clean")], {"ovl": np.zeros(0, dtype=O.OVL_DTYPE), "win": np.zeros(0, dtype=O.GWIN_DTYPE)}]
    got = run(ctx, "dense", sets, 0)
    flagged = np.flatnonzero(got["warn"] & _lib.W_ANCHOR_TRUNC)
    assert list(flagged) == [int(got["set_start"][1])], flagged
    assert got["overflow"] == 0
    report(check_records("dense", sets, got, want, skip={("truncated", 0, 1)}))
    # without the filler the batch is in the compact layout, whose wide tile (4 096) holds the pair: no flag, and the oracle's record
    got = run(ctx, "dense", sets[:3], 0)
    assert not got["warn"].any()
    report(check_records("dense", sets[:3], got, want[:3]) + check_tasks("dense", sets[:3], got, want[:3]))


def test_context_reuse():
    """a large batch, then small ones of every pass on the same context: the small ones' results equal those of a context that has run
    nothing else (a stale wide list, counters, warnings, pair tables or re-chain list would show)"""
    small = [CC.set_named("dense", "clean-b"), CC.set_named("dense", "zigzag17-0+")]
    trunc, filler = CC.truncation_set()
    steps = [(0, ()), (1, ()), (2, (0, 3, 6)), (0, ())]
    with _lib.Context(0) as c:
        fresh = [run(c, "dense", small, p, l) for p, l in steps[:1]]
    for p, l in steps[1:]:
        with _lib.Context(0) as c:
            fresh.append(run(c, "dense", small, p, l))
    with _lib.Context(0) as c:
        run(c, "dense", CC.sets_of("dense") + [trunc, filler], 0)       # wide list in use, a truncation warning, the long layout
        run(c, "dense", CC.sets_of("dense"), 2, list(range(40)))
        for (p, l), want in zip(steps, fresh):
            got = run(c, "dense", small, p, l)
            assert got["ovl"].tobytes() == want["ovl"].tobytes() and got["overflow"] == want["overflow"] == 0, (p, l)
            assert got["warn"].tobytes() == want["warn"].tobytes() and not got["warn"].any()
            assert [_per_set(got, si, len(s["reads"])) for si, s in enumerate(small)] == [_per_set(want, si, len(s["reads"])) for si, s in enumerate(small)], (p, l)
        run(c, "ont", CC.sets_of("ont"), 0)                              # the 4 096 tile, no wide list
        got = run(c, "dense", small, 0)
        assert [_per_set(got, si, len(s["reads"])) for si, s in enumerate(small)] == [_per_set(fresh[0], si, len(s["reads"])) for si, s in enumerate(small)]
    report(check_records("dense", small, fresh[0], [CC.expected("dense", 0)[[s["name"] for s in CC.sets_of("dense")].index(x["name"])] for x in small]))
