"""Chaining beyond the tile on the GPU: fsv_asm_overlaps with full_lists = 1 on the pairs of tests/long_list_cases.py -- more shared
minimizers than the 4 096 (compact layout) or 2 560 (long layout) anchors a tile holds, so k_chain_spill chains them in HBM -- against
the oracle's orc_set_overlaps, which has no tile: every record, every window task, no truncation flag.  Pass 0, the final pass, and
the gapped re-chain of the over-tile pairs from either read's side."""
import numpy as np
import pytest

from focalsv_amd import _lib
from tests import chain_cases as CC
from tests import long_list_cases as L
from tests import oracle_lib as O
from tests.test_gpu_chain import check_records, check_tasks, report
from tests.test_gpu_chain import run as run_default

pytestmark = pytest.mark.gpu
NO_PAIRS = {"ovl": np.zeros(0, dtype=O.OVL_DTYPE), "win": np.zeros(0, dtype=O.GWIN_DTYPE)}


@pytest.fixture(scope="module")
def ctx():
    with _lib.Context(0) as c:
        yield c


def run(ctx, scheme, sets, pass_, rechain=(), full_lists=1, w=None):
    """tests.test_gpu_chain.run with the option set (w: another minimizer window than the scheme's)"""
    reads = [r for s in sets for r in s["reads"]]
    words, off, lens = _lib.pack_reads(reads)
    set_start = np.cumsum([0] + [len(s["reads"]) for s in sets]).astype(np.uint32)
    p = CC.lib_params(ctx.default_asm_params(), scheme)
    p.full_lists = full_lists
    if w is not None:
        p.w = w
    d = ctx.upload(words)
    try:
        ovl, pair_base, tasks, overflow, warn = ctx.asm_overlaps(d, off, lens, set_start, p, pass_, rechain)
    finally:
        ctx.dev_free(d)
    return {"ovl": ovl, "pair_base": pair_base, "tasks": tasks, "overflow": overflow, "warn": warn, "set_start": set_start, "word_off": off, "lens": lens}


_want = {}


def expected(scheme, sets, pass_):
    """the oracle's result per set, computed once per (set, pass) and shared"""
    p = CC.params(scheme)
    out = []
    for s in sets:
        if len(s["reads"]) < 2:
            out.append(NO_PAIRS)
            continue
        if (scheme, s["name"], pass_) not in _want:
            _want[scheme, s["name"], pass_] = O.set_overlaps(s["reads"], p, pass_)
        out.append(_want[scheme, s["name"], pass_])
    return out


def batches():
    """compact layout: every read below 65 536 bases; long layout: the sets with the 66 kb read, and the others behind the filler"""
    sets = list(L.chain_sets())
    compact = [s for s in sets if max(len(r) for r in s["reads"]) < 65536]
    long_ = [s for s in sets if s not in compact] + [CC.truncation_set()[1]] + [s for s in compact if not s["name"].startswith("big")]
    return {"compact": compact, "long": long_}


@pytest.mark.parametrize("layout", ["compact", "long"])
def test_pass0_records_and_tasks(ctx, layout):
    sets = batches()[layout]
    assert L.spilling_pairs(sets, L.TILE_COMPACT if layout == "compact" else L.TILE_LONG)
    got = run(ctx, "dense", sets, 0)
    assert not got["warn"].any() and got["overflow"] == 0, np.flatnonzero(got["warn"])
    want = expected("dense", sets, 0)
    report(check_records("dense", sets, got, want) + check_tasks("dense", sets, got, want))
    assert len(got["tasks"]) == sum(len(e["win"]) for e in want) > 0


@pytest.mark.parametrize("layout", ["compact", "long"])
def test_final_pass_and_rechain_of_the_over_tile_pairs(ctx, layout):
    sets = batches()[layout]
    first = run(ctx, "dense", sets, 1)
    assert not first["warn"].any()
    want1, want2 = expected("dense", sets, 1), expected("dense", sets, 2)
    report(check_records("dense", sets, first, want1))
    listed = L.spilling_pairs(sets, L.TILE_COMPACT if layout == "compact" else L.TILE_LONG)
    got = run(ctx, "dense", sets, 2, listed)
    assert not got["warn"].any() and len(got["tasks"]) == 0
    base, mixed = 0, []
    for s, w1, w2 in zip(sets, want1, want2):
        n = len(s["reads"])
        if n < 2:
            mixed.append(NO_PAIRS)
            continue
        is_listed = lambda o: base + CC.upair_index(n, min(int(o["q"]), int(o["t"])), max(int(o["q"]), int(o["t"]))) in listed
        mixed.append({"ovl": np.array([o for o in w2["ovl"] if is_listed(o)] + [o for o in w1["ovl"] if not is_listed(o)], dtype=O.OVL_DTYPE)})
        base += n * (n - 1) // 2
    report(check_records("dense", sets, got, mixed))


def test_truncation_set_with_and_without_the_option(ctx):
    """CC.truncation_set(): with the option the pair that the long layout's tile cuts equals the oracle and nothing is flagged; without
    it the query read is flagged as before (the control)"""
    trunc, filler = CC.truncation_set()
    sets = [trunc, filler]
    want = [O.set_overlaps(trunc["reads"], CC.params("dense"), 0), NO_PAIRS]
    got = run(ctx, "dense", sets, 0)
    assert not got["warn"].any() and got["overflow"] == 0
    report(check_records("dense", sets, got, want) + check_tasks("dense", sets, got, want))
    off = run(ctx, "dense", sets, 0, full_lists=0)
    assert list(np.flatnonzero(off["warn"] & _lib.W_ANCHOR_TRUNC)) == [0]


def test_long_lists_with_few_anchors(ctx):
    """ONT seeds, 10 % error: the four longest reads' lists pass 4 096 while no pair shares a tile's worth of minimizers -- the index
    class alone, no spill; with the option off the same reads are flagged FSV_W_MZ_TRUNC"""
    reads = [r.decode() for r in sorted(L.noisy_main_set()[1], key=len)[-4:]]
    sets = [{"name": "noisy-long-lists", "reads": reads, "sweep": False, "tags": {}}]
    got = run(ctx, "ont", sets, 0)
    assert not got["warn"].any() and got["overflow"] == 0
    want = expected("ont", sets, 0)
    assert min(int(n) for n in want[0]["nuq"]) > L.UQ_MAX
    report(check_records("ont", sets, got, want) + check_tasks("ont", sets, got, want))
    off = run(ctx, "ont", sets, 0, full_lists=0)
    assert (off["warn"] & _lib.W_MZ_TRUNC).all()


def test_window_of_one_through_the_overlap_stage(ctx):
    """w = 1 (every k-mer a minimizer): the unique lists take more than half a slot of len + 64 entries, so with the option the assembly
    sizes the slots for both copies of the index (mz_slots) -- the same slots the fsv_read_index hook uses.  Reads of 5 kb: lists above
    4 096, and a pair beyond the compact layout's tile"""
    g = L.genome()
    s = {"name": "w1", "reads": [g[:5000], g[200:5200], L.revcomp(g[2500:7400])], "sweep": False, "tags": {}}
    p = CC.params("dense")
    p.w = 1
    for pass_ in (0, 1):
        want = [O.set_overlaps(s["reads"], p, pass_)]
        if pass_ == 0:
            info = dict(zip(O.CHAIN_INFO, (int(v) for v in want[0]["info"][0])))
            assert min(int(n) for n in want[0]["nuq"]) > L.UQ_MAX and info["nfwd"] + info["nrev"] > L.TILE_COMPACT
        got = run(ctx, "dense", [s], pass_, w=1)
        assert not got["warn"].any() and got["overflow"] == 0, got["warn"]
        report(check_records("dense", [s], got, want) + (check_tasks("dense", [s], got, want) if pass_ == 0 else []))


def test_context_reuse_after_a_spilling_batch():
    """a spilling batch, then a small one on the same context: the small one's result is that of a fresh context (a stale spill list or
    counter would show)"""
    small = [CC.set_named("dense", "clean-b")]
    with _lib.Context(0) as c:
        fresh = [run(c, "dense", small, p, l) for p, l in ((0, ()), (2, (0, 3)))]
    with _lib.Context(0) as c:
        run(c, "dense", batches()["long"], 0)
        run(c, "dense", batches()["compact"][:6], 2, L.spilling_pairs(batches()["compact"][:6], L.TILE_LONG))
        for (p, l), want in zip(((0, ()), (2, (0, 3))), fresh):
            got = run(c, "dense", small, p, l)
            assert got["ovl"].tobytes() == want["ovl"].tobytes() and got["tasks"].tobytes() == want["tasks"].tobytes() and not got["warn"].any(), p
        plain = run_default(c, "dense", small, 0)
        assert plain["ovl"].tobytes() == fresh[0]["ovl"].tobytes()
    report(check_records("dense", small, fresh[0], [CC.expected("dense", 0)[[s["name"] for s in CC.sets_of("dense")].index("clean-b")]]))
