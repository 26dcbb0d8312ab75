"""fsv_read_index on the GPU: the per-read index as the chain kernels see it -- a read's unique minimizers sorted by hash, then the
same entries sorted by position -- against the oracle's sketch and unique filter (O.sketch -> O.unique_sorted), entry for entry, on
the reads of tests/long_list_cases.py.  With full_lists = 1 no list is cut and no warning is raised, whatever its length (k_uniq_long
beyond 4 096 entries); with 0 the long lists are cut and flagged as before and the short ones are the same bytes either way."""
import numpy as np
import pytest

from focalsv_amd import _lib
from tests import long_list_cases as L

pytestmark = pytest.mark.gpu
FIELDS = ("hash", "pos", "rev", "span")


@pytest.fixture(scope="module")
def ctx():
    with _lib.Context(0) as c:
        yield c


def index(ctx, reads, scheme, full_lists):
    words, off, lens = _lib.pack_reads(reads)
    d = ctx.upload(words)
    try:
        w, k, hpc = scheme
        return ctx.read_index(d, off, lens, w=w, k=k, hpc=hpc, full_lists=full_lists)
    finally:
        ctx.dev_free(d)


_want = {}


def wanted(scheme, read):
    """the oracle's index of a read: (by hash, by position), computed once per read"""
    if (scheme, read) not in _want:
        uq = L.lists(read, scheme)[1]
        _want[scheme, read] = (uq, uq[np.argsort(uq["pos"], kind="stable")])
    return _want[scheme, read]


def same(a, b):
    return len(a) == len(b) and all((a[f] == b[f]).all() for f in FIELDS)


@pytest.mark.parametrize("order", ["as listed", "reversed"])
@pytest.mark.parametrize("batch", ["dense", "ont", "w1"])
def test_full_lists_index_equals_the_oracle(ctx, batch, order):
    scheme, reads = L.index_batches()[batch]
    reads = list(reads) if order == "as listed" else list(reads)[::-1]
    got, warn = index(ctx, reads, scheme, 1)
    assert not warn.any(), warn
    for i, (r, g) in enumerate(zip(reads, got)):
        by_hash, by_pos = wanted(scheme, r)
        m = len(by_hash)
        assert len(g) == 2 * m, (batch, i, len(r), len(g), m)
        assert same(g[:m], by_hash), (batch, i, len(r), m, "by hash")
        assert same(g[m:], by_pos), (batch, i, len(r), m, "by position")


@pytest.mark.parametrize("order", ["as listed", "reversed"])
def test_small_classes_at_their_edges_equal_the_oracle(ctx, order):
    """raw lists of 0 .. 3, 255 .. 257, 511 .. 513 and 1 023 .. 1 025 entries and two tandem reads (L.small_index_batch): the boundary
    between k_uniq<1024> and k_uniq_walk<4096>, the padding of the sort network, the chunks of the compaction"""
    reads = list(L.small_index_batch())
    reads = reads if order == "as listed" else reads[::-1]
    got, warn = index(ctx, reads, L.DENSE, 1)
    cut, warn_cut = index(ctx, reads, L.DENSE, 0)
    assert not warn.any() and not warn_cut.any(), (warn, warn_cut)
    for i, (r, g) in enumerate(zip(reads, got)):
        by_hash, by_pos = wanted(L.DENSE, r)
        m = len(by_hash)
        assert len(g) == 2 * m, (i, len(r), len(g), m)
        assert same(g[:m], by_hash), (i, len(r), m, "by hash")
        assert same(g[m:], by_pos), (i, len(r), m, "by position")
        assert cut[i].tobytes() == g.tobytes(), (i, len(r), "full_lists 0 and 1")


@pytest.mark.parametrize("batch", ["dense", "ont"])
def test_default_cuts_and_flags_the_long_lists_only(ctx, batch):
    scheme, reads = L.index_batches()[batch]
    on, warn_on = index(ctx, list(reads), scheme, 1)
    off, warn_off = index(ctx, list(reads), scheme, 0)
    n_long = 0
    for i, r in enumerate(reads):
        raw = len(L.lists(r, scheme)[0])
        if raw > L.UQ_MAX:
            n_long += 1
            assert warn_off[i] & _lib.W_MZ_TRUNC and len(off[i]) <= 2 * L.UQ_MAX, (i, raw, warn_off[i], len(off[i]))
        else:
            assert warn_off[i] == 0 and off[i].tobytes() == on[i].tobytes(), (i, raw)
    assert n_long >= 3 and n_long < len(reads)


def test_full_lists_is_zero_or_one(ctx):
    scheme, reads = L.index_batches()["w1"]
    with pytest.raises(_lib.FsvError) as e:
        index(ctx, list(reads), scheme, 2)
    assert e.value.code == _lib.EINVAL
