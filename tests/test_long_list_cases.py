"""Floors of tests/long_list_cases.py, through the oracle alone (no GPU): no class the GPU tests rely on is silently empty."""
from tests import chain_cases as CC
from tests import long_list_cases as L
from tests import oracle_lib as O


def _sizes(scheme, reads):
    return [tuple(len(x) for x in L.lists(r, scheme)) for r in reads]


def test_list_sizes_cover_the_cap_and_its_neighbours():
    scheme, reads = L.index_batches()["dense"]
    sizes = _sizes(scheme, reads)
    for n in L.EDGE_LISTS:
        assert (n, n) in sizes, (n, sizes)
    uq = [u for _, u in sizes]
    assert any(L.UQ_MAX < u <= 2 * L.UQ_MAX for u in uq) and any(2 * L.UQ_MAX < u <= 4 * L.UQ_MAX for u in uq) and any(u > 4 * L.UQ_MAX for u in uq), uq
    assert any(u <= 1024 for u in uq) and any(1024 < u <= L.UQ_MAX for u in uq), uq       # the other two size classes, in the same batch
    scheme, reads = L.index_batches()["ont"]
    sizes = _sizes(scheme, reads)
    assert (4096, 4096) in sizes and (4097, 4097) in sizes and any(u > 5000 for _, u in sizes) and any(u <= 1024 for _, u in sizes), sizes


def test_tandem_read_has_runs_across_tile_and_merge_boundaries():
    mz, uq = L.lists(L.tandem_read(), L.DENSE)
    h = sorted(int(x) for x in mz["hash"])
    assert len(mz) > L.UQ_MAX
    repeated = {x for i, x in enumerate(h[1:]) if x == h[i]}
    assert len(repeated) >= 200 and len(uq) < len(mz) - 400, (len(repeated), len(mz), len(uq))
    assert [i for i in L.straddled(h, 1024) if i % 4096], "no run of equal hashes across a multiple of 1 024"
    assert L.straddled(h, 4096), "no run of equal hashes across a multiple of 4 096"


def test_small_batch_meets_every_raw_count_and_has_its_tandem_runs():
    reads = L.small_index_batch()
    sizes = _sizes(L.DENSE, reads)
    assert len(reads) == len(L.SMALL_LISTS) + 2 and min(len(r) for r in reads) == 14
    assert tuple(raw for raw, _ in sizes[:len(L.SMALL_LISTS)]) == L.SMALL_LISTS, sizes
    (raw_a, uq_a), (raw_b, uq_b) = sizes[-2:]
    assert uq_a < raw_a <= 1024 and 1024 < raw_b <= L.UQ_MAX and uq_b < raw_b, sizes[-2:]
    h = sorted(int(x) for x in L.lists(reads[-1], L.DENSE)[0]["hash"])
    assert L.straddled(h, 256), "no run of equal hashes across a multiple of 256"


def test_homopolymer_read_outgrows_half_its_slot():
    r = L.homopolymer_read()
    mz, uq = L.lists(r, L.DENSE)
    assert 2 * len(mz) > len(r) + 64 and len(mz) > L.UQ_MAX and 2 * len(uq) <= len(r) + 64, (len(mz), len(uq), len(r))


def test_w1_read_has_one_entry_per_kmer():
    scheme, reads = L.index_batches()["w1"]
    sizes = _sizes(scheme, reads)
    assert sizes[0][0] == len(reads[0]) - 15 + 1 > L.UQ_MAX and sizes[0][1] > L.UQ_MAX, sizes
    assert sizes[1][0] <= 1024 < sizes[2][0], sizes


def test_anchor_counts_at_and_past_either_tile_on_both_strands():
    seen = {}
    for s in L.chain_sets():
        for (q, t), (total, info, nq, nt) in L.chain_info(s).items():
            rev = int(info["nrev"] > info["nfwd"])
            key = "big" if total > 8192 else total
            seen.setdefault(key, []).append((s["name"], rev, info))
    for key in (L.TILE_LONG, L.TILE_LONG + 1, L.TILE_COMPACT, L.TILE_COMPACT + 1, "big"):
        got = seen.get(key, [])
        for rev in (0, 1):
            assert any(r == rev and i["one_diag"] for _, r, i in got), ("one diagonal", key, rev)
            assert any(r == rev and not i["one_diag"] and i["not_prev"] > 0 for _, r, i in got), ("with errors", key, rev)
        assert any(i["not_prev_run"] >= 2 for _, _, i in got), ("a run of links past the previous anchor", key)
    # the long layout's own pairs: a read of 65 536 bases or more in the set
    long_sets = [s for s in L.chain_sets() if max(len(r) for r in s["reads"]) >= 65536]
    assert sum(v[0] > L.TILE_LONG for s in long_sets for v in L.chain_info(s).values()) >= 3
    assert len(L.spilling_pairs(list(L.chain_sets()), L.TILE_COMPACT)) >= 8


def test_noisy_sets_are_what_the_end_to_end_tests_expect():
    hap, reads = L.noisy_main_set()
    assert len(hap) == 70000 and len(reads) == 28 and sum(len(r) > 33000 for r in reads) == 6
    uq = [len(L.lists(r.decode(), L.ONT)[1]) for r in reads]
    assert max(uq) > L.UQ_MAX and sum(u > L.UQ_MAX for u in uq) >= 4, uq
    # two 10 % reads share few minimizers: the lists pass the cap, the anchors stay far below any tile
    longest = sorted(reads, key=len)[-4:]
    e = O.set_overlaps([r.decode() for r in longest], CC.params("ont"), 0)
    assert max(int(v[0]) for v in e["info"]) < 1024 and min(int(n) for n in e["nuq"]) > L.UQ_MAX
    hap, reads = L.noisy_long_set()
    assert sum(len(r) >= 65536 for r in reads) >= 2 and len(reads) <= 30
