"""The generator of K5/K6 windows at real read geometry (tests/kernel_cases.py), without a GPU: its plain-string operands and its
restatement of determine_overlap_region on hand-written cases, and what the lists the GPU tests run actually exercise -- conditions
on the inputs, counted from the oracle alone, so they hold or fail here before anything touches a kernel."""
from tests import kernel_cases as KC
from tests import oracle_lib as O

Y = "ACGTTGCAAT"            # reverse complement: ATTGCAACGT


def test_padded_window_and_geometry_by_hand():
    assert KC.revcomp(Y) == "ATTGCAACGT"
    # stored read Y; (y_rev, y_start, x_len, k, k_cap) -> padded window, (y_beg, extra_begin, extra_end)
    cases = [
        ((0, 4, 3, 1, 31), "TTGCA", (3, 0, 0)),                  # inside the read, forward
        ((1, 4, 3, 1, 31), "GCAAC", (3, 0, 0)),                  # ... and on the reverse strand
        ((0, 1, 2, 3, 31), "NNACGTTG", (0, 2, 0)),               # left clip
        ((1, 1, 2, 3, 31), "NNATTGCA", (0, 2, 0)),
        ((0, 7, 4, 2, 31), "GCAATNNN", (5, 0, 3)),               # right clip
        ((1, 7, 4, 2, 31), "AACGTNNN", (5, 0, 3)),
        ((0, 2, 6, 5, 31), "NNNACGTTGCAATNNN", (0, 3, 3)),       # both
        ((0, 0, 10, 0, 31), Y, (0, 0, 0)),                       # the whole read, no band
        ((0, 9, 3, 2, 31), "AATNNNN", (7, 0, 4)),                # the last base is the predicted start
        ((1, 9, 3, 2, 31), "CGTNNNN", (7, 0, 4)),
        # the length rule, y_len - y_start + 2k + k_cap against wlen: 10 - 5 + 4 + 31 = 40
        ((0, 5, 35, 2, 31), "TTGCAAT" + "N" * 32, (3, 0, 32)),    # wlen 39: accepted
        ((0, 5, 36, 2, 31), "TTGCAAT" + "N" * 33, (3, 0, 33)),    # wlen 40: accepted, the last one
        ((0, 5, 37, 2, 31), "TTGCAAT" + "N" * 34, None),          # wlen 41: rejected
        ((1, 5, 37, 2, 31), "GCAACGT" + "N" * 34, None),
        ((0, 5, 37, 2, 95), "TTGCAAT" + "N" * 34, (3, 0, 34)),    # a wide list's k_cap accepts it
        ((0, -1, 3, 1, 31), "NNACG", None),        # y_start < 0
        ((0, 10, 3, 1, 31), "TNNNN", None),                      # y_start >= y_len
        ((1, 10, 3, 1, 31), "TNNNN", None),
    ]
    for (y_rev, y_start, x_len, k, k_cap), ypad, geom in cases:
        got = KC.padded_window(Y, y_rev, y_start, x_len, k)     # the stored read is Y on both strands
        assert len(got) == x_len + 2 * k
        assert got == ypad, (y_rev, y_start, x_len, k)
        assert KC.overlap_region(y_start, len(Y), x_len, k, k_cap) == geom, (y_rev, y_start, x_len, k, k_cap)
    # a Placements object gives the same through its task fields
    P = KC.Placements()
    P.reads = ["ACGTACGTAC", Y]
    P.specs = [dict(xi=0, yi=1, x_start=3, y_start=7, x_len=4, k=2, y_rev=1, kind="hand")]
    assert P.operands(0) == ("TACG", "AACGTNNN", 2, (5, 0, 3))


def test_k6_classes_by_hand():
    assert KC.k6_class(15, 0, True) == KC.k6_class(95, 7, True) == "gap-free"
    assert [KC.k6_class(15, e, False) for e in (1, 2, 3, 4, 7, 8, 15)] == ["err 1", "err 2", "err 3"] + ["k<=15 err 4..7"] * 2 + ["k<=15 err>7"] * 2
    assert [KC.k6_class(k, e, False) for k, e in ((16, 3), (16, 4), (31, 31), (32, 1), (95, 60))] == ["err 3", "16<=k<=31 err>3", "16<=k<=31 err>3", "k>31", "k>31"]


def test_mutated_copy_keeps_its_coordinate_map():
    import random
    rng = random.Random(3)
    core = KC._core(rng, 600, False)
    m = KC._Mutated(rng, core, 0.06)
    assert 10 < len(m.at) < 80 and m.seq != core
    kept = [c for c in range(len(core)) if c not in m.at]
    assert all(m.seq[m.pos(c)] == core[c] for c in kept)
    assert all(m.pos(m.inv(t)) >= t and (m.inv(t) == 0 or m.pos(m.inv(t) - 1) < t) for t in range(len(m.seq)))


def test_main_list_exercises_what_it_claims():
    P = KC.suite_list("main")
    assert len(P.specs) >= 20000
    lens_x = {len(P.reads[s["xi"]]) % 16 for s in P.specs}
    lens_y = {len(P.reads[s["yi"]]) % 16 for s in P.specs}
    assert lens_x == lens_y == set(range(16)) and all(400 <= len(r) <= 3000 for r in P.reads)
    assert {s["x_start"] % 16 for s in P.specs} == set(range(16)) and {s["x_len"] for s in P.specs} >= set(range(1, 376, 7))
    assert max(s["k"] for s in P.specs) <= P.k_cap == 31
    C = P.coverage()
    acc = C["accepted"]
    assert min(C["accepted", 0], C["accepted", 1]) >= 0.40 * acc
    assert C["x_start % 16 != 0"] >= 0.85 * acc
    assert C["y offset % 16 != 0"] >= 0.85 * acc
    KC.check_floors(C, [c for c in KC.K6_CLASSES if c != "k>31"], 300, 100)
    KC.check_floors(C, ["left clip", "right clip"], 300, 100)
    for kind in ("y_start < 0", "y_start >= y_len", "length rule"):
        assert C["rejected: " + kind] >= 100, kind
    assert C["accepted at the length rule"] >= 100
    assert C["x ends at its read's last base"] >= 200
    # the forced windows meet both strands
    for kind in KC.FORCED:
        assert {s["y_rev"] for s in P.specs if s["kind"] == kind} == {0, 1}, kind
    # the K6 check takes the path of a hit that is not gap-free from O.bpm_path and its end from O.bpm: they must agree
    walked = [i for i in range(len(P.specs)) if P.hit(i)[2] not in (None, "gap-free")][::10]
    assert len(walked) > 500
    for i in walked:
        x, ypad, k, geom = P.operands(i)
        site, err, start, path = O.bpm_path(x, ypad, k)
        assert (site, err) == P.hit(i)[:2], KC.describe(P, i)


def test_wide_list_exercises_what_it_claims():
    P = KC.suite_list("wide")
    assert P.k_cap == 95 and P.specs[0]["k"] == 95 and {s["k"] for s in P.specs} >= set(KC.WIDE_KS)
    assert len(P.specs) > max(KC.PREFIXES)
    C = P.coverage()
    KC.check_floors(C, ["k>31"], 300, 100)
    KC.check_floors(C, ["left clip", "right clip"], 100, 30)
    for kind in ("y_start < 0", "y_start >= y_len", "length rule"):
        assert C["rejected: " + kind] >= 30, kind
    walked = [i for i in range(len(P.specs)) if P.hit(i)[2] == "k>31"][::10]
    for i in walked:
        x, ypad, k, geom = P.operands(i)
        assert O.bpm_path(x, ypad, k, wide=True)[:2] == P.hit(i)[:2], KC.describe(P, i)


def test_every_end_of_store_list_reaches_the_store_s_last_base():
    for profile in ("main", "wide"):
        stores = KC.suite_end_stores(profile)
        assert sorted((last, res) for P, last, res in stores) == sorted((last, res) for last in "xy" for res in range(16))
        for P, last, res in stores:
            tail = len(P.reads) - 1
            assert len(P.reads[tail]) % 16 == res and 20 <= len(P.specs) <= 64
            assert all((s["xi"] if last == "x" else s["yi"]) == tail for s in P.specs if s["pair"] == P.specs[-1]["pair"])
            assert any(KC.at_store_end(P, i) and P.hit(i)[1] >= 0 for i in range(len(P.specs))), (profile, last, res)
            if profile == "wide":
                assert P.specs[0]["k"] == P.k_cap == 95
