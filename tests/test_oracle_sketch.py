"""oracle/sketch.c against minimizers minted from the reference's ha_sketch."""
import gzip
import json
import os

import numpy as np

from tests import oracle_lib as O


def test_sketch_matches_reference_golden(golden_dir):
    cases = json.load(open(os.path.join(golden_dir, "sketch.json")))["cases"]
    total = 0
    for c in cases:
        got = O.sketch(c["seq"], c["w"], c["k"], c["hpc"])
        exp = c["mz"]
        assert len(got) == len(exp), (c["w"], c["k"], c["hpc"], len(c["seq"]))
        for g, e in zip(got, exp):
            assert [int(g["hash"]), int(g["pos"]), int(g["rev"]), int(g["span"])] == e
        total += len(exp)
    assert total > 10000


def test_sketch_grid_matches_reference_digests(golden_dir):
    """tests/golden/sketch_grid.json.gz (tools/make_golden_sketch_grid.py): the reference's ha_sketch over 19 windows x 13 k x both HPC
    settings, every edge length of tests/sketch_cases.py at every grid point.  The oracle reproduces every count and digest."""
    from tests import sketch_cases as SC
    doc = json.load(gzip.open(os.path.join(golden_dir, "sketch_grid.json.gz"), "rt"))
    assert [(p["w"], p["k"], p["hpc"]) for p in doc["points"]] == list(SC.GRID)
    n_cases = n_mz = 0
    for p in doc["points"]:
        w, k, hpc = p["w"], p["k"], p["hpc"]
        cases = SC.fixture_cases(w, k, hpc)
        assert [c["tag"] for c in cases if c["kind"] == "edge"] == [str(n) for n in SC.edge_lengths(w, k)]
        assert [c["kind"] + ":" + c["tag"] for c in cases if c["kind"] != "edge"] == p["extra"]
        assert len(cases) == len(p["len"]) == len(p["n"]) and len(p["seq"]) == SC.SEQ_DIGEST * len(cases) and len(p["mz"]) == SC.MZ_DIGEST * len(cases)
        for i, c in enumerate(cases):
            what = (w, k, hpc, c["kind"], c["tag"])
            assert len(c["seq"]) == p["len"][i] and SC.seq_digest(c["seq"]) == p["seq"][SC.SEQ_DIGEST * i: SC.SEQ_DIGEST * (i + 1)], ("generator drift", what)
            got = O.sketch(c["seq"], w, k, hpc)
            assert len(got) == p["n"][i], what
            assert SC.mz_digest(SC.mz_text(got)) == p["mz"][SC.MZ_DIGEST * i: SC.MZ_DIGEST * (i + 1)], what
            n_mz += len(got)
        n_cases += len(cases)
    assert (n_cases, n_mz) == (doc["cases"], doc["minimizers"]) and n_cases > 17000


def test_sketch_grid_order_and_coverage():
    """on every case of the generator (the GPU tests run all of them against the oracle): positions strictly increasing, and the
    coverage floors -- each condition the kernels treat apart is met at every grid point whose geometry allows it"""
    from tests import sketch_cases as SC
    cases = list(SC.all_cases())
    for c in cases:
        pos = O.sketch(c["seq"], c["w"], c["k"], c["hpc"])["pos"].astype(np.int64)
        assert (np.diff(pos) > 0).all() and (len(pos) == 0 or pos[-1] < len(c["seq"])), (c["w"], c["k"], c["hpc"], c["kind"], c["tag"])
    cov = SC.coverage(cases, O.sketch_info)
    assert sorted(cov) == sorted(SC.GRID)
    assert SC.check_floors(cov) == []
    for gp in SC.GRID:      # an exemption is a statement about the geometry: the count is not merely missed, it cannot be met
        for name in SC.COUNTS:
            if SC.exempt(*gp, name):
                assert cov[gp][name] == 0, (gp, name)
    kinds = {(c["w"], c["k"], c["hpc"], c["kind"]) for c in cases}
    assert all((w, k, hpc, kind) in kinds for (w, k, hpc) in SC.GRID for kind in SC.KINDS)
    total = {n: sum(cov[gp][n] for gp in cov) for n in SC.COUNTS}
    print("sketch grid coverage:", len(cases), "cases,", total)
