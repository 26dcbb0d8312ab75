"""The read sets the chain-kernel tests run (tests/chain_cases.py), without a GPU: what every pair exercises, counted from the inputs and
from the oracle's counters alone, so the list is shown adequate here before anything touches a kernel; and the two oracle exports the
GPU test stands on (orc_set_overlaps, orc_chain_pair_ex) against each other and against cases small enough to check by hand."""
import ctypes

import numpy as np

from tests import chain_cases as CC
from tests import oracle_lib as O


def test_every_class_has_its_floor():
    C = CC.coverage()
    for c, per_strand in sorted(CC.FLOORS.items()):
        print("%-72s %4d pairs (forward %d, reverse %d)" % (c, C[c], C[c, 0], C[c, 1]))
    anchors, pairs, ends = CC.ties()
    print("no floor: %d anchors with tied predecessors in %d pairs; %d pairs with a tied best chain end (pairs with several diagonals)" % (anchors, pairs, ends))
    short = [c for c, per_strand in CC.FLOORS.items() if (min(C[c, 0], C[c, 1]) if per_strand else C[c]) < CC.FLOOR]
    assert not short, short
    # the nearer-predecessor rule is met where the DP runs; the count is reported, not guaranteed by construction
    assert anchors > 0


def test_sets_are_what_the_tests_take_them_for():
    for scheme in CC.SCHEMES:
        sets = CC.sets_of(scheme)
        names = [s["name"] for s in sets]
        assert len(set(names)) == len(names), scheme
        for pass_ in (0, 1):        # (the ONT scheme sketches its final pass with another window)
            for s, e in zip(sets, CC.expected(scheme, pass_)):
                assert len(e["nuq"]) == len(s["reads"]) and int(e["nuq"].max()) <= CC.UQ_MAX, (scheme, s["name"])
                assert all(len(r) < 65536 for r in s["reads"])
    sizes = {len(s["reads"]) for s in CC.sets_of("dense")}
    assert sizes >= {1, 2, 3, 9, 12}
    assert {len(s["reads"]) for s in CC.sets_of("dense_bw0")} >= {2, 3, 9} and len(CC.sets_of("dense_bw0")) < len(CC.sets_of("dense"))
    p = CC.params("ont")
    assert (p.k, p.w, p.hpc, p.bw_ec, p.min_ovlp, p.min_anchors) == (15, 15, 0, 150, 500, 3) and p.k_cap > 31
    p = CC.params("hifi")
    assert (p.k, p.w, p.hpc, p.bw_ec, p.bw_final, p.bw_rechain) == (51, 51, 1, 20, 0, 1)
    assert [CC.params(s).bw_ec for s in CC.SCHEMES[:4]] == [20, 0, 1, 150]
    # the pair that must overflow the long layout's wide tile, and the read that switches a batch to that layout
    trunc, filler = CC.truncation_set()
    e = O.set_overlaps(trunc["reads"], CC.params("dense"), 0)
    assert 2560 < min(e["nuq"][:2]) and max(e["nuq"]) <= CC.UQ_MAX and e["info"][0][O.CHAIN_INFO.index("anchors")] > 2560
    assert len(filler["reads"]) == 1 and len(filler["reads"][0]) == 65536


def test_slot_and_pair_indices():
    for n in (2, 3, 9, 12):
        slots = [CC.slot_index(n, q, t) for q in range(n) for t in range(n) if q != t]
        assert slots == list(range(n * (n - 1)))
        assert [CC.upair_index(n, q, t) for q in range(n) for t in range(q + 1, n)] == list(range(n * (n - 1) // 2))


def test_set_overlaps_is_chain_pair_on_every_pair():
    """orc_set_overlaps against orc_chain_pair_ex called pair by pair on the same sketches: records, chains and counters; the mirrored
    record by the rule of collect_overlaps; the window grid by hand"""
    for scheme, names in (("dense", ("locus", "clean-b", "invert0-", "strays1+")), ("ont", ("ont-noisy",)), ("hifi", ("hifi-clean",))):
        p = CC.params(scheme)
        for name in names:
            s = CC.set_named(scheme, name)
            e = CC.expected(scheme, 0)[[x["name"] for x in CC.sets_of(scheme)].index(name)]
            uq = [O.unique_sorted(O.sketch(r, p.w, p.k, p.hpc)) for r in s["reads"]]
            assert [len(u) for u in uq] == list(e["nuq"])
            rec = {(int(o["q"]), int(o["t"])): o for o in e["ovl"]}
            n = len(s["reads"])
            for q in range(n):
                for t in range(q + 1, n):
                    lq, lt = len(s["reads"][q]), len(s["reads"][t])
                    o, (cq, ct), info = O.chain_pair_info(uq[q], lq, uq[t], lt, p, p.bw_ec)
                    assert [info[k] for k in O.CHAIN_INFO] == list(e["info"][CC.upair_index(n, q, t)])
                    assert (o is None) == ((q, t) not in rec) == ((t, q) not in rec)
                    if o is None:
                        continue
                    a, m = rec[q, t], rec[t, q]
                    for f in ("x_s", "x_e", "y_s", "y_e", "score", "n_chain", "rev"):
                        assert a[f] == o[f]
                    nc = int(a["n_chain"])
                    assert np.array_equal(e["cq"][a["chain_off"]: a["chain_off"] + nc], cq) and np.array_equal(e["ct"][a["chain_off"]: a["chain_off"] + nc], ct)
                    assert np.all(np.diff(cq) > 0) and np.all(np.diff(ct) > 0)
                    if not a["rev"]:
                        assert (m["x_s"], m["x_e"], m["y_s"], m["y_e"]) == (a["y_s"], a["y_e"], a["x_s"], a["x_e"])
                        mq, mt = ct, cq
                    else:
                        assert (m["x_s"], m["x_e"], m["y_s"], m["y_e"]) == (lt - 1 - a["y_e"], lt - 1 - a["y_s"], lq - 1 - a["x_e"], lq - 1 - a["x_s"])
                        mq, mt = (lt - 1 - ct)[::-1], (lq - 1 - cq)[::-1]
                    assert np.array_equal(e["cq"][m["chain_off"]: m["chain_off"] + nc], mq) and np.array_equal(e["ct"][m["chain_off"]: m["chain_off"] + nc], mt)
                    for r, xq, xt in ((a, cq, ct), (m, mq, mt)):
                        assert r["n_win"] == r["x_e"] // 375 - r["x_s"] // 375 + 1
                        for j in range(int(r["n_win"])):
                            w = e["win"][int(r["first_win"]) + j]
                            x0 = max(int(r["x_s"]), (int(r["x_s"]) // 375 + j) * 375)
                            x1 = min(int(r["x_e"]), (int(r["x_s"]) // 375 + j) * 375 + 374)
                            at = max(0, int(np.searchsorted(xq, x0, side="right")) - 1)     # the last anchor at or before x0, else the first
                            assert (w["x_start"], w["x_len"], w["y_start"], w["k"]) == (x0, x1 - x0 + 1, x0 + int(xt[at]) - int(xq[at]), O.lib().orc_thr_for_len_p(ctypes.byref(p), x1 - x0 + 1))


def test_chain_pair_by_hand():
    """three anchors on one diagonal, then with the middle one moved: scores, links and counters as the DP of Hash_Table.cpp:425-616 gives them"""
    p = CC.params("dense")
    mz = lambda rows: np.array([(h, pos, 0, 15, 0) for h, pos in rows], dtype=O.MZ_DTYPE)
    q = mz([(10, 100), (20, 110), (30, 140)])
    o, (cq, ct), info = O.chain_pair_info(q, 400, mz([(10, 50), (20, 60), (30, 90)]), 300, p, 20)
    assert (o["score"], o["n_chain"], o["rev"]) == (15 + 10 + 15, 3, 0) and (o["x_s"], o["y_s"], o["x_e"], o["y_e"]) == (50, 0, 349, 299)
    assert (info["anchors"], info["one_diag"], info["not_prev"], info["refused"], info["first"], info["best"]) == (3, 1, 0, 0, 0, 2)
    assert info["pred_ties"] == 0          # 15 + 10 + 15 by the middle anchor, 15 + 15 without it
    # the middle anchor 3 bases off the diagonal.  At 20 per mille a span of 10 allows no indel: the link to it is refused, and so is the
    # third anchor's link to it (3 indels over 30); the third links to the first.  At 150 per mille the third anchor may link to the second
    # (3 <= 4.5) but scores 15 + 15 - 10 against 15 + 15 by the first.  At 400 the second anchor is chained (15 + 10 - 7), the third
    # still prefers the first (30 against 18 + 15 - 5): in all three the best chain skips the middle anchor.
    t = mz([(10, 50), (20, 63), (30, 90)])
    for bw, refused, not_prev in ((20, 2, 2), (150, 1, 2), (400, 0, 1)):
        o, (cq, ct), info = O.chain_pair_info(q, 400, t, 300, p, bw)
        assert (o["n_chain"], o["score"], list(cq), list(ct)) == (2, 30, [100, 140], [50, 90]), bw
        assert (info["one_diag"], info["refused"], info["not_prev"], info["pred_ties"]) == (0, refused, not_prev, 0), bw
    # a tie between predecessors: anchors 5 apart on one diagonal score 15 + 5 + 5 by the nearer and 15 + 10 by the farther one
    o, (cq, ct), info = O.chain_pair_info(mz([(10, 100), (20, 105), (30, 110)]), 400, mz([(10, 50), (20, 55), (30, 60)]), 300, p, 20)
    assert (o["score"], o["n_chain"], info["pred_ties"], info["not_prev"]) == (25, 3, 1, 0)
    # reverse strand: the query runs on its reverse strand (k-mer ends there), anchors in that order
    o, (cq, ct), info = O.chain_pair_info(mz([(10, 100), (20, 110)]), 400, np.array([(10, 60, 1, 15, 0), (20, 50, 1, 15, 0)], dtype=O.MZ_DTYPE), 300, p, 20)
    assert (info["nrev"], info["nfwd"], o["rev"], o["n_chain"], o["score"]) == (2, 0, 1, 2, 25)
    assert list(cq) == [100 - 14, 110 - 14] and list(ct) == [300 - 1 - 60, 300 - 1 - 50]


# ---- what the GPU test would notice: the kernel's rules restated in plain Python, each once as it is and once reverted, on the
# ---- suite's own pairs.  The rule as it is reproduces the oracle; reverted, it changes a field tests/test_gpu_chain.py compares.
def _anchors(p, rq, rt, turn=True):
    """the anchor list chain_pair builds: lookups in query order, majority strand, reverse-strand pairs on the query's reverse strand and
    turned around so that they ascend"""
    sq, st = O.sketch(rq, p.w, p.k, p.hpc), O.unique_sorted(O.sketch(rt, p.w, p.k, p.hpc))
    uq = O.unique_sorted(sq)
    uq = uq[np.argsort(uq["pos"])]
    at = {int(h): i for i, h in enumerate(st["hash"])}
    hits = [(m, st[at[int(m["hash"])]]) for m in uq if int(m["hash"]) in at]
    nrev = sum(int(a["rev"]) ^ int(b["rev"]) for a, b in hits)
    rev = int(nrev > len(hits) - nrev)
    keep = [(a, b) for a, b in hits if (int(a["rev"]) ^ int(b["rev"])) == rev]
    out = [((len(rq) - 1) - (int(a["pos"]) - int(a["span"]) + 1) if rev else int(a["pos"]), int(b["pos"])) for a, b in keep]
    return (out[::-1] if rev and turn else out), rev


def _chain(anchors, k, bw, nearer_wins=True):
    """the DP of chain_pair (64 predecessors, nearest first) -> (score, chain as anchor indices)"""
    f, pre, ind, sl = [], [], [], []
    for i, (qe, te) in enumerate(anchors):
        bs, bp, bi, bl = k, -1, 0, 0
        for j in range(i - 1, max(-1, i - 65), -1):
            dq, dt = qe - anchors[j][0], te - anchors[j][1]
            if dq <= 0 or dt <= 0:
                continue
            ti, tl = ind[j] + abs(dq - dt), sl[j] + dq
            if ti * 1000 > tl * bw:
                continue
            sc = min(dq, dt, k)
            if ti:
                sc -= (ti * sc * 1000) // (tl * bw)
            sc += f[j]
            if sc > bs or (not nearer_wins and sc == bs and bp >= 0):
                bs, bp, bi, bl = sc, j, ti, tl
        f.append(bs); pre.append(bp); ind.append(bi); sl.append(bl)
    best = max(range(len(f)), key=lambda i: (f[i], -i))
    chain, c = [], best
    while c >= 0:
        chain.append(c)
        c = pre[c]
    return f[best], chain[::-1]


def _several_diagonals(scheme, want_rev=None, limit=12):
    bw = CC.params(scheme).bw_ec
    prs = [pr for pr in CC.classified(scheme) if "several diagonals, bw %d" % bw in pr["classes"] and 20 <= pr["info"]["anchors"] <= 700
           and (want_rev is None or pr["rev"] == want_rev)]
    return prs[:: max(1, len(prs) // limit)][:limit]


def _record(scheme, pr, q, t):
    e = CC.expected(scheme, 0)[pr["set"]]
    return e, next((o for o in e["ovl"] if (int(o["q"]), int(o["t"])) == (q, t)), None)


def test_reverting_the_tie_rule_or_the_turn_around_changes_a_record():
    p = CC.params("dense")
    changed_tie = changed_turn = 0
    for pr in _several_diagonals("dense", 0, 10) + _several_diagonals("dense", 1, 10):
        reads = CC.sets_of("dense")[pr["set"]]["reads"]
        e, o = _record("dense", pr, pr["q"], pr["t"])
        a, rev = _anchors(p, reads[pr["q"]], reads[pr["t"]])
        assert len(a) == pr["info"]["anchors"] and rev == pr["rev"] and a == sorted(a)
        score, chain = _chain(a, p.k, p.bw_ec)
        assert o is not None and (score, len(chain)) == (int(o["score"]), int(o["n_chain"])), pr["name"]       # the restatement is the oracle's DP
        if pr["info"]["pred_ties"]:
            s2, c2 = _chain(a, p.k, p.bw_ec, nearer_wins=False)
            changed_tie += (s2, len(c2)) != (score, len(chain))
        if rev:
            s3, c3 = _chain(_anchors(p, reads[pr["q"]], reads[pr["t"]], turn=False)[0], p.k, p.bw_ec)
            assert len(c3) == 1 and len(chain) > 1      # a descending list links nothing
            changed_turn += 1
    print("records a farther-predecessor tie rule changes: %d; reverse-strand records an unturned list changes: %d" % (changed_tie, changed_turn))
    assert changed_tie >= 2 and changed_turn >= 2


def test_reverting_the_mirrored_diagonal_search_changes_a_task():
    """the mirrored tasks of a reverse-strand overlap: the kernel searches its chain (kept in the primary side's order) by the target
    coordinate from the far end; searched as on the forward strand, window starts land on another anchor's diagonal"""
    p = CC.params("dense")
    changed = 0
    for pr in _several_diagonals("dense", 1, 12):
        reads = CC.sets_of("dense")[pr["set"]]["reads"]
        lq, lt = len(reads[pr["q"]]), len(reads[pr["t"]])
        e, o = _record("dense", pr, pr["q"], pr["t"])
        _, m = _record("dense", pr, pr["t"], pr["q"])
        nc = int(o["n_chain"])
        cq, ct = e["cq"][o["chain_off"]: o["chain_off"] + nc], e["ct"][o["chain_off"]: o["chain_off"] + nc]     # ascending in q; t in strand coordinates
        for j in range(int(m["n_win"])):
            w = e["win"][int(m["first_win"]) + j]
            x0 = int(w["x_start"])
            # kernel, rev: anchors (CH_Q, CH_T) = (cq, ct) ascending; mirrored query coordinate lt-1-ct descends: first e with ct >= lt-1-x0, else the last
            i = int(np.searchsorted(ct, lt - 1 - x0, side="left"))
            i = nc - 1 if i == nc else i
            assert x0 + (lq - 1 - int(cq[i])) - (lt - 1 - int(ct[i])) == int(w["y_start"]), (pr["name"], j)
            # reverted: the forward strand's search (last anchor with ct <= x0, else the first) and its diagonal
            i2 = max(0, int(np.searchsorted(ct, x0, side="right")) - 1)
            changed += x0 + int(cq[i2]) - int(ct[i2]) != int(w["y_start"])
    print("mirrored reverse-strand tasks the forward search would move: %d" % changed)
    assert changed >= 2
