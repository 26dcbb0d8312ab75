"""Read sets for the chain kernel (k_chain: chain_pair and its three launch forms), built from plain strings, and what they exercise.

A case is a (scheme, read set, unordered pair).  Every pair is classified from its inputs and from the counters of the oracle's
orc_chain_pair_ex alone -- never through the library -- and tests/test_chain_cases.py asserts the floors below on a machine without
a GPU; tests/test_gpu_chain.py then compares the kernel's raw records and window tasks on the same sets with the oracle's.

Schemes (a scheme is a parameter block; the sets of a scheme go through the library as one batch):
  dense        k = 15, w = 5, no HPC: about one unique minimizer per 3 bases, so the list-size regimes of chain_pair (768 entries in
               registers, 1 024 in the tile) sit at reads of 2-4 kb instead of 27-36 kb.  bw_ec 20, bw_final 0 (the defaults).
  dense_bw0, dense_bw1, dense_bw150
               the same seeds with that indel budget in both passes, on the sets marked `sweep` (the DP shapes and the clean reads):
               0 and 1 with 20 take the 32-bit budget arithmetic, 150 the 64-bit one.
  hifi         the default scheme (51 / 51 / HPC), a smaller slice.
  ont          the ONT profile (15 / 15 / no HPC, bw_ec 150, min_ovlp 500, min_anchors 3; wide bands: the 4 096 tile, no wide list).

What SEED yields: pairs per class as forward + reverse strand, summed over the schemes (test_chain_cases.py prints the table and
asserts FLOOR pairs for every class of FLOORS, on each strand where the strand applies):
  lists q <= 768, t <= 1024: 230 + 253; q > 768, t <= 1024: 18 + 15; t > 1024, searched in global memory: 8 + 12; both > 1024, wide
  list: 2 + 4; ONT batch, both > 1024 in the 4 096 tile: 2 + 4.
  anchors: 0 shared minimizers 7; below min_anchors 2 + 2; exactly 1: 3 + 3, 2: 3 + 3, 64: 8 + 9, 65: 8 + 8, 66: 2 + 2, 129: 8 + 8,
  130: 2 + 2; above 1 024: 2 + 3.
  one diagonal at bw 0: 3 + 6, bw 1: 3 + 6, bw 20: 22 + 22, bw 150: 7 + 10; several diagonals at bw 0: 44 + 48, bw 1: 44 + 48,
  bw 20: 86 + 98, bw 150: 50 + 58; of those, every link to the previous anchor 102 + 120, chain skips anchors 122 + 132, a link refused
  by the budget 114 + 119, a run of more than 8 links not to the previous anchor 4 + 4, best chain starting after the first anchor and
  ending before the last 44 + 51.
  forward only 251, reverse only 292, both strands with the minority dropped 8 + 8, nrev == nfwd 4.
  q contained in t 46 + 52, t contained in q 55 + 58; x_s % 375 == 0: primary 7 + 4, mirror 3 + 3; == 374: 3 + 3, 3 + 3; x_e % 375 == 0:
  2 + 2, 2 + 3; == 374: 6 + 6, 2 + 2; last window of 1-3 bases: primary 8 + 8, mirror 8 + 9; one base below min_ovlp 2 + 2, at
  min_ovlp 2 + 2; repeated hashes dropped on both sides 2 + 4.
The two classes without a floor, counted on the pairs with several diagonals (a pair on one diagonal never reaches the DP):
  anchors whose best score two predecessors reach, so that the nearer-predecessor rule decides: 146 498 anchors in 473 pairs (wherever
  the chain has had no indel yet the score is the distance covered, and two short steps tie with one long one);
  pairs in which another anchor scores as much as the best chain end (the first one wins): 12.
"""
import random
from collections import Counter
from functools import lru_cache

import numpy as np

from tests import oracle_lib as O
from tests.kernel_cases import _bases, _core, revcomp

SEED = 20
UQ_MAX = 4096            # FSV_UQ_MAX: unique minimizers a read's list holds (the oracle has no cap)
QR, AMAX = 768, 1024     # 64 x FSV_CHAIN_QR, FSV_AMAX
WINDOW = 375
SCHEMES = ("dense", "dense_bw0", "dense_bw1", "dense_bw150", "hifi", "ont")
ANCHOR_COUNTS = (1, 2, 64, 65, 66, 129, 130)
# the parameters both sides share by name: copied from the oracle's block into the library's
SHARED_PARAMS = ("k", "w", "hpc", "min_ovlp", "min_anchors", "lookback", "bw_ec", "bw_final", "bw_rechain", "w_later", "win_rate_pm", "k_cap",
                 "min_anchors_final", "min_ovlp_final")


def params(scheme):
    """the oracle's parameter block of a scheme"""
    if scheme == "ont":
        return O.ont_params()
    p = O.default_params()
    if scheme.startswith("dense"):
        p.k, p.w, p.hpc = 15, 5, 0
        if "_bw" in scheme:
            p.bw_ec = p.bw_final = int(scheme.split("_bw")[1])
    return p


def lib_params(lib_block, scheme):
    """the library's parameter block (an _lib.AsmParams with its defaults) set to the scheme"""
    p = params(scheme)
    for name in SHARED_PARAMS:
        setattr(lib_block, name, getattr(p, name))
    return lib_block


def _mutate(rng, s, rate):
    out = []
    for c in s:
        if rng.random() >= rate:
            out.append(c)
            continue
        kind = rng.randrange(3)
        if kind == 0:
            out.append(rng.choice("ACGT".replace(c, "")))
        elif kind == 1:
            out.append(c + rng.choice("ACGT"))
    return "".join(out)


def _info(x, y, p):
    return dict(zip(O.CHAIN_INFO, (int(v) for v in O.set_overlaps([x, y], p, 0)["info"][0])))


def _strands(pairs):
    """every (x, y) also with y on the other strand"""
    return [(n + s, x, revcomp(y) if s == "-" else y) for n, x, y in pairs for s in "+-"]


def _trimmed_to(rng, p, want, indel, key="anchors"):
    """two reads of one genome whose overlap is grown base by base until the oracle counts `want` anchors on the majority strand;
    indel: 0 none, 1 a base deleted / 2 a base inserted in the middle of the overlap (so that the anchors leave the diagonal)"""
    per = 3.2 if p.w == 5 else 8.5
    for attempt in range(40):
        g = _bases(rng, 4000)
        x = g[:1500]

        def make(ov):
            y = g[1500 - ov: 1500 - ov + 1300]
            m = ov // 2
            return y if not indel or ov < 40 else (y[:m] + y[m + 1:] if indel == 1 else y[:m] + "ACGT"[(ov + attempt) & 3] + y[m:])
        ov = max(p.k, int(want * per) - 25)
        for step in range(400):
            got = _info(x, make(ov), p)[key]
            if got == want:
                return x, make(ov)
            if got > want:
                break
            ov += max(1, int((want - got) * per * 0.6))
    raise AssertionError("no overlap with %d anchors" % want)


def _equal_strands(rng, p):
    """x = P Q, y = P rc(Q'), Q' grown until as many anchors are on the reverse strand as on the forward one"""
    for attempt in range(40):
        g = _bases(rng, 1400)
        x, head = g[:1200], g[:420]
        want = _info(x, head, p)["nfwd"]
        for m in range(380, 520):
            y = head + revcomp(g[600:600 + m])
            i = _info(x, y, p)
            if i["nfwd"] == i["nrev"] > 0:
                return x, y
            if i["nrev"] > want + 2:
                break
    raise AssertionError("no pair with nrev == nfwd")


def _zigzag(rng, x, lo, hi, step, size=2):
    """a copy of x in which `size` bases are inserted and deleted in turn every `step` bases of [lo, hi): the anchors alternate
    between two diagonals"""
    out, at, ins = [x[:lo]], lo, True
    while at + step < hi:
        seg = x[at:at + step]
        out.append(seg + _bases(rng, size) if ins else seg[:-size])
        at += step
        ins = not ins
    out.append(x[at:])
    return "".join(out)


def _layout_reads(rng, g, lens, rate, n_rev=None):
    """reads of the given lengths placed over the genome g so that neighbours overlap, errors at `rate`, strands mixed"""
    reads = []
    for i, n in enumerate(lens):
        a = rng.randrange(0, max(1, len(g) - n))
        r = _mutate(rng, g[a:a + n], rate)
        reads.append(revcomp(r) if (i % 2 if n_rev is None else i < n_rev) else r)
    return reads


def _dense_sets(rng, p):
    sets = []
    add = lambda name, reads, sweep=False, tags=None: sets.append({"name": name, "reads": list(reads), "sweep": sweep, "tags": tags or {}})
    # list regimes: four reads each with <= 768, 769..1024 and > 1024 unique minimizers, in shuffled order (12 reads, 66 pairs)
    g = _bases(rng, 4700)
    lens = [1500, 1800, 2050, 2150, 2450, 2600, 2800, 2950, 3500, 3800, 4100, 4400]
    reads = _layout_reads(rng, g, lens, 0.004)
    rng.shuffle(reads)
    add("regimes", reads)
    # HiFi-like reads of one locus (9 reads, 36 pairs)
    g = _bases(rng, 3200)
    add("locus", _layout_reads(rng, g, [1300, 1500, 1700, 1900, 2000, 1400, 1600, 1800, 1250], 0.006), sweep=True)
    # error-free reads: one diagonal; containment
    g = _bases(rng, 2800)
    add("clean", [g[:2000], g[375:1500], revcomp(g[1000:2600])], sweep=True)
    add("clean-b", [revcomp(g[200:2300]), g[700:2800], g[900:1700], revcomp(g[1000:1450])], sweep=True)
    add("single", [_bases(rng, 777)])
    add("unrelated", [_bases(rng, 900), _bases(rng, 1100)])
    add("unrelated-b", [_bases(rng, 40), _bases(rng, 14), _bases(rng, 1500)])
    # exact anchor counts, with and without an indel in the overlap
    for want in ANCHOR_COUNTS:
        for rep, indel in enumerate((1, 2) if want > 2 else (0, 0)):
            x, y = _trimmed_to(rng, p, want, indel)
            for nm, a, b in _strands([("", x, y)]):
                add("anchors-%d-%s%d%s" % (want, "ndi"[indel], rep, nm), [a, b] if rep == 0 else [b, a], sweep=want in (64, 65, 129))
    # DP shapes
    shapes = []
    for rep in range(2):
        a, b, c, d = (_bases(rng, n) for n in (520, 480 + 37 * rep, 610, 450))
        shapes.append(("swap%d" % rep, a + b + c + d, _mutate(rng, a + c + b + d, 0.003)))
        shapes.append(("invert%d" % rep, a + b + c, _mutate(rng, a + revcomp(b) + c, 0.003)))
        x = a + b + c + d
        shapes.append(("ins40-%d" % rep, x, x[:1000 + rep] + _bases(rng, 40) + x[1000 + rep:]))
        shapes.append(("del25-%d" % rep, x, x[:900 - rep] + x[925 - rep:]))
        shapes.append(("noisy%d" % rep, x, _mutate(rng, x, 0.04)))
        for step in (16, 17, 18, 19, 21):
            shapes.append(("zigzag%d-%d" % (step, rep), x, _zigzag(rng, x, 700, 1500, step)))
        # a few anchors of x's tail in front of y and of its head behind: the best chain starts and ends inside the anchor list
        shapes.append(("strays%d" % rep, x, _bases(rng, 30) + x[1900:1960] + _bases(rng, 50) + x[300:1700] + _bases(rng, 40) + x[100:170] + _bases(rng, 20)))
    for nm, x, y in _strands(shapes):
        add(nm, [x, y] if "1" != nm[-2] else [y, x], sweep=True)
    for rep in range(2):
        x, y = _equal_strands(rng, p)
        add("equal-strands%d" % rep, [x, y])
        add("equal-strands%d-swapped" % rep, [y, x])
    # overlap ends on the 375 grid, from either side and on either strand: y lies inside x
    g = _bases(rng, 2700)
    for a in (375, 749):
        for b in (1500, 1501, 1503):
            for nm, x, y in _strands([("grid-%d-%d" % (a, b), g[:2600], g[a:b])]):
                add(nm, [x, y])
                add(nm + "-swapped", [y, x])
    # repeat-rich reads: k_uniq drops the repeated hashes of both reads
    g = _core(rng, 3400, True)
    add("repeats", _layout_reads(rng, g, [2000, 2300, 2600, 1900], 0.003))
    return sets


def _hifi_sets(rng, p):
    g = _bases(rng, 15000)
    sets = [{"name": "hifi-locus", "reads": _layout_reads(rng, g, [7000, 9000, 11000, 8000, 12000, 6000], 0.005), "sweep": False, "tags": {}}]
    g = _bases(rng, 6000)
    sets.append({"name": "hifi-clean", "reads": [g[:4000], revcomp(g[1500:6000]), g[2000:3500]], "sweep": False, "tags": {}})
    return sets


def _ont_sets(rng, p):
    sets = []
    add = lambda name, reads: sets.append({"name": name, "reads": list(reads), "sweep": False, "tags": {}})
    g = _bases(rng, 12500)
    add("ont-long", _layout_reads(rng, g, [9800, 10400, 11000, 10100], 0.01))
    g = _bases(rng, 5000)
    add("ont-noisy", _layout_reads(rng, g, [3000, 3400, 2800, 3600, 3100], 0.06))
    for want in (1, 2):
        x, y = _trimmed_to(rng, p, want, 0)
        for nm, a, b in _strands([("ont-anchors-%d" % want, x, y)]):
            add(nm, [a, b])
    g = _bases(rng, 3000)
    for ov in (p.min_ovlp - 1, p.min_ovlp):
        for nm, x, y in _strands([("ont-ovlp-%d" % ov, g[:1500], g[1500 - ov:2900])]):
            add(nm, [x, y])
            add(nm + "-swapped", [y, x])
    return sets


@lru_cache(maxsize=None)
def _all_sets():
    rng = random.Random(SEED)
    return {"dense": _dense_sets(rng, params("dense")), "hifi": _hifi_sets(rng, params("hifi")), "ont": _ont_sets(rng, params("ont"))}


def sets_of(scheme):
    """the read sets of a scheme, in batch order: dicts with name, reads"""
    if "_bw" in scheme:
        return [s for s in _all_sets()["dense"] if s["sweep"]]
    return _all_sets()[scheme]


@lru_cache(maxsize=None)
def expected(scheme, pass_):
    """the oracle's result per set of the scheme (O.set_overlaps), computed once and shared"""
    p = params(scheme)
    return [O.set_overlaps(s["reads"], p, pass_) for s in sets_of(scheme)]


def upair_index(n, q, t):
    """index of the unordered pair (q < t) among those of a set of n reads, row-major"""
    return q * (2 * n - q - 1) // 2 + (t - q - 1)


def slot_index(n, q, t):
    """ordered slot of (q, t) inside its set's block of n (n - 1) slots"""
    return q * (n - 1) + (t if t < q else t - 1)


@lru_cache(maxsize=None)
def classified(scheme):
    """every unordered pair of the scheme: dict(set, name, q, t, rev, info, classes) -- classes from the inputs and the oracle alone"""
    p, out = params(scheme), []
    loose = None
    if p.min_ovlp > 1:       # the overlaps a lower min_ovlp would keep: how long is what min_ovlp drops?
        lp = params(scheme)
        lp.min_ovlp = 1
        loose = [O.set_overlaps(s["reads"], lp, 0) for s in sets_of(scheme)]
    for si, (s, e) in enumerate(zip(sets_of(scheme), expected(scheme, 0))):
        n = len(s["reads"])
        raw = [len(O.sketch(r, p.w, p.k, p.hpc)) for r in s["reads"]]
        rec = {(int(o["q"]), int(o["t"])): o for o in e["ovl"]}
        for q in range(n):
            for t in range(q + 1, n):
                info = dict(zip(O.CHAIN_INFO, (int(v) for v in e["info"][upair_index(n, q, t)])))
                nq, nt, a = int(e["nuq"][q]), int(e["nuq"][t]), info["anchors"]
                rev = int(info["nrev"] > info["nfwd"])
                c = set()
                if scheme == "ont":
                    if min(nq, nt) > AMAX:
                        c.add("ont batch: both lists > 1024 in the 4096 tile")
                elif min(nq, nt) > AMAX:
                    c.add("lists both > 1024 (wide list)")
                elif nt > AMAX:
                    c.add("lists t > 1024 (searched in global memory)")
                else:
                    c.add("lists q <= 768, t <= 1024" if nq <= QR else "lists q > 768, t <= 1024")
                if info["nfwd"] + info["nrev"] == 0:
                    c.add("anchors 0")
                elif a < p.min_anchors:
                    c.add("anchors below min_anchors")
                if a in ANCHOR_COUNTS:
                    c.add("anchors %d" % a)
                if a > 1024:
                    c.add("anchors > 1024")
                if a >= 2 and a >= p.min_anchors:
                    if info["one_diag"]:
                        c.add("one diagonal, bw %d" % p.bw_ec)
                    else:
                        c.add("several diagonals, bw %d" % p.bw_ec)
                        if info["not_prev"] == 0:
                            c.add("several diagonals, every link to the previous anchor")
                        if info["not_prev_run"] > 8:
                            c.add("run of > 8 links not to the previous anchor")
                        if info["refused"]:
                            c.add("link refused by the budget")
                        if info["first"] > 0 and info["best"] < a - 1:
                            c.add("best chain starts after the first anchor and ends before the last")
                        if (q, t) in rec and int(rec[q, t]["n_chain"]) < a:
                            c.add("chain skips anchors")
                if info["nfwd"] and info["nrev"]:
                    c.add("nrev == nfwd" if info["nfwd"] == info["nrev"] else "both strands, minority dropped")
                elif a:
                    c.add("reverse" if rev else "forward")
                if raw[q] > nq and raw[t] > nt and a:
                    c.add("repeated hashes dropped on both sides")
                for side, (u, v) in (("primary", (q, t)), ("mirror", (t, q))):
                    o = rec.get((u, v))
                    if o is None:
                        if loose is not None:
                            lo = {(int(x["q"]), int(x["t"])): x for x in loose[si]["ovl"]}.get((u, v))
                            if lo is not None and int(lo["x_e"]) - int(lo["x_s"]) + 1 == p.min_ovlp - 1:
                                c.add("overlap one base below min_ovlp")
                        continue
                    xs, xe, lu, lv = int(o["x_s"]), int(o["x_e"]), len(s["reads"][u]), len(s["reads"][v])
                    if p.min_ovlp > 1 and xe - xs + 1 == p.min_ovlp:
                        c.add("overlap at min_ovlp")
                    if side == "primary":
                        if xs == 0 and xe == lu - 1 and lv > lu:
                            c.add("q contained in t")
                        if int(o["y_s"]) == 0 and int(o["y_e"]) == lv - 1 and lu > lv:
                            c.add("t contained in q")
                    if xs > 0 and xs % WINDOW in (0, WINDOW - 1):
                        c.add("%s: x_s %% 375 == %d" % (side, xs % WINDOW))
                    if xe < lu - 1 and xe % WINDOW in (0, WINDOW - 1):
                        c.add("%s: x_e %% 375 == %d" % (side, xe % WINDOW))
                    if xe // WINDOW > xs // WINDOW and xe % WINDOW <= 2:
                        c.add("%s: last window of 1-3 bases" % side)
                out.append({"scheme": scheme, "set": si, "name": s["name"], "q": q, "t": t, "rev": rev, "info": info, "classes": c, "nq": nq, "nt": nt})
    return out


GRID_CLASSES = tuple("%s: x_%s %% 375 == %d" % (side, end, r) for side in ("primary", "mirror") for end in "se" for r in (0, 374))
# class -> does the strand apply (then the floor holds on each strand)
FLOORS = dict([(c, True) for c in (
    "lists q <= 768, t <= 1024", "lists q > 768, t <= 1024", "lists t > 1024 (searched in global memory)", "lists both > 1024 (wide list)",
    "ont batch: both lists > 1024 in the 4096 tile", "anchors below min_anchors", "anchors > 1024",
    "several diagonals, every link to the previous anchor", "chain skips anchors", "link refused by the budget",
    "run of > 8 links not to the previous anchor", "best chain starts after the first anchor and ends before the last",
    "both strands, minority dropped", "q contained in t", "t contained in q", "overlap one base below min_ovlp", "overlap at min_ovlp",
    "primary: last window of 1-3 bases", "mirror: last window of 1-3 bases", "repeated hashes dropped on both sides")]
    + [("anchors %d" % a, True) for a in ANCHOR_COUNTS]
    + [("%s, bw %d" % (shape, bw), True) for shape in ("one diagonal", "several diagonals") for bw in (0, 1, 20, 150)]
    + [(c, True) for c in GRID_CLASSES]
    + [("anchors 0", False), ("nrev == nfwd", False), ("forward", False), ("reverse", False)])
FLOOR = 2


def coverage():
    """Counter over every scheme: pairs per class, and per (class, strand)"""
    C = Counter()
    for scheme in SCHEMES:
        for pr in classified(scheme):
            for c in pr["classes"]:
                C[c] += 1
                C[c, pr["rev"]] += 1
    return C


def ties():
    """the two classes without a floor, on pairs with several diagonals: (anchors with tied predecessors, pairs with such an anchor,
    pairs whose best chain end is tied)"""
    multi = [pr for scheme in SCHEMES for pr in classified(scheme) if not pr["info"]["one_diag"] and pr["info"]["anchors"] >= 2]
    return (sum(pr["info"]["pred_ties"] for pr in multi), sum(pr["info"]["pred_ties"] > 0 for pr in multi), sum(pr["info"]["end_ties"] > 0 for pr in multi))


def describe(scheme, name, q, t):
    """what a failure message says about the ordered pair (q, t) of the set called `name`: lengths, list sizes, classes, the oracle's counters"""
    for pr in classified(scheme):
        if pr["name"] == name and (pr["q"], pr["t"]) == (min(q, t), max(q, t)):
            s = sets_of(scheme)[pr["set"]]
            return "%s set '%s' pair (%d, %d) lens (%d, %d) lists (%d, %d) %s %s" % (
                scheme, name, q, t, len(s["reads"][q]), len(s["reads"][t]), pr["nq"] if q < t else pr["nt"], pr["nt"] if q < t else pr["nq"],
                sorted(pr["classes"]), pr["info"])
    return "%s set '%s' pair (%d, %d)" % (scheme, name, q, t)


def set_named(scheme, name):
    return next(s for s in sets_of(scheme) if s["name"] == name)


@lru_cache(maxsize=None)
def truncation_set():
    """(dense scheme) three reads, the first two of about 9 kb sharing all their bases: lists in (2 560, 4 096] and more anchors than the
    long layout's wide tile (FSV_AMAX_WIDE_LONG = 2 560) holds; and a read of 65 536 bases, which puts a batch into the long layout"""
    rng = random.Random(SEED + 1)
    g = _bases(rng, 9600)
    return ({"name": "truncated", "reads": [g[:9300], g[200:9600], g[4000:5500]], "sweep": False, "tags": {}},
            {"name": "filler", "reads": [_bases(rng, 65536)], "sweep": False, "tags": {}})
