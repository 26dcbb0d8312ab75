"""The extension kernel of the partial charge (k_bpm_ext through fsv_bpm_extensions: Reserve_Banded_BPM_Extension,
Levenshtein_distance.h:14-205) on host tasks, bit for bit against the reference-minted vectors of tests/golden/bpm_ext.json and against
oracle/bpm.c:orc_bpm_extension on windows cut the way non_trim_error_rate cuts them: any offset in either read, both strands of y,
both directions, windows hanging over either end of y, windows the geometry rule rejects."""
import collections
import functools
import json
import os
import random

import numpy as np
import pytest

from focalsv_amd import _lib
from tests import kernel_cases as KC
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu

NS = (1, 2, 15, 16, 17, 63, 64, 65, 374, 375)
KS = (0, 1, 7, 8, 23, 24, 30, 31)      # 23 | 24: where K5's bpm_run changes form; 0: a mismatching first base leaves nothing
N_CASES = 4800


@pytest.fixture(scope="module")
def ctx():
    with _lib.Context(0) as c:
        yield c


def as_reference(row, direction, x_len, y_len):
    """a kernel row -> (aligned, err, p_end, t_end) as tests/oracle_lib.py:bpm_extension reports an extension"""
    te, err, pe = int(row["t_end"]), int(row["err"]), int(row["p_end"])
    if te < 0:
        assert (err, pe) == (-1, -1)
        return 0, -1, -1, -1
    return (te + 1, err, pe, te) if not direction else (te + 1, err, y_len - pe, x_len - te)


def test_golden_vectors(ctx, golden_dir):
    cases = json.load(open(os.path.join(golden_dir, "bpm_ext.json")))["cases"]
    assert len(cases) == 400 and all(KC.usable(c) for c in cases)
    assert collections.Counter(c["dir"] for c in cases) == {0: 160, 1: 240}
    assert {c["k"] for c in cases} >= {1, 31} and all(len(c["y"]) == len(c["x"]) + 2 * c["k"] for c in cases)
    words, tasks = KC.tasks_from_cases(cases)
    out = ctx.bpm_extensions(words, tasks, [c["dir"] for c in cases])
    assert (out["pad"] == 0).all()
    for c, row in zip(cases, out):
        assert as_reference(row, c["dir"], len(c["x"]), len(c["y"])) == (c["aligned"], c["err"], c["p_end"], c["t_end"]), c


# ---- random windows ---------------------------------------------------------------------------------------------------------------
def _disrupt(rng, x, kind, c0):
    """x (a list of bases, in the order the extension walks them) with an event beginning at column c0"""
    n = len(x)
    if kind == "subs":
        for _ in range(rng.randint(1, 3)):
            x[rng.randrange(n)] = rng.choice("ACGT")
    elif kind == "ins":
        x[c0:c0] = list(KC._bases(rng, rng.randint(1, 40)))
    elif kind == "del":
        del x[c0:c0 + rng.randint(1, 40)]
        x += list(KC._bases(rng, n))
    elif kind == "unrelated":
        x[c0:] = list(KC._bases(rng, n - c0))
    return x[:n]


@functools.lru_cache(maxsize=None)
def random_cases(seed=20):
    """-> (Placements, dirs, kinds): N_CASES windows over the (n, k, direction, strand) grid"""
    rng = random.Random(seed)
    P = KC.Placements()
    dirs, kinds = [], []
    for i in range(N_CASES):
        n, k = NS[i % len(NS)], KS[(i // len(NS)) % len(KS)]
        d, y_rev = (i // 80) & 1, (i // 160) & 1
        place = ("inside", "inside", "inside", "left", "right", "reject")[rng.randrange(6)]
        L = n + 2 * k + rng.randint(0, 60)
        strand = KC._bases(rng, L)
        if place == "inside":
            ys = rng.randint(k, L - n - k)
        elif place == "left":            # the padded window starts before the read
            ys = rng.randint(0, max(0, k - 1))
        elif place == "right":           # ... runs past its end, up to where the geometry rule still takes it
            ys = min(L - 1, L - n - k + rng.randint(1, 2 * k + 31))
        else:
            ys = rng.choice((-rng.randint(1, 20), L + rng.randint(0, 20), L + 31 - n - rng.randint(-1, 1)))
        x = [strand[p] if 0 <= p < L else rng.choice("ACGT") for p in range(ys, ys + n)]
        kind = ("none", "subs", "ins", "del", "unrelated", "unrelated")[rng.randrange(6)]
        c0 = 0 if rng.random() < 0.3 else rng.randrange(n)
        if k == 0 and rng.random() < 0.7:      # k = 0 and a first base that differs: the one way an accepted window is left with nothing
            kind, c0 = "unrelated", 0
        if d:
            x.reverse()
        x = _disrupt(rng, x, kind, c0)
        if d:
            x.reverse()
        pre, post = KC._bases(rng, rng.randint(0, 40)), KC._bases(rng, rng.randint(0, 40))
        P.reads += [pre + "".join(x) + post, KC.revcomp(strand) if y_rev else strand]
        P.specs.append(dict(xi=2 * i, yi=2 * i + 1, x_start=len(pre), y_start=ys, x_len=n, k=k, y_rev=y_rev, kind=place, pair=i))
        dirs.append(d)
        # a tail of unrelated sequence longer than 8k + 8 columns: its top diagonal collects more than 3k errors (three in four columns
        # mismatch), which is where the recurrence gives up early (Levenshtein_distance.h:367-375)
        kinds.append("gives up" if kind == "unrelated" and n - c0 > 8 * k + 8 else kind)
    return P, dirs, kinds


def expected(P, dirs, i):
    x, ypad, k, geom = P.operands(i)
    return None if geom is None else O.bpm_extension(x, ypad, k, dirs[i])


def check_rows(P, dirs, out, idx):
    for row, i in zip(out, idx):
        want = expected(P, dirs, i)
        x, ypad, k, geom = P.operands(i)
        if want is None:
            assert (int(row["t_end"]), int(row["err"]), int(row["p_end"])) == (-1, -1, -1), ("rejected geometry", i, P.specs[i], row)
        else:
            assert as_reference(row, dirs[i], len(x), len(ypad)) == want, (i, dirs[i], P.specs[i], x, ypad, row)


def test_random_windows_against_the_oracle(ctx):
    P, dirs, kinds = random_cases()
    words, tasks = P.pack()
    out = ctx.bpm_extensions(words, tasks, dirs)
    check_rows(P, dirs, out, range(len(dirs)))
    # what the list exercised, from the inputs and the oracle alone
    C = collections.Counter()
    for i, s in enumerate(P.specs):
        want = expected(P, dirs, i)
        C["n", s["x_len"]] += 1
        C["k", s["k"]] += 1
        if want is None:
            C["rejected"] += 1
            C["rejected: " + P.reject_kind(i)] += 1
            continue
        geom = P.operands(i)[3]
        C["dir", dirs[i]] += 1
        C["y_rev", s["y_rev"]] += 1
        C["dir x y_rev", dirs[i], s["y_rev"]] += 1
        C["left overhang"] += geom[1] > 0
        C["right overhang"] += geom[2] > 0
        C["none"] += want[0] == 0
        C["ends early"] += 0 < want[0] < s["x_len"]
        C["reaches the end"] += want[0] == s["x_len"]
        C["gives up"] += kinds[i] == "gives up"
        C["k <= 23"] += s["k"] <= 23
        C["k >= 24"] += s["k"] >= 24
    assert all(C["n", n] == N_CASES // len(NS) for n in NS) and all(C["k", k] == N_CASES // len(KS) for k in KS)
    for name, floor in (("none", 200), ("ends early", 200), ("reaches the end", 200), ("gives up", 200), ("rejected", 200), ("left overhang", 100),
                        ("right overhang", 100), ("k <= 23", 1000), ("k >= 24", 500), ("rejected: y_start < 0", 30),
                        ("rejected: y_start >= y_len", 30), ("rejected: length rule", 30)):
        assert C[name] >= floor, (name, C[name], floor)
    assert min(C["dir x y_rev", d, r] for d in (0, 1) for r in (0, 1)) >= 500


def test_order_and_neighbours_do_not_matter(ctx):
    P, dirs, _ = random_cases()
    words, tasks = P.pack()
    base = ctx.bpm_extensions(words, tasks, dirs)
    order = list(range(len(dirs)))
    random.Random(3).shuffle(order)
    for filler in ("A", "random"):
        w2, t2 = P.pack(filler=filler, order=order, seed=11)
        out = ctx.bpm_extensions(w2, t2, [dirs[i] for i in order])
        assert (out == base[order]).all(), (filler, np.nonzero(out != base[order])[0][:5])


def test_bad_tasks_are_refused(ctx):
    P, dirs, _ = random_cases()
    words, tasks = P.pack()
    t = tasks[:4].copy()
    t["k"][1] = 32
    with pytest.raises(_lib.FsvError) as e:
        ctx.bpm_extensions(words, t, dirs[:4])
    assert e.value.code == _lib.EINVAL and "31" in str(e.value)
    t = tasks[:4].copy()
    t["y_word"][2] = len(words)
    with pytest.raises(_lib.FsvError) as e:
        ctx.bpm_extensions(words, t, dirs[:4])
    assert e.value.code == _lib.EINVAL
