"""K6 on the GPU (fsv_bpm_paths through the C ABI): alignment path + generate_cigar against the reference-minted golden
vectors (tests/golden/bpm_k6.json) and the CPU oracle on random windows, single-indel windows in repeats included."""
import json
import os
import random

import pytest

from focalsv_amd import _lib
from tests import kernel_cases as KC
from tests import oracle_lib as O
from tests.kernel_cases import strip_pad, tasks_from_cases, usable

pytestmark = pytest.mark.gpu
OPS = {"M": 0, "X": 1, "I": 2, "D": 3}


@pytest.fixture(scope="module")
def ctx():
    with _lib.Context(0) as c:
        yield c


def expected(c):
    """oracle, in the order the assembler uses (Levenshtein_distance.h:516-531): K5's result first; distance 0 or a gap-free
    placement with exactly that many mismatches (try_cigar) needs no DP; else the banded DP with traceback.
    -> (err after generate_cigar, start, end, ops start-to-end) or None when no alignment within k"""
    site, err = O.bpm(c["x"], c["y"], c["k"])
    if err < 0:
        return None
    fast = (site - len(c["x"]) + 1, bytes(len(c["x"]))) if err == 0 else O.try_cigar(c["x"], c["y"], site, err)
    if fast is not None:
        start, path = fast
    else:
        site2, err2, start, path = O.bpm_path(c["x"], c["y"], c["k"], wide=c["k"] > 31)
        assert (site2, err2) == (site, err)
    st, en, er, cg = O.generate_cigar(path, c["x"], c["y"], start, site, err)
    ops, num = [], ""
    for ch in cg:
        if ch.isdigit():
            num += ch
        else:
            ops += [OPS[ch]] * int(num); num = ""
    if len(ops) > 416:
        return "too long"        # more ops than a path record holds: the window is left without a path (wide bands only)
    return er, st, en, bytes(ops)


def check_paths(items, res, paths, tasks=None, describe=repr):
    """fsv_bpm_paths' output against expected().  items: (x, ypad, k, origin) per task (None: a window the geometry rejects, which
    must come back without result and without path), ypad the x_len + 2k columns of y the window is
    compared with ('N' outside the read) and origin the read position of its first column (the task's y_start - k): ry_start / ry_end
    are read positions.  tasks: when given, the record's y_rev / y_word / y_len must be the task's.  -> number of paths checked"""
    n = 0
    assert len(items) == len(res) == len(paths)
    for i, (item, r, p) in enumerate(zip(items, res, paths)):
        if item is None:
            assert int(r["err"]) < 0 and int(p["state"]) == 0, describe(i)
            continue
        x, ypad, k, origin = item
        e = expected({"k": k, "x": x, "y": ypad})
        if e is None:
            assert int(r["err"]) < 0 and int(p["state"]) == 0, describe(i)
            continue
        if e == "too long":
            assert int(p["state"]) == 0, describe(i)
            continue
        n += 1
        er, st, en, ops = e
        assert int(p["state"]) == 1, describe(i)
        assert (int(p["err"]), int(p["ry_start"]), int(p["ry_end"])) == (er, st + origin, en + origin), (describe(i), e[:3])
        assert _lib.path_ops(p) == ops, describe(i)
        if tasks is not None:
            t = tasks[i]
            assert (int(p["y_rev"]), int(p["y_word"]), int(p["y_len"])) == (int(t["y_rev"]), int(t["y_word"]), int(t["y_len"])), describe(i)
    return n


def check(ctx, cases):
    """cases as the goldens give them: x, and y with its out-of-read columns as 'N' at the ends (padl of them in front: the window's
    first column is read position -padl)"""
    cases = [c for c in cases if usable(c)]
    words, tasks = tasks_from_cases(cases)
    res, paths = ctx.bpm_paths(words, tasks)
    return check_paths([(c["x"], c["y"], c["k"], -strip_pad(c["y"])[0]) for c in cases], res, paths, describe=lambda i: cases[i])


def test_k6_golden(ctx, golden_dir):
    """the goldens were minted from the reference's pure DP (old_error = -1); wherever the assembler's gap-free shortcut does not
    apply, or gives the same path, the GPU must reproduce the reference's own output"""
    cases = [c for c in json.load(open(os.path.join(golden_dir, "bpm_k6.json")))["cases"] if usable(c)]
    assert check(ctx, cases) > 150
    words, tasks = tasks_from_cases(cases)
    res, paths = ctx.bpm_paths(words, tasks)
    n_ref = 0
    for c, p in zip(cases, paths):
        if c["err"] < 0:
            continue
        site, err = O.bpm(c["x"], c["y"], c["k"])
        if err > 0 and O.try_cigar(c["x"], c["y"], site, err) is not None:
            continue   # the shortcut may pick another of the equally good paths
        ops, num = [], ""
        for ch in c["cigar"]:
            if ch.isdigit():
                num += ch
            else:
                ops += [OPS[ch]] * int(num); num = ""
        assert _lib.path_ops(p) == bytes(ops) and int(p["err"]) == c["cigar_err"], c
        n_ref += 1
    assert n_ref > 100


def test_k6_random_vs_oracle(ctx):
    rng = random.Random(6)
    cases = []
    for i in range(6000):
        n = 375 if i % 3 else rng.randint(8, 375)
        k = 15 if n == 375 else max(1, int(n * 0.04))
        core = "".join(rng.choice("ACGT") for _ in range(n + 2 * k + 40))
        x = core[20 + k: 20 + k + n]
        rate = rng.choice([0.0, 0.003, 0.003, 0.01, 0.03])
        other = []
        for ch in core:
            r = rng.random()
            if r < rate / 3: other.append(rng.choice("ACGT"))
            elif r < 2 * rate / 3: other.append(ch + rng.choice("ACGT"))
            elif r < rate: pass
            else: other.append(ch)
        other = "".join(other)
        d = rng.choice([0, 0, 1, -1, 2])
        y = other[20 + d: 20 + d + n + 2 * k]
        if len(y) < n + 2 * k:
            y = y + "N" * (n + 2 * k - len(y))
        cases.append({"k": k, "x": x, "y": y})
    assert check(ctx, cases) > 3000


def test_k6_single_indels_in_repeats(ctx):
    """one inserted or deleted base inside low-complexity sequence: many equally good gap placements, the reference's walk-back
    and greedy left shift decide"""
    rng = random.Random(66)
    cases = []
    for i in range(3000):
        n = rng.choice([375, 375, 120, 40])
        k = 15 if n == 375 else max(1, int(n * 0.04))
        unit = "".join(rng.choice("ACGT") for _ in range(rng.randint(1, 4)))
        core = []
        while len(core) < n + 2 * k + 8:
            if rng.random() < 0.5:
                core += list(unit * rng.randint(2, 12))
            else:
                core += [rng.choice("ACGT") for _ in range(rng.randint(1, 30))]
        core = "".join(core)[: n + 2 * k + 8]
        x = core[k: k + n]
        y = list(core)
        p = rng.randrange(k, k + n)
        if i % 2:
            del y[p]
        else:
            y.insert(p, rng.choice("ACGT"))
        y = "".join(y)[: n + 2 * k]
        if len(y) < n + 2 * k:
            y += "N" * (n + 2 * k - len(y))
        cases.append({"k": k, "x": x, "y": y})
    assert check(ctx, cases) > 2000


def test_k6_wide_bands_vs_oracle(ctx):
    """paths of wide-band windows (k up to 95): walk, generate_cigar and record identical to the oracle's; a path of more than
    416 ops leaves the window without a record"""
    from tests.test_oracle_bpm import _noisy_cases
    cases = _noisy_cases(22, 2500, [40, 63, 80, 93, 95], rates=(0.02, 0.1, 0.2, 0.25))
    assert check(ctx, cases) > 800


# ---- windows at real read geometry (tests/kernel_cases.py: placements) ------------------------------------------
# the placements of test_gpu_k5.py through fsv_bpm_paths: every walk kernel has a strand-aware y fetch of its own

PROFILES = ["main", "wide"]
CLASSES = [c for c in KC.K6_CLASSES if c != "k>31"]


def run_and_check(ctx, P):
    words, tasks = P.pack()
    res, paths = ctx.bpm_paths(words, tasks)
    KC.check_windows(P, res)
    items = []
    for i, s in enumerate(P.specs):
        x, ypad, k, geom = P.operands(i)
        items.append((x, ypad, k, s["y_start"] - k) if geom is not None else None)
    return check_paths(items, res, paths, tasks, describe=lambda i: KC.describe(P, i))


@pytest.mark.parametrize("profile", PROFILES)
def test_k6_placements_vs_oracle(ctx, profile):
    """paths, intervals and record headers of every window of the list against the oracle; the list must fill every list
    k_path_fast sorts windows into (classes from the oracle alone), on both strands -- a class without windows tests no kernel"""
    P = KC.suite_list(profile)
    C = P.coverage()
    print("\nK6", profile, len(P.specs), "tasks:", {c: (C[c, 0], C[c, 1]) for c in KC.K6_CLASSES})
    KC.check_floors(C, CLASSES if profile == "main" else ["k>31"], 300, 100)
    assert run_and_check(ctx, P) == C["hits"]      # no path here is too long for its record


@pytest.mark.parametrize("profile", PROFILES)
def test_k6_placements_at_the_end_of_the_store(ctx, profile):
    for P, last, residue in KC.suite_end_stores(profile):
        run_and_check(ctx, P)
        assert any(KC.at_store_end(P, i) and P.hit(i)[1] >= 0 for i in range(len(P.specs))), (last, residue)


@pytest.mark.parametrize("profile", PROFILES)
def test_k6_placements_order_and_list_length(ctx, profile):
    """the ballot that sorts windows into lists works per wave, the grids round to blocks and to 8 blocks: permuting the tasks or
    cutting the list at those edges must not change any window's result or path"""
    P = KC.suite_list(profile)
    words, tasks = P.pack()
    res, paths = ctx.bpm_paths(words, tasks)
    order = list(range(len(tasks)))
    random.Random(606).shuffle(order)
    res2, paths2 = ctx.bpm_paths(words, P.pack(order=order)[1])
    assert not KC.differing_results(res2, res[order])
    assert not KC.differing_paths(paths2, paths[order])
    for n in KC.PREFIXES:
        assert n <= len(tasks)
        res2, paths2 = ctx.bpm_paths(words, tasks[:n])
        assert not KC.differing_results(res2, res[:n]), n
        assert not KC.differing_paths(paths2, paths[:n]), n


@pytest.mark.parametrize("profile", PROFILES)
def test_k6_placements_ignore_other_reads(ctx, profile):
    """two stores that differ only in the reads in front of and behind every read of the list (all A / random bases) and in their
    slack words: identical results and paths, and equal to those of the store without the extra reads (word offsets aside)"""
    P = KC.suite_list(profile)
    res, paths = ctx.bpm_paths(*P.pack())
    res_a, paths_a = ctx.bpm_paths(*P.pack(filler="A", seed=8))
    res_r, paths_r = ctx.bpm_paths(*P.pack(filler="random", seed=8))
    assert not KC.differing_results(res_a, res_r)
    assert not KC.differing_paths(paths_a, paths_r)
    assert not KC.differing_results(res_a, res)
    assert not KC.differing_paths(paths_a, paths, ignore_y_word=True)
    for Q, last, residue in KC.suite_end_stores(profile):
        res_a, paths_a = ctx.bpm_paths(*Q.pack(filler="A", seed=residue))
        res_r, paths_r = ctx.bpm_paths(*Q.pack(filler="random", seed=residue))
        assert not KC.differing_results(res_a, res_r), (last, residue)
        assert not KC.differing_paths(paths_a, paths_r), (last, residue)
