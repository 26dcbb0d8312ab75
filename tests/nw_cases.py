"""Pairs for the event DP alone (fsv_nw / orc_nw): one fixed list that puts every size class of run_nw on its boundaries, wraps
every LDS ring, runs four scoring sets in each class, and holds ties, reference N and both sides of the 1024-run CIGAR cap --
with two checks that share nothing with oracle/aln.c: cigar_score re-scores a CIGAR, plain_score is a score-only DP.
Shared by tests/test_oracle_nw.py (CPU: the oracle against both) and tests/test_gpu_nw.py (the kernels against the oracle)."""
from functools import lru_cache

import numpy as np

MAX_CELLS = 1 << 26           # fsv_aln_default_params / orc_aln_default_params
CG_CAP = 1024                 # ALN_CG_CAP: CIGAR runs per event

# (a, b, q, e, q2, e2); q2 < 0: single affine
ASM5 = (1, 19, 39, 3, 81, 1)
SINGLE = (2, 4, 4, 2, -1, -1)
DUAL_24 = (2, 4, 4, 2, 24, 1)
DUAL_41 = (1, 9, 16, 2, 41, 1)
PARAM_SETS = (ASM5, SINGLE, DUAL_24, DUAL_41)


def nw_class(ql, tl):
    """the kernel run_nw gives an event to (focalsv_amd/csrc/aln.hip: nw_class, NW_LDS_Q = 3072): 0 k_nw<256, 64>,
    3 k_nw_rows<256, 64>, 1 k_nw<3072, 1024>, 2 k_nw_any.  The tests only count cases per class with it."""
    return 0 if ql <= 256 else 3 if tl <= 256 else 1 if ql <= 3072 else 2


def set_params(p, params):
    """the six scoring fields of a parameter block (the oracle's or the library's)"""
    p.a, p.b, p.q, p.e, p.q2, p.e2 = params
    return p


def gap_cost(l, params):
    a, b, q, e, q2, e2 = params
    return q + e * l if q2 < 0 else min(q + e * l, q2 + e2 * l)


def cigar_score(t, q, cigar, params):
    """the score of a CIGAR (uint32 words, length << 4 | op; 0 M, 1 I, 2 D) under the parameters: a match a, a mismatch -b, a target
    base outside ACGT -1 whatever it faces, a gap run of l bases -min(q + e l, q2 + e2 l).  The CIGAR must consume both sequences."""
    a, b = params[0], params[1]
    i = j = sc = 0
    for w in cigar:
        op, n = int(w) & 0xf, int(w) >> 4
        assert n > 0 and op in (0, 1, 2), (op, n)
        if op == 0:
            ts, qs = np.frombuffer(t[i:i + n], np.uint8), np.frombuffer(q[j:j + n], np.uint8)
            assert len(ts) == n and len(qs) == n
            amb = ~np.isin(ts, np.frombuffer(b"ACGT", np.uint8))
            eq = (ts == qs) & ~amb
            sc += a * int(eq.sum()) - int(amb.sum()) - b * int(n - eq.sum() - amb.sum())
            i += n
            j += n
        else:
            sc -= gap_cost(n, params)
            if op == 1:
                j += n
            else:
                i += n
    assert i == len(t) and j == len(q), (i, len(t), j, len(q))
    return sc


def plain_score(t, q, params):
    """the best global score under the piecewise gap cost w(l) = min(q + e l, q2 + e2 l), score only: int64, one target base per
    row.  Per gap piece k a vertical state V_k(i, j) = max(V_k(i-1, j), H(i-1, j) - q_k) - e_k; a row's horizontal gaps come
    from a prefix maximum over the cells the row enters by a pair or a vertical gap,
        H(i, j) = max(D(i, j), max_k(max_{j' < j}(D(i, j') + e_k j') - q_k - e_k j)),  D = max(pair, V_1, V_2),
    (a horizontal gap that follows a horizontal gap is never better than the two as one: w(l1) + w(l2) >= w(l1 + l2)).
    The boundaries H(-1, j) = -w(j) and H(i, -1) = -w(i) come from the same w.  No traceback, no flags, no tie rule."""
    a, b = params[0], params[1]
    pieces = [(params[2], params[3])] + ([(params[4], params[5])] if params[4] >= 0 else [])
    ql = len(q)
    NEG = -(1 << 40)
    qa = np.frombuffer(q, np.uint8)
    cols = np.arange(ql + 1, dtype=np.int64)
    w = np.min([qk + ek * cols for qk, ek in pieces], axis=0)
    H = -w
    H[0] = 0
    V = [np.full(ql + 1, NEG, np.int64) for _ in pieces]
    for i in range(len(t)):
        tc = t[i]
        pair = np.full(ql, -1, np.int64) if tc not in b"ACGT" else np.where(qa == tc, a, -b).astype(np.int64)
        D = np.empty(ql + 1, np.int64)
        D[0] = -min(qk + ek * (i + 1) for qk, ek in pieces)
        D[1:] = H[:-1] + pair
        for k, (qk, ek) in enumerate(pieces):
            V[k] = np.maximum(V[k], H - qk) - ek
            V[k][0] = NEG                    # column -1 is the boundary itself
            np.maximum(D, V[k], out=D)
        Hn = D.copy()
        for qk, ek in pieces:
            best = np.maximum.accumulate(D + ek * cols)
            np.maximum(Hn[1:], best[:-1] - qk - ek * cols[1:], out=Hn[1:])
        H = Hn
    return int(H[ql])


# ------------------------------------------------------------------------------------------------ sequences
_A = np.frombuffer(b"ACGT", np.uint8)


def _rnd(rng, n, letters=4):
    return _A[rng.integers(0, letters, n)].tobytes()


def _subst(rng, s, rate, letters=4):
    b = bytearray(s)
    alpha = b"ACGT"[:letters]
    for i in np.nonzero(rng.random(len(b)) < rate)[0]:
        b[i] = alpha[(alpha.index(b[i]) + 1 + int(rng.integers(0, letters - 1))) % letters]
    return bytes(b)


def _indel(rng, s, at, size, letters=4):
    """size > 0: that many new bases in front of s[at]; size < 0: s[at : at - size] leaves"""
    return s[:at] + _rnd(rng, size, letters) + s[at:] if size > 0 else s[:at] + s[at - size:]


def related(rng, tl, ql, at=(), n_indel=3, letters=4):
    """(target of tl bases, query of ql): the query is the target with 0-3 % substitutions, a small indel (1-7 bases, alternately
    out and in) at every target position of `at`, n_indel more of 1-200 bases anywhere, and then one long indel that brings it
    to exactly ql bases -- only where the shape asks for one."""
    t = _rnd(rng, tl, letters)
    q = _subst(rng, t, float(rng.random()) * 0.03, letters)
    for n, pos in enumerate(sorted(at, reverse=True)):         # from the right: the positions in front stay where they are
        size = int(rng.integers(1, 8))
        q = _indel(rng, q, min(pos, len(q)), size if n & 1 else -min(size, max(0, len(q) - pos)), letters)
    for _ in range(n_indel):
        size = int(rng.choice([1, 1, 2, 3, 8, 40, 200]))
        size = min(size, max(1, len(q) // 4))
        pos = int(rng.integers(0, len(q) + 1))
        q = _indel(rng, q, pos, size if rng.random() < 0.5 else -min(size, len(q) - pos), letters)
    if len(q) > ql:
        pos = int(rng.integers(0, ql + 1))
        q = q[:pos] + q[pos + len(q) - ql:]
    elif len(q) < ql:
        pos = int(rng.integers(0, len(q) + 1))
        q = _indel(rng, q, pos, ql - len(q), letters)
    assert len(t) == tl and len(q) == ql and ql >= 1 and tl >= 1
    return t, q


def thinned(rng, tl, step, n_cut, first):
    """the cap construction: a random target and the target without one base every `step`, n_cut of them from base `first`"""
    t = _rnd(rng, tl)
    cut = set(range(first, first + step * n_cut, step))
    assert max(cut) < tl
    return t, bytes(c for i, c in enumerate(t) if i not in cut)


# the cap cases by name -> the number of CIGAR runs the oracle must give (test_oracle_nw.py): exactly the cap, or more
CAP_RUNS = {"cap-c2-1024": 1024, "cap-c2-1027": 1027, "cap-c1-1024": 1024, "cap-c1-over": None}
# removals of the class-1 cap pair at spacing 6: neighbouring removals merge where the bases in between repeat, so the counts
# were chosen with the oracle -- test_oracle_nw.py asserts what they give
CAP_C1_STEP, CAP_C1_EXACT, CAP_C1_OVER = 6, 517, 520


@lru_cache(maxsize=1)
def cases():
    """the fixed list of (name, target, query, params).  Queries hold only ACGT: the device stores a query N as a base hashed from
    its position, so a query N is outside the contract (N is allowed in reference windows only); targets may hold N.  Pairs are
    related -- mutated copies -- since under asm5 two unrelated sequences align as one long I plus one long D and the DP interior
    is never consulted.  Nothing is dropped: the largest shape is far below max_cells, which is asserted."""
    rng = np.random.default_rng(1024)
    out = []

    def add(name, t, q, params):
        assert len(t) * len(q) <= MAX_CELLS and all(c in b"ACGT" for c in set(q)), name
        out.append((name, t, q, params))

    # ---- boundary grid: every ql on either side of a class / block boundary against the short targets and one of its own size
    n = 0
    for ql in (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 3071, 3072, 3073):
        for k, tl in enumerate((1, 2, 255, 256, 257, max(1, ql + (3, -2, 0, 5)[n % 4]))):
            t, q = related(rng, tl, ql, n_indel=2)
            add("grid-q%d-t%d%s" % (ql, tl, "-near" if k == 5 else ""), t, q, PARAM_SETS[n % 4])
            n += 1
    for ql, tl in ((257, 1), (4000, 1), (1, 3000)):
        t, q = related(rng, tl, ql, n_indel=0)
        add("row-q%d-t%d" % (ql, tl), t, q, PARAM_SETS[n % 4])
        n += 1
    # ---- ring wraps, small indels on both sides of every wrap position, every parameter set
    for params in PARAM_SETS:
        s = "-p%d" % PARAM_SETS.index(params)
        for ql, tl in ((250, 513), (251, 1100)):                         # class 0: 512 target bases
            t, q = related(rng, tl, ql, at=[x for x in (470, 500, 530, 560, 1000, 1050) if x < tl])
            add("wrap-c0-q%d-t%d%s" % (ql, tl, s), t, q, params)
        for ql in (257, 1000, 3072):                                     # class 1: 4096 target bases
            t, q = related(rng, 4500, ql, at=(3900, 4050, 4140, 4300))
            add("wrap-c1-q%d%s" % (ql, s), t, q, params)
        for tl in (1, 200, 256):                                         # class 3: 512 query bases
            for ql in (600, 4000):
                # the target in two halves with the new bases between them, so that related bases lie behind the wraps too
                t, q0 = related(rng, tl, tl, at=[x for x in (tl // 4, 3 * tl // 4) if x], n_indel=0)
                h = len(q0) // 2
                q = q0[:h] + _rnd(rng, ql - len(q0)) + q0[h:]
                add("wrap-c3-q%d-t%d%s" % (ql, tl, s), t, q, params)
        t, q = related(rng, 257, 3073, n_indel=1)                        # class 2: its smallest shape
        add("small-c2%s" % s, t, q, params)
        t, q = related(rng, 3400, 3500, at=(500, 1700, 3000))
        add("wide-c2%s" % s, t, q, params)
        for ql, tl in ((3100, 300), (3329, 513)):                        # class 2 past a block of 256 columns, short targets
            t, q = related(rng, tl, ql, at=(100, 250))
            add("short-c2-q%d-t%d%s" % (ql, tl, s), t, q, params)
    # ---- ties: repeats and two letters, where the order diagonal > E > F > E2 > F2 and the continuation bits decide the CIGAR
    shapes = {0: (200, 230), 1: (400, 300), 3: (300, 200)}             # class -> (ql, tl)
    for cls, (ql, tl) in shapes.items():
        for params in (ASM5, SINGLE):
            s = "-c%d-p%d" % (cls, PARAM_SETS.index(params))
            for kind, unit in (("homopolymer", b"A"), ("dinucleotide", b"AC"), ("tandem7", b"ACGTTCA")):
                add("tie-%s%s" % (kind, s), (unit * tl)[:tl], (unit * ql)[:ql], params)
            t, q = related(rng, tl, ql, n_indel=4, letters=2)
            add("tie-two-letter%s" % s, t, q, params)
            # a unit fewer (or more) in a repeat that begins the pair, and in one that ends it
            m, grow = {0: (150, 0), 1: (300, 0), 3: (150, 100)}[cls]
            mid_t = _rnd(rng, m)
            mid_q = _subst(rng, mid_t, 0.01)
            mid_q = mid_q[:m // 2] + _rnd(rng, grow) + mid_q[m // 2:]
            add("tie-first-base%s" % s, b"AC" * 20 + mid_t + b"G" * 40, b"AC" * 18 + mid_q + b"G" * 40, params)
            add("tie-last-base%s" % s, b"G" * 40 + mid_t + b"CT" * 20, b"G" * 40 + mid_q + b"CT" * 22, params)
    # ---- reference N
    n = 0
    for cls, (ql, tl) in ((0, (240, 300)), (1, (700, 690)), (3, (600, 250)), (2, (3073, 300))):
        for run in (1, 5, 60):
            t, q = related(rng, tl, ql, n_indel=2)
            at = tl // 3
            add("N-run%d-c%d" % (run, cls), t[:at] + b"N" * run + t[at + run:], q, PARAM_SETS[n % 4])
            n += 1
    for params in (ASM5, SINGLE):
        s = "-p%d" % PARAM_SETS.index(params)
        t, q = related(rng, 4500, 1000, at=(4000, 4200))
        add("N-straddles-4096%s" % s, t[:4090] + b"N" * 12 + t[4102:], q, params)
        for ql, tl in ((200, 210), (600, 610), (600, 200)):
            t, q = related(rng, tl, ql, n_indel=1)
            add("N-first-base-q%d-t%d%s" % (ql, tl, s), b"N" + t[1:], q, params)
            add("N-last-base-q%d-t%d%s" % (ql, tl, s), t[:-1] + b"N", q, params)
            add("N-both-ends-q%d-t%d%s" % (ql, tl, s), b"NNN" + t[3:-2] + b"NN", q, params)
    # ---- the CIGAR cap: one base of a random target removed every `step`
    t, q = thinned(rng, 12 * 512, 12, 512, 0)                            # D M D M ... M: 2 x 512 runs
    add("cap-c2-1024", t, q, SINGLE)
    t, q = thinned(rng, 12 * 513 + 8, 12, 513, 5)                        # M D M ... D M: 2 x 513 + 1
    add("cap-c2-1027", t, q, SINGLE)
    t, q = thinned(rng, CAP_C1_STEP * CAP_C1_EXACT, CAP_C1_STEP, CAP_C1_EXACT, 0)
    add("cap-c1-1024", t, q, SINGLE)
    t, q = thinned(rng, CAP_C1_STEP * CAP_C1_OVER + 3, CAP_C1_STEP, CAP_C1_OVER, 2)
    add("cap-c1-over", t, q, SINGLE)
    assert len({c[0] for c in out}) == len(out)
    return tuple(out)


def by_class():
    """class -> its cases, in list order"""
    d = {0: [], 1: [], 2: [], 3: []}
    for c in cases():
        d[nw_class(len(c[2]), len(c[1]))].append(c)
    return d


def check_floors():
    """at least 20 cases in every class and every parameter set in every class; the cap cases where they belong"""
    d = by_class()
    for cls, cs in d.items():
        assert len(cs) >= 20, (cls, len(cs))
        assert {c[3] for c in cs} == set(PARAM_SETS), (cls, {c[3] for c in cs})
    assert sum(len(cs) for cs in d.values()) == len(cases())
    names = {c[0]: nw_class(len(c[2]), len(c[1])) for c in cases()}
    assert [names[k] for k in CAP_RUNS] == [2, 2, 1, 1]
    return {cls: len(cs) for cls, cs in d.items()}
