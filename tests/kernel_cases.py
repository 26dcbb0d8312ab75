"""Shared helpers: turn (x, y, k) window cases into a packed store + fsv_wtask array, and generate windows at real read geometry."""
import bisect
import functools
import math
import random

import numpy as np

from focalsv_amd import _lib


def strip_pad(y):
    padl = len(y) - len(y.lstrip("N"))
    padr = len(y) - len(y.rstrip("N"))
    return padl, padr, y[padl: len(y) - padr if padr else len(y)]


def tasks_from_cases(cases):
    """Each case's x and y become two reads; 'N' pads at the ends of y become out-of-read columns."""
    reads, meta = [], []
    for c in cases:
        padl, padr, core = strip_pad(c["y"])
        reads.append(c["x"])
        reads.append(core if core else "A")
        meta.append((padl, padr, len(core)))
    words, off, lens = _lib.pack_reads(reads)
    tasks = np.zeros(len(cases), dtype=_lib.WTASK_DTYPE)
    for i, c in enumerate(cases):
        padl, padr, ylen = meta[i]
        k = c["k"]
        tasks[i] = (off[2 * i], off[2 * i + 1], 0, k - padl, ylen, len(c["x"]), k, 0, i, 0)
    return words, tasks


def usable(c):
    """cases expressible as a task: pads only at the ends, no inner N, left pad <= k."""
    padl, padr, core = strip_pad(c["y"])
    return "N" not in core and "N" not in c["x"] and padl <= c["k"] and len(core) > c["k"] - padl >= 0 and len(c["x"]) >= 1


# ---- windows at real read geometry -------------------------------------------------------------------------
# tasks_from_cases puts every window at base 0 of two fresh reads, forward strand.  The generator below cuts windows out
# of read pairs the way the assembler does: any bit offset in x and in y, both strands, windows that end at a read's
# last base, windows clipped at either end of y, and the geometric rejection rule on both of its sides.  What each task
# should see (x, the padded y window, the clip geometry) is worked out here on plain strings, never through the library.

COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
JITTER = (0, 0, 1, -1, 2, -3)
MAIN_RATES = (0.0, 0.003, 0.01, 0.03, 0.06)
WIDE_RATES = (0.02, 0.1, 0.2, 0.25)
WIDE_KS = (40, 63, 80, 93, 95)
K6_CLASSES = ("gap-free", "err 1", "err 2", "err 3", "k<=15 err 4..7", "k<=15 err>7", "16<=k<=31 err>3", "k>31")
# the kernel that settles each class (k_path.h: k_path_fast sorts the windows, one walk kernel per list)
K6_KERNEL = {"gap-free": "k_path_fast/path_gapfree", "err 1": "k_path_fr<1>", "err 2": "k_path_fr<2>", "err 3": "k_path_fr<3>",
             "k<=15 err 4..7": "k_path_sb", "k<=15 err>7": "k_path_dp<uint32_t>", "16<=k<=31 err>3": "k_path_dp<uint64_t>",
             "k>31": "k_path_wide"}


def revcomp(s):
    return "".join(COMP[c] for c in reversed(s))


@functools.lru_cache(maxsize=64)
def _strand(y_read, y_rev):
    return revcomp(y_read) if y_rev else y_read


def overlap_region(y_start, y_len, x_len, k, k_cap):
    """determine_overlap_region (hifiasm-0.14 Correct.cpp:212-250) on plain integers: None when the window is geometrically
    impossible, else (y_beg, extra_begin, extra_end) of the padded window of x_len + 2k columns"""
    wlen = x_len + 2 * k
    if y_start < 0 or y_len <= y_start or y_len - y_start + 2 * k + k_cap < wlen:
        return None
    y_start -= k
    o_len = min(wlen, y_len - y_start)
    extra_begin, extra_end = 0, wlen - o_len
    if y_start < 0:
        extra_begin, y_start = -y_start, 0
    return y_start, extra_begin, extra_end


def padded_window(y_read, y_rev, y_start, x_len, k):
    """the x_len + 2k columns the kernels compare x with: column j is base y_start - k + j of the strand, 'N' outside the read"""
    s = _strand(y_read, y_rev)
    a = y_start - k
    return "".join(s[p] if 0 <= p < len(s) else "N" for p in range(a, a + x_len + 2 * k))


def k6_class(k, err, gapfree):
    """the list k_path_fast puts a hit on (k_path.h), from the oracle's numbers alone"""
    if gapfree:
        return "gap-free"
    if k > 31:
        return "k>31"
    if err <= 3:
        return "err %d" % err
    if k <= 15:
        return "k<=15 err 4..7" if err <= 7 else "k<=15 err>7"
    return "16<=k<=31 err>3"


_ACGT = bytes(ord("ACGT"[b & 3]) for b in range(256))


def _bases(rng, n):
    return rng.randbytes(n).translate(_ACGT).decode()


def _core(rng, n, low):
    if not low:
        return _bases(rng, n)
    unit = "".join(rng.choice("ACGT") for _ in range(rng.randint(1, 4)))   # as test_k6_single_indels_in_repeats builds it
    core = []
    while len(core) < n:
        if rng.random() < 0.5:
            core += list(unit * rng.randint(2, 12))
        else:
            core += list(_bases(rng, rng.randint(1, 30)))
    return "".join(core[:n])


class _Mutated:
    """a copy of `core` with substitutions, insertions and deletions at `rate`, and the map between the two coordinates"""

    def __init__(self, rng, core, rate):
        self.at, m = [], -1
        while rate:      # each base mutated with probability `rate`: geometric gaps between the mutated ones
            m += 1 + int(math.log(1.0 - rng.random()) / math.log(1.0 - rate))
            if m >= len(core):
                break
            self.at.append(m)
        self.shift, out, last, sh = [0], [], 0, 0
        for m in self.at:
            out.append(core[last:m])
            op = rng.randrange(3)
            if op == 0:
                out.append(rng.choice("ACGT"))
            elif op == 1:
                out.append(core[m] + rng.choice("ACGT")); sh += 1
            else:
                sh -= 1
            last = m + 1
            self.shift.append(sh)
        out.append(core[last:])
        self.seq, self.n = "".join(out), len(core)

    def pos(self, c):
        """where base c of the core went (a deleted base: where its successor went)"""
        return c + self.shift[bisect.bisect_left(self.at, c)]

    def inv(self, t):
        """the first core base that went to position t or beyond"""
        lo, hi = 0, self.n
        while lo < hi:
            mid = (lo + hi) // 2
            if self.pos(mid) < t:
                lo = mid + 1
            else:
                hi = mid
        return lo


def _pick_k(rng, n, wide):
    if wide:
        return rng.choice(WIDE_KS) if n >= 200 else rng.choice((1, 3, 8))
    return 15 if n == 375 else min(31, max(1, int(n * 0.04)) * rng.choice((1, 2)))


FORCED = ("left", "right", "rule-1", "rule+0", "rule+1", "neg", "past")


class Placements:
    """reads + tasks of one list.  specs[i] = dict(xi, yi, x_start, y_start, x_len, k, y_rev, kind); operands(i) gives the plain
    strings; pack() lays the reads out in a store (optionally with other reads in between) and fills in the word offsets."""

    def __init__(self):
        self.reads, self.specs, self.k_cap = [], [], 31
        self._ops, self._hit, self._cov = {}, {}, None

    def operands(self, i):
        """-> (x, ypad, k, geometry or None)"""
        if i not in self._ops:
            s = self.specs[i]
            y = self.reads[s["yi"]]
            x = self.reads[s["xi"]][s["x_start"]: s["x_start"] + s["x_len"]]
            assert len(x) == s["x_len"]
            self._ops[i] = (x, padded_window(y, s["y_rev"], s["y_start"], s["x_len"], s["k"]), s["k"],
                            overlap_region(s["y_start"], len(y), s["x_len"], s["k"], self.k_cap))
        return self._ops[i]

    def hit(self, i):
        """the oracle on task i -> (end site, err, K6 class or None); (-1, -1, None) for a window the geometry rejects"""
        if i not in self._hit:
            from tests import oracle_lib as O
            x, ypad, k, geom = self.operands(i)
            site, err = O.bpm(x, ypad, k) if geom is not None else (-1, -1)
            cls = None
            if err >= 0:
                cls = k6_class(k, err, err == 0 or O.try_cigar(x, ypad, site, err) is not None)
            self._hit[i] = (site, err, cls)
        return self._hit[i]

    def reject_kind(self, i):
        s = self.specs[i]
        return "y_start < 0" if s["y_start"] < 0 else "y_start >= y_len" if s["y_start"] >= len(self.reads[s["yi"]]) else "length rule"

    def coverage(self):
        """what the list exercises, counted from the inputs and the oracle alone: a Counter over plain names and (name, strand)"""
        if self._cov is None:
            import collections
            C = collections.Counter()
            for i, s in enumerate(self.specs):
                x, ypad, k, geom = self.operands(i)
                st = s["y_rev"]
                if geom is None:
                    C["rejected: " + self.reject_kind(i)] += 1
                    continue
                C["accepted"] += 1
                C["accepted", st] += 1
                C["x_start % 16 != 0"] += s["x_start"] % 16 != 0
                C["y offset % 16 != 0"] += (s["y_start"] - k) % 16 != 0 and s["y_start"] - k > 0
                y_len = len(self.reads[s["yi"]])
                C["accepted at the length rule"] += y_len - s["y_start"] + 2 * k + self.k_cap - (s["x_len"] + 2 * k) <= 1
                site, err, cls = self.hit(i)
                if err < 0:
                    continue
                for name in ("hits", cls) + (("left clip",) if geom[1] > 0 else ()) + (("right clip",) if geom[2] > 0 else ()):
                    C[name] += 1
                    C[name, st] += 1
                C["x ends at its read's last base"] += s["x_start"] + s["x_len"] == len(self.reads[s["xi"]])
            self._cov = C
        return self._cov

    def pack(self, filler=None, order=None, seed=0):
        """-> (words, tasks).  filler: None, or 'A' / 'random' -- a read of that content in front of the first read and behind
        every read, and the slack words behind the store set to match (all zero bits / random bits); the lengths of the fillers
        depend on `seed` alone, so two stores built with different content have the same layout.  order: task permutation."""
        from focalsv_amd import _lib
        reads, at = [], []
        if filler is None:
            reads, at = list(self.reads), list(range(len(self.reads)))
        else:
            lrng, crng = random.Random(seed), random.Random(seed + 1)
            fill = (lambda n: "A" * n) if filler == "A" else (lambda n: _bases(crng, n))
            reads.append(fill(lrng.randint(1, 48)))
            for r in self.reads:
                at.append(len(reads))
                reads.append(r)
                reads.append(fill(lrng.randint(1, 100)))
        words, off, lens = _lib.pack_reads(reads)
        used = int(off[len(reads)])
        if filler == "random":
            words[used:] = np.frombuffer(crng.randbytes(4 * (len(words) - used)), dtype=np.uint32)
        else:
            words[used:] = 0
        idx = list(range(len(self.specs))) if order is None else list(order)
        tasks = np.zeros(len(idx), dtype=_lib.WTASK_DTYPE)
        for j, i in enumerate(idx):
            s = self.specs[i]
            tasks[j] = (off[at[s["xi"]]], off[at[s["yi"]]], s["x_start"], s["y_start"], len(self.reads[s["yi"]]), s["x_len"], s["k"], s["y_rev"], 0, j)
        return words, tasks


def _add_pair(P, rng, pair_no, wide, shape="any", rate=None, forced=(), res_x=None, res_y=None, y_last=True):
    """one (x read, y read) pair cut from one sequence, its tiling windows and the forced edge windows it can hold.
    shape: 'any' -- both reads start and end within 60 bases of the sequence's ends; 'x_in_y' / 'y_in_x' -- one read lies
    inside the other with at least 40 bases to spare on both sides."""
    low = pair_no % 4 == 3
    y_rev = pair_no & 1
    rates = WIDE_RATES if wide else MAIN_RATES
    rate = rates[(pair_no // 2) % len(rates)] if rate is None else rate
    core = _core(rng, rng.randint(540, 2980), low)
    mut = _Mutated(rng, core, rate)
    cx = [rng.randint(0, 60), rng.randint(0, 60)]      # bases cut off x in front / behind
    cy = [rng.randint(0, 60), rng.randint(0, 60)]
    if shape == "x_in_y":
        cx, cy = [rng.randint(45, 60), rng.randint(45, 60)], [0, 0]
    elif shape == "y_in_x":
        cx, cy = [0, 0], [rng.randint(45, 60), rng.randint(45, 60)]
    # lengths cover every residue modulo 16: the last few bases are trimmed until the residue is the wanted one
    res_x = pair_no % 16 if res_x is None else res_x
    res_y = (pair_no * 7 + 3) % 16 if res_y is None else res_y
    x_read = core[cx[0]: len(core) - cx[1]]
    x_read = x_read[: len(x_read) - (len(x_read) - res_x) % 16]
    y_fwd = mut.seq[cy[0]: len(mut.seq) - cy[1]]
    y_fwd = y_fwd[: min(len(y_fwd), 3000)]
    y_fwd = y_fwd[: len(y_fwd) - (len(y_fwd) - res_y) % 16]
    xl, yl = len(x_read), len(y_fwd)
    assert 400 <= xl <= 3000 and 400 <= yl <= 3000
    xi = len(P.reads)
    if y_last:
        P.reads += [x_read, revcomp(y_fwd) if y_rev else y_fwd]
        yi = xi + 1
    else:
        P.reads += [revcomp(y_fwd) if y_rev else y_fwd, x_read]
        xi, yi = xi + 1, xi

    def partner(xs):
        return mut.pos(cx[0] + xs) - cy[0]

    def x_for(ys):
        return mut.inv(ys + cy[0]) - cx[0]

    def add(xs, n, k, ys, kind):
        assert 0 <= xs and xs + n <= xl and 1 <= n <= 375
        P.specs.append(dict(xi=xi, yi=yi, x_start=xs, y_start=ys, x_len=n, k=k, y_rev=y_rev, kind=kind, pair=pair_no))

    xs = rng.randint(0, 15)
    while xs < xl:
        n = 375 if rng.random() < 0.6 else rng.randint(1, 375)
        n = min(n, xl - xs)           # the last window ends at the read's last base
        add(xs, n, _pick_k(rng, n, wide), partner(xs) + rng.choice(JITTER), "tile")
        xs += n
    for kind in forced:
        n = 375 if rng.random() < 0.6 else rng.randint(130 if wide else 40, 375)
        k = _pick_k(rng, n, wide)
        if kind == "left":            # y_start in 0..k-1: the padded window starts before the read
            ys = rng.randint(0, k - 1)
        elif kind == "right":         # the padded window runs 1..2k bases past the read
            ys = yl + rng.randint(1, 2 * k) - n - k
        elif kind.startswith("rule"): # y_len - y_start + 2k + k_cap = wlen - 1, wlen, wlen + 1
            ys = yl + P.k_cap - n - int(kind[4:])
        elif kind == "neg":
            ys = -rng.randint(1, 20)
        elif kind == "past":
            ys = yl + rng.randint(0, 20)
        else:                          # "xend": one more window that ends at x's last base, on its true diagonal
            add(xl - n, n, k, partner(xl - n), kind)
            continue
        xs = x_for(ys)
        if kind in ("left", "right"):
            if xs < 0 or xs + n > xl or not 0 <= ys < yl:
                continue               # this pair does not hold the placement
            ys = partner(xs)           # a base deleted there moves it by one
            if kind == "left" and not 0 <= ys < k:
                continue
            if kind == "right" and not 1 <= ys + n + k - yl <= 2 * k:
                continue
        else:
            xs = min(max(xs, 0), xl - n)
        add(xs, n, k, ys, kind)


def _widest_first(P):
    """a wide list starts with a task of the largest threshold, so that every prefix of it takes the wide kernels with the same k_cap"""
    assert max(s["k"] for s in P.specs) <= P.k_cap
    if P.k_cap > 31:
        i = next((i for i, s in enumerate(P.specs) if s["k"] == P.k_cap), None)
        if i is None:     # a small list whose draws missed it: one window of 200 bases or more takes it (its rule draws from WIDE_KS)
            i = next(i for i, s in enumerate(P.specs) if s["x_len"] >= 200 and s["kind"] == "tile")
            P.specs[i]["k"] = P.k_cap
        P.specs[0], P.specs[i] = P.specs[i], P.specs[0]


@functools.lru_cache(maxsize=None)
def placements(seed, profile="main", n_pairs=2400):
    """the main list of a profile ('main': k <= 31; 'wide': k from WIDE_KS, everything through the wide kernels)"""
    rng = random.Random(seed)
    wide = profile == "wide"
    P = Placements()
    P.k_cap = max(WIDE_KS) if wide else 31
    for p in range(n_pairs):
        # four forced kinds per pair, rotating so that each kind meets both strands, every rate and both kinds of sequence
        shape = ("any", "y_in_x", "any", "any")[(p // 2) % 4]
        f = [FORCED[(p // 2 + j) % len(FORCED)] for j in range(2)]
        if shape == "y_in_x":
            f = [("left", "right")[(p // 8) % 2]] + f
        _add_pair(P, rng, p, wide, shape=shape, forced=f)
    _widest_first(P)
    return P


@functools.lru_cache(maxsize=None)
def end_of_store_placements(seed, profile="main"):
    """32 small stores: for each residue of the last read's length modulo 16, one whose last read is an x read and one whose last
    read is a y read.  The last pair's other read reaches past the last read at both ends, so the windows at the last read's ends are
    real placements; -> list of (Placements, 'x' | 'y', residue)"""
    rng = random.Random(seed)
    wide = profile == "wide"
    out = []
    for res in range(16):
        for last in "xy":
            P = Placements()
            P.k_cap = max(WIDE_KS) if wide else 31
            for p in range(3):
                _add_pair(P, rng, 2 * p + res, wide, forced=("left", "right"))
            rate = 0.02 if wide else 0.003
            if last == "x":
                _add_pair(P, rng, 6 + res, wide, shape="x_in_y", rate=rate, res_x=res, y_last=False, forced=("xend", "xend"))
            else:
                _add_pair(P, rng, 6 + res, wide, shape="y_in_x", rate=rate, res_y=res, forced=("left", "right") * 3)
            _widest_first(P)
            out.append((P, last, res))
    return out


def at_store_end(P, i):
    """task i reads the last base the store holds: x ends at the last read's last base, or the padded y window covers the stored
    last base of the last read (the strand's last base forward, its first base on the reverse strand)"""
    s = P.specs[i]
    last = len(P.reads) - 1
    if s["xi"] == last:
        return s["x_start"] + s["x_len"] == len(P.reads[last])
    if s["yi"] == last:
        a = s["y_start"] - s["k"]
        return a <= 0 if s["y_rev"] else a + s["x_len"] + 2 * s["k"] >= len(P.reads[last])
    return False


def describe(P, i):
    """task i for an assertion message: the fields, the operands and the kernel its class goes to"""
    s, (x, ypad, k, geom), (site, err, cls) = P.specs[i], P.operands(i), P.hit(i)
    return dict(task=i, spec={f: s[f] for f in ("x_start", "y_start", "x_len", "k", "y_rev", "kind")}, y_len=len(P.reads[s["yi"]]),
                geometry=geom, oracle=(site, err), k6_class=cls, kernel=K6_KERNEL.get(cls), x=x, ypad=ypad)


def check_windows(P, res, idx=None):
    """fsv_wres of P's tasks (idx: which task each result row belongs to) against the oracle on the plain operands and the restated
    geometry -> number of hits"""
    idx = range(len(P.specs)) if idx is None else idx
    assert len(res) == len(idx)
    n_hit = 0
    for r, i in zip(res, idx):
        geom = P.operands(i)[3]
        got = (int(r["end_site"]), int(r["err"]), int(r["y_beg"]), int(r["extra_begin"]), int(r["extra_end"]))
        if geom is None:
            assert got == (-1, -1, -1, -1, -1), ("rejected window (%s)" % P.reject_kind(i), got, describe(P, i))
            continue
        site, err, cls = P.hit(i)
        assert got[2:] == geom, ("window geometry", got, describe(P, i))
        assert got[1] == err, ("K5 distance", got, describe(P, i))
        if err >= 0:
            n_hit += 1
            assert got[0] == site, ("K5 end site", got, describe(P, i))
    return n_hit


def differing_results(res_a, res_b):
    """rows (the first few) in which two runs' fsv_wres differ; empty when they agree"""
    assert len(res_a) == len(res_b)
    return [(int(j), res_a[j], res_b[j]) for j in np.nonzero(res_a != res_b)[0][:5]]


def differing_paths(paths_a, paths_b, ignore_y_word=False):
    """rows (the first few) in which two runs' fsv_wpath records differ in something a consumer may read: the header fields, and
    the ops up to path_len (the bytes behind them are nobody's business)"""
    from focalsv_amd import _lib
    assert len(paths_a) == len(paths_b)
    fields = ["ry_start", "ry_end", "path_len", "err", "state", "y_rev", "pad", "y_len"] + ([] if ignore_y_word else ["y_word"])
    raw = (paths_a.view(np.uint8).reshape(len(paths_a), -1) != paths_b.view(np.uint8).reshape(len(paths_b), -1)).any(axis=1)
    out = []
    for j in np.nonzero(raw)[0]:
        a, b = paths_a[j], paths_b[j]
        if any(a[f] != b[f] for f in fields) or (int(a["state"]) == 1 and _lib.path_ops(a) != _lib.path_ops(b)):
            out.append((int(j), a, b))
            if len(out) == 5:
                break
    return out


PREFIXES = (1, 63, 64, 65, 255, 256, 257, 2049)     # wave, block and 8-block rounding edges of the launches


def check_floors(C, names, total, per_strand):
    for name in names:
        assert C[name] >= total and min(C[name, 0], C[name, 1]) >= per_strand, (name, K6_KERNEL.get(name), C[name], C[name, 0], C[name, 1])


# what the GPU tests of K5/K6 and the CPU test of the generator run: one seed, one size per profile
SEED = 56
PAIRS = {"main": 2400, "wide": 500}


def suite_list(profile):
    return placements(SEED, profile, PAIRS[profile])


def suite_end_stores(profile):
    return end_of_store_placements(SEED + 1, profile)
