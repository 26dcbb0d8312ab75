"""Minimizer-sketch cases over the whole (w, k, HPC) range the library accepts: one deterministic generator, shared by the CPU tests
(oracle against the reference-minted digests of tests/golden/sketch_grid.json.gz) and the -m gpu tests (both kernels against the oracle).

Lengths are counted in ENTRIES -- the bases that are left after homopolymer compression, i.e. what the window of w slides over --
because every edge of the kernels is an edge in entries: T0 = w + k - 2 is the entry of the first full window, the position-parallel
kernel works in tiles of 1 024 entries.  With hpc = 1 the compressed sequence is built first and its runs are expanded afterwards.
Every case has a random.Random of its own, seeded by a string of its grid point, kind and tag, so dropping or adding cases never
changes another case's sequence.  What the cases exercise is counted by coverage() from the oracle alone."""
import base64
import hashlib
import random

WS = (1, 2, 3, 15, 16, 17, 31, 32, 33, 51, 63, 64, 65, 100, 128, 129, 200, 254, 255)
KS = (1, 2, 3, 15, 19, 20, 31, 32, 33, 50, 51, 62, 63)
GRID = tuple((w, k, hpc) for w in WS for k in KS for hpc in (0, 1))
TILE = 1024                     # entries per tile of the position-parallel kernel (SKF_T)
HP_RUNS = (1, 1, 2, 3, 5, 9, 40, 254, 255, 256, 300)
SHORT_RUNS = (1, 1, 1, 2, 3, 6)
KINDS = ("edge", "tandem", "homopolymer", "endrun")
COUNTS = ("short", "first_window", "tied_flush", "wide_span", "two_tiles")


def gpu_limit(w, k, variant):
    """why fsv_sketch_reads refuses this grid point (None: it is accepted).  The position-parallel kernel (odd k, variant 0) holds
    w <= 255; the replay kernel (even k, or variant 1) keeps its deque of w slots per lane in LDS and is documented for w <= 64."""
    if (k % 2 == 0 or variant == 1) and w > 64:
        return "replay kernel: w <= 64"
    return None


def edge_lengths(w, k):
    """entry counts around every edge: one window, the first full window, 64 lanes / 16-base words, one and two tiles, and the
    mask i < TILE + w - 1 of the sliding-maximum pass; 48..63 gives every residue mod 16 below 64 (replay lanes with empty slices)"""
    t0 = w + k - 2
    n = {1, 2, k - 1, k, k + 1, t0 - 1, t0, t0 + 1, t0 + 2, t0 + w, 63, 64, 65, TILE - 1, TILE, TILE + 1, TILE + w - 2, TILE + w - 1,
         TILE + w, 2 * TILE + t0}
    n |= set(range(48, 64))
    return sorted(x for x in n if x >= 1)


def _rng(w, k, hpc, kind, tag):
    return random.Random("sketch-grid/%d/%d/%d/%s/%s" % (w, k, hpc, kind, tag))


def _compressed(rng, n):
    """n bases, no two neighbours alike"""
    c = rng.randrange(4)
    out = [c]
    for d in rng.choices((1, 2, 3), k=n - 1):
        c = (c + d) & 3
        out.append(c)
    return "".join("ACGT"[c] for c in out)


def _expand(rng, comp, runs):
    return "".join(b * n for b, n in zip(comp, rng.choices(runs, k=len(comp))))


def _oracle_entries(seq, k, hpc):
    from tests import oracle_lib as O
    return O.sketch_info(seq, 1, k, hpc)[1]


def _entries_seq(rng, n, hpc, k):
    """a random sequence of exactly n entries.  For an odd k the entries are the compressed bases.  For an even k they are fewer:
    ha_sketch skips, as palindromes, the k-mers whose high bit plane is its own reverse complement (sketch.cpp:84; every other
    2-mer, one 20-mer in 1 024), also among the first k - 1 bases, so there the oracle counts them: the sequence is the shortest
    prefix of a longer random one that has n entries (one more base adds one entry or none)."""
    m = n if k & 1 else 2 * n + 4 * k + 64
    seq = _expand(rng, _compressed(rng, m), SHORT_RUNS) if hpc else "".join(rng.choices("ACGT", k=m))
    if k & 1:
        return seq
    while _oracle_entries(seq, k, hpc) < n:     # (two compressed 2-mers in three are skipped)
        seq += "ACGT"[("ACGT".index(seq[-1]) + 1) & 3] + _entries_seq(rng, m, hpc, 1)
    lo, hi = 1, len(seq)          # smallest prefix with >= n entries
    while lo < hi:
        mid = (lo + hi) // 2
        if _oracle_entries(seq[:mid], k, hpc) >= n:
            hi = mid
        else:
            lo = mid + 1
    assert _oracle_entries(seq[:lo], k, hpc) == n
    return seq[:lo]


def _tandem_units(w, k):
    return sorted({u for u in (1, 2, 3, 5, 7, w - 1, w, w + 1, k, 37) if u >= 1})


def _homopolymer_rich(rng, n_runs, runs, long_every=0):
    """n_runs runs; with long_every, one run in long_every comes from HP_RUNS' long end and the others from the short end.  A run of
    300 is forced across base 4 096 (the end of the first 256-word tile of phase 0) once the read gets there, and the last run is 256
    long, so a >= 256 run also touches the read's end.  Any run above 16 bases crosses a 16-base word."""
    out, total, c, crossed = [], 0, rng.randrange(4), False
    for i in range(n_runs):
        c = (c + rng.choice((1, 2, 3))) & 3
        if long_every:
            n = rng.choice(HP_RUNS[6:]) if rng.randrange(long_every) == 0 else rng.choice(HP_RUNS[:6])
        else:
            n = rng.choice(runs)
        if not crossed and 3800 <= total < 4096:
            n, crossed = 300, True
        if i == n_runs - 1:
            n = 256
        out.append("ACGT"[c] * n)
        total += n
    return "".join(out)


def cases_for(w, k, hpc):
    """every case of one grid point: dicts with w, k, hpc, kind, tag, seq"""
    t0 = w + k - 2
    out = []

    def add(kind, tag, seq):
        out.append({"w": w, "k": k, "hpc": hpc, "kind": kind, "tag": str(tag), "seq": seq})

    for n in edge_lengths(w, k):
        add("edge", n, _entries_seq(_rng(w, k, hpc, "edge", n), n, hpc, k))
    # tandem repeats: every k-mer recurs with the unit's period, so window minima tie; lengths straddle the first full window -- T0
    # (no full window: the last of the tied minima alone), T0 + 1 (the first full window, where copies of the partial window's
    # minimum are flushed, is the last), T0 + 3 -- and one tile.  Unit 1 is a homopolymer: one entry under compression.
    # The AT unit makes every odd k-mer the reverse complement of its neighbour: one hash for all entries, also under compression.
    # The ACGT unit does the same for an even k: every other k-mer is skipped as a palindrome, the ones between are each other's
    # reverse complement -- the only way to a tie between the two entries of w = 3's partial window under compression.
    lengths = tuple(n for n in (t0, t0 + 1) if n >= 1) + (t0 + 3, TILE + w + 5)
    for u in _tandem_units(w, k):
        for n in lengths:
            rng = _rng(w, k, hpc, "tandem", "%d/%d" % (u, n))
            unit = "".join(rng.choices("ACGT", k=u))
            add("tandem", "%d/%d" % (u, n), (unit * (n // u + 1))[:n])
    for unit in ("AT", "ACGT"):
        for n in lengths:
            add("tandem", "%s/%d" % (unit, n), (unit * n)[:n if k & 1 else 2 * n])
    if hpc:   # the same with runs: a tandem repeat of the compressed sequence (n entries for an odd k), runs expanded per copy
        for u in (2, 3, 7):
            for n in tuple(n for n in (t0, t0 + 1) if n >= 1) + (t0 + w + 8,):
                rng = _rng(w, k, hpc, "tandem", "runs/%d/%d" % (u, n))
                unit = _compressed(rng, u)
                if unit[0] == unit[-1]:
                    unit = unit[:-1] + next(b for b in "ACGT" if b not in (unit[0], unit[-2]))
                add("tandem", "runs/%d/%d" % (u, n), _expand(rng, (unit * (n // u + 1))[:n], SHORT_RUNS))
    # homopolymer-rich: runs from HP_RUNS (saturating run lengths, spans of 256 and more, runs across words, tiles and the read's end)
    add("homopolymer", "dense", _homopolymer_rich(_rng(w, k, hpc, "homopolymer", "dense"), 64, HP_RUNS))
    add("homopolymer", "sparse", _homopolymer_rich(_rng(w, k, hpc, "homopolymer", "sparse"), t0 + w + 40, None, long_every=16))
    add("homopolymer", "long-first", "A" * 300 + _entries_seq(_rng(w, k, hpc, "homopolymer", "long-first"), t0 + 5, hpc, k) + "C" * 255)
    # a read that ends inside a run: the last run is cut short (2 bases of it are left), at the first full window and past one tile
    for n in (t0 + 1, TILE + 1):
        rng = _rng(w, k, hpc, "endrun", n)
        comp = _compressed(rng, n)
        add("endrun", n, _expand(rng, comp[:-1], SHORT_RUNS if hpc else (1,)) + comp[-1] * 2)
    return out


def all_cases():
    for (w, k, hpc) in GRID:
        yield from cases_for(w, k, hpc)


def fixture_cases(w, k, hpc):
    """the part of cases_for() that tests/golden/sketch_grid.json.gz records: every edge length at every grid point; of the other
    kinds a rotating few per grid point (the digests of all of them would be several times the largest fixture in the tree) --
    over the grid every kind, unit and length is recorded at many points"""
    cs = cases_for(w, k, hpc)
    rest = [c for c in cs if c["kind"] != "edge"]
    rot = (WS.index(w) * len(KS) + KS.index(k)) * 2 + hpc
    keep = {(rot * 5 + j * 7) % len(rest) for j in range(5)}
    return [c for c in cs if c["kind"] == "edge"] + [c for i, c in enumerate(rest) if i in keep]


SEQ_DIGEST, MZ_DIGEST = 4, 11   # base64 characters kept of an md5: 24 bits notice a drifted generator, 66 bits pin a result


def digest(data: bytes, n):
    """the first n base64 characters of the md5 (the fixture holds some 18 000 cases: full digests would make it the largest in the tree)"""
    return base64.b64encode(hashlib.md5(data).digest()).decode()[:n]


def seq_digest(seq):
    return digest(seq.encode(), SEQ_DIGEST)


def mz_text(mz):
    """the reference harness's reply format: hash:pos:rev:span, blank-separated"""
    return " ".join("%d:%d:%d:%d" % (int(m["hash"]), int(m["pos"]), int(m["rev"]), int(m["span"])) for m in mz)


def mz_digest(text):
    return digest(text.encode(), MZ_DIGEST)


# ---- what the cases exercise, counted from the oracle alone ------------------------------------------------------------------
def coverage(cases, oracle_info):
    """oracle_info(seq, w, k, hpc) -> (minimizers, entries, flushed copies, entries with span >= 256), as oracle_lib.sketch_info.
    -> {(w, k, hpc): {count name: reads}}:
      short         reads of at most T0 entries (no full window: only the last minimum is reported)
      first_window  reads of exactly T0 + 1 entries (the irregular first full window is also the last)
      tied_flush    reads whose partial first window has a tied minimum, the copies flushed at the first full window
      wide_span     reads with an entry whose k-mer spans 256 bases or more (no minimizer there)
      two_tiles     reads of more than 1 024 entries"""
    cov = {}
    for c in cases:
        w, k, hpc = c["w"], c["k"], c["hpc"]
        d = cov.setdefault((w, k, hpc), dict.fromkeys(COUNTS, 0))
        _, m, flushed, wide = oracle_info(c["seq"], w, k, hpc)
        t0 = w + k - 2
        d["short"] += m <= t0
        d["first_window"] += m == t0 + 1
        d["tied_flush"] += flushed > 0
        d["wide_span"] += wide > 0
        d["two_tiles"] += m > TILE
    return cov


def exempt(w, k, hpc, name):
    """the reason a count cannot be reached at a grid point (None: the floor applies)"""
    if name == "short" and w + k - 2 == 0:
        return "w = k = 1: T0 = 0, and every read has at least one entry"
    if name == "tied_flush" and w <= 2:
        return "the partial first window holds w - 1 entries: a tie needs two"
    if name == "wide_span" and not hpc:
        return "without compression a k-mer spans k <= 63 bases"
    return None


def check_floors(cov):
    """every count >= 1 at every grid point where the geometry allows it -> list of (grid point, count) that miss"""
    miss = []
    for gp in GRID:
        for name in COUNTS:
            if exempt(*gp, name) is None and cov.get(gp, {}).get(name, 0) < 1:
                miss.append((gp, name))
    return miss
