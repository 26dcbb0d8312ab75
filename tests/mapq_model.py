"""Python model of the chromosome index and of the contig records' mapping quality (fsv_ref_index_*, fsv_contig_mapq): tiles and
ownership, the N rule, the table as a dict, the query set and its thinning, the three hit classes, the occurrence cutoff c*, the
reference-major chain DP and mapq_of (Li 2018, Bioinformatics 34:3094, section 2.1.4).  It sketches through tests/oracle_lib.sketch and
restates n_substitute and chain_dp from oracle/aln.c.  TEST INFRASTRUCTURE."""
import math

import numpy as np

from tests import oracle_lib as O

TILE, HALO, AMAX, QMAX = 65536, 64, 8192, 4096
MQ_TRUNC = 1


def n_substitute(pos):
    """oracle/aln.c:n_substitute on an array of positions (32-bit wrap-around arithmetic)"""
    x = (np.asarray(pos, dtype=np.uint64) * 0x9E3779B1) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x85EBCA77) & 0xFFFFFFFF
    x ^= x >> 13
    return (x >> 30).astype(np.uint8)


def seed_text(seq):
    """-> (the text the seeds are taken from: an N holds the base hashed from its position, N mask as a bool array)"""
    b = (seq.encode() if isinstance(seq, str) else bytes(seq)).upper()
    a = np.frombuffer(b, dtype=np.uint8).copy()
    mask = ~np.isin(a, np.frombuffer(b"ACGT", dtype=np.uint8))
    at = np.nonzero(mask)[0]
    a[at] = np.frombuffer(b"ACGT", dtype=np.uint8)[n_substitute(at)]
    return a.tobytes().decode(), mask


def table_slots(entries):
    n = 1024
    while n < 2 * entries:
        n <<= 1
    return n


class Index:
    def __init__(self, seq, k=19, w=19, max_occ=50, tiled=True):
        """tiled=False: the same sequence sketched in one piece (what the tiling must reproduce)"""
        self.k, self.w, self.max_occ, self.len = k, w, max_occ, len(seq)
        text, mask = seed_text(seq)
        ncum = np.concatenate([[0], np.cumsum(mask)])
        n_tiles = (len(seq) + TILE - 1) // TILE
        owned = dropped = 0
        table = {}
        pieces = [(0, len(seq), 0, len(seq))] if not tiled else \
            [(max(0, t * TILE - HALO), min(len(seq), (t + 1) * TILE + HALO), t * TILE, (t + 1) * TILE) for t in range(n_tiles)]
        for lo, hi, own_lo, own_hi in pieces:
            for z in O.sketch(text[lo:hi], w, k, 0):
                g = lo + int(z["pos"])
                if not own_lo <= g < own_hi:
                    continue
                owned += 1
                if ncum[g + 1] - ncum[g - k + 1]:      # the k bases [g - k + 1, g] cover an N
                    dropped += 1
                    continue
                table.setdefault(int(z["hash"]), []).append(g | int(z["rev"]) << 31)
        for v in table.values():
            v.sort(key=lambda x: x & 0x7FFFFFFF)
        self.table = table
        cnt = [len(v) for v in table.values()]
        self.stats = {"tiles": n_tiles, "owned": owned, "dropped_n": dropped, "keys": len(table), "keys_above": sum(c > max_occ for c in cnt),
                      "stored": sum(c for c in cnt if c <= max_occ), "slots": table_slots(owned - dropped), "max_count": max(cnt, default=0)}

    def lookup(self, hashes):
        """-> (counts, occurrences per hash: none for a count above max_occ)"""
        cnt = [len(self.table.get(int(h), ())) for h in hashes]
        return cnt, [list(self.table.get(int(h), ())) if c <= self.max_occ else [] for h, c in zip(hashes, cnt)]


def mapq_of(f1, f2, m):
    if f1 <= 0 or m <= 0 or f2 >= f1:
        return 0
    v = 40.0 * (1.0 - f2 / f1) * min(1.0, m / 10.0) * math.log(f1)
    return 60 if v >= 60.0 else 0 if v <= 0.0 else int(v)


def _ilog2(v):
    return int(v).bit_length() - 1


def chain_dp(anchors, k=19, max_gap=50000, lookback=64):
    """oracle/aln.c:chain_dp on anchors (chromosome coordinate, contig coordinate) sorted by that pair -- the two roles swapped, which the
    score does not see.  -> (f, pre, best): the nearer predecessor wins a tie, the first best end wins"""
    n = len(anchors)
    f, pre = [0] * n, [-1] * n
    for i in range(n):
        bs, bp = k, -1
        ri, qi = anchors[i]
        for j in range(i - 1, max(0, i - lookback) - 1, -1):
            dr, dq = ri - anchors[j][0], qi - anchors[j][1]
            if dr <= 0 or dq <= 0:
                continue
            gap = abs(dr - dq)
            if gap > max_gap:
                continue
            sc = min(dr, dq, k)
            if gap:
                sc -= (gap >> 7) + (_ilog2(gap) >> 1) + 1
            sc += f[j]
            if sc > bs:
                bs, bp = sc, j
        f[i], pre[i] = bs, bp
    best = -1
    for i in range(n):
        if best < 0 or f[i] > f[best]:
            best = i
    return f, pre, best


def classify(hits, rev, own_lo, own_hi, max_occ):
    """hits: (count of the seed's key, relative strand, chromosome position, contig coordinate).  -> (c*, the three classes' anchors sorted
    reference-major: own locus, elsewhere forward, elsewhere reverse)"""
    def cls(rel, p):
        return 0 if rel == rev and own_lo <= p < own_hi else 1 + rel
    hist = [[0] * (max_occ + 1) for _ in range(3)]
    for c, rel, p, q in hits:
        hist[cls(rel, p)][c] += 1
    cut = 0
    for c in range(1, max_occ + 1):
        if any(sum(h[1:c + 1]) > AMAX for h in hist):
            break
        cut = c
    cut = max(1, cut)
    out = [[], [], []]
    for c, rel, p, q in hits:
        if c <= cut:
            out[cls(rel, p)].append((p, q))
    return cut, [sorted(a)[:AMAX] for a in out]


def score(classes, k=19, max_gap=50000):
    """-> (f1, f2, m) of classify()'s three anchor lists"""
    best = []
    for a in classes:
        if not a:
            best.append((0, 0))
            continue
        f, pre, b = chain_dp(a, k, max_gap)
        m, c = 0, b
        while c >= 0:
            m, c = m + 1, pre[c]
        best.append((f[b], m))
    return best[0][0], max(best[1][0], best[2][0]), best[0][1]


def place(index, contig, rec, origin, k=19, max_gap=50000):
    """one record (a row of ALN_REC_DTYPE, or a dict with q_start q_end ref_start ref_end rev) of `contig` whose window starts at
    chromosome position `origin` -> dict(f1, f2, m, cutoff, thin, flags, mapq)"""
    L = len(contig)
    rev = int(rec["rev"])
    q_lo, q_hi = (L - int(rec["q_end"]), L - int(rec["q_start"])) if rev else (int(rec["q_start"]), int(rec["q_end"]))
    own_lo, own_hi = origin + int(rec["ref_start"]), origin + int(rec["ref_end"])
    mz = O.sketch(seed_text(contig)[0], index.w, index.k, 0)
    Q = [z for z in mz if q_lo <= int(z["pos"]) < q_hi]
    t = max(1, (len(Q) + QMAX - 1) // QMAX)
    if t > 1:
        Q = [z for z in Q if (int(z["hash"]) >> 11) % t == 0]
    hits = []
    for z in Q:
        occ = index.table.get(int(z["hash"]), ())
        if not 1 <= len(occ) <= index.max_occ:
            continue
        for v in occ:
            rel = int(z["rev"]) ^ (v >> 31)
            q = (L - 1) - (int(z["pos"]) - int(z["span"]) + 1) if rel else int(z["pos"])
            hits.append((len(occ), rel, v & 0x7FFFFFFF, q))
    cut, classes = classify(hits, rev, own_lo, own_hi, index.max_occ)
    f1, f2, m = score(classes, k, max_gap)
    return {"f1": f1, "f2": f2, "m": m, "cutoff": cut, "thin": t, "flags": MQ_TRUNC if cut < index.max_occ else 0, "mapq": mapq_of(f1, f2, m)}
