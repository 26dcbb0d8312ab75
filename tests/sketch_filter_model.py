"""A Python restatement of hifiasm-0.14's ha_sketch WITH its high-count k-mer filter (sketch.cpp:39-137; the filter is line 89: a k-mer
whose hash ha_ft_isflt knows keeps its slot of the window buffer, but the slot holds the dummy entry).  TEST INFRASTRUCTURE, beside
kmer_model.py: the reference for fsv_sketch_reads_filtered and fsv_kmer_index.

Two forms of the same function:
  sketch_literal   the loop of sketch.cpp line by line on Python integers (slow: the yardstick of the other form)
  sketch           the slots of the window buffer computed with numpy (slots()), then the window loop of sketch.cpp:99-136 over them
Both handle what takes a slot and what does not: the first k - 1 entries and the entries whose k-mer spans 256 bases or more are dummies
IN a slot; a palindromic k-mer (even k only) takes no slot at all (line 83 `continue`s in front of ++l); without compression an entry's
span is min(l + 1, k).  Reads hold A, C, G, T only.  With an empty filter both equal oracle.sketch (tests/test_sketch_filter_model.py)."""
from itertools import chain

import numpy as np

from tests import kmer_model as KM
from tests.oracle_lib import MZ_DTYPE

MAX = (1 << 64) - 1      # the dummy entry's hash (UINT64_MAX), which no real k-mer is given
_M = MAX
_CODE = np.full(256, 4, dtype=np.uint8)
for _i, _ch in enumerate("ACGT"):
    _CODE[ord(_ch)] = _i
    _CODE[ord(_ch.lower())] = _i


def mix64(key):
    """yak_hash64_64 without a mask (htab.cpp): Thomas Wang's 64-bit mix, on a Python integer"""
    key = (~key + (key << 21)) & _M
    key ^= key >> 24
    key = (key + (key << 3) + (key << 8)) & _M
    key ^= key >> 14
    key = (key + (key << 2) + (key << 4)) & _M
    key ^= key >> 28
    return (key + (key << 31)) & _M


def _mix64_np(key):
    with np.errstate(over="ignore"):
        key = ~key + (key << np.uint64(21))
        key = key ^ (key >> np.uint64(24))
        key = key + (key << np.uint64(3)) + (key << np.uint64(8))
        key = key ^ (key >> np.uint64(14))
        key = key + (key << np.uint64(2)) + (key << np.uint64(4))
        key = key ^ (key >> np.uint64(28))
        return key + (key << np.uint64(31))


def start_slot(h, n_slots):
    """where the probe of key h starts in a filter set of n_slots slots (a power of two): bits of the hash itself; from there the
    probe steps one slot at a time and wraps behind the last one"""
    return (h ^ (h >> 29)) & (n_slots - 1)


def sketch_literal(seq, w, k, hpc, flt=()):
    """sketch.cpp:39-137 line by line -> list of (hash, pos, rev, span) in the order ha_sketch pushes them"""
    flt = flt if isinstance(flt, (set, frozenset)) else {int(x) for x in flt}
    dummy = (MAX, 0, 0, 0)
    mask, shift1 = (1 << k) - 1, k - 1
    kmer = [0, 0, 0, 0]
    buf = [dummy] * w
    mn, out = dummy, []
    tq = []
    length = len(seq)
    i = l = buf_pos = min_pos = kmer_span = 0
    while i < length:
        c = int(_CODE[ord(seq[i])])
        assert c < 4, "the model takes reads without ambiguous bases"
        info = dummy
        if hpc:
            skip_len = 1
            while i + skip_len < length and int(_CODE[ord(seq[i + skip_len])]) == c:
                skip_len += 1
            i += skip_len - 1
            tq.append(skip_len)
            kmer_span += skip_len
            if len(tq) > k:
                kmer_span -= tq.pop(0)
        else:
            kmer_span = l + 1 if l + 1 < k else k
        kmer[0] = (kmer[0] << 1 | (c & 1)) & mask
        kmer[1] = (kmer[1] << 1 | (c >> 1)) & mask
        kmer[2] = kmer[2] >> 1 | (1 - (c & 1)) << shift1
        kmer[3] = kmer[3] >> 1 | (1 - (c >> 1)) << shift1
        if kmer[1] == kmer[3]:
            i += 1
            continue
        z = 0 if kmer[1] < kmer[3] else 1
        l += 1
        if l >= k and kmer_span < 256:
            y = (mix64(kmer[z << 1 | 0]) + mix64(kmer[z << 1 | 1])) & _M
            if y not in flt:
                info = (y, i, z, kmer_span)
        buf[buf_pos] = info
        if l == w + k - 1 and mn[0] != MAX:
            for j in chain(range(buf_pos + 1, w), range(0, buf_pos)):
                if mn[0] == buf[j][0] and buf[j][1] != mn[1]:
                    out.append(buf[j])
        if info[0] <= mn[0]:
            if l >= w + k and mn[0] != MAX:
                out.append(mn)
            mn, min_pos = info, buf_pos
        elif buf_pos == min_pos:
            if l >= w + k - 1 and mn[0] != MAX:
                out.append(mn)
            mn = dummy
            for j in chain(range(buf_pos + 1, w), range(0, buf_pos + 1)):
                if mn[0] >= buf[j][0]:
                    mn, min_pos = buf[j], j
            if l >= w + k - 1 and mn[0] != MAX:
                for j in chain(range(buf_pos + 1, w), range(0, buf_pos + 1)):
                    if mn[0] == buf[j][0] and mn[1] != buf[j][1]:
                        out.append(buf[j])
        buf_pos += 1
        if buf_pos == w:
            buf_pos = 0
        i += 1
    if mn[0] != MAX:
        out.append(mn)
    return out


def slots(seq, k, hpc):
    """what ha_sketch writes into the window buffer, slot after slot, with no filter -> structured array (MZ_DTYPE): hash MAX and
    pos = rev = span = 0 for a dummy.  Slot s is the entry with l == s + 1."""
    c = _CODE[np.frombuffer(seq.encode() if isinstance(seq, str) else seq, dtype=np.uint8)]
    assert len(c) and int(c.max()) < 4, "the model takes reads without ambiguous bases"
    if hpc:
        ends = np.flatnonzero(np.r_[c[1:] != c[:-1], True])
        runs = np.diff(np.r_[-1, ends]).astype(np.int64)
        c = c[ends]
    else:
        ends = np.arange(len(c))
    n = len(c)
    b0, b1 = (c & 1).astype(np.uint64), (c >> 1).astype(np.uint64)
    km = [np.zeros(n, dtype=np.uint64) for _ in range(4)]
    for j in range(min(k, n)):     # the base j entries back: bit j of the forward planes, bit k - 1 - j of the reverse ones
        for plane, b in ((0, b0), (1, b1)):
            km[plane][j:] |= b[:n - j] << np.uint64(j)
            km[plane + 2][j:] |= (np.uint64(1) - b[:n - j]) << np.uint64(k - 1 - j)
    keep = km[1] != km[3]
    z = ~(km[1] < km[3])
    l = np.cumsum(keep)
    if hpc:
        cs = np.cumsum(runs)
        span = cs - np.r_[np.zeros(min(k, n), dtype=np.int64), cs[:max(0, n - k)]]
    else:
        span = np.minimum(l, k)        # kmer_span = min(l + 1, k) with l read before ++l
    valid = keep & (l >= k) & (span < 256)
    with np.errstate(over="ignore"):
        y = _mix64_np(np.where(z, km[2], km[0])) + _mix64_np(np.where(z, km[3], km[1]))
    out = np.zeros(int(keep.sum()), dtype=MZ_DTYPE)
    v = valid[keep]
    out["hash"] = np.where(v, y[keep], np.uint64(MAX))
    out["pos"] = np.where(v, ends[keep], 0)
    out["rev"] = np.where(v, z[keep], 0)
    out["span"] = np.where(v, span[keep], 0)
    return out


def window(x, w, k):
    """sketch.cpp:99-136 over the hashes of the slots (a list of Python integers, MAX = dummy) -> the slots pushed, in push order"""
    out = []
    bx, bs = [MAX] * w, [-1] * w
    min_x, min_s, min_pos, buf_pos = MAX, -1, 0, 0
    first, full = w + k - 1, w + k
    for s, xs in enumerate(x):
        l = s + 1
        bx[buf_pos] = xs
        bs[buf_pos] = s
        if l == first and min_x != MAX:
            for j in chain(range(buf_pos + 1, w), range(0, buf_pos)):
                if bx[j] == min_x and bs[j] != min_s:
                    out.append(bs[j])
        if xs <= min_x:
            if l >= full and min_x != MAX:
                out.append(min_s)
            min_x, min_s, min_pos = xs, s, buf_pos
        elif buf_pos == min_pos:
            if l >= first and min_x != MAX:
                out.append(min_s)
            min_x = MAX
            for j in chain(range(buf_pos + 1, w), range(0, buf_pos + 1)):
                if min_x >= bx[j]:
                    min_x, min_s, min_pos = bx[j], bs[j], j
            if l >= first and min_x != MAX:
                for j in chain(range(buf_pos + 1, w), range(0, buf_pos + 1)):
                    if bx[j] == min_x and bs[j] != min_s:
                        out.append(bs[j])
        buf_pos += 1
        if buf_pos == w:
            buf_pos = 0
    if min_x != MAX:
        out.append(min_s)
    return out


def sketch(seq, w, k, hpc, flt=None, sl=None):
    """ha_sketch(seq, w, k, hpc, hf = flt) -> MZ_DTYPE array in push order.  flt: hashes (any iterable, or None); sl: slots(seq, k, hpc)
    when the caller has them already"""
    sl = slots(seq, k, hpc) if sl is None else sl
    x = sl["hash"]
    if flt is not None and len(flt):
        x = np.where(np.isin(x, np.asarray(sorted(int(v) for v in flt), dtype=np.uint64)), np.uint64(MAX), x)
    return sl[np.asarray(window(x.tolist(), w, k), dtype=np.int64)]


def kmer_index(reads, w=51, k=51, hpc=1):
    """hifiasm's first ha_pt_gen on one read set (htab.cpp:952-998): the count table at w = 1 (kmer_model.kmer_table), its filter, the
    filtered sketch at w, counted -> (table, index): two dicts as kmer_model.kmer_table returns them; index["n_entries"] counts the
    filtered sketch's entries.  A set without a peak filters every k-mer: an index of nothing."""
    seqs = [r.decode() if isinstance(r, bytes) else r for r in reads]
    all_slots = [slots(s, k, hpc) for s in seqs]
    hashes = np.concatenate([sl["hash"][sl["hash"] != np.uint64(MAX)] for sl in all_slots]) if seqs else np.zeros(0, np.uint64)
    keys, counts, hist = KM.count_table(hashes)
    tab = KM.analyze_count(hist)
    cutoff = min(int(tab["peak_hom"] * KM.HIGH_FACTOR), KM.MAX_COUNT - 1)
    flt = keys[counts >= cutoff]
    tab.update(cutoff=cutoff, n_entries=int(len(hashes)), n_distinct=int(len(keys)), n_filtered=int(len(flt)),
               n_indexed=int(sum(c * int(hist[c]) for c in range(2, KM.MAX_COUNT))), hist=hist, filter=flt)
    parts = [sketch(s, w, k, hpc, flt, sl)["hash"] for s, sl in zip(seqs, all_slots)]
    ih = np.concatenate(parts) if parts else np.zeros(0, np.uint64)
    ikeys, _, ihist = KM.count_table(ih)
    idx = KM.analyze_count(ihist)
    idx.update(n_entries=int(len(ih)), n_distinct=int(len(ikeys)), n_indexed=int(sum(c * int(ihist[c]) for c in range(2, KM.MAX_COUNT))), hist=ihist)
    return tab, idx
