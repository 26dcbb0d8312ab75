"""oracle/aln.c: (1) the DP against the reference tree's own ksw2 (golden from ksw_extz2_sse, single affine),
(2) contig-vs-window alignment recovers the planted SVs."""
import json
import os

from focalsv_amd import synth
from tests import oracle_lib as O


def test_nw_matches_ksw2_golden(golden_dir):
    cases = json.load(open(os.path.join(golden_dir, "ksw_extz2.json")))["cases"]
    checked = 0
    for c in cases:
        p = O.aln_default_params()
        p.a, p.b, p.q, p.e, p.q2, p.e2 = c["a"], c["b"], c["q"], c["e"], -1, -1
        import re
        ops = re.findall(r"(\d+)([MID])", c["cigar"])
        qlen = sum(int(n) for n, o in ops if o in "MI")
        tlen = sum(int(n) for n, o in ops if o in "MD")
        if qlen != len(c["query"]) or tlen != len(c["target"]):
            continue  # z-dropped extension, not a global alignment
        sc, cg = O.nw(c["target"].encode(), c["query"].encode(), p)
        assert sc == c["score"], c
        assert O.cigar_str(cg) == c["cigar"], (O.cigar_str(cg), c["cigar"])
        checked += 1
    assert checked >= 40


def _events(aln):
    pos, out = aln["ref_start"], []
    for op, n in aln["cigar"]:
        if op == 0:
            pos += n
        elif op == 2:
            if n >= 30:
                out.append(("DEL", pos, n))
            pos += n
        elif op == 1 and n >= 30:
            out.append(("INS", pos, n))
    return out


def test_alignment_recovers_planted_svs():
    for i in (0, 1, 4, 7, 15):
        r = synth.make_region(i)
        for h in (0, 1):
            for contig in (r.haps[h], synth.revcomp(r.haps[h])):
                a = O.align_contig(contig, r.ref)
                assert a is not None and a["mapq"] == 60
                assert a["ref_start"] == 0 and a["ref_end"] == len(r.ref)
                qlen = sum(n for op, n in a["cigar"] if op in (0, 1, 4))
                assert qlen == len(contig)
                ev = _events(a)
                truth = [(t.svtype, t.pos, t.length) for t in r.truth if t.hap in (h + 1, 3)]
                assert len(ev) == len(truth), (i, h, ev, truth)
                for (ty, pos, ln), (tty, tpos, tln) in zip(sorted(ev, key=lambda e: e[1]), truth):
                    assert ty == tty and ln == tln, (i, h, ev, truth)
                    # our gaps are left-aligned; the planted position can only be at or right of it (repeat context)
                    assert pos <= tpos, (i, h, ev, truth)
                    if i % 8 != 7:
                        assert tpos - pos <= 8, (i, h, ev, truth)


# regions where round 1's aligner put a DEL 2-9 bp right of its leftmost position: the gap sat at
# the left edge of its DP event and could not travel further; the CIGAR-wide left shift (minimap2's mm_fix_cigar rule) fixes it
LEFT_SHIFT_REGRESSIONS = (367, 423, 559, 703, 791, 823, 1039, 1175, 1359)


def sv_position_tolerance(region, t, hap):
    """+-1 bp of the left-aligned truth; on haplotype 2 a SNP next to a breakpoint may be absorbed into the gap (synth.position_tolerance)"""
    return synth.position_tolerance(region, t) if hap == 1 else 1


def check_planted(region, hap, aln):
    """every planted SV of the haplotype called with its exact length within the tolerance, nothing else called"""
    ev = _events(aln)
    want = [t for t in region.truth if t.hap & (hap + 1)]
    misses = [(t.svtype, t.pos_left, t.length) for t in want
              if not any(k == t.svtype and n == t.length and abs(p - t.pos_left) <= sv_position_tolerance(region, t, hap) for k, p, n in ev)]
    return misses, len(ev) - len(want)


def test_planted_svs_left_aligned_over_2000_seeds():
    """seeds 1000 + i for i < 2000 (all 250 tandem-repeat regions i % 8 == 7 included): 0 misses, 0 extra calls"""
    n_sv = 0
    full = os.environ.get("FSV_FULL_GOLDEN")
    for i in range(2000):
        if not full and (i % 16 != 7 if i % 8 == 7 else i % 6 != 0):   # by default every second tandem-repeat region and a sixth of the others (the CPU suite's time)
            continue
        r = synth.make_region(i, depth_per_hap=0.3)      # reads are not needed here: the haplotypes themselves are aligned
        for h in (0, 1):
            a = O.align_contig(r.haps[h], r.ref)
            assert a is not None
            misses, extra = check_planted(r, h, a)
            assert not misses and extra == 0, (i, h, misses, extra, _events(a))
            n_sv += sum(1 for t in r.truth if t.hap & (h + 1))
    assert n_sv > (5000 if full else 1000)


def test_gap_shift_rule():
    """shift_gaps_left on hand-made cases: a deletion inside a tandem repeat goes to the repeat's first base, an M run shifted
    away completely merges the neighbouring gaps"""
    import numpy as np
    rng = np.random.default_rng(11)
    A = np.frombuffer(b"ACGT", dtype=np.uint8)
    left, right = A[rng.integers(0, 4, 3000)].tobytes(), A[rng.integers(0, 4, 3000)].tobytes()
    unit = b"ACGGTCATTGCAAGTCCTGA"
    while left[-1:] == unit[-1:]:
        left = left[:-1]
    ref = left + unit * 40 + right
    hap = left + unit * 33 + right                      # 7 units deleted, wherever
    a = O.align_contig(hap, ref)
    assert _events(a) == [("DEL", len(left), 140)], O.cigar_str(a["raw"])
    hap = left + unit * 45 + right                      # 5 units inserted
    a = O.align_contig(hap, ref)
    assert _events(a) == [("INS", len(left), 100)], O.cigar_str(a["raw"])
    s = b"TTTTACACACACACACGGGG"
    assert O.lib().orc_gap_max_shift(s, 10, 2, 10) == 6    # a 2-base gap at 10 can move back to 4 (the first AC)
    assert O.lib().orc_gap_max_shift(s, 10, 2, 3) == 3


def test_duplications_beyond_max_cells_are_aligned():
    """a tandem duplication of 6 kb and more put both copies between two unique seeds -- an event of more than 2^26
    cells, and the whole contig was refused.  Now the event's box is seeded again on its own (oracle/aln.c:sub_align): every case
    comes back as one record with the SV at its left-aligned position and exact length, and the contig's other SV with it."""
    from tests import aln_cases as A
    for case in A.duplication_cases() + A.other_cases():
        recs = O.align_contig_multi(case.hap, case.ref)
        A.check_case(case, recs)


def test_small_boxes_and_corner_runs():
    """aln_cases.small_box_cases under max_cells = 2^16, the oracle alone: every contig comes back as one record on its strand;
    a box that seeds again shows its planted 400-base gap, left-aligned, and nothing else; a box with nothing to seed is closed
    from its corners: exactly one insertion run next to one deletion run, 30 bases apart in length as the fills are (a DP of
    the two unrelated fills would pair bases inside them instead).  So the set cannot silently stop reaching the path.  The GPU
    test runs the same cases in one batch and also checks that every contig made a box."""
    from tests import aln_cases as A
    cases, recs = A.small_box_oracle()
    assert len(cases) == 2 * (4 + 3 * len(A.CORNER_RUNS)) and all(3300 <= len(c.hap) <= 3900 for c in cases)
    assert sum(1 for c in cases if c.kind == "corner") == 2 * (2 + 3 * len(A.CORNER_RUNS))
    for case, r in zip(cases, recs):
        assert r is not None, case.name     # status 0
        A.check_box_case(case, r)


def test_inversions_make_no_call():
    """an inversion came back as one forward record with INS + DEL at the breakpoint.  Now the inverted piece is a
    record of the other strand and the forward record is cut around it; DipPAV's split rule ignores pairs of different strands"""
    from tests import aln_cases as A
    for case in A.inversion_cases():
        recs = O.align_contig_multi(case.hap, case.ref)
        A.check_case(case, recs)
        assert A.split_calls(recs) == [], case.name


def test_split_records_beyond_max_gap():
    """a 30 kb deletion / insertion with max_gap at minimap2's 20 kb: two records, and DipPAV's split rule makes the call;
    with the default max_gap (50 kb) the same SV sits in one record's CIGAR"""
    import numpy as np
    from tests import aln_cases as A
    rng = np.random.default_rng(5)
    ref = A.rnd(rng, 150000)
    for hap, want in ((ref[:40000] + ref[70000:], ("DEL", 40000, 30000)), (ref[:40000] + A.rnd(rng, 30000) + ref[40000:], ("INS", 40000, 30000))):
        recs = O.align_contig_multi(hap, ref)
        assert len(recs) == 1 and A.events(recs[0]) == [want]
        p = O.aln_default_params()
        p.max_gap = 20000
        recs = O.align_contig_multi(hap, ref, p)
        assert len(recs) == 2
        calls = A.split_calls(recs)
        assert len(calls) == 1 and calls[0][1] == want[0] and abs(calls[0][2] - want[1]) <= 2 and abs(calls[0][3] - want[2]) <= 2


def test_single_base_deletions_ten_apart_share_one_event():
    """n = 1 ... 9 single-base deletions ten bases apart: one record of 2n + 1 runs, exactly n deletions of length 1 (at n = 10 the
    DP prefers one long gap).  The GPU test aligns all nine in one batch: DP events of up to and of more than 8 runs"""
    from tests import aln_cases as A
    for n, case in enumerate(A.cigar_head_cases(), 1):
        recs = O.align_contig_multi(case.hap, case.ref)
        assert len(case.hap) == len(case.ref) - n and len(recs) == 1, case.name
        cg = recs[0]["cigar"]
        assert len(cg) == 2 * n + 1 and [x for x in cg if x[0] != 0] == [(2, 1)] * n, (case.name, cg)


def test_reference_windows_with_n_runs():
    """an N of the reference window pairs with nothing and costs 1 (minimap2's sc_ambi), N runs do not
    seed -- the alignment runs through runs of 1 .. 1 500 N as 'M', no SV is called there (nor where the contig has poly-A against
    the N), and the contig's real SVs come out at their left-aligned positions"""
    from tests import aln_cases as A
    for case in A.n_window_cases():
        recs = O.align_contig_multi(case.hap, case.ref)
        A.check_case(case, recs)


def test_one_contig_with_an_event_for_every_dp_class():
    """aln_cases.dp_class_cases: five events between unique flanks, one record per strand with exactly these gaps -- a 100-base
    deletion, two replacements and a third of 3 300 by 3 500 bases as an insertion in front of a deletion, a 2 000-base insertion.
    The GPU test runs both strands in one batch: each of the four DP kernels gets an event of each."""
    from tests import aln_cases as A
    cases = A.dp_class_cases()
    assert [len(c.ref) for c in cases] == [51100, 51100] and cases[1].hap == synth.revcomp(cases[0].hap)
    for case in cases:
        recs = O.align_contig_multi(case.hap, case.ref)
        A.check_case(case, recs)
        gaps = [(op, n) for op, n in recs[0]["cigar"] if op != 0]
        assert gaps == [(2, 100), (1, 1200), (2, 1000), (1, 600), (2, 5000), (1, 3500), (2, 3300), (1, 2000)], (case.name, gaps)
