#!/usr/bin/env python3
"""What the NM / cs tags cost: fsv_align_batch alone and fsv_align_batch + fsv_aln_tags (on the sequences the aligner left on the device)
on the bench geometry -- both haplotypes of synthetic 50 kb regions as contigs, 512 by default, each against its region's window -- with
the tags off and on alternating in one process, three repeats each after one untimed pass over both.  Prints per setting the median wall
time, the aligner's own total (fsv_aln_stats.ms_total) and, with the tags on, the wall time of the tags call, its kernel time
(fsv_aln_tags.ms: count + scan + emit) and the bytes it produced, then one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from focalsv_amd import _lib, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--contigs", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    regs = [synth.make_region(i, depth_per_hap=0.3) for i in range((args.contigs + 1) // 2)]
    contigs = [r.haps[h] for r in regs for h in (0, 1)][: args.contigs]
    cref = [i // 2 for i in range(len(contigs))]
    refs = _lib.join_refs([r.ref for r in regs])
    runs = {0: [], 1: []}
    with _lib.Context(args.device) as ctx:
        for rep in range(args.repeats + 1):      # the first pass over both settings is the warm-up
            for on in (0, 1):
                ctx.sync()
                t0 = time.perf_counter()
                rec, cigar, status = ctx.align_batch(contigs, cref, refs)
                ctx.sync()
                t1 = time.perf_counter()
                row = {"align_wall_ms": (t1 - t0) * 1e3, "aln_ms_total": ctx.aln_stats()["ms_total"], "tags_wall_ms": 0.0, "tags_kernel_ms": 0.0}
                if on:
                    nm, cs, st, ms = ctx.aln_tags(rec, cigar, n_contigs=len(contigs), n_refs=len(regs))
                    ctx.sync()
                    row.update(tags_wall_ms=(time.perf_counter() - t1) * 1e3, tags_kernel_ms=ms, cs_bytes=sum(len(c) for c in cs), nm_sum=int(nm.sum()),
                               records=len(rec), columns=int(sum(int(r["ref_end"]) - int(r["ref_start"]) for r in rec)))
                    assert not st.any()
                row["wall_ms"] = row["align_wall_ms"] + row["tags_wall_ms"]
                if rep:
                    runs[on].append(row)
    out = {"contigs": len(contigs), "bases": sum(len(c) for c in contigs)}
    for on in (0, 1):
        med = {k: statistics.median(r[k] for r in runs[on]) for k in ("wall_ms", "align_wall_ms", "aln_ms_total", "tags_wall_ms", "tags_kernel_ms")}
        med["wall_ms_all"] = [round(r["wall_ms"], 2) for r in runs[on]]
        if on:
            med.update({k: runs[on][-1][k] for k in ("cs_bytes", "nm_sum", "records", "columns")})
        out["tags=%d" % on] = med
        print("tags=%d  wall %8.2f ms (%s)  align %8.2f (library %8.2f)  tags call %7.2f  tags kernels %6.3f" % (
            on, med["wall_ms"], ", ".join("%.1f" % w for w in med["wall_ms_all"]), med["align_wall_ms"], med["aln_ms_total"], med["tags_wall_ms"], med["tags_kernel_ms"]))
    print(json.dumps({"time_aln_tags": out}))


if __name__ == "__main__":
    main()
