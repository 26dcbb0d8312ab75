#!/usr/bin/env python3
"""What the chromosome-level mapping quality costs: the index build (fsv_ref_index_build) for a synthetic chromosome of 46 Mb by default
-- random sequence with the bench geometry's synthetic 50 kb regions pasted in every 80 kb -- and fsv_contig_mapq for both haplotypes of
those regions as contigs, 512 by default, on the contigs fsv_align_batch left on the device.  The option off and on alternate in one
process, three repeats each after one untimed pass over both.  Prints per setting the median wall time and the aligner's own total
(fsv_aln_stats.ms_total), with the option on the wall time of the mapq call and its kernel time (fsv_contig_mapq.ms: the contigs'
sketch and k_place), the build's wall and kernel time (fsv_ref_stats.ms) with the index's statistics, then one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from focalsv_amd import _lib, synth  # noqa: E402

STRIDE = 80_000


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--contigs", type=int, default=512)
    ap.add_argument("--chrom-mb", type=float, default=46.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    regs = [synth.make_region(i, depth_per_hap=0.3) for i in range((args.contigs + 1) // 2)]
    contigs = [r.haps[h] for r in regs for h in (0, 1)][: args.contigs]
    cref = [i // 2 for i in range(len(contigs))]
    refs = _lib.join_refs([r.ref for r in regs])
    n = max(int(args.chrom_mb * 1e6), STRIDE * len(regs) + STRIDE)
    chrom = np.random.default_rng(1).choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n)
    origin = [10_000 + STRIDE * i for i in range(len(regs))]
    for o, r in zip(origin, regs):
        assert len(r.ref) <= STRIDE - 10_000
        chrom[o:o + len(r.ref)] = np.frombuffer(r.ref, dtype=np.uint8)
    chrom = chrom.tobytes()
    runs, builds = {0: [], 1: []}, []
    with _lib.Context(args.device) as ctx:
        for rep in range(args.repeats + 1):      # the first pass over both settings is the warm-up
            for on in (0, 1):
                row = {"build_wall_ms": 0.0, "build_kernel_ms": 0.0, "mapq_wall_ms": 0.0, "mapq_kernel_ms": 0.0}
                if on:
                    ctx.sync()
                    t0 = time.perf_counter()
                    stats = ctx.ref_index(chrom)
                    ctx.sync()
                    row.update(build_wall_ms=(time.perf_counter() - t0) * 1e3, build_kernel_ms=stats["ms"])
                ctx.sync()
                t0 = time.perf_counter()
                rec, cigar, status = ctx.align_batch(contigs, cref, refs)
                ctx.sync()
                t1 = time.perf_counter()
                row.update(align_wall_ms=(t1 - t0) * 1e3, aln_ms_total=ctx.aln_stats()["ms_total"])
                if on:
                    rec, out = ctx.contig_mapq(rec, cigar, origin, n_contigs=len(contigs))
                    ctx.sync()
                    row.update(mapq_wall_ms=(time.perf_counter() - t1) * 1e3, mapq_kernel_ms=out["ms"], records=len(rec),
                               below_50=int((rec["mapq"] < 50).sum()), truncated=int((out["flags"] & _lib.MQ_TRUNC != 0).sum()))
                    assert not out["rec_status"].any()
                    ctx.ref_index_drop()
                row["wall_ms"] = row["align_wall_ms"] + row["mapq_wall_ms"]
                if rep:
                    runs[on].append(row)
                    if on:
                        builds.append(stats)
    keys = ("wall_ms", "align_wall_ms", "aln_ms_total", "mapq_wall_ms", "mapq_kernel_ms", "build_wall_ms", "build_kernel_ms")
    res = {"contigs": len(contigs), "bases": sum(len(c) for c in contigs), "chrom_bases": len(chrom)}
    for on in (0, 1):
        med = {k: statistics.median(r[k] for r in runs[on]) for k in keys}
        med["wall_ms_all"] = [round(r["wall_ms"], 2) for r in runs[on]]
        if on:
            med["build_kernel_ms_all"] = [round(r["build_kernel_ms"], 2) for r in runs[on]]
            med["mapq_kernel_ms_all"] = [round(r["mapq_kernel_ms"], 3) for r in runs[on]]
            med.update({k: runs[on][-1][k] for k in ("records", "below_50", "truncated")})
            med["index"] = {k: v for k, v in builds[-1].items() if k != "ms"}
        res["chrom_mapq=%d" % on] = med
        print("chrom_mapq=%d  align + mapq wall %8.2f ms (%s)  align %8.2f (library %8.2f)  mapq call %7.2f  mapq kernels %7.3f  build %8.2f  build kernels %8.2f" % (
            on, med["wall_ms"], ", ".join("%.1f" % w for w in med["wall_ms_all"]), med["align_wall_ms"], med["aln_ms_total"], med["mapq_wall_ms"],
            med["mapq_kernel_ms"], med["build_wall_ms"], med["build_kernel_ms"]))
    print(json.dumps({"time_contig_mapq": res}))


if __name__ == "__main__":
    main()
