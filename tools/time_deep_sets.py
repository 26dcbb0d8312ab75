#!/usr/bin/env python3
"""What fsv_asm_params.deep_sets = 1 costs: fsv_assemble_batch with the HiFi profile on (i) a phased batch of the bench geometry (64 synthetic
regions, both haplotypes: no window near the cap, so the option should cost its empty launches and nothing else) and (ii) one 50 kb region
at 80 x per haplotype (tools/stress.py's recipe: windows past the 256 events of the LDS buffer), with the option 0 and 1 alternating in one
process, three repeats each after one untimed call of each.  Prints per workload and setting the median wall time of the call, the summed
kernel time of the consensus rows (k_consensus, k_partition, k_bnd_consensus) and of the option's two kernels on their own
(k_consensus_deep, k_bnd_consensus_deep: rows of fsv_asm_stats.kernels), with what they took over all rounds
(fsv_asm_last_deep_windows).  Then one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from focalsv_amd import _lib, synth  # noqa: E402
from focalsv_amd.readsets import pack_sets  # noqa: E402

ROWS = ("k_consensus", "k_partition", "k_bnd_consensus", "k_consensus_deep", "k_bnd_consensus_deep")


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--regions", type=int, default=64)
    ap.add_argument("--depth", type=float, default=80.0)
    ap.add_argument("--workloads", default="bench,deep", help="which of the two to run")
    args = ap.parse_args()
    work = {}
    if "bench" in args.workloads.split(","):
        work["bench"] = [rd for i in range(args.regions) for rd in synth.make_region(i).reads]
    if "deep" in args.workloads.split(","):
        work["deep"] = list(synth.make_region(702, width=50000, depth_per_hap=args.depth, start=600000).reads)
    result = {}
    with _lib.Context(args.device) as ctx:
        for name, sets in work.items():
            b = pack_sets(sets)
            d = ctx.upload(b.words)
            runs = {0: [], 1: []}
            try:
                for rep in range(args.repeats + 1):      # the first pass over both settings is the warm-up
                    for deep in (0, 1):
                        p = ctx.default_asm_params()
                        p.deep_sets = deep
                        ctx.sync()
                        t0 = time.perf_counter()
                        contigs, cset, cnr, status = ctx.assemble_batch(d, b.word_off, b.read_len, b.set_start, p)
                        ctx.sync()
                        wall = (time.perf_counter() - t0) * 1e3
                        st = ctx.asm_stats()
                        row = {"wall_ms": wall, "ms_total": st["ms_total"]}
                        row.update({k + "_ms": st["kernels"][k]["ms"] for k in ROWS})
                        row.update({k: st[k] for k in ("n_deep_windows", "n_deep_junctions", "max_events")})
                        row["status_or"] = int(np.bitwise_or.reduce(status)) if len(status) else 0
                        row["contig_bases"] = int(sum(len(c) for c in contigs))
                        if rep:
                            runs[deep].append(row)
            finally:
                ctx.dev_free(d)
            out = {"sets": len(sets), "reads": int(b.n_reads), "largest_set": int(np.diff(b.set_start).max())}
            for deep in (0, 1):
                med = {k: statistics.median(r[k] for r in runs[deep]) for k in ("wall_ms", "ms_total") + tuple(k + "_ms" for k in ROWS)}
                med.update({k: runs[deep][-1][k] for k in ("n_deep_windows", "n_deep_junctions", "max_events", "status_or", "contig_bases")})
                med["wall_ms_all"] = [round(r["wall_ms"], 2) for r in runs[deep]]
                out["deep_sets=%d" % deep] = med
                print("%-6s deep_sets=%d  wall %9.2f ms (%s)  k_consensus %7.2f  k_partition %7.2f  k_bnd_consensus %7.2f  k_consensus_deep %6.2f (%d windows)  "
                      "k_bnd_consensus_deep %6.2f (%d junctions)  most events %d  status bits %d  contig bases %d" % (
                          name, deep, med["wall_ms"], ", ".join("%.1f" % w for w in med["wall_ms_all"]), med["k_consensus_ms"], med["k_partition_ms"],
                          med["k_bnd_consensus_ms"], med["k_consensus_deep_ms"], med["n_deep_windows"], med["k_bnd_consensus_deep_ms"], med["n_deep_junctions"],
                          med["max_events"], med["status_or"], med["contig_bases"]))
            print("       %d reads in %d sets, the largest of %d reads" % (out["reads"], out["sets"], out["largest_set"]))
            result[name] = out
    print(json.dumps({"time_deep_sets": result}))


if __name__ == "__main__":
    main()
