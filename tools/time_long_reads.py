#!/usr/bin/env python3
"""What fsv_asm_params.full_lists = 1 costs: fsv_assemble_batch with the ONT profile on (i) the 12-region batch of tests/test_gpu_ont.py
(reads of 10-30 kb: no list above the cap, so the option should change nothing beyond the repeat-to-repeat spread) and (ii) 16 sets of
reads of 30-90 kb at 10 % error over 100 kb stretches, with the option 0 and 1 alternating in one process, three repeats each after one
untimed call of each.  Prints per workload and setting the median wall time of the call, the summed kernel time of the sketch, the index
(k_uniq: the two LDS classes) and the chaining (k_chain), and of the two kernels of the option on their own (k_uniq_long, k_chain_spill:
rows of fsv_asm_stats.kernels), with how many lists and pairs they took over all rounds (fsv_asm_last_long_lists).  Then one JSON line."""
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


def long_sets(n_sets):
    sets = []
    for i in range(n_sets):
        rng = np.random.default_rng(9000 + i)
        hap = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 100000)]
        sets.append(synth._sample_reads(rng, hap, 6.0, 30000, 90000, 0.10))
    return sets


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--long-sets", type=int, default=16)
    ap.add_argument("--workloads", default="ont12,long", help="which of the two to run")
    args = ap.parse_args()
    work = {}
    if "ont12" in args.workloads.split(","):
        regs = [synth.make_region(i, width=50000, profile="ont", start=i * 60000) for i in range(12)]
        work["ont12"] = [rd for r in regs for rd in r.reads]
    if "long" in args.workloads.split(","):
        work["long"] = long_sets(args.long_sets)
    result = {}
    with _lib.Context(args.device) as ctx:
        for name, sets in work.items():
            b = pack_sets(sets)
            d = ctx.upload(b.words)
            runs = {0: [], 1: []}
            try:
                p = ctx.ont_asm_params()
                for rep in range(args.repeats + 1):      # the first pass over both settings is the warm-up
                    for fl in (0, 1):
                        p = ctx.ont_asm_params()
                        p.full_lists = fl
                        ctx.sync()
                        t0 = time.perf_counter()
                        contigs, cset, cnr, status = ctx.assemble_batch(d, b.word_off, b.read_len, b.set_start, p)
                        ctx.sync()
                        wall = (time.perf_counter() - t0) * 1e3
                        st = ctx.asm_stats()
                        row = {"wall_ms": wall, "ms_total": st["ms_total"], "k_uniq_ms": st["kernels"]["k_uniq"]["ms"], "k_chain_ms": st["kernels"]["k_chain"]["ms"],
                               "k_sketch_ms": st["kernels"]["k_sketch"]["ms"], "k_uniq_long_ms": st["kernels"]["k_uniq_long"]["ms"],
                               "k_chain_spill_ms": st["kernels"]["k_chain_spill"]["ms"], "long_lists": st["n_long_list_reads"], "spilled_pairs": st["n_spilled_pairs"], "status_or": int(np.bitwise_or.reduce(status)) if len(status) else 0,
                               "contig_bases": int(sum(len(c) for c in contigs))}
                        if rep:
                            runs[fl].append(row)
            finally:
                ctx.dev_free(d)
            out = {"sets": len(sets), "reads": int(b.n_reads), "longest_read": int(b.read_len.max())}
            for fl in (0, 1):
                med = {k: statistics.median(r[k] for r in runs[fl]) for k in ("wall_ms", "ms_total", "k_sketch_ms", "k_uniq_ms", "k_chain_ms", "k_uniq_long_ms", "k_chain_spill_ms")}
                med["long_lists"], med["spilled_pairs"] = runs[fl][-1]["long_lists"], runs[fl][-1]["spilled_pairs"]
                med["wall_ms_all"] = [round(r["wall_ms"], 2) for r in runs[fl]]
                med["status_or"] = runs[fl][-1]["status_or"]
                med["contig_bases"] = runs[fl][-1]["contig_bases"]
                out["full_lists=%d" % fl] = med
                print("%-6s full_lists=%d  wall %9.2f ms (%s)  k_sketch %7.2f  k_uniq %7.2f  k_chain %7.2f  k_uniq_long %6.2f (%d lists)  k_chain_spill %6.2f (%d pairs)  status bits %d  contig bases %d" % (
                    name, fl, med["wall_ms"], ", ".join("%.1f" % w for w in med["wall_ms_all"]), med["k_sketch_ms"], med["k_uniq_ms"], med["k_chain_ms"],
                    med["k_uniq_long_ms"], med["long_lists"], med["k_chain_spill_ms"], med["spilled_pairs"], med["status_or"], med["contig_bases"]))
            print("       %d reads in %d sets, longest %d bases" % (out["reads"], out["sets"], out["longest_read"]))
            result[name] = out
    print(json.dumps({"time_long_reads": result}))


if __name__ == "__main__":
    main()
