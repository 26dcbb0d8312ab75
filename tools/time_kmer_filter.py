#!/usr/bin/env python3
"""What fsv_asm_params.kmer_filter = 1 costs: fsv_assemble_batch on (i) the 36 repeat-rich read sets of tests/golden/hifiasm_repeats.json in
one call (21 of them have a filter) and (ii) a phased batch of the bench geometry (64 synthetic regions, both haplotypes: 128 read sets,
nearly every filter empty), with the settings alternating in one process -- kmer_table = 0, kmer_table = 1, kmer_table = 1 with
kmer_filter = 1 -- three repeats each after one untimed call of each.  Prints per workload and setting the median wall time of the call, the
sketch kernel's summed time over the rounds and the final pass (fsv_asm_stats: k_sketch is k_sketch_fast for hifiasm's odd k), the sketch
stage's time, the count table stage's kernel time and -- with the filter -- the kernel time of the filter-set build plus the index
(fsv_asm_last_kmer_index), then one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from focalsv_amd import _lib, synth  # noqa: E402
from focalsv_amd.readsets import pack_sets  # noqa: E402

SETTINGS = (("kmer_table=0", 0, 0), ("kmer_table=1", 1, 0), ("kmer_filter=1", 1, 1))


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--regions", type=int, default=64, help="phased batch: synthetic regions (two read sets each)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--workloads", default="repeats,phased", help="which of the two to run (under a profiler: one at a time)")
    args = ap.parse_args()
    gold = json.load(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "hifiasm_repeats.json")))["sets"]
    work = {}
    if "repeats" in args.workloads.split(","):
        work["repeats"] = [synth.make_repeat_region(g["index"]).reads[0] for g in gold]
    if "phased" in args.workloads.split(","):
        work["phased"] = [rd for i in range(args.regions) for rd in synth.make_region(i).reads]
    result = {}
    keys = ("wall_ms", "k_sketch_ms", "ms_sketch", "table_ms", "filter_ms")
    with _lib.Context(args.device) as ctx:
        for name, sets in work.items():
            b = pack_sets(sets)
            d = ctx.upload(b.words)
            runs = {s[0]: [] for s in SETTINGS}
            n_flt = 0
            try:
                for rep in range(args.repeats + 1):      # the first pass over the settings is the warm-up
                    for label, kt, kf in SETTINGS:
                        p = ctx.default_asm_params()
                        p.kmer_table, p.kmer_filter = kt, kf
                        ctx.sync()
                        t0 = time.perf_counter()
                        ctx.assemble_batch(d, b.word_off, b.read_len, b.set_start, p)
                        ctx.sync()
                        wall = (time.perf_counter() - t0) * 1e3
                        st = ctx.asm_stats()
                        row = {"wall_ms": wall, "k_sketch_ms": st["kernels"]["k_sketch"]["ms"], "ms_sketch": st["ms_sketch"], "table_ms": 0.0, "filter_ms": 0.0}
                        if kt:
                            verdicts, row["table_ms"] = ctx.last_kmer_table(b.n_sets)
                            n_flt = int((verdicts["n_filtered"][verdicts["peak_hom"] >= 0] > 0).sum())
                        if kf:
                            row["filter_ms"] = ctx.last_kmer_index(b.n_sets)[1]
                        if rep:
                            runs[label].append(row)
            finally:
                ctx.dev_free(d)
            out = {"sets": len(sets), "reads": int(b.n_reads), "sets_with_a_filter": n_flt}
            for label, _, _ in SETTINGS:
                med = {k: statistics.median(r[k] for r in runs[label]) for k in keys}
                med["wall_ms_all"] = [round(r["wall_ms"], 2) for r in runs[label]]
                out[label] = med
                print("%-8s %-14s wall %8.2f ms (%s)  k_sketch %6.3f  sketch stage %7.2f  table stage %6.2f  filter sets + index %6.2f" % (
                    name, label, med["wall_ms"], ", ".join("%.1f" % w for w in med["wall_ms_all"]), med["k_sketch_ms"], med["ms_sketch"], med["table_ms"], med["filter_ms"]))
            result[name] = out
    print(json.dumps({"time_kmer_filter": result}))


if __name__ == "__main__":
    main()
