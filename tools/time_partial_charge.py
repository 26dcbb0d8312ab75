#!/usr/bin/env python3
"""What fsv_asm_params.partial_charge = 1 costs: fsv_assemble_batch on a phased batch (64 synthetic regions of the bench geometry, both
haplotypes: 128 read sets) and on the 48 mixed sets of tests/golden/hifiasm_mixed_reads.json (flagged FSV_SET_UNPHASED), with the option
0 and 1 alternating in one process, three repeats each after one untimed call of each.  Prints per workload and setting the median wall
time of the call, the library's stage times (fsv_asm_stats), and with 1 the stage's own counters and kernel time (fsv_charge_stats: the
three kernels k_charge_tasks / k_bpm_ext / k_charge_accept between one pair of events per round), then one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from focalsv_amd import _lib, synth  # noqa: E402
from focalsv_amd.readsets import pack_sets  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--regions", type=int, default=64, help="phased batch: synthetic regions (two read sets each)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--workloads", default="phased,mixed", help="which of the two to run (under a profiler: one at a time)")
    args = ap.parse_args()
    gold = json.load(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "hifiasm_mixed_reads.json")))["sets"]
    work = {}
    if "phased" in args.workloads.split(","):
        regs = [synth.make_region(i) for i in range(args.regions)]
        work["phased"] = ([rd for r in regs for rd in r.reads], None)
    if "mixed" in args.workloads.split(","):
        mixed = [synth.make_region(g["region"]) for g in gold]
        work["mixed"] = ([r.reads[0] + r.reads[1] for r in mixed], [1] * len(mixed))
    result = {}
    with _lib.Context(args.device) as ctx:
        for name, (sets, flags) in work.items():
            b = pack_sets(sets)
            d = ctx.upload(b.words)
            runs = {0: [], 1: []}
            try:
                for rep in range(args.repeats + 1):      # the first pass over both settings is the warm-up
                    for pc in (0, 1):
                        p = ctx.default_asm_params()
                        p.partial_charge = pc
                        ctx.sync()
                        t0 = time.perf_counter()
                        ctx.assemble_batch(d, b.word_off, b.read_len, b.set_start, p, flags)
                        ctx.sync()
                        wall = (time.perf_counter() - t0) * 1e3
                        st = ctx.asm_stats()
                        row = {"wall_ms": wall, "ms_verify": st["ms_verify"], "ms_path": st["ms_path"], "ms_consensus": st["ms_consensus"], "ms_total": st["ms_total"]}
                        if pc:
                            row["charge"] = ctx.last_charge()
                        if rep:
                            runs[pc].append(row)
            finally:
                ctx.dev_free(d)
            out = {"sets": len(sets), "reads": int(b.n_reads)}
            for pc in (0, 1):
                med = {k: statistics.median(r[k] for r in runs[pc]) for k in ("wall_ms", "ms_verify", "ms_path", "ms_consensus", "ms_total")}
                med["wall_ms_all"] = [round(r["wall_ms"], 2) for r in runs[pc]]
                if pc:
                    med["charge"] = dict(runs[pc][-1]["charge"], ms=statistics.median(r["charge"]["ms"] for r in runs[pc]))
                out["partial_charge=%d" % pc] = med
                print("%-6s partial_charge=%d  wall %8.2f ms (%s)  verify %7.2f  path %7.2f  consensus %7.2f" % (
                    name, pc, med["wall_ms"], ", ".join("%.1f" % w for w in med["wall_ms_all"]), med["ms_verify"], med["ms_path"], med["ms_consensus"]))
                if pc:
                    print("       fsv_charge_stats (three rounds):", med["charge"])
            result[name] = out
    print(json.dumps({"time_partial_charge": result}))


if __name__ == "__main__":
    main()
