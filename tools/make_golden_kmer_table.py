#!/usr/bin/env python3
"""Golden data for the k-mer count table stage: what the reference's hifiasm-0.14 (oracle/_ref, `-f0 --write-ec`) logs about its
count histograms on the 30 low-coverage sets of hifiasm_lowcov.json, the 36 repeat sets of hifiasm_repeats.json and 8 unphased
sets (both haplotypes' reads of synth.make_region(0..7)) -> tests/golden/hifiasm_kmer_table.json.  Per set: the md5 of the reads, and
from ha_ft_gen (every k-mer, w = 1) and from the first ha_pt_gen (minimizers, w = 51, ha_ft_gen's filter applied) the lowest point,
the highest peak, the left and right peaks, peak_hom / peak_het, and the filtered / counted / indexed totals.  Digests and integers
only.  Needs /root/reference (oracle/ref.mk)."""
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.kmer_model import reads_of  # noqa: E402

HIFIASM = os.path.join(ROOT, "oracle", "_ref", "hifiasm-0.14")


def analysis(lines):
    """the figures of one ha_analyze_count call and of the function that made it, out of its log lines"""
    out = {"lowest": None, "highest": None, "left": None, "right": None, "peak_hom": -1, "peak_het": -1}
    for l in lines:
        m = re.search(r"ha_analyze_count\] (lowest|highest|left|right): count\[(\d+)\] = (-?\d+)", l)
        if m:
            out[m.group(1)] = [int(m.group(2)), int(m.group(3))]
        m = re.search(r"peak_hom: (-?\d+); peak_het: (-?\d+)", l)
        if m:
            out["peak_hom"], out["peak_het"] = int(m.group(1)), int(m.group(2))
        m = re.search(r"filtered out (\d+) k-mers occurring (-?\d+) or more times", l)
        if m:
            out["filtered"], out["cutoff"] = int(m.group(1)), int(m.group(2))
        m = re.search(r"counted (\d+) distinct minimizer k-mers", l)
        if m:
            out["counted"] = int(m.group(1))
        m = re.search(r"indexed (\d+) positions", l)
        if m:
            out["indexed"] = int(m.group(1))
    return out


def run(tmp, name, reads):
    d = os.path.join(tmp, name)
    os.makedirs(d)
    with open(os.path.join(d, "x.fa"), "w") as f:
        for j, rd in enumerate(reads):
            f.write(f">r{j}\n{rd.decode()}\n")
    p = subprocess.run([HIFIASM, "-f0", "--write-ec", "-o", "x.asm", "-t", "8", "x.fa"], cwd=d, check=True, stdout=subprocess.DEVNULL,
                       stderr=subprocess.PIPE, text=True)
    lines = [l for l in p.stderr.splitlines() if "ha_hist_line" not in l]
    ft_end = next(i for i, l in enumerate(lines) if "ha_ft_gen::" in l)
    pt_end = next(i for i, l in enumerate(lines) if "indexed" in l)
    return analysis(lines[:ft_end + 1]), analysis(lines[ft_end + 1:pt_end + 1])


def main():
    gold = lambda n: json.load(open(os.path.join(ROOT, "tests", "golden", n)))["sets"]
    sets = [{"kind": "lowcov", "region": g["region"], "hap": g["hap"], "width": g["width"], "depth": g["depth"],
             "reference_left_reads_uncorrected": g["reference_left_reads_uncorrected"]} for g in gold("hifiasm_lowcov.json")]
    sets += [{"kind": "repeat", "index": g["index"]} for g in gold("hifiasm_repeats.json")]
    sets += [{"kind": "unphased", "region": i} for i in range(8)]
    with tempfile.TemporaryDirectory() as tmp:
        for n, g in enumerate(sets):
            reads = reads_of(g)
            g["n_reads"] = len(reads)
            g["reads_md5"] = hashlib.md5(b"\n".join(reads)).hexdigest()
            g["ft"], g["pt"] = run(tmp, f"s{n}", reads)
            print(n, g["kind"], g["ft"], flush=True)
    json.dump({"source": "tools/make_golden_kmer_table.py: the stderr of hifiasm-0.14 -f0 --write-ec -t 8 (the reference's, built in place by oracle/ref.mk)",
               "sets": sets}, open(os.path.join(ROOT, "tests", "golden", "hifiasm_kmer_table.json"), "w"), indent=0)


if __name__ == "__main__":
    main()
