#!/usr/bin/env python3
"""Mint tests/golden/sketch_grid.json.gz: the reference's own ha_sketch (sketch.cpp:39-137) over the (w, k, HPC) grid of
tests/sketch_cases.py -- 19 windows from 1 to 255 x 13 k-mer lengths from 1 to 63 x both HPC settings.

Runs only where oracle/_ref/ha14_kernels exists (`make -f oracle/ref.mk`, from the reference's hifiasm-0.14 sources).  Per grid point
the fixture holds, for every edge length and a rotating few of the tandem / homopolymer / cut-run cases (sketch_cases.fixture_cases),
parallel lists: the sequence length, a digest of the sequence (sequences are not stored: the digest only tells a drifted generator
from a wrong sketch), the number of minimizers the reference reports, and a digest of its reply "hash:pos:rev:span ..." as the
harness prints it.  Digests are the leading base64 characters of an md5 (sketch_cases.SEQ_DIGEST / MZ_DIGEST): two full ones for
each of the ~18 000 cases would make this the largest fixture in the tree; the JSON is gzipped (bed_whole_genome.bed.gz is the
precedent) and written without a time stamp, so a second run gives the same bytes.  Only recorded results are written."""
import gzip
import io
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import sketch_cases as SC  # noqa: E402

HARNESS = os.path.join(ROOT, "oracle", "_ref", "ha14_kernels")
OUT = os.path.join(ROOT, "tests", "golden", "sketch_grid.json.gz")


def ask(lines):
    p = subprocess.run([HARNESS], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
    out = p.stdout.strip("\n").split("\n")
    assert len(out) == len(lines), (len(out), len(lines))
    return out


def main():
    if not os.path.exists(HARNESS):
        sys.exit("build the reference harness first: make -f oracle/ref.mk")
    points, n_cases, n_mz = [], 0, 0
    for (w, k, hpc) in SC.GRID:
        cases = SC.fixture_cases(w, k, hpc)
        rep = ask(["sketch %d %d %d %s" % (w, k, hpc, c["seq"]) for c in cases])
        cnt, dig = [], []
        for r in rep:
            n, _, text = r.partition(" ")
            assert int(n) == (len(text.split(" ")) if text else 0)
            cnt.append(int(n))
            dig.append(SC.mz_digest(text))
        points.append({"w": w, "k": k, "hpc": hpc, "extra": [c["kind"] + ":" + c["tag"] for c in cases if c["kind"] != "edge"],
                       "len": [len(c["seq"]) for c in cases], "seq": "".join(SC.seq_digest(c["seq"]) for c in cases),
                       "n": cnt, "mz": "".join(dig)})
        n_cases += len(cases)
        n_mz += sum(cnt)
    doc = {"source": "ha_sketch via oracle/_ref/ha14_kernels on tests/sketch_cases.fixture_cases",
           "fields": "per grid point, one entry per case in generator order: len = bases, seq = %d base64 characters of md5(sequence), "
                     "n = minimizers, mz = %d base64 characters of md5('hash:pos:rev:span' joined by blanks)" % (SC.SEQ_DIGEST, SC.MZ_DIGEST),
           "cases": n_cases, "minimizers": n_mz, "points": points}
    # gzip with no name and no time stamp in its header: the same cases give the same bytes
    with open(OUT, "wb") as raw, gzip.GzipFile(filename="", mode="wb", compresslevel=9, fileobj=raw, mtime=0) as gz, io.TextIOWrapper(gz, newline="\n") as f:
        f.write("{" + ",\n".join(json.dumps(key) + ":" + json.dumps(doc[key], separators=(",", ":")) for key in ("source", "fields", "cases", "minimizers")))
        f.write(',\n"points":[\n' + ",\n".join(json.dumps(p, separators=(",", ":")) for p in points) + "\n]}\n")
    print("sketch_grid: %d grid points, %d cases, %d minimizers, %d bytes" % (len(points), n_cases, n_mz, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
