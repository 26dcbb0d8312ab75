#!/usr/bin/env python3
"""GPU drop-in for focalsv/3_assembly.py: same flags (3_assembly.py:11-17), same region-directory contract."""
import os
import sys
from argparse import ArgumentParser

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from focalsv_amd.assembly import assembly, setup_logging  # noqa: E402

parser = ArgumentParser(description="Assemble sequences and call SVs:")
parser.add_argument('--bam_file', '-bam', help="BAM file", required=True)
parser.add_argument('--chr_num', '-chr', type=int, help="Chromosome number for target variant or region", required=True)
parser.add_argument('--ref_file', '-r', help="Reference FASTA file", required=True)
parser.add_argument('--out_dir', '-o', required=True, help="Output directory")
parser.add_argument('--num_threads', '-t_chr', type=int, help="Number of threads, default = 8 (accepted for compatibility)", default=8)
parser.add_argument('--num_cpus', '-t', type=int, help="Number of CPUs, default = 10 (accepted for compatibility)", default=10)
parser.add_argument('--data_type', '-d', type=int, help="HIFI = 0 or CLR = 1 data", default=0)
parser.add_argument('--device', type=int, default=0, help="GPU index (extension)")
parser.add_argument('--kmer-table', action='store_true',
                    help="hifiasm's k-mer count table per read set first: a set without a coverage peak yields no contig, as in hifiasm (extension; default off)")
parser.add_argument('--kmer-filter', action='store_true',
                    help="hifiasm's high-count k-mer filter in every minimizer sketch: a k-mer that occurs 5 x the coverage peak times or more in its "
                         "read set is no minimizer candidate (implies --kmer-table; extension; default off)")
parser.add_argument('--partial-charge', action='store_true',
                    help="hifiasm's non_trim_error_rate: an unmatched window beside a matched one is charged what two extension alignments leave "
                         "uncovered, not its whole length (HiFi only; extension; default off)")
parser.add_argument('--long-reads', action='store_true',
                    help="index every minimizer of a read and chain every anchor of a pair (fsv_asm_params.full_lists): noisy reads above ~32 kb "
                         "keep the seeds beyond their first 4 096 minimizers (extension; default off)")
parser.add_argument('--deep-sets', action='store_true',
                    help="keep every inserted-base vote of a consensus window (fsv_asm_params.deep_sets): read sets deeper than ~45 x per haplotype "
                         "no longer drop votes beyond a window's 256 events and raise status bit 8 (extension; default off)")

if __name__ == "__main__":
    args = parser.parse_args()
    logger = setup_logging("3_ASSEMBLY", args.out_dir)
    logger.info("Starting assembly process (MI355X)")
    if args.data_type != 0:
        logger.warning("CLR/ONT read sets go through the same GPU assembler (the reference uses Flye/Shasta there)")
    st = assembly(args.out_dir, args.num_cpus, args.num_threads, args.data_type, logger, device=args.device, kmer_table=args.kmer_table or args.kmer_filter,
                  partial_charge=args.partial_charge, kmer_filter=args.kmer_filter, long_reads=args.long_reads, deep_sets=args.deep_sets)
    bad = {k: v for k, v in st.items() if v}
    if bad:
        logger.warning(f"read sets with a non-zero status: {bad}")
