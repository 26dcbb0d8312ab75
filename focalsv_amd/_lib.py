"""ctypes binding of libfocalsv_hip.so (include/focalsv_hip.h).

The library is built in-tree by `make -C focalsv_amd/csrc` (see __graft_entry__.build).
Nothing here falls back to a CPU implementation: a missing library or device raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfocalsv_hip.so")

FSV_WINDOW, FSV_K_FULL, FSV_K_MAX = 375, 15, 31

WTASK_DTYPE = np.dtype(
    [("x_word", "<u4"), ("y_word", "<u4"), ("x_start", "<i4"), ("y_start", "<i4"), ("y_len", "<i4"),
     ("x_len", "<u2"), ("k", "u1"), ("y_rev", "u1"), ("ovl", "<u4"), ("win", "<u4")], align=False)
MZ_DTYPE = np.dtype([("hash", "<u8"), ("pos", "<u4"), ("rev", "u1"), ("span", "u1"), ("pad", "<u2")])
WRES_DTYPE = np.dtype(
    [("end_site", "<i4"), ("err", "<i4"), ("y_beg", "<i4"), ("extra_begin", "<i2"), ("extra_end", "<i2")], align=False)
assert WTASK_DTYPE.itemsize == 32 and WRES_DTYPE.itemsize == 16
WPATH_DTYPE = np.dtype([("ry_start", "<i4"), ("ry_end", "<i4"), ("path_len", "<i2"), ("err", "<i2"), ("state", "u1"), ("y_rev", "u1"),
                        ("pad", "<u2"), ("y_word", "<u4"), ("y_len", "<i4"), ("ops", "u1", (104,))], align=False)
assert WPATH_DTYPE.itemsize == 128
OVL_DTYPE = np.dtype([("q", "<u4"), ("t", "<u4"), ("x_s", "<i4"), ("x_e", "<i4"), ("y_s", "<i4"), ("y_e", "<i4"), ("score", "<i4"), ("n_chain", "<i4"),
                      ("chain_off", "<i4"), ("first_win", "<i4"), ("n_win", "<i4"), ("align_len", "<i4"), ("err_sum", "<i4"),
                      ("rev", "u1"), ("is_match", "u1"), ("exact", "u1"), ("valid", "u1")], align=False)
assert OVL_DTYPE.itemsize == 56


class AsmParams(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("k", "w", "hpc", "n_rounds", "min_ovlp", "min_anchors", "lookback", "bw_ec", "bw_final",
                                         "min_contig_reads", "win_rate_pm", "k_cap", "accept_err_pm", "bw_rechain", "w_later", "partition", "second_round", "ins_dag",
                                         "min_anchors_final", "min_ovlp_final", "graph_layout", "junction_cigars", "deep_sets", "full_lists", "kmer_filter", "kmer_table", "partial_charge")]


class ReadSets(C.Structure):
    _fields_ = [("store_dev", C.c_void_p), ("word_off", C.c_void_p), ("read_len", C.c_void_p), ("set_start", C.c_void_p),
                ("n_reads", C.c_uint32), ("n_sets", C.c_uint32), ("set_flags", C.c_void_p)]


SET_UNPHASED = 1
# return / status codes of include/focalsv_hip.h
OK, ENODEV, EINVAL, ENOMEM, EHIP, ECAP, EUNSUP = 0, -1, -2, -3, -4, -5, -6
# set_status warning bits (FSV_W_*)
W_MZ_TRUNC, W_ANCHOR_TRUNC, W_NO_LAYOUT, W_INS_EVENTS, W_WINDOW_KEPT, W_INTERNAL, W_SITES = 1, 2, 4, 8, 16, 32, 64
W_LOW_COV = 128
KMER_BINS = 4096
# fsv_kmer_set: the verdict of the k-mer count table stage on one read set
KMER_SET_DTYPE = np.dtype([("peak_hom", "<i4"), ("peak_het", "<i4"), ("cutoff", "<i4"), ("low_i", "<i4"), ("max_i", "<i4"), ("pad", "<i4"),
                           ("n_entries", "<u8"), ("n_distinct", "<u8"), ("n_filtered", "<u8"), ("n_indexed", "<u8")])
assert KMER_SET_DTYPE.itemsize == 56
# fsv_kmer_index_set: the figures of hifiasm's first ha_pt_gen on one read set (the filtered sketch, counted)
KMER_INDEX_DTYPE = np.dtype([("n_entries", "<u8"), ("n_distinct", "<u8"), ("n_indexed", "<u8"), ("low_i", "<i4"), ("max_i", "<i4"),
                             ("peak_hom", "<i4"), ("peak_het", "<i4")])
assert KMER_INDEX_DTYPE.itemsize == 40
# fsv_wext: the result of one extension alignment (fsv_bpm_extensions)
WEXT_DTYPE = np.dtype([("t_end", "<i4"), ("err", "<i4"), ("p_end", "<i4"), ("pad", "<i4")])
assert WEXT_DTYPE.itemsize == 16


class ChargeStats(C.Structure):
    """fsv_charge_stats: counters of the partial-charge stage of the last assemble_batch with partial_charge = 1"""
    _fields_ = [(n, C.c_uint64) for n in ("n_overlaps", "n_windows", "n_ext", "n_accepted", "n_flipped")] + [("ms", C.c_double)]


class Contigs(C.Structure):
    _fields_ = [("seq", C.c_void_p), ("seq_cap", C.c_uint64), ("off", C.c_void_p), ("set", C.c_void_p), ("n_reads", C.c_void_p),
                ("contig_cap", C.c_uint32), ("n_contigs", C.c_uint32), ("set_status", C.c_void_p)]


class KernelStat(C.Structure):
    _fields_ = [("name", C.c_char * 24), ("ms", C.c_double), ("launches", C.c_uint64), ("algo_bytes", C.c_uint64)]


class AsmStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_pairs", "n_overlaps", "n_windows", "n_windows_matched", "n_paths", "n_path_dp",
                                          "dp_columns", "algo_bytes", "n_exact_overlaps", "n_inexact_candidates", "n_path_fr", "n_junction_cigars", "n_junction_used")] + \
               [(n, C.c_double) for n in ("ms_sketch", "ms_chain", "ms_verify", "ms_path", "ms_consensus", "ms_final", "ms_total")] + \
               [("n_kernels", C.c_uint32), ("pad", C.c_uint32), ("kernels", KernelStat * 24)]     # FSV_MAX_KERNEL_STATS


class AlnParams(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("k", "w", "min_anchors", "lookback", "max_gap", "a", "b", "q", "e", "q2", "e2", "pad",
                                         "max_mm_run", "xdrop", "max_cells")]


class Alns(C.Structure):
    _fields_ = [("rec", C.c_void_p), ("rec_cap", C.c_uint32), ("n_rec", C.c_uint32), ("cigar", C.c_void_p), ("cigar_cap", C.c_uint64),
                ("n_cigar", C.c_uint64), ("contig_status", C.c_void_p)]


class AlnTags(C.Structure):
    """struct fsv_aln_tags"""
    _fields_ = [("nm", C.c_void_p), ("cs_off", C.c_void_p), ("cs", C.c_void_p), ("cs_cap", C.c_uint64), ("cs_bytes", C.c_uint64),
                ("rec_status", C.c_void_p), ("ms", C.c_double)]


class RefStats(C.Structure):
    """fsv_ref_stats"""
    _fields_ = [(n, C.c_uint64) for n in ("tiles", "owned", "dropped_n", "keys", "keys_above", "stored", "slots", "max_count")] + [("ms", C.c_double)]


class ContigMapq(C.Structure):
    """struct fsv_contig_mapq"""
    _fields_ = [(n, C.c_void_p) for n in ("f1", "f2", "m", "cutoff", "thin", "flags", "rec_status")] + [("ms", C.c_double)]


MQ_TRUNC = 1   # FSV_MQ_TRUNC


class BamOut(C.Structure):
    """fsv_bam_out"""
    _fields_ = [("n_refs", C.c_uint32), ("ref_name", C.POINTER(C.c_char_p)), ("ref_len", C.c_void_p), ("header_text", C.c_char_p),
                ("n_rec", C.c_uint64)] + \
               [(n, C.c_void_p) for n in ("ref_id", "pos", "flag", "mapq", "qname_off", "qname", "cigar_off", "n_cigar_op", "cigar", "seq_off", "seq",
                                          "nm", "cs_off", "cs", "sa_off", "sa")]


class AlnStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_pairs", "n_events", "dp_cells", "algo_bytes")] + \
               [(n, C.c_double) for n in ("ms_seed", "ms_chain", "ms_events", "ms_dp", "ms_total")] + [("n_boxes", C.c_uint64)]


ALN_REC_DTYPE = np.dtype([("ref_start", "<i4"), ("ref_end", "<i4"), ("q_start", "<i4"), ("q_end", "<i4"), ("n_cigar", "<u4"),
                          ("n_chain", "<u4"), ("cigar_off", "<u8"), ("contig", "<u4"), ("rev", "u1"), ("mapq", "u1"), ("pad", "u1", (2,))])
assert ALN_REC_DTYPE.itemsize == 40


class BamRecords(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("pos", "ref_end", "flag", "mapq", "cigar_off", "n_cigar_op", "qname_off", "l_seq", "cigar", "qname",
                                          "seq_word_off", "seq_words_buf", "seq_ascii", "seq_ascii_off", "ref_id", "sa", "sa_off", "ps", "hp")] + \
               [(n, C.c_uint64) for n in ("rec_cap", "cigar_cap", "qname_cap", "seq_cap", "seq_ascii_cap", "sa_cap", "n_rec", "n_cigar", "qname_bytes",
                                          "seq_words", "seq_ascii_bytes", "sa_bytes")]


READ_SIG_DTYPE = np.dtype([("rec", "<u4"), ("type", "<u4"), ("ref_pos", "<i4"), ("len", "<i4"), ("read_off", "<i4"), ("pad", "<u4")])
assert READ_SIG_DTYPE.itemsize == 24


class FsvError(RuntimeError):
    def __init__(self, code, where, detail=""):
        self.code = code
        super().__init__(f"{where}: {strerror(code)} ({code}){': ' + detail if detail else ''}")


_lib = None


def load():
    """Load the shared library; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(make -C focalsv_amd/csrc). focalsv_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    vp, u32p, u64p = C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    sig = {
        "fsv_version": (C.c_int, []),
        "fsv_strerror": (C.c_char_p, [C.c_int]),
        "fsv_ctx_create": (C.c_int, [C.c_int, C.POINTER(vp)]),
        "fsv_ctx_destroy": (None, [vp]),
        "fsv_ctx_set_stream": (C.c_int, [vp, vp]),
        "fsv_ctx_sync": (C.c_int, [vp]),
        "fsv_last_error": (C.c_char_p, [vp]),
        "fsv_device_info": (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), u64p, C.c_char_p, C.c_size_t]),
        "fsv_dev_alloc": (C.c_int, [vp, C.c_size_t, C.POINTER(vp)]),
        "fsv_dev_free": (C.c_int, [vp, vp]),
        "fsv_h2d": (C.c_int, [vp, vp, vp, C.c_size_t]),
        "fsv_d2h": (C.c_int, [vp, vp, vp, C.c_size_t]),
        "fsv_pack_bound": (C.c_size_t, [vp, C.c_uint32]),
        "fsv_pack_reads": (C.c_int, [vp, vp, C.c_uint32, vp, C.c_size_t, vp]),
        "fsv_bpm_windows_dev": (C.c_int, [vp, vp, vp, C.c_uint32, vp]),
        "fsv_bpm_windows": (C.c_int, [vp, vp, C.c_size_t, vp, C.c_uint32, vp]),
        "fsv_bpm_paths": (C.c_int, [vp, vp, C.c_size_t, vp, C.c_uint32, vp, vp]),
        "fsv_asm_default_params": (None, [C.POINTER(AsmParams)]),
        "fsv_asm_ont_params": (None, [C.POINTER(AsmParams)]),
        "fsv_asm_clr_params": (None, [C.POINTER(AsmParams)]),
        "fsv_assemble_batch_bound": (C.c_int, [C.POINTER(ReadSets), u64p, u32p]),
        "fsv_assemble_batch": (C.c_int, [vp, C.POINTER(ReadSets), C.POINTER(AsmParams), C.POINTER(Contigs)]),
        "fsv_asm_last_stats": (C.c_int, [vp, C.POINTER(AsmStats)]),
        "fsv_asm_fetch_reads": (C.c_int, [vp, vp, C.c_uint64, vp, C.c_uint32]),
        "fsv_sketch_reads": (C.c_int, [vp, C.POINTER(ReadSets), C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, C.c_uint64, vp]),
        "fsv_asm_overlaps": (C.c_int, [vp, C.POINTER(ReadSets), C.POINTER(AsmParams), C.c_int32, vp, C.c_uint32, vp, C.c_uint64, vp, vp, C.c_uint64,
                                       u32p, u32p, vp]),
        "fsv_asm_last_long_lists": (C.c_int, [vp, vp, vp]),
        "fsv_asm_last_deep_windows": (C.c_int, [vp, vp, vp, vp]),
        "fsv_read_index": (C.c_int, [vp, C.POINTER(ReadSets), C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, C.c_uint64, vp, vp]),
        "fsv_sketch_reads_filtered": (C.c_int, [vp, C.POINTER(ReadSets), C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, C.c_uint64, vp, vp, vp]),
        "fsv_kmer_index": (C.c_int, [vp, C.POINTER(ReadSets), C.c_int32, C.c_int32, C.c_int32, vp, vp, vp]),
        "fsv_asm_last_kmer_index": (C.c_int, [vp, vp, C.c_uint32, C.POINTER(C.c_double)]),
        "fsv_kmer_peaks": (C.c_int, [vp, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
        "fsv_kmer_table": (C.c_int, [vp, C.POINTER(ReadSets), C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, C.c_uint64, vp]),
        "fsv_asm_last_kmer_table": (C.c_int, [vp, vp, C.c_uint32, C.POINTER(C.c_double)]),
        "fsv_bpm_extensions": (C.c_int, [vp, vp, C.c_size_t, vp, vp, C.c_uint32, C.c_int32, vp]),
        "fsv_partial_charge": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64]),
        "fsv_asm_last_charge": (C.c_int, [vp, C.POINTER(ChargeStats)]),
        "fsv_aln_default_params": (None, [C.POINTER(AlnParams)]),
        "fsv_align_batch": (C.c_int, [vp, vp, vp, C.c_uint32, vp, vp, vp, C.c_uint32, C.POINTER(AlnParams), C.POINTER(Alns)]),
        "fsv_aln_last_stats": (C.c_int, [vp, C.POINTER(AlnStats)]),
        "fsv_aln_tags": (C.c_int, [vp, vp, vp, C.c_uint32, vp, vp, vp, C.c_uint32, C.POINTER(Alns), C.POINTER(AlnTags)]),
        "fsv_ref_index_build": (C.c_int, [vp, vp, C.c_uint64, C.c_int32, C.c_int32, C.c_int32]),
        "fsv_ref_index_stats": (C.c_int, [vp, C.POINTER(RefStats)]),
        "fsv_ref_index_drop": (C.c_int, [vp]),
        "fsv_ref_index_lookup": (C.c_int, [vp, vp, C.c_uint32, vp, vp, vp, C.c_uint64]),
        "fsv_mapq_of": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32]),
        "fsv_contig_mapq": (C.c_int, [vp, vp, vp, C.c_uint32, vp, vp, C.c_uint32, C.POINTER(Alns), C.POINTER(AlnParams), C.POINTER(ContigMapq)]),
        "fsv_bam_write": (C.c_int, [C.c_char_p, C.POINTER(BamOut), C.c_int]),
        "fsv_bam_open": (C.c_int, [C.c_char_p, C.POINTER(vp)]),
        "fsv_bam_close": (None, [vp]),
        "fsv_bam_n_refs": (C.c_int, [vp]),
        "fsv_bam_ref_name": (C.c_char_p, [vp, C.c_int]),
        "fsv_bam_ref_length": (C.c_int64, [vp, C.c_int]),
        "fsv_bam_ref_id": (C.c_int, [vp, C.c_char_p]),
        "fsv_bam_has_index": (C.c_int, [vp]),
        "fsv_bam_set_threads": (None, [vp, C.c_int]),
        "fsv_bam_fetch": (C.c_int, [vp, C.c_int, C.c_int64, C.c_int64, C.POINTER(BamRecords), C.c_int]),
        "fsv_read_signatures": (C.c_int, [vp, C.POINTER(BamRecords), C.c_int, C.c_int, vp, C.c_uint32, u32p]),
        "fsv_nw": (C.c_int, [vp, C.c_char_p, C.c_int32, C.c_char_p, C.c_int32, C.POINTER(AlnParams), C.POINTER(C.c_int32), vp, C.c_uint32,
                             C.POINTER(C.c_uint32)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)  # AttributeError here = header/library mismatch
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def strerror(code):
    return load().fsv_strerror(code).decode()


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def pack_reads(reads):
    """K0: list of str/bytes -> (words uint32[], word_off uint64[n+1], lens int32[n])."""
    lib = load()
    bs = [r.encode() if isinstance(r, str) else bytes(r) for r in reads]
    lens = np.array([len(b) for b in bs], dtype=np.int64)
    seq_off = np.zeros(len(bs) + 1, dtype=np.uint64)
    np.cumsum(lens, out=seq_off[1:])
    seqs = np.frombuffer(b"".join(bs), dtype=np.uint8) if bs else np.zeros(0, np.uint8)
    cap = lib.fsv_pack_bound(_ptr(seq_off), len(bs))
    words = np.empty(cap, dtype=np.uint32)
    word_off = np.zeros(len(bs) + 1, dtype=np.uint64)
    rc = lib.fsv_pack_reads(_ptr(seqs), _ptr(seq_off), len(bs), _ptr(words), cap, _ptr(word_off))
    if rc:
        raise FsvError(rc, "fsv_pack_reads")
    return words, word_off, lens.astype(np.int32)


def join_refs(refs):
    """reference windows (list of bytes) -> (concatenated uint8 array, uint64 offsets) as fsv_align_batch takes them"""
    roff = np.zeros(len(refs) + 1, dtype=np.uint64)
    np.cumsum([len(r) for r in refs], out=roff[1:])
    return np.frombuffer(b"".join(refs) + b"\0", dtype=np.uint8), roff


def bam_write(path, refs, records, header_text="@HD\tVN:1.6\tSO:coordinate\n", threads=4):
    """fsv_bam_write (host only, no GPU): a coordinate-sorted BAM at `path` and its index at path + '.bai'.
    refs: [(name, length)]; records: dicts with ref (index, -1 unmapped), pos (0-based, -1 unmapped), flag, mapq, qname, cigar ([(op, len)]
    or a uint32 array in BAM encoding), seq (str / bytes), and optionally nm (int), cs (str / bytes), sa (str); the writer sorts them.
    Raises FsvError on a bad argument or an unwritable path (no file is left behind)."""
    n = len(records)

    def b(x):
        return x.encode() if isinstance(x, str) else bytes(x)

    def joined(parts, terminated):
        off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum([len(p) + terminated for p in parts], out=off[1:])
        return np.frombuffer((b"\0" if terminated else b"").join(parts) + b"\0", dtype=np.uint8), off

    cig = [np.asarray([(int(l) << 4) | int(op) for op, l in r["cigar"]] if not isinstance(r["cigar"], np.ndarray) else r["cigar"], dtype=np.uint32)
           for r in records]
    ncig = np.asarray([len(c) for c in cig], dtype=np.uint32)
    coff = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(ncig, out=coff[1:])
    cigar = np.concatenate(cig + [np.zeros(1, np.uint32)])
    qname, qoff = joined([b(r["qname"]) for r in records], 1)
    seq, soff = joined([b(r.get("seq", "")) for r in records], 0)
    a = {"ref_id": np.asarray([r["ref"] for r in records], dtype=np.int32), "pos": np.asarray([r["pos"] for r in records], dtype=np.int32),
         "flag": np.asarray([r.get("flag", 0) for r in records], dtype=np.uint16), "mapq": np.asarray([r.get("mapq", 60) for r in records], dtype=np.uint8),
         "qname_off": qoff, "qname": qname, "cigar_off": coff, "n_cigar_op": ncig, "cigar": cigar, "seq_off": soff, "seq": seq}
    if any(r.get("nm") is not None for r in records):
        a["nm"] = np.asarray([-(1 << 31) if r.get("nm") is None else r["nm"] for r in records], dtype=np.int32)
    if any(r.get("cs") for r in records):
        a["cs"], a["cs_off"] = joined([b(r.get("cs") or "") for r in records], 0)
    if any(r.get("sa") for r in records):
        a["sa"], a["sa_off"] = joined([b(r.get("sa") or "") for r in records], 1)
    names = (C.c_char_p * max(1, len(refs)))(*[nm.encode() for nm, _ in refs])
    rlen = np.asarray([ln for _, ln in refs] + [0], dtype=np.int32)
    out = BamOut(len(refs), names, _ptr(rlen), header_text.encode(), n)
    for k, v in a.items():
        setattr(out, k, _ptr(v).value)
    rc = load().fsv_bam_write(os.fsencode(path), C.byref(out), int(threads))
    if rc:
        raise FsvError(rc, "fsv_bam_write", str(path))
    return path


def kmer_peaks(hist, start_cnt=5):
    """fsv_kmer_peaks (host only, no GPU): hifiasm's ha_analyze_count on a k-mer count histogram
    -> (peak_hom, peak_het, low_i, max_i); peak_hom -1 when the histogram has no coverage peak"""
    h = np.ascontiguousarray(hist, dtype=np.int64)
    het, low, mx = C.c_int32(), C.c_int32(), C.c_int32()
    hom = load().fsv_kmer_peaks(_ptr(h), len(h), int(start_cnt), C.byref(het), C.byref(low), C.byref(mx))
    if hom < -1:
        raise FsvError(hom, "fsv_kmer_peaks")
    return hom, het.value, low.value, mx.value


def mapq_of(f1, f2, m):
    """fsv_mapq_of (host only, no GPU): the mapping quality of Li 2018, section 2.1.4, from the best chain score at a record's own locus, the
    best elsewhere and the own chain's anchors"""
    return int(load().fsv_mapq_of(int(f1), int(f2), int(m)))


def partial_charge(n, al0, er0, al1, er1, terr):
    """fsv_partial_charge (host only, no GPU): non_trim_error_rate's charge for an unmatched window of n bases that the extension from the
    left covers al0 bases of with er0 errors and the one from the right al1 with er1 (al = 0: none) -> the new running total"""
    return int(load().fsv_partial_charge(int(n), int(al0), int(er0), int(al1), int(er1), int(terr)))


def path_ops(p) -> bytes:
    """fsv_wpath record -> its ops start-to-end, one per byte (0 match 1 mismatch 2 y-only 3 x-only)"""
    b = np.asarray(p["ops"], dtype=np.uint8)
    fields = np.stack([(b >> s) & 3 for s in (0, 2, 4, 6)], axis=1).reshape(-1)
    return bytes(fields[: int(p["path_len"])])


class ContigBatch:
    """The contigs of one fsv_assemble_batch call: a read-only sequence of `bytes`, cut out of the library's output buffer
    on access (a batch is tens of MB; most callers touch a few contigs or none -- the aligner takes them from the device)."""

    def __init__(self, seq: np.ndarray, off: np.ndarray):
        self._seq, self._off = seq, off

    def __len__(self):
        return len(self._off) - 1

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self)))]
        if i < 0:
            i += len(self)
        if not 0 <= i < len(self):
            raise IndexError(i)
        return self._seq[int(self._off[i]):int(self._off[i + 1])].tobytes()

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def __eq__(self, other):
        return list(self) == list(other)

    def length(self, i) -> int:
        return int(self._off[i + 1] - self._off[i])


class Context:
    """One fsv_ctx (= one GPU + one stream).  Raises FsvError(FSV_ENODEV) without an MI355X."""

    def __init__(self, device=0, stream=None):
        self._lib = load()
        h = C.c_void_p()
        rc = self._lib.fsv_ctx_create(int(device), C.byref(h))
        if rc:
            raise FsvError(rc, "fsv_ctx_create")
        self._h = h
        if stream is not None:
            self.check(self._lib.fsv_ctx_set_stream(self._h, C.c_void_p(stream)), "fsv_ctx_set_stream")

    def close(self):
        if getattr(self, "_h", None):
            self._lib.fsv_ctx_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def check(self, rc, where):
        if rc:
            raise FsvError(rc, where, self._lib.fsv_last_error(self._h).decode())

    def sync(self):
        self.check(self._lib.fsv_ctx_sync(self._h), "fsv_ctx_sync")

    def device_info(self):
        ncu, clk, hbm = C.c_int(), C.c_int(), C.c_uint64()
        name = C.create_string_buffer(128)
        self.check(self._lib.fsv_device_info(self._h, C.byref(ncu), C.byref(clk), C.byref(hbm), name, 128), "fsv_device_info")
        return {"n_cu": ncu.value, "clock_khz": clk.value, "hbm_bytes": hbm.value, "name": name.value.decode()}

    # K5 -----------------------------------------------------------------------------
    def bpm_windows(self, words, tasks):
        """host arrays in, host results out (fsv_bpm_windows)."""
        tasks = np.ascontiguousarray(tasks, dtype=WTASK_DTYPE)
        words = np.ascontiguousarray(words, dtype=np.uint32)
        res = np.empty(len(tasks), dtype=WRES_DTYPE)
        self.check(self._lib.fsv_bpm_windows(self._h, _ptr(words), words.size, _ptr(tasks), len(tasks), _ptr(res)), "fsv_bpm_windows")
        return res

    def bpm_paths(self, words, tasks):
        """K5 + K6 on host tasks (fsv_bpm_paths) -> (results, paths); `path_ops(paths[i])` unpacks the 2-bit ops"""
        tasks = np.ascontiguousarray(tasks, dtype=WTASK_DTYPE)
        words = np.ascontiguousarray(words, dtype=np.uint32)
        res = np.empty(len(tasks), dtype=WRES_DTYPE)
        paths = np.zeros(len(tasks), dtype=WPATH_DTYPE)
        self.check(self._lib.fsv_bpm_paths(self._h, _ptr(words), words.size, _ptr(tasks), len(tasks), _ptr(res), _ptr(paths)), "fsv_bpm_paths")
        return res, paths

    def bpm_extensions(self, words, tasks, dirs, k_cap=31):
        """the extension kernel of the partial charge on host tasks (fsv_bpm_extensions) -> WEXT_DTYPE rows; dirs[i] = 1 aligns both
        strings reversed and answers in the reversed coordinates"""
        tasks = np.ascontiguousarray(tasks, dtype=WTASK_DTYPE)
        words = np.ascontiguousarray(words, dtype=np.uint32)
        dirs = np.ascontiguousarray(dirs, dtype=np.uint8)
        assert len(dirs) == len(tasks)
        out = np.zeros(len(tasks), dtype=WEXT_DTYPE)
        self.check(self._lib.fsv_bpm_extensions(self._h, _ptr(words), words.size, _ptr(tasks), _ptr(dirs), len(tasks), int(k_cap), _ptr(out)),
                   "fsv_bpm_extensions")
        return out

    def bpm_windows_dev(self, store_ptr, tasks_ptr, n_tasks, res_ptr):
        self.check(self._lib.fsv_bpm_windows_dev(self._h, C.c_void_p(store_ptr), C.c_void_p(tasks_ptr), n_tasks, C.c_void_p(res_ptr)),
                   "fsv_bpm_windows_dev")


    # assembler boundary -------------------------------------------------------------
    def default_asm_params(self):
        p = AsmParams()
        self._lib.fsv_asm_default_params(C.byref(p))
        return p

    def ont_asm_params(self):
        """the error model for ONT-profile reads (fsv_asm_ont_params)"""
        p = AsmParams()
        self._lib.fsv_asm_ont_params(C.byref(p))
        return p

    def clr_asm_params(self):
        """the error model for PacBio CLR reads (fsv_asm_clr_params)"""
        p = AsmParams()
        self._lib.fsv_asm_clr_params(C.byref(p))
        return p

    def upload(self, arr):
        """numpy array -> device pointer (caller frees with dev_free)."""
        arr = np.ascontiguousarray(arr)
        ptr = C.c_void_p()
        self.check(self._lib.fsv_dev_alloc(self._h, arr.nbytes + 64, C.byref(ptr)), "fsv_dev_alloc")
        self.check(self._lib.fsv_h2d(self._h, ptr, _ptr(arr), arr.nbytes), "fsv_h2d")
        return ptr.value

    def dev_free(self, ptr):
        self.check(self._lib.fsv_dev_free(self._h, C.c_void_p(ptr)), "fsv_dev_free")

    def assemble_batch(self, store_dev, word_off, read_len, set_start, params=None, set_flags=None):
        """fsv_assemble_batch.  store_dev: device pointer of the 2-bit store; the rest are host numpy arrays.
        -> (contigs: list[bytes], contig_set: ndarray, contig_n_reads: ndarray, set_status: ndarray)"""
        word_off = np.ascontiguousarray(word_off, dtype=np.uint64)
        read_len = np.ascontiguousarray(read_len, dtype=np.int32)
        set_start = np.ascontiguousarray(set_start, dtype=np.uint32)
        flags = None if set_flags is None else np.ascontiguousarray(set_flags, dtype=np.uint8)
        assert flags is None or len(flags) == len(set_start) - 1
        rs = ReadSets(C.c_void_p(store_dev), _ptr(word_off).value, _ptr(read_len).value, _ptr(set_start).value, len(read_len), len(set_start) - 1,
                      None if flags is None else _ptr(flags).value)
        cap, ccap = C.c_uint64(), C.c_uint32()
        self.check(self._lib.fsv_assemble_batch_bound(C.byref(rs), C.byref(cap), C.byref(ccap)), "fsv_assemble_batch_bound")
        seq = np.empty(cap.value, dtype=np.uint8)
        off = np.zeros(ccap.value + 1, dtype=np.uint64)
        cset = np.zeros(ccap.value, dtype=np.uint32)
        cnr = np.zeros(ccap.value, dtype=np.uint32)
        status = np.zeros(max(1, rs.n_sets), dtype=np.int32)
        out = Contigs(_ptr(seq).value, cap.value, _ptr(off).value, _ptr(cset).value, _ptr(cnr).value, ccap.value, 0, _ptr(status).value)
        p = params if params is not None else self.default_asm_params()
        self.check(self._lib.fsv_assemble_batch(self._h, C.byref(rs), C.byref(p), C.byref(out)), "fsv_assemble_batch")
        n = out.n_contigs
        self._last_contig_bytes = int(off[n])
        return ContigBatch(seq, off[: n + 1].copy()), cset[:n].copy(), cnr[:n].copy(), status[:rs.n_sets].copy()

    def sketch_reads(self, store_dev, word_off, read_len, w=51, k=51, hpc=1, variant=0, out_cap=None):
        """K1 exposed: per read, its minimizers in position order -> list of structured arrays (hash, pos, rev, span).
        out_cap: entries of the output buffer (default: one per base and some, which always suffices)"""
        word_off = np.ascontiguousarray(word_off, dtype=np.uint64)
        read_len = np.ascontiguousarray(read_len, dtype=np.int32)
        ss = np.asarray([0, len(read_len)], dtype=np.uint32)
        rs = ReadSets(C.c_void_p(store_dev), _ptr(word_off).value, _ptr(read_len).value, _ptr(ss).value, len(read_len), 1)
        cap = int(read_len.sum()) + 64 * len(read_len) + 64 if out_cap is None else int(out_cap)
        out = np.zeros(max(cap, 1), dtype=MZ_DTYPE)
        off = np.zeros(len(read_len) + 1, dtype=np.uint64)
        self.check(self._lib.fsv_sketch_reads(self._h, C.byref(rs), w, k, hpc, variant, _ptr(out), cap, _ptr(off)), "fsv_sketch_reads")
        return [out[int(off[i]):int(off[i + 1])].copy() for i in range(len(read_len))]

    def read_index(self, store_dev, word_off, read_len, w=51, k=51, hpc=1, full_lists=0):
        """fsv_read_index (test hook): per read the index the chain kernels see -- 2m entries, [0, m) by hash, [m, 2m) by position -- and the
        reads' warning bits -> (list of structured arrays, warn[n_reads])"""
        word_off = np.ascontiguousarray(word_off, dtype=np.uint64)
        read_len = np.ascontiguousarray(read_len, dtype=np.int32)
        ss = np.asarray([0, len(read_len)], dtype=np.uint32)
        rs = ReadSets(C.c_void_p(store_dev), _ptr(word_off).value, _ptr(read_len).value, _ptr(ss).value, len(read_len), 1)
        cap = 2 * int(read_len.sum()) + 64 * len(read_len) + 64
        out = np.zeros(max(cap, 1), dtype=MZ_DTYPE)
        off = np.zeros(len(read_len) + 1, dtype=np.uint64)
        warn = np.zeros(max(1, len(read_len)), dtype=np.uint32)
        self.check(self._lib.fsv_read_index(self._h, C.byref(rs), w, k, hpc, int(full_lists), _ptr(out), cap, _ptr(off), _ptr(warn)), "fsv_read_index")
        return [out[int(off[i]):int(off[i + 1])].copy() for i in range(len(read_len))], warn[: len(read_len)]

    def sketch_reads_filtered(self, store_dev, word_off, read_len, set_start, filters, w=51, k=51, hpc=1, variant=0, out_cap=None):
        """fsv_sketch_reads_filtered: the sketch through the sets' high-count k-mer filters.  filters: one sequence of uint64 hashes per
        read set (any order, duplicates allowed), or None for no lists at all -> per read its minimizers, as sketch_reads"""
        word_off = np.ascontiguousarray(word_off, dtype=np.uint64)
        read_len = np.ascontiguousarray(read_len, dtype=np.int32)
        set_start = np.ascontiguousarray(set_start, dtype=np.uint32)
        n_sets = len(set_start) - 1
        rs = ReadSets(C.c_void_p(store_dev), _ptr(word_off).value, _ptr(read_len).value, _ptr(set_start).value, len(read_len), n_sets, None)
        flt = off = None
        if filters is not None:
            assert len(filters) == n_sets
            lists = [np.ascontiguousarray(f, dtype=np.uint64) for f in filters]
            off = np.zeros(n_sets + 1, dtype=np.uint64)
            off[1:] = np.cumsum([len(f) for f in lists])
            flt = np.concatenate(lists + [np.zeros(1, dtype=np.uint64)])      # (never an empty buffer)
        cap = int(read_len.sum()) + 64 * len(read_len) + 64 if out_cap is None else int(out_cap)
        out = np.zeros(max(cap, 1), dtype=MZ_DTYPE)
        o = np.zeros(len(read_len) + 1, dtype=np.uint64)
        self.check(self._lib.fsv_sketch_reads_filtered(self._h, C.byref(rs), w, k, hpc, variant, _ptr(out), cap, _ptr(o), None if flt is None else _ptr(flt),
                                                       None if off is None else _ptr(off)), "fsv_sketch_reads_filtered")
        return [out[int(o[i]):int(o[i + 1])].copy() for i in range(len(read_len))]

    def asm_overlaps(self, store_dev, word_off, read_len, set_start, params=None, pass_=0, rechain=()):
        """fsv_asm_overlaps (test hook): the overlap stage of one pass -> (ovl[OVL_DTYPE] per ordered pair slot, pair_base[n_sets + 1],
        tasks[WTASK_DTYPE], overflow flag, warn[n_reads]); see include/focalsv_hip.h for the slot formula"""
        word_off = np.ascontiguousarray(word_off, dtype=np.uint64)
        read_len = np.ascontiguousarray(read_len, dtype=np.int32)
        set_start = np.ascontiguousarray(set_start, dtype=np.uint32)
        rs = ReadSets(C.c_void_p(store_dev), _ptr(word_off).value, _ptr(read_len).value, _ptr(set_start).value, len(read_len), len(set_start) - 1, None)
        n_pairs = task_cap = 0
        for s in range(len(set_start) - 1):
            ns = int(set_start[s + 1]) - int(set_start[s])
            n_pairs += ns * (ns - 1)
            task_cap += int(((read_len[int(set_start[s]):int(set_start[s + 1])].astype(np.int64) + FSV_WINDOW - 1) // FSV_WINDOW).sum()) * max(0, ns - 1)
        ovl = np.zeros(max(1, n_pairs), dtype=OVL_DTYPE)
        pair_base = np.zeros(len(set_start), dtype=np.uint32)
        tasks = np.zeros(max(1, task_cap), dtype=WTASK_DTYPE)
        warn = np.zeros(max(1, len(read_len)), dtype=np.uint32)
        lst = np.ascontiguousarray(rechain, dtype=np.uint32)
        n_tasks, overflow = C.c_uint32(0), C.c_uint32(0)
        p = params if params is not None else self.default_asm_params()
        self.check(self._lib.fsv_asm_overlaps(self._h, C.byref(rs), C.byref(p), int(pass_), _ptr(lst) if len(lst) else None, len(lst), _ptr(ovl), n_pairs,
                                              _ptr(pair_base), _ptr(tasks), task_cap, C.byref(n_tasks), C.byref(overflow), _ptr(warn)), "fsv_asm_overlaps")
        return ovl[:n_pairs], pair_base, tasks[: n_tasks.value], int(overflow.value), warn[: len(read_len)]

    def kmer_table(self, store_dev, word_off, read_len, set_start, w=1, k=51, hpc=1, want_hist=True, want_filter=True):
        """fsv_kmer_table: the k-mer count table stage alone, per read set -> (sets[KMER_SET_DTYPE], hist uint64[n_sets, 4096] or None,
        filter: list of ascending uint64 arrays, one per set, or None)"""
        word_off = np.ascontiguousarray(word_off, dtype=np.uint64)
        read_len = np.ascontiguousarray(read_len, dtype=np.int32)
        set_start = np.ascontiguousarray(set_start, dtype=np.uint32)
        n_sets = len(set_start) - 1
        rs = ReadSets(C.c_void_p(store_dev), _ptr(word_off).value, _ptr(read_len).value, _ptr(set_start).value, len(read_len), n_sets, None)
        out = np.zeros(max(1, n_sets), dtype=KMER_SET_DTYPE)
        hist = np.zeros((max(1, n_sets), KMER_BINS), dtype=np.uint64) if want_hist else None
        cap = int(read_len.astype(np.int64).sum()) + 1 if want_filter else 0       # at most one key per base
        flt = np.zeros(cap, dtype=np.uint64) if want_filter else None
        off = np.zeros(n_sets + 1, dtype=np.uint64) if want_filter else None
        self.check(self._lib.fsv_kmer_table(self._h, C.byref(rs), int(w), int(k), int(hpc), _ptr(out), None if hist is None else _ptr(hist),
                                            None if flt is None else _ptr(flt), cap, None if off is None else _ptr(off)), "fsv_kmer_table")
        lists = None if flt is None else [flt[int(off[s]):int(off[s + 1])].copy() for s in range(n_sets)]
        return out[:n_sets], (None if hist is None else hist[:n_sets]), lists

    def last_kmer_table(self, n_sets):
        """fsv_asm_last_kmer_table: the verdicts of the last assemble_batch with kmer_table = 1, in set order
        -> (sets[KMER_SET_DTYPE], the stage's summed kernel time in ms)"""
        out = np.zeros(max(1, n_sets), dtype=KMER_SET_DTYPE)
        ms = C.c_double(0.0)
        self.check(self._lib.fsv_asm_last_kmer_table(self._h, _ptr(out), int(n_sets), C.byref(ms)), "fsv_asm_last_kmer_table")
        return out[:n_sets], ms.value

    def kmer_index(self, store_dev, word_off, read_len, set_start, w=51, k=51, hpc=1, want_hist=True):
        """fsv_kmer_index: hifiasm's first ha_pt_gen per read set -- the count table at w = 1, its filter, the filtered sketch at w, counted
        -> (table[KMER_SET_DTYPE], index[KMER_INDEX_DTYPE], index hist uint64[n_sets, 4096] or None)"""
        word_off = np.ascontiguousarray(word_off, dtype=np.uint64)
        read_len = np.ascontiguousarray(read_len, dtype=np.int32)
        set_start = np.ascontiguousarray(set_start, dtype=np.uint32)
        n_sets = len(set_start) - 1
        rs = ReadSets(C.c_void_p(store_dev), _ptr(word_off).value, _ptr(read_len).value, _ptr(set_start).value, len(read_len), n_sets, None)
        tab = np.zeros(max(1, n_sets), dtype=KMER_SET_DTYPE)
        idx = np.zeros(max(1, n_sets), dtype=KMER_INDEX_DTYPE)
        hist = np.zeros((max(1, n_sets), KMER_BINS), dtype=np.uint64) if want_hist else None
        self.check(self._lib.fsv_kmer_index(self._h, C.byref(rs), int(w), int(k), int(hpc), _ptr(tab), _ptr(idx), None if hist is None else _ptr(hist)),
                   "fsv_kmer_index")
        return tab[:n_sets], idx[:n_sets], (None if hist is None else hist[:n_sets])

    def last_kmer_index(self, n_sets):
        """fsv_asm_last_kmer_index: the index figures of round 0 of the last assemble_batch with kmer_filter = 1, in set order
        -> (index[KMER_INDEX_DTYPE], the summed kernel time of the filter-set build and the index in ms)"""
        out = np.zeros(max(1, n_sets), dtype=KMER_INDEX_DTYPE)
        ms = C.c_double(0.0)
        self.check(self._lib.fsv_asm_last_kmer_index(self._h, _ptr(out), int(n_sets), C.byref(ms)), "fsv_asm_last_kmer_index")
        return out[:n_sets], ms.value

    def last_charge(self):
        """fsv_asm_last_charge: counters of the last assemble_batch with partial_charge = 1 (all rounds and chunks) -> dict;
        FsvError(EINVAL) when that call ran with partial_charge = 0"""
        st = ChargeStats()
        self.check(self._lib.fsv_asm_last_charge(self._h, C.byref(st)), "fsv_asm_last_charge")
        return {n: getattr(st, n) for n, _ in ChargeStats._fields_}

    def asm_stats(self):
        st = AsmStats()
        self.check(self._lib.fsv_asm_last_stats(self._h, C.byref(st)), "fsv_asm_last_stats")
        out = {n: getattr(st, n) for n, _ in AsmStats._fields_ if n not in ("kernels", "pad", "n_kernels")}
        out["kernels"] = {st.kernels[i].name.decode(): {"ms": st.kernels[i].ms, "launches": st.kernels[i].launches,
                                                        "algo_bytes": st.kernels[i].algo_bytes} for i in range(st.n_kernels)}
        nr, np_ = C.c_uint64(0), C.c_uint64(0)      # full_lists = 1: what the two long-read kernels took (0, 0 otherwise)
        self.check(self._lib.fsv_asm_last_long_lists(self._h, C.byref(nr), C.byref(np_)), "fsv_asm_last_long_lists")
        out["n_long_list_reads"], out["n_spilled_pairs"] = int(nr.value), int(np_.value)
        out.update(self.deep_windows())
        return out

    def deep_windows(self):
        """fsv_asm_last_deep_windows: what the last assemble_batch with deep_sets = 1 handed to k_consensus_deep / k_bnd_consensus_deep (all
        rounds and chunks) -> {"n_deep_windows", "n_deep_junctions", "max_events"}; all 0 after a call with deep_sets = 0"""
        nw, nj, me = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
        self.check(self._lib.fsv_asm_last_deep_windows(self._h, C.byref(nw), C.byref(nj), C.byref(me)), "fsv_asm_last_deep_windows")
        return {"n_deep_windows": int(nw.value), "n_deep_junctions": int(nj.value), "max_events": int(me.value)}

    def fetch_reads(self, n_reads, total_cap):
        seq = np.empty(total_cap, dtype=np.uint8)
        off = np.zeros(n_reads + 1, dtype=np.uint64)
        self.check(self._lib.fsv_asm_fetch_reads(self._h, _ptr(seq), total_cap, _ptr(off), n_reads), "fsv_asm_fetch_reads")
        return [seq[int(off[i]):int(off[i + 1])].tobytes() for i in range(n_reads)]

    # aligner boundary ---------------------------------------------------------------
    def default_aln_params(self):
        p = AlnParams()
        self._lib.fsv_aln_default_params(C.byref(p))
        return p

    def align_batch(self, contigs, contig_ref, refs, params=None):
        """fsv_align_batch.  contigs / refs: lists of bytes; contig_ref[i] = index of the window contig i belongs to.
        -> (records ndarray[ALN_REC_DTYPE], cigar ndarray[uint32], contig_status ndarray[int32])"""
        from_dev = contigs is None   # contigs of the last assemble_batch, still on the device
        n = len(contig_ref) if from_dev else len(contigs)
        coff = np.zeros(n + 1, dtype=np.uint64)
        if isinstance(refs, tuple):   # already joined by join_refs()
            rseq, roff = refs
        else:
            rseq, roff = join_refs(refs)
        n_refs = len(roff) - 1
        if from_dev:
            cseq = None
            total = int(self._last_contig_bytes)
        else:
            np.cumsum([len(c) for c in contigs], out=coff[1:])
            cseq = np.frombuffer(b"".join(contigs) + b"\0", dtype=np.uint8)
            total = int(coff[-1])
        cref = np.ascontiguousarray(contig_ref, dtype=np.uint32)
        rec = np.zeros(max(1, 5 * n), dtype=ALN_REC_DTYPE)   # FSV_ALN_MAX_REC records per contig
        cap = total // 8 + 4096 * max(1, n)
        cigar = np.empty(cap, dtype=np.uint32)
        status = np.zeros(max(1, n), dtype=np.int32)
        out = Alns(_ptr(rec).value, len(rec), 0, _ptr(cigar).value, cap, 0, _ptr(status).value)
        p = params if params is not None else self.default_aln_params()
        self.check(self._lib.fsv_align_batch(self._h, None if from_dev else _ptr(cseq), _ptr(coff), n, _ptr(cref), _ptr(rseq), _ptr(roff), n_refs, C.byref(p),
                                             C.byref(out)), "fsv_align_batch")
        return rec[: out.n_rec].copy(), cigar[: out.n_cigar].copy(), status[:n].copy()

    def aln_tags(self, rec, cigar, contigs=None, contig_ref=None, refs=None, n_contigs=None, n_refs=None):
        """fsv_aln_tags: NM and the cs difference string of alignment records (any CIGAR of M / I / D / S / H ops).
        contigs / contig_ref / refs as align_batch takes them, or contigs = refs = None with n_contigs / n_refs: the sequences the last
        align_batch left on the device -> (nm int32[n_rec], cs: list of bytes, rec_status int32[n_rec], kernel ms)"""
        rec = np.ascontiguousarray(rec, dtype=ALN_REC_DTYPE)
        cigar = np.ascontiguousarray(cigar, dtype=np.uint32)
        n = len(rec)
        cg = cigar if len(cigar) else np.zeros(1, np.uint32)
        alns = Alns(_ptr(rec).value if n else None, n, n, _ptr(cg).value, len(cigar), len(cigar), None)
        if contigs is None and refs is None:
            args = (None, None, int(n_contigs), None, None, None, int(n_refs))
            keep = ()
        else:
            rseq, roff = refs if isinstance(refs, tuple) else join_refs(refs)
            coff = np.zeros(len(contigs) + 1, dtype=np.uint64)
            np.cumsum([len(c) for c in contigs], out=coff[1:])
            cseq = np.frombuffer(b"".join(contigs) + b"\0", dtype=np.uint8)
            cref = np.ascontiguousarray(contig_ref, dtype=np.uint32)
            keep = (rseq, roff, coff, cseq, cref)
            args = (_ptr(cseq), _ptr(coff), len(contigs), _ptr(cref), _ptr(rseq), _ptr(roff), len(roff) - 1)
        nm = np.zeros(max(1, n), dtype=np.int32)
        off = np.zeros(n + 1, dtype=np.uint64)
        status = np.zeros(max(1, n), dtype=np.int32)
        out = AlnTags(_ptr(nm).value, _ptr(off).value, None, 0, 0, _ptr(status).value, 0.0)
        self.check(self._lib.fsv_aln_tags(self._h, *args, C.byref(alns), C.byref(out)), "fsv_aln_tags")   # the sizing call
        cs = np.zeros(max(1, int(out.cs_bytes)), dtype=np.uint8)
        out.cs, out.cs_cap = _ptr(cs).value, int(out.cs_bytes)
        ms = out.ms
        if out.cs_bytes:
            self.check(self._lib.fsv_aln_tags(self._h, *args, C.byref(alns), C.byref(out)), "fsv_aln_tags")
            ms = out.ms
        del keep
        return nm[:n].copy(), [cs[int(off[i]):int(off[i + 1])].tobytes() for i in range(n)], status[:n].copy(), ms

    # chromosome-level mapping quality (opt-in) ------------------------------------
    def ref_index(self, seq, k=19, w=19, max_occ=50):
        """fsv_ref_index_build: the chromosome's minimizer index on this context (it replaces an earlier one) -> its statistics as a dict"""
        b = seq.encode() if isinstance(seq, str) else seq
        a = np.frombuffer(b, dtype=np.uint8) if not isinstance(b, np.ndarray) else np.ascontiguousarray(b, dtype=np.uint8)
        self.check(self._lib.fsv_ref_index_build(self._h, _ptr(a) if len(a) else None, len(a), int(k), int(w), int(max_occ)), "fsv_ref_index_build")
        return self.ref_index_stats()

    def ref_index_stats(self):
        st = RefStats()
        self.check(self._lib.fsv_ref_index_stats(self._h, C.byref(st)), "fsv_ref_index_stats")
        return {n: getattr(st, n) for n, _ in RefStats._fields_}

    def ref_index_drop(self):
        self.check(self._lib.fsv_ref_index_drop(self._h), "fsv_ref_index_drop")

    def ref_index_lookup(self, hashes):
        """fsv_ref_index_lookup -> (count uint32[n], off uint64[n + 1], occ uint32[]: pos | rev << 31, ascending position per hash; a hash
        whose count is above the index's max_occ has its count and no occurrences)"""
        h = np.ascontiguousarray(hashes, dtype=np.uint64)
        n = len(h)
        cnt = np.zeros(max(1, n), dtype=np.uint32)
        off = np.zeros(n + 1, dtype=np.uint64)
        cap = 64 * n + 1      # max_occ <= 64
        occ = np.zeros(cap, dtype=np.uint32)
        self.check(self._lib.fsv_ref_index_lookup(self._h, _ptr(h) if n else None, n, _ptr(cnt), _ptr(off), _ptr(occ), cap), "fsv_ref_index_lookup")
        return cnt[:n].copy(), off, occ[: int(off[n])].copy()

    def contig_mapq(self, rec, cigar, ref_origin, contigs=None, contig_ref=None, n_contigs=None, params=None):
        """fsv_contig_mapq on the records of align_batch.  ref_origin[r]: chromosome position of window r's first base.  contigs / contig_ref
        as align_batch takes them, or contigs = None with n_contigs: the contigs the last align_batch left on the device.
        -> (rec with mapq set, dict of int32 arrays f1 f2 m cutoff thin flags rec_status, and ms)"""
        rec = np.ascontiguousarray(rec, dtype=ALN_REC_DTYPE).copy()
        cigar = np.ascontiguousarray(cigar, dtype=np.uint32)
        n = len(rec)
        cg = cigar if len(cigar) else np.zeros(1, np.uint32)
        alns = Alns(_ptr(rec).value if n else None, n, n, _ptr(cg).value, len(cigar), len(cigar), None)
        origin = np.ascontiguousarray(ref_origin, dtype=np.int64)
        if contigs is None:
            args = (None, None, int(n_contigs), None)
            keep = ()
        else:
            coff = np.zeros(len(contigs) + 1, dtype=np.uint64)
            np.cumsum([len(c) for c in contigs], out=coff[1:])
            cseq = np.frombuffer(b"".join(contigs) + b"\0", dtype=np.uint8)
            cref = np.ascontiguousarray(contig_ref, dtype=np.uint32)
            keep = (coff, cseq, cref)
            args = (_ptr(cseq), _ptr(coff), len(contigs), _ptr(cref))
        names = ("f1", "f2", "m", "cutoff", "thin", "flags", "rec_status")
        arr = {k: np.zeros(max(1, n), dtype=np.int32) for k in names}
        out = ContigMapq(*[_ptr(arr[k]).value for k in names], 0.0)
        p = params if params is not None else self.default_aln_params()
        self.check(self._lib.fsv_contig_mapq(self._h, *args, _ptr(origin), len(origin), C.byref(alns), C.byref(p), C.byref(out)), "fsv_contig_mapq")
        del keep
        res = {k: arr[k][:n].copy() for k in names}
        res["ms"] = out.ms
        return rec, res

    def aln_stats(self):
        st = AlnStats()
        self.check(self._lib.fsv_aln_last_stats(self._h, C.byref(st)), "fsv_aln_last_stats")
        return {n: getattr(st, n) for n, _ in AlnStats._fields_}

    def nw(self, target: bytes, query: bytes, params=None):
        p = params if params is not None else self.default_aln_params()
        cap = len(target) + len(query) + 4
        cg = np.zeros(cap, dtype=np.uint32)
        sc, n = C.c_int32(0), C.c_uint32(0)
        self.check(self._lib.fsv_nw(self._h, target, len(target), query, len(query), C.byref(p), C.byref(sc), _ptr(cg), cap, C.byref(n)), "fsv_nw")
        return sc.value, cg[: n.value].copy()
