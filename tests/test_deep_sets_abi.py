"""fsv_asm_params.deep_sets at the boundary: where the field sits, its defaults, the CLI flag, the export, the values it takes."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from focalsv_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_fields():
    hdr = open(os.path.join(ROOT, "include", "focalsv_hip.h")).read()
    body = hdr[hdr.index("typedef struct fsv_asm_params {"): hdr.index("} fsv_asm_params;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [n.strip() for decl in re.findall(r"int32_t\s+([^;]+);", body) for n in decl.split(",")]


def test_field_sits_between_junction_cigars_and_full_lists_in_header_and_binding():
    fields = header_fields()
    i = fields.index("deep_sets")
    assert fields[i - 1] == "junction_cigars" and fields[i + 1] == "full_lists"
    assert fields[-4:] == ["full_lists", "kmer_filter", "kmer_table", "partial_charge"]
    assert [n for n, _ in _lib.AsmParams._fields_] == fields
    assert C.sizeof(_lib.AsmParams) == 4 * len(fields)


def test_off_in_every_profile():
    lib = _lib.load()
    for name in ("fsv_asm_default_params", "fsv_asm_ont_params", "fsv_asm_clr_params"):
        p = _lib.AsmParams()
        C.memset(C.byref(p), 0x55, C.sizeof(p))
        getattr(lib, name)(C.byref(p))
        assert p.deep_sets == 0, name


def test_export_and_cli_flag():
    hdr = open(os.path.join(ROOT, "include", "focalsv_hip.h")).read()
    assert "fsv_asm_last_deep_windows" in hdr and hasattr(_lib.load(), "fsv_asm_last_deep_windows")
    assert hasattr(_lib.Context, "deep_windows")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "3_assembly.py"), "--help"], capture_output=True, text=True, check=True).stdout
    assert "--deep-sets" in out


def test_the_kernel_table_holds_the_two_new_rows():
    hdr = open(os.path.join(ROOT, "include", "focalsv_hip.h")).read()
    n = int(re.search(r"#define FSV_MAX_KERNEL_STATS (\d+)", hdr).group(1))
    assert n >= 18 and _lib.AsmStats.kernels.size == n * C.sizeof(_lib.KernelStat)
    assert _lib.AsmStats.kernels.offset + _lib.AsmStats.kernels.size == C.sizeof(_lib.AsmStats)


@pytest.mark.gpu
def test_other_values_are_refused():
    from focalsv_amd.readsets import pack_sets
    b = pack_sets([[b"ACGTTGCAAGGCTTAACCGGATAT" * 20, b"TTGCAAGGCTTAACCGGATATACG" * 20]])
    with _lib.Context(0) as ctx:
        d = ctx.upload(b.words)
        try:
            for bad in (2, -1):
                p = ctx.default_asm_params()
                p.deep_sets = bad
                with pytest.raises(_lib.FsvError) as e:
                    ctx.assemble_batch(d, b.word_off, b.read_len, b.set_start, p)
                assert e.value.code == _lib.EINVAL
                with pytest.raises(_lib.FsvError) as e:
                    ctx.asm_overlaps(d, b.word_off, b.read_len, b.set_start, p, 0)
                assert e.value.code == _lib.EINVAL
            p = ctx.default_asm_params()
            p.deep_sets = 1
            ctx.asm_overlaps(d, b.word_off, b.read_len, b.set_start, p, 0)
            ctx.assemble_batch(d, b.word_off, b.read_len, b.set_start, p)
            assert ctx.deep_windows() == {"n_deep_windows": 0, "n_deep_junctions": 0, "max_events": 0}
        finally:
            ctx.dev_free(d)
