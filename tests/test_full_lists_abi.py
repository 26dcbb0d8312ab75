"""fsv_asm_params.full_lists at the boundary: where the field sits, its defaults, the CLI flag, the values it takes."""
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


def test_field_sits_in_front_of_kmer_filter_in_header_and_binding():
    fields = header_fields()
    assert fields[fields.index("full_lists") + 1] == "kmer_filter"
    assert fields[-3:] == ["kmer_filter", "kmer_table", "partial_charge"]
    assert [n for n, _ in _lib.AsmParams._fields_] == fields
    assert C.sizeof(_lib.AsmParams) == 4 * len(fields)


def test_off_in_every_profile():
    lib = _lib.load()
    for name in ("fsv_asm_default_params", "fsv_asm_ont_params", "fsv_asm_clr_params"):
        p = _lib.AsmParams()
        C.memset(C.byref(p), 0x55, C.sizeof(p))
        getattr(lib, name)(C.byref(p))
        assert p.full_lists == 0, name


def test_entry_point_and_cli_flag():
    hdr = open(os.path.join(ROOT, "include", "focalsv_hip.h")).read()
    assert "fsv_read_index" in hdr and hasattr(_lib.load(), "fsv_read_index")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "3_assembly.py"), "--help"], capture_output=True, text=True, check=True).stdout
    assert "--long-reads" in out


@pytest.mark.gpu
def test_other_values_are_refused():
    from focalsv_amd.readsets import pack_sets
    b = pack_sets([[b"ACGTTGCAAGGCTTAACCGGATAT" * 20, b"TTGCAAGGCTTAACCGGATATACG" * 20]])
    with _lib.Context(0) as ctx:
        d = ctx.upload(b.words)
        try:
            for bad in (2, -1):
                p = ctx.default_asm_params()
                p.full_lists = bad
                with pytest.raises(_lib.FsvError) as e:
                    ctx.assemble_batch(d, b.word_off, b.read_len, b.set_start, p)
                assert e.value.code == _lib.EINVAL
                with pytest.raises(_lib.FsvError) as e:
                    ctx.asm_overlaps(d, b.word_off, b.read_len, b.set_start, p, 0)
                assert e.value.code == _lib.EINVAL
            p = ctx.default_asm_params()
            p.full_lists = 1
            ctx.asm_overlaps(d, b.word_off, b.read_len, b.set_start, p, 0)
        finally:
            ctx.dev_free(d)
