"""The host half of the partial charge (fsv_asm_params.partial_charge, non_trim_error_rate's charge for an unmatched window), no device:
the parameter and its defaults, the CLI flag, and fsv_partial_charge against a numpy float32 restatement of oracle/asm.c:307-312 --

    if (al[0] && al[1]) {
        if (al[0] + al[1] <= n) return terr + er[0] + er[1] + (n - al[0] - al[1]);
        { const float rate = (float)n / (float)(al[0] + al[1]); return (long)((float)terr + (float)(unsigned)(er[0] + er[1]) * rate); }
    }
    if (!al[0] && !al[1]) return terr + n;
    return al[0] ? terr + er[0] + (n - al[0]) : terr + er[1] + (n - al[1]);

-- every float operation rounded to single precision on its own (gcc -O2 on x86-64 without FMA), which is what numpy's float32 scalars do."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np

from focalsv_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_param_exists_and_is_off_in_every_profile():
    assert AsmParamsFields()[-1] == "partial_charge", "appended after kmer_table"
    assert AsmParamsFields()[-2] == "kmer_table"
    lib = _lib.load()
    for name in ("fsv_asm_default_params", "fsv_asm_ont_params", "fsv_asm_clr_params"):
        p = _lib.AsmParams()
        C.memset(C.byref(p), 0x55, C.sizeof(p))
        getattr(lib, name)(C.byref(p))
        assert p.partial_charge == 0, name
        assert p.kmer_table == 0, name


def AsmParamsFields():
    return [n for n, _ in _lib.AsmParams._fields_]


def test_header_declares_the_field_last_and_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "focalsv_hip.h")).read()
    body = hdr[hdr.index("typedef struct fsv_asm_params {"): hdr.index("} fsv_asm_params;")]
    assert body.index("int32_t kmer_table;") < body.index("int32_t partial_charge;")
    assert body.rindex("int32_t") == body.index("int32_t partial_charge;"), "partial_charge is the struct's last field"
    for name in ("fsv_bpm_extensions", "fsv_partial_charge", "fsv_asm_last_charge", "fsv_wext", "fsv_charge_stats"):
        assert name in hdr
    lib = _lib.load()
    for name in ("fsv_bpm_extensions", "fsv_partial_charge", "fsv_asm_last_charge"):
        assert hasattr(lib, name)
    assert _lib.WEXT_DTYPE.itemsize == 16 and C.sizeof(_lib.ChargeStats) == 48


def test_cli_lists_the_flag():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "3_assembly.py"), "--help"], capture_output=True, text=True, check=True).stdout
    assert "--partial-charge" in out and "--kmer-table" in out


def test_assembly_refuses_the_flag_for_noisy_reads(tmp_path):
    import pytest
    from focalsv_amd import assembly
    with pytest.raises(ValueError):
        assembly.assembly(str(tmp_path), data_type=1, partial_charge=True)


def model(n, al0, er0, al1, er1, terr):
    """oracle/asm.c:307-312, operation by operation"""
    f = np.float32
    if al0 and al1:
        if al0 + al1 <= n:
            return terr + er0 + er1 + (n - al0 - al1)
        rate = f(f(n) / f(al0 + al1))
        return int(f(f(terr) + f(f(er0 + er1) * rate)))       # (long): truncation; every value here is >= 0
    if not al0 and not al1:
        return terr + n
    return terr + er0 + (n - al0) if al0 else terr + er1 + (n - al1)


def _als(n):
    """covered lengths in [0, n]: the ends, their neighbours, the middle"""
    return sorted({a for a in (0, 1, 2, n // 3, n // 2, n // 2 + 1, n - 2, n - 1, n) if 0 <= a <= n})


def _ers(al):
    return sorted({e for e in (0, 1, al // 7, al // 2, al) if 0 <= e <= al}) if al else [0]


def test_charge_equals_the_float32_model_on_the_grid():
    seen = {"sum <= n": 0, "sum > n": 0, "one side": 0, "neither": 0}
    for n in (1, 17, 200, 375):
        for al0, al1 in itertools.product(_als(n), _als(n)):
            for er0, er1 in itertools.product(_ers(al0), _ers(al1)):
                for terr in (0, 1, 999, 2 ** 24 - 1, 2 ** 24 + 1):
                    want = model(n, al0, er0, al1, er1, terr)
                    got = _lib.partial_charge(n, al0, er0, al1, er1, terr)
                    assert got == want, (n, al0, er0, al1, er1, terr, got, want)
                    if al0 and al1:
                        seen["sum <= n" if al0 + al1 <= n else "sum > n"] += 1
                    elif al0 or al1:
                        seen["one side"] += 1
                    else:
                        seen["neither"] += 1
    assert all(v > 0 for v in seen.values()), seen


def test_charge_float_branch_known_answers():
    # 2^24 + 1 is not a float: the running total itself is rounded (to even: 2^24) before the scaled errors (4 x 2 / 4 = 2) are added
    assert _lib.partial_charge(2, 2, 2, 2, 2, 2 ** 24 + 1) == model(2, 2, 2, 2, 2, 2 ** 24 + 1) == 2 ** 24 + 2
    # 10 x (375 / 376) stays below 10: truncated, not rounded
    assert _lib.partial_charge(375, 188, 5, 188, 5, 0) == model(375, 188, 5, 188, 5, 0) == 9
    assert _lib.partial_charge(17, 9, 3, 9, 4, 1) == model(17, 9, 3, 9, 4, 1) == 7
    # the integer branches
    assert _lib.partial_charge(375, 100, 4, 200, 6, 50) == 50 + 10 + 75
    assert _lib.partial_charge(375, 0, 0, 200, 6, 50) == 50 + 6 + 175
    assert _lib.partial_charge(375, 0, 0, 0, 0, 50) == 425
