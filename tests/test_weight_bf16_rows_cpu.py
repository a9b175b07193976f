"""bf16 weight storage for 2-64 rows (DESIGN.md "bf16 weight storage for 2-64 rows"), the parts that
need no GPU: the new ABI symbols and the argument checks that fail before a device is touched."""

import ctypes
import re
import subprocess

import pytest

import l3hip

NEW_SYMBOLS = ["l3_set_weight_bf16_rows", "l3_weight_bf16_rows_info", "l3_op_linear_bf16_rows_host"]


def test_new_symbols_declared_exported_and_bound():
    lib = l3hip.lib()
    declared = l3hip.header_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", l3hip.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert s in l3hip._SIGNATURES, s
        assert s in exported and hasattr(lib, s), s
    with open(l3hip.HEADER) as f:
        text = f.read()
    for s in NEW_SYMBOLS:  # each comment cites the reference lines it extends
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int\s+" + s + r"\s*\(", text, re.S)
        assert m and "llama3.py:" in m.group(1), s
    for name in ("set_weight_bf16_rows", "weight_bf16_rows_info", "op_linear_bf16_rows"):
        assert callable(getattr(l3hip.Context, name)), name


def test_null_context_fails_with_a_message():
    lib = l3hip.lib()
    assert lib.l3_set_weight_bf16_rows(None, 8, 0) != 0
    assert b"null context" in lib.l3_last_error()
    assert lib.l3_set_weight_bf16_rows(None, -1, -1) != 0
    assert b"null context" in lib.l3_last_error()
    r, b, n = ctypes.c_int32(7), ctypes.c_int64(8), ctypes.c_int64(9)
    assert lib.l3_weight_bf16_rows_info(None, ctypes.byref(r), ctypes.byref(b), ctypes.byref(n)) != 0
    assert b"null context" in lib.l3_last_error() and (r.value, b.value, n.value) == (7, 8, 9)
    assert lib.l3_op_linear_bf16_rows_host(None, None, 2, 32, 4, None, None, ctypes.c_float(0), None) != 0
    assert b"null context" in lib.l3_last_error()


@pytest.mark.parametrize("max_rows", [1, 65, -2])
def test_max_rows_out_of_range_is_refused_before_a_device_is_touched(max_rows):
    """The values are checked before the context: the message names the range, not the context."""
    lib = l3hip.lib()
    assert lib.l3_set_weight_bf16_rows(None, max_rows, 0) != 0
    msg = lib.l3_last_error()
    assert b"max_rows" in msg and str(max_rows).encode() in msg and b"null context" not in msg


def test_min_bytes_out_of_range_is_refused_before_a_device_is_touched():
    lib = l3hip.lib()
    assert lib.l3_set_weight_bf16_rows(None, 8, -2) != 0
    msg = lib.l3_last_error()
    assert b"min_bytes" in msg and b"-2" in msg and b"null context" not in msg
