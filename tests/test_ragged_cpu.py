"""Ragged batches (DESIGN.md "Ragged batches"), the part that needs no GPU: the header declares
the two entry points, l3hip binds them with the header's argument types, and the built library
exports them as C symbols (the checks of tests/test_abi.py, for these two)."""

import ctypes
import re
import subprocess

import l3hip

ENTRY_POINTS = ("l3_ragged_forward_host", "l3_ragged_generate_host")

# C parameter type -> the ctypes type the binding must declare
CTYPE = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}


def _declaration(name):
    with open(l3hip.HEADER) as f:
        text = f.read()
    m = re.search(r"^int\s+" + name + r"\s*\(([^)]*)\)\s*;", text, re.M | re.S)
    assert m, f"{name} is not declared in include/llama3hip.h"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_header_declares_the_entry_points():
    declared = l3hip.header_symbols()
    for name in ENTRY_POINTS:
        assert name in declared
    fwd = _declaration("l3_ragged_forward_host")
    assert fwd == ["l3_ctx* ctx", "const int64_t* ids_host", "const int32_t* lens", "int32_t B", "int32_t Lmax",
                   "float* logits_host"]
    gen = _declaration("l3_ragged_generate_host")
    assert gen == ["l3_ctx* ctx", "const int64_t* ids_host", "const int32_t* lens", "int32_t B", "int32_t Lmax",
                   "int32_t max_new_tokens", "const int64_t* stop_ids", "int32_t n_stop", "int64_t* out_ids_host",
                   "int32_t* out_lens"]


def test_binding_argument_types_match_the_header():
    for name in ENTRY_POINTS:
        res, args = l3hip._SIGNATURES[name]
        assert res is ctypes.c_int
        params = _declaration(name)
        assert len(args) == len(params), name
        for a, p in zip(args, params):
            ctype = p.rsplit(" ", 1)[0]
            want = ctypes.c_void_p if ctype.endswith("*") else CTYPE[ctype]
            assert a is want, (name, p, a)
        fn = getattr(l3hip.lib(), name)
        assert list(fn.argtypes) == args and fn.restype is ctypes.c_int
    assert callable(l3hip.Context.ragged_forward) and callable(l3hip.Context.ragged_generate)


def test_library_exports_the_entry_points():
    lib = l3hip.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", l3hip.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in ENTRY_POINTS:
        assert hasattr(lib, name)
        assert name in exported, name  # unmangled: extern "C"


def test_null_context_is_reported():
    lib = l3hip.lib()
    assert lib.l3_ragged_forward_host(None, None, None, 1, 1, None) != 0
    assert b"null context" in lib.l3_last_error()
    assert lib.l3_ragged_generate_host(None, None, None, 1, 1, 4, None, 0, None, None) != 0
    assert b"null context" in lib.l3_last_error()
