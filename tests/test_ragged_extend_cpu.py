"""Ragged continuation (DESIGN.md "Ragged continuation"), the part that needs no GPU: the fp64
reference of the extend agrees with itself across a chunk cut, the header declares the four entry
points with their argument lists, l3hip binds them with the header's argument types, the built
library exports them, and a null context is reported (the style of tests/test_ragged_split_cpu.py)."""

import ctypes
import re
import subprocess

import numpy as np
import pytest

import extend_attn_ref as ref
import l3hip

ENTRY_POINTS = ("l3_ragged_extend_host", "l3_ragged_generate_from_host", "l3_cache_copy_rows",
                "l3_op_attn_extend_ragged_host")

# C parameter type -> the ctypes type the binding must declare
CTYPE = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}


# ---- the reference itself --------------------------------------------------------------------

@pytest.mark.parametrize("hd,n_rep", [(16, 2), (96, 3)])
@pytest.mark.parametrize("cut", [1, 15, 16, 39])
def test_two_chunks_equal_one_chunk(hd, n_rep, cut):
    inp = ref.make_inputs(hd, n_rep)
    want, ck, cv = ref.reference(inp)
    got = ref.two_chunks(inp, cut)
    assert np.isfinite(want).all() and np.isfinite(got).all()  # no poisoned slot was read
    for b, (st, n) in enumerate(ref.PAIRS):
        err = float(np.abs(got[b] - want[b]).max())
        assert err <= 1e-12, (st, n, err)
        assert not want[b, n:].any() and not got[b, n:].any()  # the pads
        assert np.isfinite(ck[b, :, :st + n]).all() and np.isnan(ck[b, :, st + n:]).all()
        assert np.isfinite(cv[b, :, :st + n]).all() and np.isnan(cv[b, :, st + n:]).all()


def test_reference_single_token_and_rope():
    """(start 0, len 1): one key, so the output is the new v whatever q and k are, and the RoPE of
    position 0 is the identity; a later token's key is rotated by its own position."""
    inp = ref.make_inputs(16, 2, pairs=((0, 1), (3, 2)), smax=8, lq=2, seed=3)
    out, ck, cv = ref.reference(inp)
    H, kvh, hd = 4, 2, 16
    row = inp["qkv"][0, 0].astype(np.float64)
    v = row[(H + kvh) * hd:].reshape(kvh, hd)
    assert np.allclose(out[0, 0].reshape(H, hd), np.repeat(v, 2, axis=0), rtol=0, atol=1e-15)
    assert np.array_equal(ck[0, :, 0], row[H * hd:(H + kvh) * hd].reshape(kvh, hd))
    k = inp["qkv"][1, 1, H * hd:H * hd + 2].astype(np.float64)  # token 1 of row 1: position 4
    c, s = float(inp["rope_cos"][4, 0]), float(inp["rope_sin"][4, 0])
    assert np.allclose(ck[1, 0, 4, :2], [k[0] * c - k[1] * s, k[0] * s + k[1] * c], rtol=0, atol=1e-15)
    assert abs(c - np.cos(4.0)) < 1e-7 and abs(s - np.sin(4.0)) < 1e-7


# ---- the ABI ---------------------------------------------------------------------------------

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
    assert _declaration("l3_ragged_extend_host") == [
        "l3_ctx* ctx", "const int64_t* ids_host", "const int32_t* lens", "const int32_t* starts", "int32_t B",
        "int32_t Lmax", "float* logits_host"]
    assert _declaration("l3_ragged_generate_from_host") == [
        "l3_ctx* ctx", "const int64_t* ids_host", "const int32_t* lens", "const int32_t* starts", "int32_t B",
        "int32_t Lmax", "int32_t max_new_tokens", "const int64_t* stop_ids", "int32_t n_stop",
        "int64_t* out_ids_host", "int32_t* out_lens"]
    assert _declaration("l3_cache_copy_rows") == [
        "l3_ctx* ctx", "int32_t src_row", "const int32_t* dst_rows", "int32_t n_dst", "int32_t n_slots"]
    assert _declaration("l3_op_attn_extend_ragged_host") == [
        "l3_ctx* ctx", "const float* qkv", "float* cache_k", "float* cache_v", "const float* rope_cos",
        "const float* rope_sin", "const int32_t* starts", "const int32_t* lens", "int32_t B", "int32_t Lq",
        "int32_t H", "int32_t KVH", "int32_t HD", "int32_t Smax", "float* out"]


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
    for method in ("ragged_extend", "ragged_generate", "cache_copy_rows", "op_attn_extend_ragged"):
        assert callable(getattr(l3hip.Context, method))


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
    assert lib.l3_ragged_extend_host(None, None, None, None, 1, 1, None) != 0
    assert b"null context" in lib.l3_last_error()
    assert lib.l3_ragged_generate_from_host(None, None, None, None, 1, 1, 4, None, 0, None, None) != 0
    assert b"null context" in lib.l3_last_error()
    assert lib.l3_cache_copy_rows(None, 0, None, 0, 0) != 0
    assert b"null context" in lib.l3_last_error()
    assert lib.l3_op_attn_extend_ragged_host(None, None, None, None, None, None, None, None, 1, 1, 2, 1, 16, 8,
                                             None) != 0
    assert b"null context" in lib.l3_last_error()
