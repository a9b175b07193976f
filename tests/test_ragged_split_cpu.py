"""Split-KV decode attention (DESIGN.md "Split-KV decode attention"), the part that needs no GPU:
the fp64 chunk-and-combine model equals the plain softmax reference, the header declares the three
entry points, l3hip binds them with the header's argument types, the built library exports them,
and a null context and out-of-range settings are reported (the style of tests/test_ragged_cpu.py)."""

import ctypes
import re
import subprocess

import numpy as np
import pytest

import l3hip
import split_attn_ref as ref

ENTRY_POINTS = ("l3_set_ragged_attn_split", "l3_ragged_attn_info", "l3_op_attn_decode_ragged_host")

# C parameter type -> the ctypes type the binding must declare
CTYPE = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}


# ---- the reference itself --------------------------------------------------------------------

@pytest.mark.parametrize("hd,n_rep", [(16, 2), (128, 4)])
def test_chunked_model_equals_the_plain_reference(hd, n_rep):
    inp = ref.make_inputs(hd, n_rep, 2, 256, ref.POSITIONS)
    want, new_k, new_v = ref.reference(inp)
    got = ref.chunked(inp, 64)
    assert np.isfinite(want).all()  # no poisoned slot was read
    for b, p in enumerate(ref.POSITIONS):
        err = float(np.abs(got[b] - want[b]).max())
        assert err <= 1e-12, (p, err)
    assert not want[-1].any() and not got[-1].any()  # the finished row
    assert np.isnan(new_k[-1]).all() and np.isfinite(new_k[:-1]).all() and np.isfinite(new_v[:-1]).all()
    # one chunk holding everything is the plain softmax again
    assert float(np.abs(ref.chunked(inp, 256) - want).max()) <= 1e-12


def test_reference_rope_and_single_key():
    """pos 0: one key, so the output is the new v whatever q and k are; and the RoPE of position
    0 is the identity."""
    inp = ref.make_inputs(16, 2, 2, 8, (0, 3), n_finished=0, seed=3)
    out, new_k, new_v = ref.reference(inp)
    H, kvh, hd = 4, 2, 16
    v = inp["qkv"][0, (H + kvh) * hd:].reshape(kvh, hd).astype(np.float64)
    assert np.allclose(out[0].reshape(H, hd), np.repeat(v, 2, axis=0), rtol=0, atol=1e-15)
    assert np.array_equal(new_k[0], inp["qkv"][0, H * hd:(H + kvh) * hd].reshape(kvh, hd).astype(np.float64))
    # position 3: pair (x0, x1) of the new k rotated by the angle 3 * 10000^0
    k = inp["qkv"][1, H * hd:H * hd + 2].astype(np.float64)
    c, s = float(inp["rope_cos"][3, 0]), float(inp["rope_sin"][3, 0])
    assert np.allclose(new_k[1, 0, :2], [k[0] * c - k[1] * s, k[0] * s + k[1] * c], rtol=0, atol=1e-15)
    assert abs(c - np.cos(3.0)) < 1e-7 and abs(s - np.sin(3.0)) < 1e-7


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
    assert _declaration("l3_set_ragged_attn_split") == ["l3_ctx* ctx", "int32_t mode", "int32_t chunk"]
    assert _declaration("l3_ragged_attn_info") == ["l3_ctx* ctx", "int32_t* mode", "int32_t* chunk_in_force",
                                                   "int64_t* split_launches", "int64_t* workspace_bytes"]
    op = _declaration("l3_op_attn_decode_ragged_host")
    assert op == ["l3_ctx* ctx", "const float* qkv", "float* cache_k", "float* cache_v", "const float* rope_cos",
                  "const float* rope_sin", "const int32_t* pos", "const int32_t* finished", "int32_t B", "int32_t H",
                  "int32_t KVH", "int32_t HD", "int32_t Smax", "int32_t s_cap", "int32_t split", "float* out"]


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
    for method in ("set_ragged_attn_split", "ragged_attn_info", "op_attn_decode_ragged"):
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
    assert lib.l3_set_ragged_attn_split(None, 0, 0) != 0
    assert b"null context" in lib.l3_last_error()
    assert lib.l3_set_ragged_attn_split(None, 1, 256) != 0
    assert b"null context" in lib.l3_last_error()
    assert lib.l3_ragged_attn_info(None, None, None, None, None) != 0
    assert b"null context" in lib.l3_last_error()
    assert lib.l3_op_attn_decode_ragged_host(None, None, None, None, None, None, None, None, 1, 2, 1, 16, 8, 8, 0,
                                             None) != 0
    assert b"null context" in lib.l3_last_error()


def test_bad_settings_are_refused():
    """the values are wrong for every context, so they are reported even without one"""
    lib = l3hip.lib()
    for chunk in (63, 8192, -64, 96, 4160):
        assert lib.l3_set_ragged_attn_split(None, 0, chunk) != 0
        err = lib.l3_last_error()
        assert b"chunk %d" % chunk in err and b"multiple of 64" in err, err
    for mode in (2, -1):
        assert lib.l3_set_ragged_attn_split(None, mode, 0) != 0
        err = lib.l3_last_error()
        assert b"mode %d" % mode in err, err
