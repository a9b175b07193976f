"""fp8 weight storage (DESIGN.md "fp8 weight storage"), the parts that need no GPU: the host
restatement of the format (utils.quant_fp8_rows / round_fp8_rows / fp8_e4m3_table) against torch's
float8_e4m3fn conversion bit for bit, the new ABI symbols, and the argument checks that fail before
a device is touched."""

import ctypes
import re
import subprocess

import numpy as np
import pytest
import torch

import l3hip
import llama3
import synth
import utils

NEW_SYMBOLS = ["l3_set_weight_fp8", "l3_weight_fp8_info", "l3_op_to_fp8_rows_host", "l3_op_linear_fp8_host",
               "l3_op_linear_fp8_rows_host"]


def torch_codes(v):
    """torch's e4m3fn codes (uint8) of fp32 values, round-to-nearest-even."""
    return torch.tensor(np.ascontiguousarray(v, dtype=np.float32)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def case_rows(K=64):
    """Rows around every case of the format, [N, K] fp32."""
    rng = np.random.default_rng(0)
    rows = [rng.standard_normal(K) * s for s in (1.0, 1e-3, 37.0, 1e-30, 1e20)]
    sub = rng.standard_normal(K) * 2.0 ** -8  # with an amax of 448: elements in the subnormal range
    sub[0] = 448.0
    rows.append(sub)
    ties = np.array([448.0] + [(m + 0.5) * 2.0 ** -9 for m in range(8)] + [(1 + (m + 0.5) / 8) * 2.0 ** e
                                                                         for m in range(8) for e in (-6, 0, 7)])
    rows.append(np.resize(np.concatenate([ties, -ties]), K))
    z = np.zeros(K)
    z[1], z[2], z[3] = -0.0, 448.0, -1e-45  # +-0 beside values; a value that rounds to -0
    rows.append(z)
    for e in (-40, 0, 9):  # amax exactly 448 * 2^e, and the next fp32 above it
        a = rng.standard_normal(K)
        a = a / np.abs(a).max() * 100.0 * 2.0 ** e
        a[5] = 448.0 * 2.0 ** e
        rows.append(a.copy())
        a[5] = np.nextafter(np.float32(448.0 * 2.0 ** e), np.float32(np.inf))
        rows.append(a.copy())
    rows.append(np.zeros(K))  # all-zero
    rows.append(-np.zeros(K))
    return np.array(rows, np.float32)


def test_table_is_torch_decode_of_all_codes():
    t = utils.fp8_e4m3_table()
    want = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float().numpy()
    assert t.dtype == np.float32 and t.shape == (256,)
    nan = np.isnan(want)
    assert list(np.flatnonzero(nan)) == [0x7F, 0xFF] and np.array_equal(np.isnan(t), nan)
    assert np.array_equal(t.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
    assert t[0x7E] == 448.0 and t[0x01] == 2.0 ** -9 and t[0x08] == 2.0 ** -6 and np.signbit(t[0x80])


def test_quant_codes_are_torch_bit_for_bit():
    rng = np.random.default_rng(1)
    W = np.concatenate([case_rows(), rng.standard_normal((200, 64)).astype(np.float32),
                        (rng.standard_normal((50, 64)) * np.exp(rng.uniform(-60, 60, (50, 1)))).astype(np.float32)])
    codes, scale = utils.quant_fp8_rows(W)
    assert codes.dtype == np.uint8 and codes.shape == W.shape and scale.dtype == np.float32 and scale.shape == (len(W),)
    want = torch_codes(W / scale[:, None])  # a power-of-two quotient: exact (or a subnormal, rounded to +-0 either way)
    assert np.array_equal(codes, want)
    assert not np.any((codes & 0x7F) == 0x7F)  # no NaN code
    # -0 is kept, and a tiny negative value rounds to it
    z = case_rows()[7]
    cz = utils.quant_fp8_rows(z[None])[0][0]
    assert cz[0] == 0x00 and cz[1] == 0x80 and cz[2] == 0x7E and cz[3] == 0x80


def test_scale_is_the_smallest_admissible_power_of_two():
    rng = np.random.default_rng(2)
    W = np.concatenate([case_rows(), (rng.standard_normal((300, 64)) * np.exp(rng.uniform(-70, 70, (300, 1)))).astype(np.float32)])
    _, scale = utils.quant_fp8_rows(W)
    amax = np.abs(W).max(axis=1).astype(np.float64)
    m, e = np.frexp(scale)
    assert np.all(m == 0.5) and np.all((e - 1 >= -126) & (e - 1 <= 127))  # powers of two in range
    s = scale.astype(np.float64)
    assert np.all(amax / s <= 448.0)
    nz = (amax > 0) & (e - 1 > -126)
    assert np.all(amax[nz] / (s[nz] / 2) > 448.0)  # half the scale would not do
    assert np.all(scale[amax == 0] == 1.0)
    # exactly 448 * 2^e takes 2^e; the next fp32 above takes 2^(e + 1)
    for e0 in (-40, 0, 9):
        at = np.full((1, 32), 448.0 * 2.0 ** e0, np.float32)
        assert utils.quant_fp8_rows(at)[1][0] == np.float32(2.0 ** e0)
        assert utils.quant_fp8_rows(np.nextafter(at, np.float32(np.inf)))[1][0] == np.float32(2.0 ** (e0 + 1))
    # the clamp: a row of fp32 subnormals keeps 2^-126
    assert utils.quant_fp8_rows(np.full((1, 32), 1e-44, np.float32))[1][0] == np.float32(2.0 ** -126)


def test_round_fp8_rows_is_the_model_and_idempotent():
    rng = np.random.default_rng(3)
    W = np.concatenate([case_rows(), rng.standard_normal((100, 64)).astype(np.float32)])
    codes, scale = utils.quant_fp8_rows(W)
    r = utils.round_fp8_rows(W)
    assert r.dtype == np.float32 and r.shape == W.shape
    want = (utils.fp8_e4m3_table().astype(np.float64)[codes] * scale.astype(np.float64)[:, None])
    assert np.array_equal(r.astype(np.float64), want)  # one exact fp32 value
    assert np.array_equal(np.signbit(r), np.signbit(W))
    # idempotent in value (a row whose largest element rounds down to 224 s takes the scale s / 2
    # the second time: other codes, the same numbers)
    c2, s2 = utils.quant_fp8_rows(r)
    assert np.all((s2 == scale) | (s2 == scale / 2))
    assert np.array_equal((utils.fp8_e4m3_table()[c2] * s2[:, None]).view(np.uint32), r.view(np.uint32))
    assert np.array_equal(utils.round_fp8_rows(r).view(np.uint32), r.view(np.uint32))
    # relative error of a normal-range element: half an ulp of three mantissa bits
    big = np.abs(W) >= scale[:, None] * 2.0 ** -6
    assert np.all(np.abs(r - W)[big] <= np.abs(W)[big] * 2.0 ** -4)
    with pytest.raises(ValueError, match="non-finite"):
        utils.quant_fp8_rows(np.array([[1.0, np.inf]], np.float32))
    with pytest.raises(ValueError, match="non-finite"):
        utils.round_fp8_rows(np.array([[np.nan, 1.0]], np.float32))


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
    for fam in ("gemv_fp8", "rows_fp8"):
        assert fam in l3hip.GEMM_FAMILIES
    assert l3hip.GEMM_FAMILIES.index("rows_bf16") == 7 and l3hip.GEMM_FAMILIES.index("gemv_fp8") == 8


def test_null_context_fails_with_a_message():
    lib = l3hip.lib()
    assert lib.l3_set_weight_fp8(None, 1) != 0
    assert b"null context" in lib.l3_last_error()
    m = ctypes.c_int32(7)
    assert lib.l3_weight_fp8_info(None, ctypes.byref(m), None, None, None) != 0
    assert b"null context" in lib.l3_last_error() and m.value == 7
    assert lib.l3_op_to_fp8_rows_host(None, None, 0, 32, None, None, None) != 0
    assert b"null context" in lib.l3_last_error()
    assert lib.l3_op_linear_fp8_host(None, None, 1, 32, 4, None, None, None, ctypes.c_float(0), None, None) != 0
    assert b"null context" in lib.l3_last_error()
    assert lib.l3_op_linear_fp8_rows_host(None, None, 2, 32, 4, None, None, None, ctypes.c_float(0), None, None) != 0
    assert b"null context" in lib.l3_last_error()


def test_weight_dtype_strings():
    args = synth.tiny(1)
    w = synth.make_weights(args, synth.TINY_HIDDEN, seed=1)
    for bad in ("fp8", "int8", "fp8-e5m2", "FP8-E4M3", "fp8-e4m3fn"):
        with pytest.raises(ValueError, match="weight_dtype"):
            llama3.Llama(w, args, weight_dtype=bad)
    # the new strings pass the name check: they get as far as the multi-device refusal
    for ok in ("fp8-e4m3", "fp8-e4m3-round"):
        assert ok in llama3._WEIGHT_DTYPES
        with pytest.raises(NotImplementedError, match="multi-device"):
            llama3.Llama(w, args, devices=[0, 1], weight_dtype=ok)
    assert llama3._WEIGHT_DTYPES["fp8-e4m3"] == 1 and llama3._WEIGHT_DTYPES["fp8-e4m3-round"] == 2
