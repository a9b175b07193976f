"""bf16 weight storage (DESIGN.md "bf16 weight storage"), the parts that need no GPU: the host
restatement of the rounding (utils.round_bf16) against torch's bfloat16 conversion bit for bit, the
new ABI symbols, and the argument checks that fail before a device is touched."""

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

NEW_SYMBOLS = ["l3_set_weight_bf16", "l3_weight_bf16_info", "l3_op_to_bf16_host", "l3_op_linear_bf16_host"]


def f32(bits):
    return np.array(bits, np.uint32).view(np.float32)


def edge_values():
    """fp32 values around every case of the rounding rule."""
    ties = [0x3F808000,  # exactly between two bf16 values, lower one even: rounds down
            0x3F818000,  # ... lower one odd: rounds up
            0xBF808000, 0xBF818000,
            0x3F808001, 0x3F807FFF, 0x3F80FFFF,  # just above / below a tie, all ones below
            0x00000000, 0x80000000,  # +0, -0
            0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x80008001,  # subnormals
            0x00800000, 0x7F7FFFFF, 0xFF7FFFFF,  # smallest normal, largest finite (overflows to inf)
            0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000,  # largest bf16, below / at the tie to inf
            0x7F800000, 0xFF800000,  # +-inf
            0x7FC00000, 0x7F800001, 0xFFC12345, 0x7FFFFFFF]  # NaNs, quiet and signalling
    return f32(ties)


def test_round_bf16_is_torch_bit_for_bit():
    rng = np.random.default_rng(0)
    x = np.concatenate([
        edge_values(),
        rng.standard_normal(20000).astype(np.float32),
        (rng.standard_normal(2000) * 1e-39).astype(np.float32),  # subnormal range
        rng.integers(0, 2 ** 32, 20000, dtype=np.uint64).astype(np.uint32).view(np.float32),  # any bit pattern
    ])
    want = torch.tensor(x).to(torch.bfloat16).float().numpy()
    got = utils.round_bf16(x)
    assert got.dtype == np.float32 and got.shape == x.shape
    nan = np.isnan(x)
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(np.isnan(want), nan)  # NaN stays NaN
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
    bits = utils.bf16_bits(x)
    assert bits.dtype == np.uint16 and np.array_equal(bits.astype(np.uint32) << 16, got.view(np.uint32))
    assert np.all(bits[nan] == 0x7FC0)


def test_round_bf16_named_cases():
    r = utils.round_bf16
    assert r(f32([0x3F808000])).view(np.uint32)[0] == 0x3F800000  # tie to even: down
    assert r(f32([0x3F818000])).view(np.uint32)[0] == 0x3F820000  # tie to even: up
    assert r(f32([0x80000000])).view(np.uint32)[0] == 0x80000000  # -0 kept
    assert r(f32([0x7F7FFFFF]))[0] == np.inf and r(f32([0xFF7FFFFF]))[0] == -np.inf
    assert r(f32([0x00008000])).view(np.uint32)[0] == 0x00000000  # subnormal tie to even
    assert r(f32([0x00018000])).view(np.uint32)[0] == 0x00020000
    assert r(f32([0x007FFFFF])).view(np.uint32)[0] == 0x00800000  # subnormal rounds up to a normal
    assert r(np.float32(1.0)) == 1.0 and r(np.zeros((2, 3), np.float32)).shape == (2, 3)
    # idempotent: a rounded array is exact
    x = np.random.default_rng(1).standard_normal(1000).astype(np.float32)
    assert np.array_equal(r(r(x)), r(x))


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


def test_null_context_fails_with_a_message():
    lib = l3hip.lib()
    assert lib.l3_set_weight_bf16(None, 1) != 0
    assert b"null context" in lib.l3_last_error()
    m = ctypes.c_int32(7)
    assert lib.l3_weight_bf16_info(None, ctypes.byref(m), None, None) != 0
    assert b"null context" in lib.l3_last_error() and m.value == 7
    assert lib.l3_op_to_bf16_host(None, None, 0, None, None) != 0
    assert lib.l3_op_linear_bf16_host(None, None, 1, 32, 4, None, None, ctypes.c_float(0), None) != 0


def test_unknown_weight_dtype_raises_before_anything_is_built():
    args = synth.tiny(1)
    w = synth.make_weights(args, synth.TINY_HIDDEN, seed=1)
    for bad in ("int8", "fp8", "BF16", 1):
        with pytest.raises(ValueError, match="weight_dtype"):
            llama3.Llama(w, args, weight_dtype=bad)
    with pytest.raises(NotImplementedError, match="multi-device"):
        llama3.Llama(w, args, devices=[0, 1], weight_dtype="bf16")
