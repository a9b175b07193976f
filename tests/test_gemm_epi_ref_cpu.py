"""The float64 epilogue reference of the GEMM route matrix (tests/gemm_epi_ref.py) against the
oracle model (oracle/llama3_oracle.py): RoPE on real tables, the RMSNorm, the FFN, the cache
append, and the gate|up interleave by a round trip.  No GPU: a wrong reference must not be able to
agree quietly with a wrong kernel.
"""

import ctypes
import types

import numpy as np
import pytest

import gemm_epi_ref as ref
import l3hip
import llama3_oracle as orc


def test_gate_up_interleave_round_trip_and_layout():
    rng = np.random.default_rng(0)
    wg, wu = rng.standard_normal((48, 32)), rng.standard_normal((48, 32))
    f = ref.interleave_gate_up(wg, wu)
    assert f.shape == (96, 32)
    g2, u2 = ref.split_gate_up(f)
    assert np.array_equal(g2, wg) and np.array_equal(u2, wu)
    # hidden unit h: gate at fused row 32 (h // 16) + h % 16, up 16 rows further
    for h in (0, 15, 16, 33, 47):
        assert np.array_equal(f[32 * (h // 16) + h % 16], wg[h])
        assert np.array_equal(f[32 * (h // 16) + 16 + h % 16], wu[h])
    # the binding's helper builds the same layout
    assert np.array_equal(l3hip.interleave_gate_up(wg.astype(np.float32), wu.astype(np.float32)),
                          f.astype(np.float32))


def test_row_factor_and_store_match_the_oracle_rmsnorm():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((7, 64))
    nw = rng.uniform(0.5, 1.5, 64)
    w = rng.standard_normal((12, 64))
    eps = 1e-5
    want = orc.rmsnorm(x, nw, eps) @ w.T
    got, bound = ref.ref_store(x, w * nw, norm=True, eps=eps)  # the norm weight folded into w
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)
    assert np.all(bound > 0)
    np.testing.assert_allclose(ref.row_factor(x, eps)[:, 0], 1 / np.sqrt((x * x).mean(-1) + eps), rtol=1e-15)
    # gathered rows
    rows = np.array([3, 3, 0, 6, 1])
    got, _ = ref.ref_store(x, w * nw, norm=True, eps=eps, a_rows=rows)
    np.testing.assert_allclose(got, want[rows], rtol=1e-12, atol=1e-12)


def test_swiglu_and_resid_match_the_oracle_ffn():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((5, 32))
    wg, wu = 0.3 * rng.standard_normal((48, 32)), 0.3 * rng.standard_normal((48, 32))
    wd = 0.3 * rng.standard_normal((32, 48))
    hid, bound, g = ref.ref_swiglu(x, wg, wu)
    np.testing.assert_allclose(g, x @ wg.T, rtol=1e-13)
    res = rng.standard_normal((5, 32))
    out, _ = ref.ref_resid(hid, wd, res)
    np.testing.assert_allclose(out, res + orc.ffn(x, wg, wu, wd), rtol=1e-11, atol=1e-12)
    assert np.all(bound >= ref.swiglu_own_bound(g, x @ wu.T))
    # residual gathered from a table
    table = rng.standard_normal((9, 32))
    rr = np.array([8, 0, 0, 4, 2])
    out, _ = ref.ref_resid(hid, wd, table, res_rows=rr)
    np.testing.assert_allclose(out, table[rr] + orc.ffn(x, wg, wu, wd), rtol=1e-11, atol=1e-12)


@pytest.mark.parametrize("H,KVH,HD,L,start_pos", [(4, 2, 32, 5, 3), (4, 1, 64, 1, 7), (6, 6, 48, 4, 0)])
def test_qkv_matches_the_oracle_attention_projection(H, KVH, HD, L, start_pos):
    """q (before the score scale), and the cache slots, of OracleLayer.attention on the real RoPE
    tables; rows are b * L + t as the kernels see them."""
    rng = np.random.default_rng(3)
    D, B, Smax = 64, 3, 16
    x = rng.standard_normal((B, L, D))
    wq, wk, wv = (0.2 * rng.standard_normal((n, D)) for n in (H * HD, KVH * HD, KVH * HD))
    cos, sin = orc.rope_tables(HD, Smax)
    q = (x @ wq.T).reshape(B, L, H, HD)
    k = (x @ wk.T).reshape(B, L, KVH, HD)
    v = (x @ wv.T).reshape(B, L, KVH, HD)
    q, k = orc.rope(q, k, cos[start_pos:start_pos + L], sin[start_pos:start_pos + L])
    q_scale = 0.25
    r = ref.ref_qkv(x.reshape(B * L, D), np.concatenate([wq, wk, wv]), cos, sin, L=L, start_pos=start_pos, H=H,
                    KVH=KVH, HD=HD, q_scale=q_scale)
    assert r["B"] == B
    np.testing.assert_allclose(r["q"], q.reshape(B * L, H * HD) * q_scale, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(r["k"], k.transpose(0, 2, 1, 3), rtol=1e-12, atol=1e-13)  # [B, KVH, L, HD]
    np.testing.assert_allclose(r["v"], v.transpose(0, 2, 1, 3), rtol=1e-12, atol=1e-13)
    # the K / V-only form gives the same slots and no q
    r2 = ref.ref_qkv(x.reshape(B * L, D), np.concatenate([wk, wv]), cos, sin, L=L, start_pos=start_pos, H=H,
                     KVH=KVH, HD=HD, q_scale=q_scale, col_base=H * HD)
    assert r2["q"] is None
    assert np.array_equal(r2["k"], r["k"]) and np.array_equal(r2["v"], r["v"])
    # the q-only form gives the same q and appends nothing
    r3 = ref.ref_qkv(x.reshape(B * L, D), wq, cos, sin, L=L, start_pos=start_pos, H=H, KVH=KVH, HD=HD, q_scale=q_scale)
    assert np.array_equal(r3["q"], r["q"]) and r3["k"] is None and r3["v"] is None
    # the bounds grow with the operands and are never zero where the value is not
    assert np.all(r["q_bound"][r["q"] != 0] > 0) and np.all(r["k_bound"][r["k"] != 0] > 0)


def test_qkv_slots_are_the_oracle_layers_cache_append():
    """The oracle layer's own cache after a call holds ref_qkv's k / v at [start_pos, start_pos + L)."""
    rng = np.random.default_rng(4)
    H, KVH, HD, L, B, Smax, sp = 4, 2, 16, 3, 2, 8, 5
    D = H * HD
    args = types.SimpleNamespace(norm_eps=1e-5, n_heads=H, n_kv_heads=KVH, dim=D, max_batch_size=B, max_seq_len=Smax)
    p = "model.layers.0."
    w = {p + "self_attn.q_proj.weight": 0.2 * rng.standard_normal((D, D)),
         p + "self_attn.k_proj.weight": 0.2 * rng.standard_normal((KVH * HD, D)),
         p + "self_attn.v_proj.weight": 0.2 * rng.standard_normal((KVH * HD, D)),
         p + "self_attn.o_proj.weight": np.zeros((D, D)), p + "mlp.gate_proj.weight": np.zeros((32, D)),
         p + "mlp.up_proj.weight": np.zeros((32, D)), p + "mlp.down_proj.weight": np.zeros((D, 32)),
         p + "input_layernorm.weight": rng.uniform(0.5, 1.5, D), p + "post_attention_layernorm.weight": np.ones(D)}
    layer = orc.OracleLayer(w, 0, args)
    x = rng.standard_normal((B, L, D))
    cos, sin = orc.rope_tables(HD, Smax)
    layer(x, sp, orc.causal_mask(L, sp), cos[sp:sp + L], sin[sp:sp + L])
    wqkv = np.concatenate([w[p + f"self_attn.{n}_proj.weight"] for n in "qkv"]) * w[p + "input_layernorm.weight"]
    r = ref.ref_qkv(x.reshape(B * L, D), wqkv, cos, sin, L=L, start_pos=sp, H=H, KVH=KVH, HD=HD, q_scale=1.0,
                    norm=True, eps=args.norm_eps)
    # oracle cache [B, Smax, KVH, HD]; ref slots [B, KVH, L, HD]
    np.testing.assert_allclose(r["k"], layer.cache_k[:, sp:sp + L].transpose(0, 2, 1, 3), rtol=1e-11, atol=1e-12)
    np.testing.assert_allclose(r["v"], layer.cache_v[:, sp:sp + L].transpose(0, 2, 1, 3), rtol=1e-11, atol=1e-12)
    assert not layer.cache_k[:, :sp].any() and not layer.cache_k[:, sp + L:].any()


def test_sentinel_is_nan_free_and_varied():
    s = l3hip.gemm_sentinel((4, 1000), 7)
    assert s.dtype == np.float32 and np.isfinite(s).all()
    assert len(np.unique(s.view(np.uint32))) > 3900
    assert not np.array_equal(s, l3hip.gemm_sentinel((4, 1000), 8))


def test_entry_point_is_exported_and_loud_without_a_device():
    lib = l3hip.lib()
    assert "l3_op_gemm_host" in l3hip.header_symbols()
    op = l3hip.GemmOp()
    assert lib.l3_op_gemm_host(None, ctypes.byref(op)) != 0
    assert b"null context" in lib.l3_last_error()
    assert l3hip.version() == "0.19"
