"""float64 NumPy reference of one GEMM launch with each fused epilogue (test infrastructure).

Written from the reference model's semantics, not from the kernels: the dense contractions
`x @ W.T` (llama3.py:166-168, :211, :99-102), the RMSNorm row factor (:111-114), RoPE on
interleaved (even, odd) pairs (:41-76), the KV-cache append (:184-185) and SwiGLU (:97-103).
tests/test_gemm_epi_ref_cpu.py checks it against oracle/llama3_oracle.py.

Every function also returns a worst-case fp32 error bound for its outputs, from the accumulation
bound K * 2^-24 * (|x| @ |w|.T) of a K-term fp32 dot product in any summation order (Higham,
"Accuracy and Stability of Numerical Algorithms", eq. 3.5, gamma_K ~ K u with u = 2^-24),
propagated through the epilogue.
"""

import numpy as np

U = 2.0 ** -24  # fp32 unit roundoff

STORE, RESID, SWIGLU, QKV = 0, 1, 2, 3


def interleave_gate_up(wg, wu):
    """[hidden, K] gate and up -> the kernels' fused [2 hidden, K] layout: rows 32 g .. 32 g + 15
    are gate rows 16 g .. 16 g + 15, rows 32 g + 16 .. 32 g + 31 the up rows of the same units."""
    hidden, K = wg.shape
    assert wu.shape == wg.shape and hidden % 16 == 0
    out = np.empty((hidden // 16, 2, 16, K), wg.dtype)
    out[:, 0] = wg.reshape(hidden // 16, 16, K)
    out[:, 1] = wu.reshape(hidden // 16, 16, K)
    return out.reshape(2 * hidden, K)


def split_gate_up(wgu):
    """Inverse of interleave_gate_up."""
    n2, K = wgu.shape
    assert n2 % 32 == 0
    v = wgu.reshape(n2 // 32, 2, 16, K)
    return v[:, 0].reshape(n2 // 2, K).copy(), v[:, 1].reshape(n2 // 2, K).copy()


def row_factor(x, eps):
    """1 / sqrt(mean(x^2) + eps) per row (llama3.py:111-114 without the weight), float64."""
    x = np.asarray(x, np.float64)
    return 1.0 / np.sqrt((x * x).mean(-1, keepdims=True) + eps)


def silu(x):
    return x / (1.0 + np.exp(-x))


def pre_activation(x, w, a_rows=None, norm=False, eps=0.0):
    """(s * z, bound): z = x[a_rows] @ w.T in float64, s the row factor (1 without norm); bound is
    the fp32 worst case of the scaled value: s * K u |x| @ |w|.T for the dot product, and for s
    itself K u / 2 (a K-term sum of squares, halved by the square root) + 4 u (mean, eps add,
    reciprocal square root at 1 ulp, the final multiply)."""
    x = np.asarray(x, np.float64)
    w = np.asarray(w, np.float64)
    if a_rows is not None:
        x = x[np.asarray(a_rows)]
    K = x.shape[1]
    z = x @ w.T
    bz = K * U * (np.abs(x) @ np.abs(w).T)
    if not norm:
        return z, bz
    s = row_factor(x, eps)
    return s * z, s * bz + np.abs(s * z) * (K * U / 2 + 4 * U)


def ref_store(x, w, norm=False, eps=0.0, a_rows=None):
    return pre_activation(x, w, a_rows, norm, eps)


def ref_resid(x, w, res, a_rows=None, res_rows=None):
    """res[res_rows] + x @ w.T (llama3.py:253 / :259); one more rounding for the add."""
    z, bz = pre_activation(x, w, a_rows)
    r = np.asarray(res, np.float64)
    if res_rows is not None:
        r = r[np.asarray(res_rows)]
    r = r[: z.shape[0]]
    out = r + z
    return out, bz + U * np.abs(out)


# silu_f = g * rcp(1 + exp(-g)) in fp32 with the hardware transcendentals.  Relative error of the
# sigmoid factor: the exponential's argument -g * log2(e) is rounded once, an absolute error
# |g| log2(e) u that the exponential turns into a relative |g| u (log2(e) ln 2 = 1); v_exp_f32 and
# v_rcp_f32 are 1 ulp = 2 u each; the add 1 + e and the two multiplies (by g, by u) round once
# each: (|g| + 2 + 2 + 3) u.  d sigmoid / d e never amplifies a relative error of e.
def swiglu_own_bound(g, u):
    return (np.abs(g) + 7.0) * U * np.abs(silu(g) * u)


def ref_swiglu(x, wg, wu, norm=False, eps=0.0, a_rows=None):
    """silu(s g) * (s u) (llama3.py:97-103 before the down projection): (out, bound, g).
    |silu'| <= 1.1 carries the gate's bound; the cross term is second order but kept."""
    g, bg = pre_activation(x, wg, a_rows, norm, eps)
    u, bu = pre_activation(x, wu, a_rows, norm, eps)
    out = silu(g) * u
    bound = 1.1 * bg * (np.abs(u) + bu) + np.abs(silu(g)) * bu + swiglu_own_bound(g, u)
    return out, bound, g


def rotate_pairs(v, cos, sin):
    """llama3.py:41-76 on the last axis: (v[2i], v[2i+1]) -> (v[2i] c - v[2i+1] s, v[2i] s + v[2i+1] c)
    with cos / sin broadcastable to v[..., HD/2]."""
    re, im = v[..., 0::2], v[..., 1::2]
    out = np.empty_like(v)
    out[..., 0::2] = re * cos - im * sin
    out[..., 1::2] = re * sin + im * cos
    return out


def ref_qkv(x, w, rope_cos, rope_sin, *, L, start_pos, H, KVH, HD, q_scale, col_base=0, norm=False, eps=0.0,
            a_rows=None):
    """The QKV projection of llama3.py:166-185 for rows r = b * L + t (sequence b, position
    start_pos + t).  w holds the [q | k | v] output columns from col_base on (0, or H * HD for a
    K / V-only launch), or the H * HD q columns alone.  Returns a dict:
      q [M, H * HD] (None with col_base), q_bound; k, v [B, KVH, L, HD] — what belongs in cache
      slots [start_pos, start_pos + L) of sequences 0 .. B - 1 — and k_bound, v_bound (None for a
      q-only launch, which appends nothing).
    q and k are rotated, q then scaled by q_scale, v is not rotated."""
    z, bz = pre_activation(x, w, a_rows, norm, eps)
    M = z.shape[0]
    assert M % L == 0
    B = M // L
    qdim, kvdim = H * HD, KVH * HD
    n = z.shape[1]
    q_only = col_base == 0 and n == qdim
    assert col_base in (0, qdim) and (q_only or n + col_base == qdim + 2 * kvdim)
    full = np.zeros((M, qdim + 2 * kvdim))
    fb = np.zeros_like(full)
    full[:, col_base:col_base + n] = z
    fb[:, col_base:col_base + n] = bz
    pos = start_pos + np.arange(M) % L
    c = np.asarray(rope_cos, np.float64)[pos][:, None, :]  # [M, 1, HD / 2]
    s = np.asarray(rope_sin, np.float64)[pos][:, None, :]

    def rot(v, b):
        r = rotate_pairs(v, c, s)
        # each output is a c +- b s of two inputs: the bounds rotate by |c|, |s|, and the two
        # products and the add round once each (3 u of the magnitudes)
        def spread(a):  # |a[2i]| |c| + |a[2i+1]| |s|, |a[2i]| |s| + |a[2i+1]| |c|
            o = np.empty_like(a)
            o[..., 0::2] = a[..., 0::2] * np.abs(c) + a[..., 1::2] * np.abs(s)
            o[..., 1::2] = a[..., 0::2] * np.abs(s) + a[..., 1::2] * np.abs(c)
            return o

        return r, spread(b) + 3 * U * spread(np.abs(v))

    q, qb = rot(full[:, :qdim].reshape(M, H, HD), fb[:, :qdim].reshape(M, H, HD))
    k, kb = rot(full[:, qdim:qdim + kvdim].reshape(M, KVH, HD), fb[:, qdim:qdim + kvdim].reshape(M, KVH, HD))
    v = full[:, qdim + kvdim:].reshape(M, KVH, HD)
    vb = fb[:, qdim + kvdim:].reshape(M, KVH, HD)
    q = q * q_scale
    qb = qb * abs(q_scale) + U * np.abs(q)

    def slots(a):  # [M, KVH, HD] -> [B, KVH, L, HD]
        return a.reshape(B, L, KVH, HD).transpose(0, 2, 1, 3)

    return {
        "q": None if col_base else q.reshape(M, qdim), "q_bound": qb.reshape(M, qdim),
        "k": None if q_only else slots(k), "k_bound": slots(kb),
        "v": None if q_only else slots(v), "v_bound": slots(vb), "B": B,
    }
