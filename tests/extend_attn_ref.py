"""fp64 NumPy reference of one ragged extend (csrc/ragged_extend.hip; DESIGN.md "Ragged
continuation"), shared by tests/test_ragged_extend_cpu.py and tests/test_gpu_ragged_extend.py.

Per row b with len[b] new tokens at positions start[b] + t: adjacent-pair RoPE of the token's
n_rep * KVH query heads and of its new key, the new key / value stored to cache slot start[b] + t,
then softmax(q . k / sqrt(HD)) over the keys [0, start[b] + t] of the head's KV head, times the
values.  Pad tokens (t >= len[b]) give zeros and touch no slot."""

import numpy as np

from split_attn_ref import _rope, rope_tables

# (start, len) pairs that straddle every edge of the kernel's tiles (32-key tiles, 64 / n_rep query
# tokens per workgroup, 16-token append tiles) in a cache of 256 slots with 40-token chunks
PAIRS = ((0, 1), (0, 40), (1, 16), (63, 17), (64, 15), (65, 40), (200, 40), (216, 40), (255, 1))
SMAX, LQ = 256, 40


def make_inputs(hd, n_rep, kvh=2, smax=SMAX, lq=LQ, pairs=PAIRS, seed=0):
    """One batch, a row per (start, len) pair.  N(0, 1) inputs, pads included; every cache slot
    from start + len on holds NaN — the launches must never read it — and the slots
    [start, start + len) hold values the append must replace."""
    rng = np.random.default_rng(seed)
    H = n_rep * kvh
    starts = np.array([p[0] for p in pairs], np.int32)
    lens = np.array([p[1] for p in pairs], np.int32)
    B = len(pairs)
    qkv = rng.standard_normal((B, lq, (H + 2 * kvh) * hd)).astype(np.float32)
    ck = rng.standard_normal((B, kvh, smax, hd)).astype(np.float32)
    cv = rng.standard_normal((B, kvh, smax, hd)).astype(np.float32)
    for b in range(B):
        ck[b, :, starts[b] + lens[b]:] = np.nan
        cv[b, :, starts[b] + lens[b]:] = np.nan
    cos, sin = rope_tables(hd, smax)
    return dict(qkv=qkv, cache_k=ck, cache_v=cv, rope_cos=cos, rope_sin=sin, starts=starts, lens=lens, n_heads=H)


def reference(inp):
    """(out [B, Lq, H * HD] fp64, cache_k, cache_v fp64 copies with the new slots written)"""
    ck = inp["cache_k"].astype(np.float64)
    cv = inp["cache_v"].astype(np.float64)
    B, kvh, _, hd = ck.shape
    H = inp["n_heads"]
    n_rep = H // kvh
    lq = inp["qkv"].shape[1]
    out = np.zeros((B, lq, H * hd))
    cos, sin = inp["rope_cos"].astype(np.float64), inp["rope_sin"].astype(np.float64)
    for b in range(B):
        st, n = int(inp["starts"][b]), int(inp["lens"][b])
        rows = inp["qkv"][b, :n].astype(np.float64)
        q = np.empty((n, H, hd))
        for t in range(n):  # the append first: token t sees the new keys of tokens <= t
            p = st + t
            q[t] = _rope(rows[t, :H * hd].reshape(H, hd), cos[p], sin[p])
            ck[b, :, p] = _rope(rows[t, H * hd:(H + kvh) * hd].reshape(kvh, hd), cos[p], sin[p])
            cv[b, :, p] = rows[t, (H + kvh) * hd:].reshape(kvh, hd)
        for t in range(n):
            p = st + t
            for h in range(H):
                g = h // n_rep
                s = ck[b, g, :p + 1] @ q[t, h] / np.sqrt(hd)
                e = np.exp(s - s.max())
                out[b, t, h * hd:(h + 1) * hd] = (e / e.sum()) @ cv[b, g, :p + 1]
    return out, ck, cv


def two_chunks(inp, cut):
    """The same tokens in two extends: row b's first min(cut, len) tokens, then the rest at
    start + cut, on the caches the first extend left (re-poisoned past each chunk's end).
    Returns out [B, Lq, H * HD] assembled from the two calls."""
    lq = inp["qkv"].shape[1]
    starts, lens = inp["starts"], inp["lens"]
    n1 = np.minimum(lens, cut).astype(np.int32)
    first = dict(inp, lens=n1, cache_k=inp["cache_k"].copy(), cache_v=inp["cache_v"].copy())
    for b in range(len(lens)):
        first["cache_k"][b, :, starts[b] + n1[b]:] = np.nan
        first["cache_v"][b, :, starts[b] + n1[b]:] = np.nan
    o1, ck, cv = reference(first)
    n2 = (lens - n1).astype(np.int32)
    qkv2 = np.zeros_like(inp["qkv"])
    for b in range(len(lens)):
        qkv2[b, :n2[b]] = inp["qkv"][b, n1[b]:lens[b]]
    second = dict(inp, qkv=qkv2, lens=n2, starts=(starts + n1).astype(np.int32), cache_k=ck, cache_v=cv)
    o2, _, _ = reference(second)
    out = np.zeros_like(o1)
    for b in range(len(lens)):
        out[b, :n1[b]] = o1[b, :n1[b]]
        out[b, n1[b]:lens[b]] = o2[b, :n2[b]]
    assert out.shape[1] == lq
    return out
