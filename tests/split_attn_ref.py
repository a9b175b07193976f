"""fp64 NumPy reference of one ragged decode-attention launch (csrc/ragged.hip; DESIGN.md
"Split-KV decode attention"), shared by tests/test_ragged_split_cpu.py and
tests/test_gpu_ragged_split.py.

Per row b at position pos[b]: adjacent-pair RoPE of the row's n_rep * KVH query heads and of its new
key, the new key / value appended to cache slot pos[b], softmax(q . k / sqrt(HD)) over the keys
[0, pos[b]] of the head's KV head, times the values.  A finished row gives zeros and leaves its
cache alone.  ``chunked`` models the split form: per chunk of CH keys the max m (log2 domain), the
sum l of exp2(s - m) and the unnormalised o, merged in ascending chunk order."""

import numpy as np

# the positions around the boundaries of 64-key chunks that both test files walk
POSITIONS = (0, 1, 63, 64, 65, 127, 128, 191, 192, 255)
LOG2E = 1.4426950408889634


def rope_tables(hd, smax):
    """[smax, hd/2] cos / sin as the library's fp32 tables (computed in fp64, then rounded)."""
    inv = 1.0 / (10000.0 ** (np.arange(0, hd, 2) / hd))
    ang = np.outer(np.arange(smax), inv)
    return np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)


def _rope(x, c, s):
    """x [..., HD] rotated in adjacent pairs (x[2i], x[2i+1]) by the angles of c, s [HD/2]"""
    out = np.empty_like(x)
    out[..., 0::2] = x[..., 0::2] * c - x[..., 1::2] * s
    out[..., 1::2] = x[..., 0::2] * s + x[..., 1::2] * c
    return out


def make_inputs(hd, n_rep, kvh, smax, positions, n_finished=1, seed=0):
    """One batch: a row at each of ``positions`` and ``n_finished`` finished rows (whose pos is a
    valid slot, to show the flag alone stops them).  N(0, 1) inputs; the cache slots from each
    live row's pos on hold NaN — the launch must write slot pos and never read past it."""
    rng = np.random.default_rng(seed)
    H = n_rep * kvh
    pos = np.array(list(positions) + [min(5, smax - 1)] * n_finished, np.int32)
    B = pos.size
    fin = np.zeros(B, np.int32)
    fin[len(positions):] = 1
    qkv = rng.standard_normal((B, (H + 2 * kvh) * hd)).astype(np.float32)
    ck = rng.standard_normal((B, kvh, smax, hd)).astype(np.float32)
    cv = rng.standard_normal((B, kvh, smax, hd)).astype(np.float32)
    for b in range(len(positions)):
        ck[b, :, pos[b]:] = np.nan
        cv[b, :, pos[b]:] = np.nan
    cos, sin = rope_tables(hd, smax)
    return dict(qkv=qkv, cache_k=ck, cache_v=cv, rope_cos=cos, rope_sin=sin, pos=pos, finished=fin, n_heads=H)


def _row(inp, b):
    """(q [H, HD] with RoPE, keys [KVH, pos + 1, HD], values, new k [KVH, HD], new v) of a live row"""
    ck, cv = inp["cache_k"], inp["cache_v"]
    _, kvh, _, hd = ck.shape
    H, p = inp["n_heads"], int(inp["pos"][b])
    row = inp["qkv"][b].astype(np.float64)
    c, s = inp["rope_cos"][p].astype(np.float64), inp["rope_sin"][p].astype(np.float64)
    q = _rope(row[:H * hd].reshape(H, hd), c, s)
    kn = _rope(row[H * hd:(H + kvh) * hd].reshape(kvh, hd), c, s)
    vn = row[(H + kvh) * hd:].reshape(kvh, hd)
    keys = np.concatenate([ck[b, :, :p].astype(np.float64), kn[:, None]], axis=1)
    vals = np.concatenate([cv[b, :, :p].astype(np.float64), vn[:, None]], axis=1)
    return q, keys, vals, kn, vn


def reference(inp):
    """(out [B, H * HD] fp64, new_k [B, KVH, HD] fp64, new_v [B, KVH, HD] fp64): the attention
    output and what slot pos[b] of the caches must hold afterwards (finished rows: zeros / NaN)."""
    B, kvh, _, hd = inp["cache_k"].shape
    H = inp["n_heads"]
    n_rep = H // kvh
    out = np.zeros((B, H * hd))
    new_k = np.full((B, kvh, hd), np.nan)
    new_v = np.full((B, kvh, hd), np.nan)
    for b in range(B):
        if inp["finished"][b]:
            continue
        q, keys, vals, kn, vn = _row(inp, b)
        new_k[b], new_v[b] = kn, vn
        for h in range(H):
            g = h // n_rep
            s = keys[g] @ q[h] / np.sqrt(hd)
            e = np.exp(s - s.max())
            out[b, h * hd:(h + 1) * hd] = (e / e.sum()) @ vals[g]
    return out, new_k, new_v


def chunked(inp, ch):
    """The same output by the chunk-and-combine rule at ``ch`` keys per chunk, in fp64."""
    B, kvh, _, hd = inp["cache_k"].shape
    H = inp["n_heads"]
    n_rep = H // kvh
    out = np.zeros((B, H * hd))
    for b in range(B):
        if inp["finished"][b]:
            continue
        q, keys, vals, _, _ = _row(inp, b)
        n = int(inp["pos"][b]) + 1
        for h in range(H):
            g = h // n_rep
            s = keys[g] @ q[h] * (LOG2E / np.sqrt(hd))  # log2 domain
            parts = []
            for k0 in range(0, n, ch):  # chunks 0 .. pos // ch
                sc = s[k0:k0 + ch]
                m = sc.max()
                e = np.exp2(sc - m)
                parts.append((m, e.sum(), e @ vals[g][k0:k0 + ch]))
            M = max(m for m, _, _ in parts)
            num, den = np.zeros(hd), 0.0
            for m, l, o in parts:  # ascending
                w = np.exp2(m - M)
                num += o * w
                den += l * w
            out[b, h * hd:(h + 1) * hd] = num / den
    return out
