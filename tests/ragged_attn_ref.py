"""fp64 NumPy reference, inputs and case tables of the ragged attention kernels (csrc/ragged.hip,
csrc/ragged_extend.hip; DESIGN.md "Ragged attention at kernel level"), shared by
tests/test_ragged_attn_cpu.py, tests/test_gpu_ragged_attn.py and tests/ragged_attn_checks_workload.py.

Parameters: head size in HDS x n_rep in 1..8; KVH is 3 for n_rep <= 4 and 1 above, so H stays at
most 12.  A batch is the rows of a table plus one guard row placed last — a finished row (decode)
or a row of length 0 (extend): zeros out, its cache bit for bit what went in.

Input kinds (``kind``):
  random  N(0, 1) with the library's RoPE tables and NaN in every slot no query may read, as
          split_attn_ref.make_inputs / extend_attn_ref.make_inputs build them;
  census  identity RoPE (cos = 1, sin = 0), q = 0, V one-hot by slot % HD (the new tokens' v
          included): every p is exactly 1, so out * keys is the number of visible keys of each
          residue class — an integer for every query row;
  stress  identity RoPE, q = e_0 on every head, so the log2-domain score of key j is the one
          product K[j, 0] * fl32(q_scale): a ramp of at least 1 per key up or down, or one key
          200 above a flat rest.  V is N(0, 1).  The reference takes that product in fp32 — it is
          the score's only term, so whatever the summation order the kernel holds exactly this
          value — and everything after it in fp64.

Tables are data derived from the kernels' tile constants; tests/test_ragged_attn_cpu.py asserts
by name every edge they are meant to reach."""

import functools
import math

import numpy as np

import extend_attn_ref as ext
import kv_bf16_ref as kv
import split_attn_ref as dec
from attn_dense_ref import HDS, STRESS

N_REPS = tuple(range(1, 9))
PARAMS = [(hd, n_rep) for hd in HDS for n_rep in N_REPS]
KTS = ("f32", "bf16")
SMAX = 320
EXT_KT, EXT_TA = 32, 16                  # ragged_extend.hip: keys per tile, tokens per append tile
RAGGED_LDS_BYTES = 65536                 # kernels.h
SPREAD_MIN = 150.0                       # a stress row counts from this log2-domain spread on
RAMP_SPREAD, SPIKE = 160.0, 200.0


def kvh_of(n_rep):
    return 3 if n_rep <= 4 else 1


def rows_of(hd):
    """R = 256 / (HD / 4): key groups of the decode kernels' P.V (2 R over a bf16 cache)"""
    return 256 // (hd // 4)


def q_scale(hd):
    """log2(e) / sqrt(HD) as the host passes it: computed in double, rounded to fp32"""
    return np.float32(dec.LOG2E / math.sqrt(float(hd)))


def decode_lds_bytes(n_rep, hd, s_cap):
    """ragged.hip attn_decode_ragged_lds (and, with the chunk for s_cap, attn_decode_split_lds)"""
    return (n_rep * hd + 2 * hd + 8 + n_rep * rows_of(hd) * hd + n_rep * s_cap) * 4


# ---- decode tables -------------------------------------------------------------------------------
def single_positions(hd):
    """0, 1; the softmax lane stride; R and 2 R (the P.V groups, doubled over bf16); the score
    loop's second trip; the last slot"""
    r = rows_of(hd)
    return tuple(sorted({0, 1, 63, 64, 65, r - 1, r, r + 1, 2 * r - 1, 2 * r, 2 * r + 1, 255, 256, 257, SMAX - 1}))


SPLITS = ((64, 320), (320, 384), (128, 320))     # (chunk, s_cap = Smax)


def split_positions(chunk, s_cap):
    """every pos whose owner chunk holds only the new key (pos % chunk == 0), one cached key, or
    the new key in its last slot; and the last slot"""
    return tuple(sorted({p for p in range(s_cap) if p % chunk in (0, 1, chunk - 1)} | {s_cap - 1}))


# ---- extend tables -------------------------------------------------------------------------------
def tq_of(n_rep):
    return 64 // n_rep


def lq_of(n_rep):
    return min(2 * tq_of(n_rep) + 17, SMAX)


def wave_lo(start, t0, wid, n_live, n_rep):
    """ragged_extend.hip w_lo: the first visible-key limit of wave wid of the tile at token t0"""
    return start + t0 + min(wid * 16, n_live * n_rep - 1) // n_rep


def masked_edge_starts(n_rep):
    """Starts that put the first query of a wave of the first or second query tile exactly on a
    key tile's last key (w_lo == k0 + EXT_KT - 1: the unmasked body) and one short of it (masked),
    one full key tile in front; for rows of Lq tokens"""
    tq, out = tq_of(n_rep), set()
    for t0 in (0, tq):
        for wid in range(4):
            if wid * 16 >= tq * n_rep:
                continue
            off = wave_lo(0, t0, wid, tq, n_rep)
            for side in (EXT_KT - 1, EXT_KT - 2):
                out.add(EXT_KT + (side - off) % EXT_KT)
    return tuple(sorted(out))


@functools.lru_cache(maxsize=None)
def extend_pairs(n_rep):
    """(start, len) rows; the last is the guard row (len 0)"""
    tq, lq = tq_of(n_rep), lq_of(n_rep)
    lens = (1, tq - 1, tq, tq + 1, 2 * tq + 1, lq)
    rot = (1, 30, 31, 32, 17)
    pairs = [(s, lq) for s in (0, 1, 17, EXT_KT - 2, EXT_KT - 1, EXT_KT, SMAX - lq)]
    for i, n in enumerate(lens[:-1]):
        pairs += [(0, n), (rot[i], n), (SMAX - n, n)]
    pairs += [(s, lq) for s in masked_edge_starts(n_rep)]
    pairs += [(0, 0)]
    seen, out = set(), []
    for p in pairs:
        if p not in seen:
            seen.add(p)
            out.append(p)
    return tuple(out) + ((17, 0),)


LQ_LONG = 130     # at n_rep = 1: three query tiles of 64
LONG_PAIRS = ((0, 130), (31, 130), (SMAX - 130, 130), (17, 129), (30, 65), (1, 0))


# ---- inputs --------------------------------------------------------------------------------------
def _identity_rope(inp):
    inp["rope_cos"] = np.ones_like(inp["rope_cos"])
    inp["rope_sin"] = np.zeros_like(inp["rope_sin"])


def _one_hot(slots, hd):
    v = np.zeros((len(slots), hd), np.float32)
    v[np.arange(len(slots)), np.asarray(slots) % hd] = 1.0
    return v


def stress_scores(shape, n, at_new=False):
    """fp64 [n]: the intended scores of a row's n visible keys.  Ramps: slope max(1, 160 / (n - 1))
    per key, an integer, with its zero at the last key (rising) or the first (falling).  Spikes:
    one key 200 above a flat 0 — key 5 (spike_low), or the last key but one, or with ``at_new``
    the last, new, key (spike_high); clamped into the row"""
    j = np.arange(n, dtype=np.float64)
    slope = max(1.0, math.ceil(RAMP_SPREAD / max(n - 1, 1)))
    if shape == "rising":
        return slope * (j - (n - 1))
    if shape == "falling":
        return -slope * j
    s = np.zeros(n)
    at = min(5, n - 1) if shape == "spike_low" else max(n - 1 if at_new else n - 2, 0)
    s[at] = SPIKE
    return s


@functools.lru_cache(maxsize=4)
def _decode_base(hd, n_rep, positions, smax):
    return dec.make_inputs(hd, n_rep, kvh_of(n_rep), smax, positions, n_finished=1,
                           seed=[hd, n_rep, smax, len(positions)])


@functools.lru_cache(maxsize=2)
def _extend_base(hd, n_rep, pairs, lq):
    return ext.make_inputs(hd, n_rep, kvh_of(n_rep), SMAX, lq, pairs, seed=[hd, n_rep, lq, len(pairs)])


def _editable(base):
    """a copy whose qkv and caches may be written (the N(0, 1) draw is made once per table)"""
    return dict(base, qkv=base["qkv"].copy(), cache_k=base["cache_k"].copy(), cache_v=base["cache_v"].copy())


def decode_inputs(hd, n_rep, positions, smax, kind="random", shape=None):
    """A row at each of ``positions`` and the finished guard row, of the given kind.  The random
    kind's arrays are shared between calls: read only"""
    kvh = kvh_of(n_rep)
    base = _decode_base(hd, n_rep, tuple(positions), smax)
    if kind == "random":
        return base
    inp = _editable(base)
    H, B = inp["n_heads"], len(inp["pos"])
    _identity_rope(inp)
    qkv, ck, cv = inp["qkv"], inp["cache_k"], inp["cache_v"]
    q = qkv[:, :H * hd].reshape(B, H, hd)
    kn = qkv[:, H * hd:(H + kvh) * hd].reshape(B, kvh, hd)
    vn = qkv[:, (H + kvh) * hd:].reshape(B, kvh, hd)
    assert np.shares_memory(q, qkv) and np.shares_memory(kn, qkv) and np.shares_memory(vn, qkv)
    q[:] = 0
    for b, p in enumerate(inp["pos"]):
        live = not inp["finished"][b]
        if kind == "census":
            hot = _one_hot(np.arange(p + 1), hd)
            cv[b, :, :p] = hot[:p]
            vn[b] = hot[p]
        else:
            q[b, :, 0] = 1.0
            s = stress_scores(shape, p + 1, at_new=b % 3 == 0) if live else np.zeros(p + 1)
            k0 = (s / float(q_scale(hd))).astype(np.float32)
            ck[b, :, :p, 0] = k0[:p]
            kn[b, :, 0] = k0[p]
    return inp


def extend_inputs(hd, n_rep, pairs, lq, kind="random", shape=None):
    """A row per (start, len) pair, of the given kind (random: shared, read only)"""
    kvh = kvh_of(n_rep)
    base = _extend_base(hd, n_rep, tuple(pairs), lq)
    if kind == "random":
        return base
    inp = _editable(base)
    H, B = inp["n_heads"], len(pairs)
    _identity_rope(inp)
    qkv, ck, cv = inp["qkv"], inp["cache_k"], inp["cache_v"]
    q = qkv[:, :, :H * hd].reshape(B, lq, H, hd)
    kn = qkv[:, :, H * hd:(H + kvh) * hd].reshape(B, lq, kvh, hd)
    vn = qkv[:, :, (H + kvh) * hd:].reshape(B, lq, kvh, hd)
    assert np.shares_memory(q, qkv) and np.shares_memory(kn, qkv) and np.shares_memory(vn, qkv)
    q[:] = 0
    for b, (st, n) in enumerate(pairs):
        if kind == "census":
            hot = _one_hot(np.arange(st + n), hd)
            cv[b, :, :st] = hot[:st]
            vn[b, :n] = hot[st:, None]
        else:
            q[b, :, :, 0] = 1.0
            s = stress_scores(shape, st + n) if n else np.zeros(st)
            k0 = (s / float(q_scale(hd))).astype(np.float32)
            ck[b, :, :st, 0] = k0[:st]
            kn[b, :n, :, 0] = k0[st:, None]
    return inp


def to_bf16(inp):
    """the inputs with their caches as bf16 bit patterns (NaN poison: 0x7fc0)"""
    return dict(inp, cache_k=kv.to_bits(inp["cache_k"]), cache_v=kv.to_bits(inp["cache_v"]))


# ---- reference -----------------------------------------------------------------------------------
def _attend(q, keys, vals, hd, start, e0, scores_only=False):
    """q [T, g, r, d] (RoPE'd, unscaled), keys / vals [g, S, d], all fp64; query t sees the keys
    j <= start + t.  Returns (out [T, g, r, d], spread of the visible log2-domain scores).
    e0 (stress): the score is the fp32 product K[j, 0] * fl32(q_scale)"""
    T, g, r, d = q.shape
    S = keys.shape[1]
    if e0:
        s = (keys[:, :, 0].astype(np.float32) * q_scale(hd)).astype(np.float64)            # [g, S]
        s = np.broadcast_to(s[:, None, None, :], (g, T, r, S))
    else:
        qm = q.transpose(1, 0, 2, 3).reshape(g, T * r, d)
        s = (qm @ keys.transpose(0, 2, 1)).reshape(g, T, r, S) * (dec.LOG2E / math.sqrt(hd))
    live = np.arange(S)[None, :] <= start + np.arange(T)[:, None]                           # [T, S]
    s = np.where(live[None, :, None, :], s, -np.inf)
    top = s.max(axis=-1, keepdims=True)
    spread = float((top - np.where(live[None, :, None, :], s, np.inf).min(axis=-1, keepdims=True)).max())
    if scores_only:
        return None, spread
    p = np.exp2(s - top)
    p /= p.sum(axis=-1, keepdims=True)
    o = (p.reshape(g, T * r, S) @ vals).reshape(g, T, r, d)
    return o.transpose(1, 0, 2, 3), spread


def decode_reference(inp, kind="random", caches=None, scores_only=False):
    """(out [B, H * HD], new_k [B, KVH, HD], new_v, spread [B]) in fp64.  Without ``caches`` the
    new key / value are the reference's own (fp32 caches); with ``caches`` = the launch's returned
    (k, v) as fp64 values it attends over them as they are, slot pos included (bf16 caches).
    spread: max - min of each row's visible log2-domain scores"""
    B, kvh, _, hd = inp["cache_k"].shape
    H = inp["n_heads"]
    out, spread = np.zeros((B, H * hd)), np.zeros(B)
    new_k, new_v = np.full((B, kvh, hd), np.nan), np.full((B, kvh, hd), np.nan)
    for b in range(B):
        if inp["finished"][b]:
            continue
        p = int(inp["pos"][b])
        row = inp["qkv"][b].astype(np.float64)
        c, s = inp["rope_cos"][p].astype(np.float64), inp["rope_sin"][p].astype(np.float64)
        q = dec._rope(row[:H * hd].reshape(1, kvh, H // kvh, hd), c, s)
        new_k[b] = dec._rope(row[H * hd:(H + kvh) * hd].reshape(kvh, hd), c, s)
        new_v[b] = row[(H + kvh) * hd:].reshape(kvh, hd)
        if caches is None:
            keys = np.concatenate([inp["cache_k"][b, :, :p].astype(np.float64), new_k[b][:, None]], axis=1)
            vals = np.concatenate([inp["cache_v"][b, :, :p].astype(np.float64), new_v[b][:, None]], axis=1)
        else:
            keys, vals = caches[0][b, :, :p + 1], caches[1][b, :, :p + 1]
        o, spread[b] = _attend(q, keys, vals, hd, p, kind == "stress", scores_only)
        if not scores_only:
            out[b] = o.reshape(-1)
    return out, new_k, new_v, spread


def _extend_row(inp, b, caches):
    """row b: (q [n, g, r, d], keys [g, start + n, d], vals, new_k [g, n, d], new_v), fp64"""
    kvh, hd = inp["cache_k"].shape[1], inp["cache_k"].shape[3]
    H = inp["n_heads"]
    st, n = int(inp["starts"][b]), int(inp["lens"][b])
    rows = inp["qkv"][b, :n].astype(np.float64)
    c = inp["rope_cos"][st:st + n, None, None].astype(np.float64)                           # [n, 1, 1, d/2]
    s = inp["rope_sin"][st:st + n, None, None].astype(np.float64)
    q = dec._rope(rows[:, :H * hd].reshape(n, kvh, H // kvh, hd), c, s)
    new_k = dec._rope(rows[:, H * hd:(H + kvh) * hd].reshape(n, kvh, hd), c[:, 0], s[:, 0]).transpose(1, 0, 2)
    new_v = rows[:, (H + kvh) * hd:].reshape(n, kvh, hd).transpose(1, 0, 2)
    if caches is None:
        keys = np.concatenate([inp["cache_k"][b, :, :st].astype(np.float64), new_k], axis=1)
        vals = np.concatenate([inp["cache_v"][b, :, :st].astype(np.float64), new_v], axis=1)
    else:
        keys, vals = caches[0][b, :, :st + n], caches[1][b, :, :st + n]
    return q, keys, vals, new_k, new_v


def extend_reference(inp, kind="random", caches=None, scores_only=False):
    """(out [B, Lq, H * HD], new_k, new_v: per row [KVH, len, HD], spread [B]) in fp64; ``caches``
    as in decode_reference"""
    B, lq = inp["qkv"].shape[:2]
    out, spread, new_k, new_v = np.zeros((B, lq, inp["n_heads"] * inp["cache_k"].shape[3])), np.zeros(B), [], []
    for b in range(B):
        st, n = int(inp["starts"][b]), int(inp["lens"][b])
        q, keys, vals, nk, nv = _extend_row(inp, b, caches)
        new_k.append(nk)
        new_v.append(nv)
        if n == 0:
            continue
        o, spread[b] = _attend(q, keys, vals, inp["cache_k"].shape[3], st, kind == "stress", scores_only)
        if not scores_only:
            out[b, :n] = o.reshape(n, -1)
    return out, new_k, new_v, spread


def decode_census(inp):
    """[B, HD] int64: keys j <= pos[b] with j % HD == d"""
    hd = inp["cache_k"].shape[3]
    n = inp["pos"].astype(np.int64)[:, None] + 1
    return (n - np.arange(hd)[None, :] + hd - 1) // hd


def extend_census(inp):
    """[B, Lq, HD] int64: keys j <= starts[b] + t with j % HD == d"""
    hd, lq = inp["cache_k"].shape[3], inp["qkv"].shape[1]
    n = inp["starts"].astype(np.int64)[:, None, None] + np.arange(lq)[None, :, None] + 1
    return (n - np.arange(hd)[None, None, :] + hd - 1) // hd


def masked_full(inp):
    """extend_reference's out in the reference model's own formulation, one row at a time: the
    full score matrix q k^T / sqrt(HD) plus the -inf upper triangle, softmax, times v"""
    import llama3_oracle as orc
    B, kvh, _, hd = inp["cache_k"].shape
    H, lq = inp["n_heads"], inp["qkv"].shape[1]
    out = np.zeros((B, lq, H * hd))
    for b in range(B):
        st, n = int(inp["starts"][b]), int(inp["lens"][b])
        if n == 0:
            continue
        q, keys, vals, _, _ = _extend_row(inp, b, None)
        q = q.reshape(n, H, hd).transpose(1, 0, 2)                                           # [H, n, d]
        keys, vals = np.repeat(keys, H // kvh, axis=0), np.repeat(vals, H // kvh, axis=0)    # [H, S, d]
        mask = np.concatenate([np.zeros((n, st)), np.triu(np.full((n, n), -np.inf), k=1)], axis=1)
        o = orc.softmax(q @ keys.transpose(0, 2, 1) / math.sqrt(hd) + mask[None]) @ vals
        out[b, :n] = o.transpose(1, 0, 2).reshape(n, H * hd)
    return out
