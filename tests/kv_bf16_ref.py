"""fp64 NumPy references for the bf16 KV cache (DESIGN.md "bf16 KV-cache storage"), shared by
tests/test_kv_bf16_cpu.py and tests/test_gpu_kv_bf16.py.

The device rounds keys and values it computed in fp32, so a value within fp32 error of a bf16 tie
may round either way, and one flip moves the logits by more than the project's 1e-4.  No test
therefore compares the device with an independently rounded reference.  Two questions are asked
separately instead:

  A  is each stored value a correct rounding?  ``check_a``: the stored value d is correct for the
     oracle's unrounded fp64 value x when |d - x| <= ulp_bf16(d) / 2 + eps;
  B  given the cache bits, is the attention right?  ``attend_decode`` / ``attend_extend`` (op level)
     and ``ForcedOracle`` (model level) attend over the device's own stored values, widened, so only
     fp32 arithmetic error remains and the project's existing bars apply."""

import math

import numpy as np

import llama3_oracle as orc
from split_attn_ref import _rope
from utils import bf16_bits

NAN_BITS = 0x7FC0  # the quiet NaN the op tests poison unread slots with


def widen(bits):
    """bf16 bit patterns (uint16) as fp64 values, exactly."""
    u = np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << 16
    return u.view(np.float32).astype(np.float64)


def ulp_bf16(d):
    """2^(floor(log2 |d|) - 7): the spacing of bf16 values in d's binade (8 significant bits); the
    smallest normal's for 0."""
    _, e = np.frexp(np.abs(np.asarray(d, np.float64)))  # |d| = m * 2^e, m in [0.5, 1)
    return np.where(np.asarray(d) == 0, 2.0 ** -133, np.ldexp(1.0, e - 8))


def check_a(d, x, eps):
    """Element-wise: is the stored value d a correct rounding of x, given that the device's own x
    lies within eps of the oracle's?"""
    d, x = np.asarray(d, np.float64), np.asarray(x, np.float64)
    return np.abs(d - x) <= ulp_bf16(d) / 2 + eps


def excess_a(d, x):
    """max(|d - x| - ulp_bf16(d) / 2): what eps must cover."""
    d, x = np.asarray(d, np.float64), np.asarray(x, np.float64)
    return float(np.max(np.abs(d - x) - ulp_bf16(d) / 2)) if d.size else 0.0


def to_bits(a):
    """fp32 values as bf16 bit patterns (utils.bf16_bits: RNE), NaN as 0x7fc0."""
    return bf16_bits(np.asarray(a, np.float32))


def _softmax_rows(q, keys, vals, hd):
    s = keys @ q / math.sqrt(hd)
    e = np.exp(s - s.max())
    return (e / e.sum()) @ vals


def attend_decode(inp, ck, cv):
    """split_attn_ref.reference without its own append: out [B, H * HD] fp64 of a decode launch
    whose caches read ck / cv (fp64 values, slot pos[b] appended already) afterwards."""
    B, kvh, _, hd = ck.shape
    H = inp["n_heads"]
    n_rep = H // kvh
    out = np.zeros((B, H * hd))
    for b in range(B):
        if inp["finished"][b]:
            continue
        p = int(inp["pos"][b])
        c, s = inp["rope_cos"][p].astype(np.float64), inp["rope_sin"][p].astype(np.float64)
        q = _rope(inp["qkv"][b, :H * hd].astype(np.float64).reshape(H, hd), c, s)
        for h in range(H):
            g = h // n_rep
            out[b, h * hd:(h + 1) * hd] = _softmax_rows(q[h], ck[b, g, :p + 1], cv[b, g, :p + 1], hd)
    return out


def attend_extend(inp, ck, cv):
    """extend_attn_ref.reference without its own append: out [B, Lq, H * HD] fp64 over the caches
    as the launches left them (fp64 values)."""
    B, kvh, _, hd = ck.shape
    H = inp["n_heads"]
    n_rep = H // kvh
    lq = inp["qkv"].shape[1]
    out = np.zeros((B, lq, H * hd))
    cos, sin = inp["rope_cos"].astype(np.float64), inp["rope_sin"].astype(np.float64)
    for b in range(B):
        st, n = int(inp["starts"][b]), int(inp["lens"][b])
        for t in range(n):
            p = st + t
            q = _rope(inp["qkv"][b, t, :H * hd].astype(np.float64).reshape(H, hd), cos[p], sin[p])
            for h in range(H):
                g = h // n_rep
                out[b, t, h * hd:(h + 1) * hd] = _softmax_rows(q[h], ck[b, g, :p + 1], cv[b, g, :p + 1], hd)
    return out


class _KvLayer(orc.OracleLayer):
    """OracleLayer whose cache entries are ``self.store(layer, start, k, v)`` of its own fp64 k / v
    [L, KVH, HD] (one row, B = 1); the own values are kept in ``own_k`` / ``own_v`` [S, KVH, HD]
    (NaN where nothing was written)."""

    def __init__(self, w, i, args, store):
        super().__init__(w, i, args)
        self.i, self.store = i, store
        self.own_k = np.full(self.cache_k.shape[1:], np.nan)
        self.own_v = np.full(self.cache_v.shape[1:], np.nan)

    def attention(self, x, start_pos, mask, cos, sin):
        B, L, _ = x.shape
        assert B == 1
        q = (x @ self.wq.T).reshape(B, L, self.H, self.HD)
        k = (x @ self.wk.T).reshape(B, L, self.KVH, self.HD)
        v = (x @ self.wv.T).reshape(B, L, self.KVH, self.HD)
        q, k = orc.rope(q, k, cos, sin)
        end = start_pos + L
        self.own_k[start_pos:end], self.own_v[start_pos:end] = k[0], v[0]
        sk, sv = self.store(self.i, start_pos, k[0], v[0])
        self.cache_k[0, start_pos:end], self.cache_v[0, start_pos:end] = sk, sv
        n_rep = self.H // self.KVH
        keys = orc.repeat_kv(self.cache_k[:B, :end], n_rep).transpose(0, 2, 1, 3)
        vals = orc.repeat_kv(self.cache_v[:B, :end], n_rep).transpose(0, 2, 1, 3)
        q = q.transpose(0, 2, 1, 3)
        scores = q @ keys.transpose(0, 1, 3, 2) / math.sqrt(self.HD)
        if mask is not None:
            scores = scores + mask[None, None, :, :]
        o = orc.softmax(scores) @ vals
        return o.transpose(0, 2, 1, 3).reshape(B, L, -1) @ self.wo.T


class _KvModel(orc.OracleModel):
    def __init__(self, weights, args, store):
        super().__init__(weights, args)
        assert args.max_batch_size == 1
        self.layers = [_KvLayer(weights, i, args, store) for i in range(args.n_layers)]


class RoundingOracle(_KvModel):
    """The simulated device of the CPU tests: every k / v is perturbed by ``rel`` relative (a fixed
    pseudo-random sign per element: the fp32 error of a device), cast to fp32 and rounded to bf16 by
    RNE as it enters the cache."""

    def __init__(self, weights, args, rel=2e-6, seed=0):
        rng = np.random.default_rng(seed)

        def store(_, __, k, v):
            def rnd(a):
                a = a * (1 + rel * rng.choice((-1.0, 1.0), a.shape))
                return widen(to_bits(a))
            return rnd(k), rnd(v)

        super().__init__(weights, args, store)

    def caches(self):
        """per layer (k, v) [KVH, S, HD] fp64: what Context.cache_read returns for the row"""
        return [(l.cache_k[0].transpose(1, 0, 2).copy(), l.cache_v[0].transpose(1, 0, 2).copy()) for l in self.layers]


class ForcedOracle(_KvModel):
    """The forced oracle: each layer computes its own fp64 k / v (kept for check A) and writes the
    device's read-back values into its cache in their place.  ``caches``: per layer (k, v)
    [KVH, S, HD] of one cache row, as Context.cache_read returns them."""

    def __init__(self, weights, args, caches):
        forced = [(np.asarray(k, np.float64).transpose(1, 0, 2), np.asarray(v, np.float64).transpose(1, 0, 2))
                  for k, v in caches]

        def store(i, start, k, v):
            n = k.shape[0]
            return forced[i][0][start:start + n], forced[i][1][start:start + n]

        super().__init__(weights, args, store)
        self.forced = forced

    def audit(self):
        """(d_k, x_k, d_v, x_v), each [n_layers, n_written, KVH, HD]: the device's values and the
        oracle's own at every slot the replay wrote."""
        out = [[], [], [], []]
        for l, (fk, fv) in zip(self.layers, self.forced):
            w = ~np.isnan(l.own_k[:, 0, 0])
            for o, a in zip(out, (fk[w], l.own_k[w], fv[w], l.own_v[w])):
                o.append(a)
        return [np.stack(o) for o in out]


def replay(model, calls, ids, max_new):
    """The reference's call sequence on one row (llama3.py:285-321): ``calls`` [(ids, start), ...]
    (the prefill and any extends, T tokens in all), then — on the device's ``ids`` — the first
    token from position T - 1 and decode step i >= 1 at T + i fed ids[i - 1] (slot T is the hole).
    Returns (logits of the last call [VS], step logits [n, VS], top-2 margins [n]): step i's
    logits are those ids[i] was chosen from."""
    lg, T = None, 0
    for chunk, start in calls:
        chunk = np.asarray(chunk, np.int64).reshape(1, -1)
        lg = model(chunk, int(start))[0, -1]
        T = int(start) + chunk.shape[1]
    last, steps = lg, []
    ids = np.asarray(ids, np.int64).reshape(-1)
    assert ids.size == max(0, max_new - T) or ids.size == 0
    for i in range(ids.size):
        if i:
            lg = model(ids[i - 1].reshape(1, 1), T + i)[0, -1]
        steps.append(lg)
    steps = np.array(steps).reshape(len(steps), last.size)
    top = np.sort(steps, axis=-1)[:, -2:] if len(steps) else np.zeros((0, 2))
    return last, steps, top[:, 1] - top[:, 0]
