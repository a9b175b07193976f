"""fp64 NumPy reference, inputs and case tables of the dense attention kernels (csrc/attn_kernel.h
behind csrc/attention.hip; DESIGN.md "Dense attention at kernel level"), shared by
tests/test_attn_dense_cpu.py, tests/test_gpu_attn_dense.py and tests/attn_dense_checks_workload.py.

Reference: from the exact fp32 arrays the kernel gets — q~ = q * log2(e) / sqrt(HD) in fp32
(l3hip.attn_scale_q) and the caches — for query row t of sequence b and head h,
p = exp2(q~ . k_j - max) over the keys j in [0, start_pos + t] of KV head h // n_rep, normalised,
times V; for the fused-O form also parts[b, h] = Wo[:, h*HD:(h+1)*HD] @ out[b, h].

Poison (make_inputs): the slots no valid query may use hold values that show a read.  The prefill
kernel (attn_fwd_kernel) works on 16-key groups: of the last group it enters it LOADS the slots
[key_end, roundup16(key_end)), key_end = start_pos + L, and multiplies them by a probability of
exactly 0 — so it requires FINITE values there (they hold 1e30), which the reference model, slicing
the cache at key_end, does not; every slot from roundup16(key_end) on holds NaN.  The decode kernel
(attn_decode_kernel) reads exactly [0, pos], so every slot from pos + 1 on holds NaN.  This is a
recorded property of the prefill kernel, not one these tests change.

Tables: data.  Each case carries the route the dispatcher is expected to report (kernel, head
size, QBW = 16-query blocks per wave, G = heads per workgroup, KT = keys per tile, grid), written
down per position of the length list — no dispatch rule is restated here — and
tests/test_attn_dense_cpu.py checks that the expected routes cover all 42 + 12 instantiations."""

import collections
import functools

import numpy as np

import l3hip

HDS = (16, 32, 48, 64, 96, 128)
N_REPS = (1, 3, 2, 6, 4, 8)                      # query heads per KV head
G_OF = {1: 1, 3: 1, 2: 2, 6: 2, 4: 4, 8: 4}      # heads per workgroup each n_rep is expected to take
KT_OF = {16: 64, 32: 64, 48: 64, 64: 64, 96: 32, 128: 32}
PARAMS = [(hd, n_rep) for hd in HDS for n_rep in N_REPS]
FINITE_POISON = np.float32(1e30)

# A case: B sequences of L queries at start_pos in caches of smax slots; route as
# Context.op_attention reports it; D: rows of the fused O-proj (0: none)
Case = collections.namedtuple("Case", "hd n_rep kvh B L start_pos smax route D", defaults=(0,))


def _route(kernel, hd, qbw, g, kt, grid):
    return {"kernel": kernel, "hd": hd, "qbw": qbw, "g": g, "kt": kt, "grid": tuple(grid)}


# ---- prefill table -----------------------------------------------------------------------------
KVH, B_PREFILL, SMAX_PREFILL = 2, 2, 300         # 300: no multiple of 16


def prefill_lengths(g):
    """With WPH = 4 / G waves per head: one row; one 16-query block per wave, and one row more;
    two blocks per wave, and one row more; and 64 WPH + 17 — a second workgroup along x (where a
    wave holds four blocks) with padding blocks and a last block of one row."""
    w = 4 // g
    return (1, 16 * w, 16 * w + 1, 32 * w, 32 * w + 1, 64 * w + 17)


# expected per position of prefill_lengths (None: L = 1 in a cache of at most 8192 slots is the
# decode kernel's).  Head sizes up to 64 go up to four blocks per wave, 96 and 128 stay at one
_QBW_AT = {True: (None, 1, 2, 2, 4, 4), False: (None, 1, 1, 1, 1, 1)}
_GRID_X_AT = {True: {4: (None, 1, 1, 1, 1, 2), 2: (None, 1, 1, 1, 1, 2), 1: (None, 1, 1, 1, 1, 2)},
              False: {4: (None, 1, 2, 2, 3, 5), 2: (None, 1, 2, 2, 3, 5), 1: (None, 1, 2, 2, 3, 6)}}  # by WPH


def _starts(kt, L, smax):
    """{0, 1, 17, KT - 2, KT - 1, KT, smax - L}: what fits the cache (start + L <= smax), ascending;
    the last, start + L == smax, always does.  KT - 1 and KT - 2 are the two sides of the choice
    between the unmasked and the masked body (a tile's last key against a q-block's first query:
    equal, and one short)"""
    return sorted({s for s in (0, 1, 17, kt - 2, kt - 1, kt, smax - L) if s + L <= smax})


@functools.lru_cache(maxsize=None)
def prefill_cases(hd, n_rep):
    g, kt, small = G_OF[n_rep], KT_OF[hd], hd <= 64
    H, w = n_rep * KVH, 4 // G_OF[n_rep]
    out = []
    for i, L in enumerate(prefill_lengths(g)):
        qbw = _QBW_AT[small][i]
        if qbw is None:
            route = _route("decode", hd, 0, 0, 0, (H, B_PREFILL, 1))
        else:
            route = _route("prefill", hd, qbw, g, kt, (_GRID_X_AT[small][w][i], H // g, B_PREFILL))
        out += [Case(hd, n_rep, KVH, B_PREFILL, L, s, SMAX_PREFILL, route) for s in _starts(kt, L, SMAX_PREFILL)]
    return tuple(out)


# ---- long-cache table --------------------------------------------------------------------------
# L = 1: past 8192 slots the prefill kernel takes the launch (one block per wave), up to 8192 the
# decode kernel; first and last position of each.  (head size, n_rep) with KVH = 1, B = 1
LONG_SHAPES = ((16, 1), (128, 4))


@functools.lru_cache(maxsize=None)
def long_cases(hd, n_rep):
    g, kt = G_OF[n_rep], KT_OF[hd]
    pre = _route("prefill", hd, 1, g, kt, (1, n_rep // g, 1))
    dec = _route("decode", hd, 0, 0, 0, (n_rep, 1, 1))
    return (Case(hd, n_rep, 1, 1, 1, 0, 8193, pre), Case(hd, n_rep, 1, 1, 1, 8192, 8193, pre),
            Case(hd, n_rep, 1, 1, 1, 0, 8192, dec), Case(hd, n_rep, 1, 1, 1, 8191, 8192, dec))


# ---- decode and fused-O tables -----------------------------------------------------------------
SMAX_DECODE, B_DECODE = 700, 2
ROWS_OF = {16: 64, 32: 32, 48: 21, 64: 16, 96: 10, 128: 8}   # R = 256 // (HD / 4) key rows per P.V pass
VP = 8                                                       # V rows a thread prefetches


def decode_lengths(hd):
    """S = pos + 1 at the edges of the kernel's passes: one key, one P.V pass of R rows and one
    more, the VP prefetched passes and one more, one score pass of 256 threads and one more, and
    the whole cache"""
    r = ROWS_OF[hd]
    return sorted({1, r, r + 1, VP * r, VP * r + 1, 256, 257, SMAX_DECODE})


@functools.lru_cache(maxsize=None)
def decode_cases(hd, n_rep):
    H = n_rep * KVH
    route = _route("decode", hd, 0, 0, 0, (H, B_DECODE, 1))
    return tuple(Case(hd, n_rep, KVH, B_DECODE, 1, s - 1, SMAX_DECODE, route) for s in decode_lengths(hd))


FUSED_D = (4, 64, 68, 192)   # one partial block of 64 rows; a full one; a full and a partial one; three
_GRID_Z_AT = {4: 1, 64: 1, 68: 2, 192: 3}


@functools.lru_cache(maxsize=None)
def fused_cases(hd, n_rep):
    """D x B, each pair at another of the decode lengths"""
    H, lens = n_rep * KVH, decode_lengths(hd)
    out = []
    for i, (D, B) in enumerate((D, B) for D in FUSED_D for B in (1, 2)):
        route = _route("decode_oproj", hd, 0, 0, 0, (H, B, _GRID_Z_AT[D]))
        out.append(Case(hd, n_rep, KVH, B, 1, lens[i % len(lens)] - 1, SMAX_DECODE, route, D))
    return tuple(out)


# ---- last-rows table ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def last_cases(hd, n_rep):
    """the last-rows launch: always one block per wave and one workgroup along x"""
    g, kt = G_OF[n_rep], KT_OF[hd]
    H, qw = n_rep * KVH, 16 * (4 // g)
    route = _route("prefill", hd, 1, g, kt, (1, H // g, B_PREFILL))
    return tuple(Case(hd, n_rep, KVH, B_PREFILL, L, s, SMAX_PREFILL, route)
                 for L in (qw - 1, qw, qw + 1, 4 * qw + 17) for s in (0, 17))


# ---- inputs ------------------------------------------------------------------------------------
def poison(case, ck, cv):
    """the poison layout of the module docstring, by the kernel the case expects"""
    key_end = case.start_pos + case.L
    for c in (ck, cv):
        if case.route["kernel"] == "prefill":
            up = (key_end + 15) // 16 * 16
            c[:, :, key_end:up] = FINITE_POISON
            c[:, :, up:] = np.nan
        else:
            c[:, :, key_end:] = np.nan


def _seed(case):
    return [case.hd, case.n_rep, case.L, case.start_pos, case.smax, case.B, case.D]


def make_inputs(case):
    """N(0, 1) q [B, L, H * HD] (plain: the wrapper scales it), K and V [B, KVH, smax, HD] with the
    poison in place, and for a fused case wo [D, H * HD] ~ N(0, 1).  q_s: q as the kernel gets it"""
    rng = np.random.default_rng(_seed(case))
    H = case.n_rep * case.kvh
    q = rng.standard_normal((case.B, case.L, H * case.hd)).astype(np.float32)
    ck = rng.standard_normal((case.B, case.kvh, case.smax, case.hd)).astype(np.float32)
    cv = rng.standard_normal((case.B, case.kvh, case.smax, case.hd)).astype(np.float32)
    poison(case, ck, cv)
    inp = dict(q=q, q_s=l3hip.attn_scale_q(q, case.hd), cache_k=ck, cache_v=cv, n_heads=H, start_pos=case.start_pos)
    if case.D:
        inp["wo"] = rng.standard_normal((case.D, H * case.hd)).astype(np.float32)
    return inp


def census_inputs(case):
    """q = 0, K as make_inputs, V[b, g, j, d] = 1 if d == j % HD else 0: every score is 0, every
    live p exactly 1, and out[t, h, d] * (start_pos + t + 1) counts the keys j <= start_pos + t
    with j % HD == d"""
    inp = make_inputs(case)
    inp["q"] = np.zeros_like(inp["q"])
    inp["q_s"] = inp["q"]
    j = np.arange(case.smax)
    v = np.zeros((case.smax, case.hd), np.float32)
    v[j, j % case.hd] = 1.0
    cv = np.broadcast_to(v, inp["cache_v"].shape).copy()
    ck = inp["cache_k"]
    poison(case, ck, cv)
    inp["cache_v"] = cv
    return inp


def census(case):
    """[L, HD] int64: keys j <= start_pos + t with j % HD == d"""
    n = case.start_pos + np.arange(case.L)[:, None] + 1      # keys of row t
    d = np.arange(case.hd)[None, :]
    return (n - d + case.hd - 1) // case.hd                  # d, d + HD, ... below n


STRESS = ("rising", "falling", "spike_low", "spike_high")


def stress_inputs(case, shape):
    """Scores exact in fp32: q~ = e_0 for every head (passed scaled), so the score of key j is
    K[..., j, 0] — a ramp j / 2 (every tile raises the running max: alpha < 1 throughout), -j / 2
    (the max sits in tile 0, later tiles underflow towards 0), or one key 40 above a flat rest:
    in the middle of tile 0 (unmasked for every later q-block), or of the last tile a query
    reaches (its diagonal tile).  The other K components and V are N(0, 1)"""
    inp = make_inputs(case)
    H, kt = inp["n_heads"], KT_OF[case.hd]
    q = np.zeros((case.B, case.L, H, case.hd), np.float32)
    q[..., 0] = 1.0
    key_end = case.start_pos + case.L
    j = np.arange(key_end, dtype=np.float32)
    if shape == "rising":
        s = j / 2
    elif shape == "falling":
        s = -j / 2
    else:
        at = kt // 2 + 5 if shape == "spike_low" else min((key_end - 1) // kt * kt + kt // 2 + 5, key_end - 2)
        s = np.zeros(key_end, np.float32)
        s[max(at, 0)] = 40.0
    inp["cache_k"][:, :, :key_end, 0] = s
    inp["q"] = inp["q_s"] = q.reshape(case.B, case.L, H * case.hd)
    return inp


# ---- reference ---------------------------------------------------------------------------------
def reference(q_s, cache_k, cache_v, start_pos, n_heads):
    """out [B, L, H * HD] fp64 from the scaled queries and the caches, sliced at start_pos + L"""
    B, kvh, _, hd = cache_k.shape
    L, n_rep = q_s.shape[1], n_heads // kvh
    S = start_pos + L
    q = q_s.astype(np.float64).reshape(B, L, kvh, n_rep, hd).transpose(0, 2, 3, 1, 4)      # [B, g, r, L, d]
    k = cache_k[:, :, None, :S].astype(np.float64)                                          # [B, g, 1, S, d]
    v = cache_v[:, :, None, :S].astype(np.float64)
    s = q @ k.transpose(0, 1, 2, 4, 3)                                                      # [B, g, r, L, S]
    live = np.arange(S)[None, :] <= start_pos + np.arange(L)[:, None]
    s = np.where(live, s, -np.inf)
    p = np.exp2(s - s.max(axis=-1, keepdims=True))
    o = (p / p.sum(axis=-1, keepdims=True)) @ v                                             # [B, g, r, L, d]
    return o.transpose(0, 3, 1, 2, 4).reshape(B, L, n_heads * hd)


def reference_parts(out, wo, n_heads):
    """parts [B, H, D] fp64: head h's share of the O-proj of decode rows out [B, H * HD]"""
    B = out.shape[0]
    D = wo.shape[0]
    o = np.asarray(out, np.float64).reshape(B, n_heads, -1)
    w = wo.astype(np.float64).reshape(D, n_heads, -1)
    return np.einsum("dhe,bhe->bhd", w, o)


def reference_masked(q_s, cache_k, cache_v, start_pos, n_heads):
    """The reference model's own formulation (oracle/llama3_oracle.py attention): the queries
    un-scaled, repeat_kv, softmax(q k^T / sqrt(HD) + mask) @ v over the full score matrix"""
    import llama3_oracle as orc
    B, kvh, _, hd = cache_k.shape
    L, n_rep = q_s.shape[1], n_heads // kvh
    end = start_pos + L
    q = (q_s.astype(np.float64) * (np.sqrt(hd) / np.log2(np.e))).reshape(B, L, n_heads, hd)
    keys = orc.repeat_kv(cache_k[:, :, :end].astype(np.float64).transpose(0, 2, 1, 3), n_rep)   # [B, end, H, d]
    vals = orc.repeat_kv(cache_v[:, :, :end].astype(np.float64).transpose(0, 2, 1, 3), n_rep)
    scores = q.transpose(0, 2, 1, 3) @ keys.transpose(0, 2, 3, 1) / np.sqrt(hd)                 # [B, H, L, end]
    mask = np.concatenate([np.zeros((L, start_pos)), np.triu(np.full((L, L), -np.inf), k=1)], axis=1)
    o = orc.softmax(scores + mask[None, None]) @ vals.transpose(0, 2, 1, 3)
    return o.transpose(0, 2, 1, 3).reshape(B, L, n_heads * hd)
