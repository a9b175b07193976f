"""NumPy reference and case tables of the captured-decode GEMV arguments (test infrastructure for
tests/test_decode_gemv_cpu.py, tests/test_gpu_decode_gemv.py and tests/decode_gemv_checks_workload.py;
DESIGN.md "Captured-decode GEMV arguments at kernel level").

Written from the reference model's semantics (llama3.py:312-320: the greedy id is np.argmax of the
last logits; :253 / :259: the residual adds), not from the kernels:

* the argmax rule is np.argmax's — the first index of the maximum, the first NaN wins, -0 == +0.  A
  per-block / per-tile partial is (value, first index) over that block's valid columns; an empty
  candidate is (-inf, 0x7fffffff); a reduction over candidates picks the NaN of the lowest index if
  there is one, else the largest value at its lowest index.
* the O-proj partial rows are summed in fp32, sequentially in head order: EPI_SWIGLU's input row is
  (((x + p0) + p1) + ...), EPI_RESID's output ((res + p0) + p1 + ...) + acc.
* with bf16 / fp8 storage the weights are the dequantised ones: float(bf16), scale * code.

Operands are small integers, so every dot product is exact in fp32 in any order and equals the
float64 one; `exact_logits` asserts that.  Each case carries its expected route: the family, the rows
per block and the lanes per unit, restated here from K and the storage (`lanes_for`).
"""

import functools
import itertools

import numpy as np

import gemm_epi_ref as epi_ref
import utils

PART = np.dtype([("v", "<f4"), ("i", "<i4")])
EMPTY_I = 0x7FFFFFFF
KS = (64, 288, 1024, 2048)  # the K of every GEMV case ...
# ... but the partial-rows forms of the compact storages: bf16 counts K / 8 pieces and fp8 K / 16, so
# EPI_RESID's 64-lane form (more than 256 pieces) needs K = 4096 in bf16 and K = 8192 in fp8, its fp8
# 32-lane form and EPI_SWIGLU's fp8 64-lane form (more than 128) K = 4096.  The weights stay tiny
# (N = 36 / 64); these are the forms a dim-4096 / dim-8192 model runs on every decode step.
PARTS_KS_COMPACT = (4096, 8192)
GEMV_LDS_K = 16384  # the GEMV range: (M rounded up to 1 / 2 / 4 / 8) * K <= 16384 (the A rows fit 64 KB of LDS)
PARTS_LANES = {"parts_swiglu": [32, 64], "parts_resid": [16, 32, 64]}  # the dispatcher's own, per storage
PIECE = {"fp32": 4, "bf16": 8, "fp8": 16}  # k per 16-byte piece of a weight row
FAMILY = {"fp32": "gemv", "bf16": "gemv_bf16", "fp8": "gemv_fp8"}
STORAGES = ("fp32", "bf16", "fp8")
KV_BAK_SLOTS = 32
SMALL_W = 4 << 20  # the GEMV's small-weight bound (elements)


def lanes_for(form, storage, K):
    """Lanes per unit of a one-row GEMV form: by the count of 16-byte pieces of a weight row — 16 up
    to 128 pieces, 32 up to 256, else 64; EPI_SWIGLU with partial rows has no 16-lane form."""
    pieces = K // PIECE[storage]
    if form == "parts_swiglu":
        return 32 if pieces <= 128 else 64
    return 16 if pieces <= 128 else 32 if pieces <= 256 else 64


def gemv_rows(K, want=3):
    """The rows of a multi-row case at this K: `want`, or the most the GEMV range holds."""
    for M in range(want, 0, -1):
        mr = 1 if M <= 1 else 2 if M <= 2 else 4 if M <= 4 else 8
        if mr * K <= GEMV_LDS_K:
            return M


def units_per_block(lanes):
    return 4 * (64 // lanes)  # four waves of 64 / lanes units


def gemv_route(storage, lanes, rows_per_block=1, row_blocks=1):
    return {"family": FAMILY[storage], "rows_per_block": rows_per_block, "lanes_per_unit": lanes, "nt": 0,
            "row_blocks": row_blocks, "launches": 1}


# ---- the argmax rule ---------------------------------------------------------------------------

def first_argmax(v):
    """np.argmax itself: first index of the maximum, the first NaN wins, -0 == +0."""
    return int(np.argmax(np.asarray(v)))


def partials(row, group, n_groups=None):
    """(value, first index) of each run of `group` columns of a logits row (the last may be short);
    groups past the row are empty candidates."""
    row = np.asarray(row, np.float32)
    n = -(-row.shape[0] // group) if n_groups is None else n_groups
    out = np.empty(n, PART)
    for b in range(n):
        seg = row[b * group:(b + 1) * group]
        if seg.size == 0:
            out[b] = (-np.inf, EMPTY_I)
        else:
            j = first_argmax(seg)
            out[b] = (seg[j], b * group + j)
    return out


def reduce_parts(parts):
    """(value, index) of a row of candidates: the NaN of the lowest index, else the largest value
    at its lowest index (what np.argmax gives on the row the candidates were taken from)."""
    p = np.asarray(parts, PART)
    v, i = p["v"], p["i"].astype(np.int64)
    nan = np.isnan(v)
    pool = np.flatnonzero(nan) if nan.any() else np.flatnonzero(v == v.max())
    k = pool[np.argmin(i[pool])]
    return p["v"][k], int(p["i"][k])


# ---- weights as stored -------------------------------------------------------------------------

def dequant(w, storage):
    """The weights a storage form computes with."""
    w = np.asarray(w, np.float32)
    if storage == "fp32":
        return w
    if storage == "bf16":
        return utils.round_bf16(w)
    codes, scale = utils.quant_fp8_rows(w)
    return (utils.fp8_e4m3_table()[codes] * scale[:, None]).astype(np.float32)


def exact_logits(x, w, norm_w=None, factor=1.0):
    """factor * ((x * norm_w) @ w.T) in float64, asserted to be what fp32 gives in ANY summation
    order: every |product| partial sum stays an integer multiple of 2^-2 below 2^22.  Rows with a
    non-finite weight are exempt (their logits are non-finite whatever the order)."""
    x64 = np.asarray(x, np.float64) * (1.0 if norm_w is None else np.asarray(norm_w, np.float64))
    w64 = np.asarray(w, np.float64)
    fin = np.isfinite(w64).all(axis=1)
    assert np.all(x64 * 4 == np.rint(x64 * 4)) and np.all(w64[fin] == np.rint(w64[fin]))
    assert (np.abs(x64) @ np.abs(w64[fin]).T).max(initial=0.0) < 2.0 ** 22
    with np.errstate(invalid="ignore", over="ignore"):
        z = factor * (x64 @ w64.T)
    z32 = z.astype(np.float32)
    assert np.array_equal(z32[:, fin].astype(np.float64), z[:, fin])
    return z32


def sum_parts_f32(base, parts):
    """((base + p0) + p1) + ... in fp32, head order.  base [M, D], parts [M, P, D]."""
    acc = np.asarray(base, np.float32).copy()
    for h in range(parts.shape[1]):
        acc = (acc + np.asarray(parts[:, h], np.float32)).astype(np.float32)
    return acc


def _seed(*key):
    s = 0
    for k in key:
        for ch in str(k):
            s = (s * 131 + ord(ch)) % (1 << 31)
    return s


# ---- A. amax_part on the one-row EPI_STORE GEMV -------------------------------------------------

class AmaxCase:
    def __init__(self, storage, K, norm):
        self.storage, self.K, self.norm = storage, K, norm
        self.lanes = lanes_for("store", storage, K)
        self.upb = units_per_block(self.lanes)
        self.upw = 64 // self.lanes
        self.N = 5 * self.upb + 4  # five full blocks and four columns (lanes 64: six full blocks)
        self.blocks = -(-self.N // self.upb)
        self.route = gemv_route(storage, self.lanes)

    @property
    def id(self):
        return f"{self.storage}-K{self.K}-l{self.lanes}-{'norm' if self.norm else 'plain'}"


AMAX_CASES = [AmaxCase("fp32", K, norm) for K, norm in
              ((288, False), (64, True), (1024, False), (1024, True), (2048, False), (2048, True))] + \
             [AmaxCase("bf16", 2048, False), AmaxCase("bf16", 2048, True),
              AmaxCase("fp8", 1024, False), AmaxCase("fp8", 1024, True)]


def amax_scenarios(case):
    """[(name, planted columns, kind)]: kind 'win' — the planted columns all hold the row's unique
    maximum (several: a tie, the lowest wins); the edge kinds are built by amax_inputs."""
    upb, upw, N = case.upb, case.upw, case.N
    s = [("col0", [0]), ("last_of_block0", [upb - 1]), ("first_of_block1", [upb]), ("last_valid", [N - 1])]
    s += [(f"wave{k}_of_block2", [2 * upb + k * upw]) for k in range(4)]
    if upw >= 2:  # two units in one wave
        s.append(("tie_in_unit_group", [3 * upb, 3 * upb + 1]))
    s.append(("tie_across_waves", [3 * upb + upw - 1, 3 * upb + upw]))
    s.append(("tie_across_blocks", [upb + 1, 4 * upb + 1]))
    out = [(n, c, "win") for n, c in s]
    if case.storage != "fp8" and not case.norm:
        out += [("zero_rows", [1, upb + 2], "zeros"), ("nan_before_inf", [2, 2 * upb + 1], "nan_inf"),
                ("nan_after_inf", [2 * upb + 1, 2], "nan_inf"), ("neginf_block", [upb], "neginf")]
    return out


def amax_inputs(case, scen):
    """x [1, K], w [N, K], norm_w (or None), eps and the expected global winner of one scenario."""
    name, cols, kind = scen
    rng = np.random.default_rng(_seed("amax", case.id, name))
    K, N = case.K, case.N
    edge = kind != "win"
    if case.norm:
        x = rng.choice([-2.0, 2.0], (1, K)).astype(np.float32)
    elif edge:
        x = rng.integers(1, 3, (1, K)).astype(np.float32)  # strictly positive: no 0 * inf
    else:
        x = rng.integers(-2, 3, (1, K)).astype(np.float32)
        x[0, :2] = (1.0, -2.0)
    w = rng.integers(-1, 2, (N, K)).astype(np.float32)
    norm_w = None
    if case.norm and case.storage != "fp32":
        norm_w = rng.choice([0.5, 1.0, 2.0], K).astype(np.float32)
    if kind == "win":
        w[cols] = 2.0 * np.sign(x[0])
        winner = min(cols)
    elif kind == "zeros":
        w[:] = -np.abs(w)  # every logit <= 0 ...
        w[:, 0] = -1.0     # ... and < 0
        w[cols] = 0.0      # zero rows: logit 0
        c2 = cols[1] + 1   # a row that cancels to 0: +1, -1 on two equal x
        x[0, 4] = x[0, 5]
        w[c2] = 0.0
        w[c2, 4:6] = (1.0, -1.0)
        winner = min(cols)
    elif kind == "nan_inf":
        w[cols[0], K // 2] = np.nan
        w[cols[1], K - 1] = np.inf
        winner = cols[0]
    else:
        w[cols[0]:cols[0] + case.upb, 3] = -np.inf  # all of one block
        w[0] = 2.0
        winner = 0
    return x, w, norm_w, 0.0, winner


def amax_reference(case, x, w, norm_w):
    """(logits [N] float32, per-block partials): the row factor of x = +-2 with eps 0 is exactly 0.5."""
    z = exact_logits(x, dequant(w, case.storage) if np.isfinite(w).all() else w, norm_w, 0.5 if case.norm else 1.0)[0]
    return z, partials(z, case.upb)


# ---- B. argmax_parts_kernel --------------------------------------------------------------------

PARTS_N = (1, 5, 1024, 4096, 4097, 9000)
PARTS_WINNERS = (0, 1023, 1024, 4095, 4096, -1)  # -1: n - 1
PARTS_PASS = 4096  # candidates per pass of the reducer


def _base_table(rng, n):
    t = np.empty(n, PART)
    t["v"] = rng.integers(-100, 100, n).astype(np.float32)
    t["i"] = 7 + 2 * np.arange(n)
    return t


def argmax_tables():
    """[(name, table [n], (value, index))]: planted winners at every listed position of every n,
    then ties, signed zeros and NaNs across the pass boundary."""
    out = []
    for n in PARTS_N:
        for wpos in sorted({n - 1 if p < 0 else p for p in PARTS_WINNERS if p < n}):
            t = _base_table(np.random.default_rng(_seed("tab", n, wpos)), n)
            t["v"][wpos] = 1000.0
            out.append((f"n{n}-win{wpos}", t))
    for n in (4097, 9000):
        r = np.random.default_rng(_seed("tie", n))
        t = _base_table(r, n); t["v"][[4095, 4096]] = 500.0; out.append((f"n{n}-tie-across-pass", t))
        t = _base_table(r, n); t["v"][[4095, 4096]] = 500.0; t["i"] = t["i"][::-1].copy()
        out.append((f"n{n}-tie-lower-index-later", t))
        t = _base_table(r, n); t["v"][[10, n - 1]] = 500.0; out.append((f"n{n}-tie-first-last", t))
        t = _base_table(r, n); t["v"][4096] = np.nan; t["v"][3] = np.inf; out.append((f"n{n}-nan-after-inf", t))
        t = _base_table(r, n); t["v"][[4095, 4096]] = np.nan; out.append((f"n{n}-nan-pair-across-pass", t))
        t = _base_table(r, n); t["v"][100] = np.nan; t["v"][4096] = np.inf; out.append((f"n{n}-nan-before-inf", t))
        t = _base_table(r, n); t["v"] = -np.abs(t["v"]) - 1; t["v"][4096] = -0.0; t["v"][4090] = 0.0
        out.append((f"n{n}-signed-zeros", t))
        t = _base_table(r, n); t["v"][:] = -np.inf; out.append((f"n{n}-all-neginf", t))
        t = _base_table(r, n); t["v"][:] = -np.inf; t["i"][:4096] = EMPTY_I; out.append((f"n{n}-empties-first-pass", t))
    return [(name, t, reduce_parts(t)) for name, t in out]


# (pos, hist_base, hist_cap, slot written or None)
STATE_CASES = [(10, 4, 8, 6), (10, 10, 8, 0), (10, 3, 8, 7), (10, 11, 8, None), (10, 2, 8, None), (0, 0, 4, 0)]


def hist_slot(pos, hist_off, base, cap):
    q = pos - hist_off - base
    return q if 0 <= q < cap else None


# ---- C. amax_rows on the tiled EPI_STORE kernels ------------------------------------------------

TILE = 64
TILED_BM = {1: 32, 2: 64, 3: 128}


class RowsCase:
    def __init__(self, M, N, K, force, norm, edge=False):
        self.M, self.N, self.K, self.force, self.norm, self.edge = M, N, K, force, norm, edge
        cfg = force or (1 if M <= 32 else 2 if M <= 64 else 3)
        self.route = {"family": "tiled", "bm": TILED_BM[cfg], "bn": 128, "bk": 16}
        self.nct = -(-N // TILE)

    @property
    def id(self):
        return f"M{self.M}-N{self.N}-K{self.K}-f{self.force}{'-norm' if self.norm else ''}{'-edge' if self.edge else ''}"


ROWS_CASES = [RowsCase(M, N, 64, f, N == 200) for f in (1, 2, 3) for M in (1, 17, 33, 70) for N in (192, 200)] + \
             [RowsCase(17, 200, 64, f, False, edge=True) for f in (1, 2, 3)] + \
             [RowsCase(M, 2052, 2048, 0, True) for M in (9, 40, 70)]  # 2052 * 2048 > SMALL_W: chosen by shape

# offsets in a 64-column tile: each 16-column group, each lane quarter, both ends
ROWS_OFFSETS = (0, 63, 5, 18, 35, 52, 15, 16, 47, 48)
ROWS_TIES = ((1, 2), (4, 8), (9, 25), (40, 40 + TILE))  # one lane; two lanes; two groups; two tiles


def rows_plan(case):
    """Row r of the launch -> the columns that hold its planted maximum (several: a tie; none: the
    row is left random).  No two rows share a column.  Row 0's only maximum is the last valid
    column, in the partial last tile where N has one."""
    N = case.N
    plans = [[N - 1], [0], [TILE - 1], [TILE], [N - 3, N - 2]]
    plans += [[a, b] for a, b in ROWS_TIES if b < N - 3]
    plans += [[t * TILE + o] for t, o in zip(itertools.cycle(range(case.nct)), ROWS_OFFSETS) if t * TILE + o < N - 3]
    used, out = set(), []
    for p in plans:
        if not used & set(p):
            used |= set(p)
            out.append(p)
    return [out[r] if r < len(out) else [] for r in range(case.M)]


def rows_inputs(case):
    """x [M, K], w [N, K]: row r's planted columns are w = 2 sign(x[r]), its unique maximum."""
    rng = np.random.default_rng(_seed("rows", case.id))
    M, N, K = case.M, case.N, case.K
    if case.norm:
        x = rng.choice([-2.0, 2.0], (M, K)).astype(np.float32)
    elif case.edge:
        x = rng.integers(1, 3, (M, K)).astype(np.float32)
    else:
        x = rng.integers(-2, 3, (M, K)).astype(np.float32)
        x[:, 0] = 1.0
    w = rng.integers(-1, 2, (N, K)).astype(np.float32)
    plan = rows_plan(case)
    if case.edge:  # non-finite columns, the same for every row: NaN before / after +inf, a -inf tile
        w[3, 1] = np.nan; w[40, 2] = np.inf          # tile 0: the NaN wins
        w[TILE + 9, 1] = np.inf; w[TILE + 30, 2] = np.nan  # tile 1: the NaN wins
        w[2 * TILE:3 * TILE, 5] = -np.inf            # tile 2: all -inf, its first column
        w[N - 2, 0] = np.inf                          # the partial tile: +inf
        return x, w, plan
    for r, cols in enumerate(plan):
        if cols:
            w[cols] = 2.0 * np.sign(x[r])
    return x, w, plan


def rows_reference(case, x, w):
    z = exact_logits(x, w, None, 0.5 if case.norm else 1.0)
    rec = np.stack([partials(z[r], TILE, case.nct) for r in range(case.M)])
    return z, rec


# ---- D. the O-proj partial rows ------------------------------------------------------------------

class PartsCase:
    def __init__(self, epi, storage, K, nparts, M=1, kind="int", norm=False):
        self.epi, self.storage, self.K, self.nparts, self.M, self.kind, self.norm = epi, storage, K, nparts, M, kind, norm
        form = "parts_swiglu" if epi == epi_ref.SWIGLU else "parts_resid"
        self.lanes = lanes_for(form, storage, K)
        self.N = 64 if epi == epi_ref.SWIGLU else 36  # units: 32 / 36, more than one block, the last one short
        self.route = gemv_route(storage, self.lanes, 1, M)

    @property
    def id(self):
        e = "swiglu" if self.epi == epi_ref.SWIGLU else "resid"
        return f"{e}-{self.storage}-K{self.K}-l{self.lanes}-p{self.nparts}-M{self.M}-{self.kind}{'-norm' if self.norm else ''}"


def _parts_cases():
    out = []
    # a K for every lane count of each form and storage (PARTS_LANES)
    ks = {(epi_ref.SWIGLU, "fp32"): (288, 1024, 2048), (epi_ref.SWIGLU, "bf16"): (1024, 2048), (epi_ref.SWIGLU, "fp8"): (2048, 4096),
          (epi_ref.RESID, "fp32"): (288, 1024, 2048), (epi_ref.RESID, "bf16"): (1024, 2048, 4096),
          (epi_ref.RESID, "fp8"): (1024, 4096, 8192)}
    for (epi, st), kk in ks.items():
        for K in kk:
            for P in (1, 3, 8):
                out.append(PartsCase(epi, st, K, P))
                if P > 1:  # (one part has one order)
                    out.append(PartsCase(epi, st, K, P, kind="order"))
            # three rows; two at K = 8192, where four staged rows are past the GEMV range
            out.append(PartsCase(epi, st, K, 3, M=gemv_rows(K)))
            out.append(PartsCase(epi, st, K, 3, M=gemv_rows(K), kind="order"))
            if epi == epi_ref.SWIGLU:
                out.append(PartsCase(epi, st, K, 3, norm=True))
    return out


PARTS_CASES = _parts_cases()
# the same x and parts under every storage: x_out must not depend on it
PARTS_XOUT_K = 2048

# Parts of one element whose fp32 sum depends on the order: added to 1 in sequence, the first three
# and all eight come back to a small integer (1 + 2^24 rounds to 2^24, and so on), and any other
# order or a pairwise tree gives another one
ORDER_PATTERNS = np.array([
    [2.0 ** 24, 1, -2.0 ** 24, 1, 2.0 ** 24, 1, -2.0 ** 24, 1],
    [-2.0 ** 24, -1, 2.0 ** 24, 2.0 ** 25, 3, 1, -2.0 ** 25, 2],
    [1, 2.0 ** 24, -2.0 ** 24, 2.0 ** 24, 1, 1, -2.0 ** 24, 1],
    [2.0 ** 25, 3, -2.0 ** 25, 1, -2.0 ** 24, -1, 2.0 ** 24, 2],
], np.float32)


def parts_inputs(case, storage=None):
    """x [M, K], the weight(s), c0 [M, N] (EPI_RESID's residual), parts [M, P, D], norm_w."""
    st = storage or case.storage
    rng = np.random.default_rng(_seed("parts", case.epi, case.K, case.nparts, case.M, case.kind, case.norm))
    M, K, N, P = case.M, case.K, case.N, case.nparts
    swiglu = case.epi == epi_ref.SWIGLU
    D = K if swiglu else N
    x = rng.integers(-1, 2, (M, K)).astype(np.float32)
    if case.kind == "order":
        pick = rng.integers(0, len(ORDER_PATTERNS), (M, D))
        parts = np.ascontiguousarray(np.moveaxis(ORDER_PATTERNS[pick][..., :P], -1, 1))
        base = np.ones((M, D), np.float32)
    else:
        parts = rng.integers(-1, 2, (M, P, D)).astype(np.float32)
        base = None
    out = {"parts": parts}
    if swiglu:
        if base is not None:
            x = base
        nh = N // 2
        wg = np.zeros((nh, K), np.float32)
        wg[:, :8] = rng.integers(-1, 2, (nh, 8))
        wg[:, -8:] = rng.integers(-1, 2, (nh, 8))
        out.update(x=x, wg=wg, wu=rng.integers(-1, 2, (nh, K)).astype(np.float32))
    else:
        c0 = rng.integers(-3, 4, (M, N)).astype(np.float32) if base is None else base
        out.update(x=x, w=rng.integers(-2, 3, (N, K)).astype(np.float32), c0=c0)
    out["norm_w"] = rng.choice([0.5, 1.0, 2.0], K).astype(np.float32) if case.norm and st != "fp32" else None
    return out


def parts_reference(case, inp):
    """EPI_SWIGLU: (x_sum float32 [M, K], out float64, bound); EPI_RESID: (None, out float32, None),
    bit exact."""
    if case.epi == epi_ref.SWIGLU:
        xs = sum_parts_f32(inp["x"], inp["parts"])
        g = 1.0 if inp["norm_w"] is None else inp["norm_w"].astype(np.float64)
        out, bound, _ = epi_ref.ref_swiglu(xs.astype(np.float64), inp["wg"] * g, inp["wu"] * g, norm=case.norm, eps=1e-5)
        if not case.norm:  # exact sums: only silu_f's own error is left
            gg = exact_logits(xs, inp["wg"]).astype(np.float64)
            uu = exact_logits(xs, inp["wu"]).astype(np.float64)
            bound = epi_ref.swiglu_own_bound(gg, uu)
        return xs, out, bound
    acc = exact_logits(inp["x"], inp["w"])
    res = sum_parts_f32(inp["c0"], inp["parts"])
    return None, (res + acc).astype(np.float32), None


# ---- E. the folded argmax (layer 0's one-row QKV) ------------------------------------------------

FOLD_N = (1, 7, 2000, 2048, 2049, 4096)
FOLD_WINNERS = (0, 255, 256, 2047, 2048, -1)
FOLD_PASS = 2048  # candidates per pass of the fold
FOLD_GEO = dict(H=2, KVH=1, HD=32)  # N = 128: 64 RoPE pairs
FOLD_VOCAB = 48
FOLD_SMAX = 12


class FoldCase:
    def __init__(self, storage, K):
        self.storage, self.K = storage, K
        self.lanes = lanes_for("fold", storage, K)
        self.N = (FOLD_GEO["H"] + 2 * FOLD_GEO["KVH"]) * FOLD_GEO["HD"]
        self.route = gemv_route(storage, self.lanes)

    @property
    def id(self):
        return f"{self.storage}-K{self.K}-l{self.lanes}"


FOLD_CASES = [FoldCase("fp32", 288), FoldCase("fp32", 1024), FoldCase("fp32", 2048), FoldCase("bf16", 2048),
              FoldCase("fp8", 1024)]


def _fold_base(rng, n):
    t = np.empty(n, PART)
    t["v"] = rng.integers(-100, 100, n).astype(np.float32)
    t["i"] = rng.integers(0, FOLD_VOCAB, n)
    return t


def fold_tables():
    """[(name, candidates [n], (value, id))]: the sweep of n and winner position, then ties, signed
    zeros and NaNs across the pass boundary.  Every index is a row of the FOLD_VOCAB-row table."""
    out = []
    for n in FOLD_N:
        for wpos in sorted({n - 1 if p < 0 else p for p in FOLD_WINNERS if p < n}):
            rng = np.random.default_rng(_seed("fold", n, wpos))
            t = _fold_base(rng, n)
            t["v"][wpos] = 1000.0
            t["i"][wpos] = 1 + (wpos * 7 + n) % (FOLD_VOCAB - 1)
            out.append((f"n{n}-win{wpos}", t))
    for n in (2049, 4096):
        r = np.random.default_rng(_seed("foldtie", n))
        t = _fold_base(r, n); t["v"][[2047, 2048]] = 500.0; t["i"][[2047, 2048]] = (9, 5); out.append((f"n{n}-tie-lower-after", t))
        t = _fold_base(r, n); t["v"][[2047, 2048]] = 500.0; t["i"][[2047, 2048]] = (5, 9); out.append((f"n{n}-tie-lower-before", t))
        t = _fold_base(r, n); t["v"][2048] = np.nan; t["i"][2048] = 11; t["v"][0] = np.inf; out.append((f"n{n}-nan-after-inf", t))
        t = _fold_base(r, n); t["v"][[2047, 2048]] = np.nan; t["i"][[2047, 2048]] = (13, 4); out.append((f"n{n}-nan-pair", t))
        t = _fold_base(r, n); t["v"] = -np.abs(t["v"]) - 1; t["v"][[2040, 2048]] = (0.0, -0.0); t["i"][[2040, 2048]] = (20, 6)
        out.append((f"n{n}-signed-zeros", t))
        t = _fold_base(r, n); t["v"][:] = -np.inf; t["i"][:] = 1 + np.arange(n) % (FOLD_VOCAB - 1); t["i"][n - 1] = 0
        out.append((f"n{n}-all-neginf", t))
    return [(name, t, reduce_parts(t)) for name, t in out]


def fold_operands(case):
    """The embedding table [FOLD_VOCAB, K] (pairwise distinct rows of +-2), wqkv [N, K] and norm_w."""
    rng = np.random.default_rng(_seed("foldop", case.id))
    tab = rng.choice([-2.0, 2.0], (FOLD_VOCAB, case.K)).astype(np.float32)
    w = rng.integers(-2, 3, (case.N, case.K)).astype(np.float32)
    norm_w = rng.choice([0.5, 1.0, 2.0], case.K).astype(np.float32) if case.storage != "fp32" else None
    return tab, w, norm_w


# (pos, hist_base, hist_cap): the id belongs at slot pos - 1 - hist_base
FOLD_STATES = [(5, 0, 8), (5, 4, 8), (5, 5, 8), (8, 0, 8), (9, 0, 8), (1, 0, 1)]


# ---- F. the undo slots ---------------------------------------------------------------------------

KV_SMAX = 40
KV_POS = (0, 31, 32, 33, KV_SMAX - 1)


class KvCase:
    def __init__(self, B, K, H, KVH, HD, rows_per_block):
        self.B, self.K, self.H, self.KVH, self.HD, self.rpb = B, K, H, KVH, HD, rows_per_block
        self.N = (H + 2 * KVH) * HD
        self.big = self.N * K > SMALL_W
        lanes = lanes_for("store", "fp32", K)
        self.route = gemv_route("fp32", lanes, rows_per_block, -(-B // rows_per_block))

    @property
    def id(self):
        return f"B{self.B}-K{self.K}-H{self.H}-KVH{self.KVH}-HD{self.HD}-rpb{self.rpb}"


# a small weight: one row per block, grid.y = B; past the small-weight bound: 2 / 4 / 8-row blocks
# (eight staged rows of K = 4096 exceed the GEMV's 64 KB of LDS, so B = 8 takes K = 2048)
KV_CASES = [KvCase(1, 64, 2, 1, 32, 1), KvCase(3, 288, 2, 2, 64, 1), KvCase(8, 64, 4, 2, 32, 1),
            KvCase(2, 4096, 16, 2, 64, 2), KvCase(4, 4096, 32, 1, 32, 4), KvCase(8, 2048, 40, 2, 64, 8)]


def kv_positions(case):
    """[(pos, from the device word?)]: every position from both sources against a small weight, the
    sources alternating against a big one."""
    if not case.big:
        return [(p, d) for p in KV_POS for d in (False, True)]
    return [(p, bool(i & 1)) for i, p in enumerate(KV_POS)]


@functools.lru_cache(maxsize=2)
def kv_weight(N, K):
    w = np.random.default_rng(_seed("kvw", N, K)).integers(-2, 3, (N, K)).astype(np.float32)
    w.setflags(write=False)
    return w


def synthetic_rope(Smax, hd2):
    """(cos, sin) [Smax, HD / 2] from the four exact rotations, varying with position and pair."""
    idx = (3 * np.arange(Smax)[:, None] + np.arange(hd2)[None, :] + (np.arange(Smax)[:, None] // 4)) % 4
    return (np.array([1.0, 0.0, -1.0, 0.0], np.float32)[idx], np.array([0.0, 1.0, 0.0, -1.0], np.float32)[idx])
