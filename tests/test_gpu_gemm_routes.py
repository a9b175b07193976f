"""Every GEMM route the dispatcher reaches x every fused epilogue it accepts there, one launch at a
time (l3_op_gemm_host), against the float64 reference of tests/gemm_epi_ref.py (DESIGN.md "GEMM
route coverage").

Each case first asserts the route report (the kernel family and the template parameters that
identify the instantiation, written by launch_gemm at the launch site), then the values:

* integer cases, bit for bit.  |x| <= 2, |w| <= 2 and K <= 4096 keep every product and partial sum
  an integer below 2^24, so fp32 is exact in any order; with the norm x = +-2 and eps = 0 make the
  row factor exactly 0.5 (only where K is a power of two: three of the kernels multiply by a
  rounded 1 / K); q_scale is a power of two; each RoPE (cos, sin) is one of (1, 0), (0, 1),
  (-1, 0), (0, -1), chosen by position and pair index, so the rotation is exact and a wrong
  position or pair changes the result.  Outputs, caches, q_out and their guard space start as a
  NaN-free sentinel, and the WHOLE buffers are compared, so a store outside the rows, slots,
  heads and columns the launch owns fails too.
* EPI_SWIGLU with integer operands: the gate and up sums are exact, the gate weight is nonzero only
  at the first and last 8 k (|g| <= 32), and the only error is silu_f's.  The bound is
  gemm_epi_ref.swiglu_own_bound: (|g| + 7) 2^-24 relative to silu(g) u, from one rounding of the
  exponential's argument (relative |g| 2^-24 after the exponential), v_exp_f32 and v_rcp_f32 at
  1 ulp each (AMD "Instinct MI300 / CDNA3 ISA reference", V_EXP_F32 / V_RCP_F32: 1 ULP) and three
  roundings (1 + e, the multiplies by g and by u).
* random cases (standard_normal x, 0.05 standard_normal w), one per family and epilogue: the
  worst-case bound K 2^-24 (|x| @ |w|.T) of any summation order, propagated through the epilogue by
  gemm_epi_ref; a second call is bitwise equal.

The worst error / bound ratio per family is printed at the end of the module (pytest -s).
"""

import functools

import numpy as np
import pytest

import gemm_epi_ref as ref
import l3hip
import utils
from gemm_epi_ref import QKV, RESID, STORE, SWIGLU

pytestmark = pytest.mark.gpu

E4 = (STORE, RESID, SWIGLU, QKV)
E3 = (RESID, SWIGLU, QKV)
EPI_NAME = {STORE: "store", RESID: "resid", SWIGLU: "swiglu", QKV: "qkv"}
SMALL_W = 4 << 20  # launch_gemm's small-weight threshold (elements)

# QKV geometries: N = (H + 2 KVH) HD
G256 = dict(H=4, KVH=2, HD=32)     # 256
G192 = dict(H=4, KVH=1, HD=32)     # 192 (a multiple of 96)
G512 = dict(H=4, KVH=2, HD=64)     # 512
G384 = dict(H=4, KVH=1, HD=64)     # 384 (a multiple of 96)
G144 = dict(H=4, KVH=1, HD=24)     # 144: heads of 24 columns straddle the 16-column groups
G1152 = dict(H=12, KVH=3, HD=64)   # past the threshold at K = 4096
G2560 = dict(H=24, KVH=8, HD=64)   # past the threshold at K = 2048
G4096 = dict(H=32, KVH=16, HD=64)  # the 64 MB weight at K = 4096
G8320 = dict(H=100, KVH=15, HD=64)  # 520 column tiles of 16
G4160 = dict(H=49, KVH=8, HD=64)    # past the threshold at K = 1024
G14592 = dict(H=200, KVH=14, HD=64)  # past the threshold at K = 288


def qn(g):
    return (g["H"] + 2 * g["KVH"]) * g["HD"]


def shape_for(epi, K, size):
    """(N, geometry) of a weight that is `size` for launch_gemm at this K: N off the tile multiples
    (100, 260, 1028, 2052; 32 k for SwiGLU), 'big' just past the small-weight threshold."""
    if size == "small":
        n, g = {STORE: (260, None), RESID: (100, None), SWIGLU: (288, None), QKV: (256, G256)}[epi]
        assert n * K <= SMALL_W
    elif size == "big":
        if K >= 4096:
            n, g = {STORE: (1028, None), RESID: (1028, None), SWIGLU: (1056, None), QKV: (1152, G1152)}[epi]
        elif K == 1024:
            n, g = {STORE: (4100, None), RESID: (4100, None), SWIGLU: (4128, None), QKV: (4160, G4160)}[epi]
        elif K == 288:
            n, g = {STORE: (14568, None), RESID: (14568, None), SWIGLU: (14592, None), QKV: (14592, G14592)}[epi]
        else:
            n, g = {STORE: (2052, None), RESID: (2052, None), SWIGLU: (2080, None), QKV: (2560, G2560)}[epi]
        assert n * K > SMALL_W
    else:
        assert size == "nt" and K == 4096
        n, g = 4096, (G4096 if epi == QKV else None)
        assert n * K * 4 >= 64 << 20
    if g is not None:
        assert qn(g) == n
    return n, g


class Case:
    def __init__(self, name, epi, M, K, N=None, geo=None, size=None, expect=None, norm=None, L=None,
                 start_pos=2, tail=3, col_base=False, q_only=False, gather=False, norm_w=False, **route):
        if N is None and geo is None:
            N, geo = shape_for(epi, K, size)
        if geo is not None:
            N = qn(geo)
        self.name, self.epi, self.M, self.K, self.N, self.geo = name, epi, M, K, N, geo
        self.expect = expect or {}
        # the norm where the epilogue has one and the exact row factor exists (K a power of two)
        self.norm = (epi != RESID and K & (K - 1) == 0) if norm is None else norm
        if L is None:
            L = M // next(b for b in (3, 2, 1) if M % b == 0)
        self.L, self.start_pos, self.tail = L, start_pos, tail
        self.col_base, self.gather, self.norm_w, self.route = col_base, gather, norm_w, route
        self.q_only = q_only
        if route.get("bf16") and self.norm:
            self.norm_w = True

    @property
    def id(self):
        return f"{self.name}-{EPI_NAME[self.epi]}-M{self.M}-K{self.K}-N{self.N}"


@functools.lru_cache(maxsize=6)
def int_weight(N, K, seed):
    w = np.random.default_rng(seed).integers(-2, 3, (N, K)).astype(np.float32)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=4)
def int_gate(Nh, K, seed):
    """Gate rows that keep |g| <= 32 for |x| <= 2: -1 / 0 / 1 at the first and last 8 k only."""
    rng = np.random.default_rng(seed)
    w = np.zeros((Nh, K), np.float32)
    w[:, :8] = rng.integers(-1, 2, (Nh, 8))
    w[:, -8:] = rng.integers(-1, 2, (Nh, 8))
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=4)
def rand_weight(N, K, seed):
    w = (0.05 * np.random.default_rng(seed).standard_normal((N, K))).astype(np.float32)
    w.setflags(write=False)
    return w


def synthetic_rope(Smax, hd2):
    """(cos, sin) [Smax, HD / 2] from the four exact rotations, varying with position and pair."""
    idx = (3 * np.arange(Smax)[:, None] + np.arange(hd2)[None, :] + (np.arange(Smax)[:, None] // 4)) % 4
    cos = np.array([1.0, 0.0, -1.0, 0.0], np.float32)[idx]
    sin = np.array([0.0, 1.0, 0.0, -1.0], np.float32)[idx]
    return cos, sin


def real_rope(Smax, HD):
    inv = 1.0 / (10000.0 ** (np.arange(0, HD, 2) / HD))
    ang = np.outer(np.arange(Smax), inv)
    return np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)


_ratios = {}  # (family, kind) -> worst error / bound


@pytest.fixture(scope="module")
def ctx():
    c = l3hip.op_context(0)
    yield c
    for key in sorted(_ratios):
        print(f"\n[gemm routes] worst error / bound, {key[0]:10s} {key[1]:12s}: {_ratios[key]:.4f}", end="")
    print()


def _bits(a):
    return (np.ascontiguousarray(a, np.float32) + np.float32(0)).view(np.uint32)  # -0 -> +0


def _same_bits(got, want, what):
    bad = np.argwhere(_bits(got) != _bits(want))
    assert bad.size == 0, (what, len(bad), bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def _within(got, want64, bound, key, what):
    err = np.abs(got.astype(np.float64) - want64)
    over = np.argwhere(err > bound)
    assert over.size == 0, (what, len(over), over[:4].tolist(), err[tuple(over[0])], bound[tuple(over[0])])
    nz = bound > 0
    if nz.any():
        _ratios[key] = max(_ratios.get(key, 0.0), float((err[nz] / bound[nz]).max()))


def _reference_is_sensitive(z, x, w):
    """On the reference alone (as test_gpu_weight_bf16_rows._check_exact): rows pairwise distinct,
    and dropping the first or the last 8 of K changes every row."""
    assert len({r.tobytes() for r in z}) == z.shape[0]
    for sl in (slice(0, -8), slice(8, None)):
        assert np.all(np.any(x[:, sl] @ w[:, sl].T != z, axis=1))


def run(ctx, case, mode="int", check_route=True):
    """One launch of `case`; returns the route.  mode 'int': bit-exact operands; 'rand': bounds."""
    rng = np.random.default_rng(abs(hash((case.M, case.K, case.N, case.epi))) % (1 << 31))
    epi, M, K, N = case.epi, case.M, case.K, case.N
    exact = mode == "int"
    norm = case.norm if exact else epi != RESID
    eps = 0.0 if exact else 1e-5
    kw = dict(case.route)
    # ---- operands ----
    rows = M
    a_rows = None
    if case.gather and epi in (SWIGLU, QKV, STORE):
        rows = M + 5
        a_rows = rng.integers(0, rows, M).astype(np.int32)  # repeats, out of order
        a_rows[:2] = (rows - 1, 0)
        if M > 3:
            a_rows[3] = a_rows[2]
    if exact:
        assert 2 * 2 * 4 * K < 2 ** 24  # |x| |w| |norm_w| K
        x = (rng.choice([-2.0, 2.0], (rows, K)) if norm else rng.integers(-2, 3, (rows, K))).astype(np.float32)
    else:
        x = rng.standard_normal((rows, K)).astype(np.float32)
    nw = None
    if case.norm_w and norm:
        nw = (rng.choice([0.5, 1.0, 2.0], K) if exact else rng.uniform(0.5, 1.5, K)).astype(np.float32)
        kw["norm_w"] = nw
    if epi == SWIGLU:
        nh = N // 2
        if exact:
            wg, wu = int_gate(nh, K, 11), int_weight(nh, K, 12)
        else:
            wg, wu = rand_weight(nh, K, 13), rand_weight(nh, K, 14)
        w_dev = dict(gate_up=(wg, wu))
        w_ref = np.concatenate([wg, wu])
    else:
        w = int_weight(N, K, 15) if exact else rand_weight(N, K, 16)
        w_dev = dict(w=w)
        w_ref = w
    if kw.get("bf16") and not exact:
        w_ref = utils.round_bf16(w_ref)  # the model the kernels compute: float(bf16(w))
    elif kw.get("bf16"):
        assert np.array_equal(utils.round_bf16(w_ref), w_ref)
    # the RMSNorm weight belongs to the columns of w: bf16 storage passes it beside the weight
    w64 = w_ref.astype(np.float64) * (nw.astype(np.float64) if nw is not None and norm else 1.0)
    if nw is not None and not kw.get("bf16"):
        raise AssertionError("norm_w goes with bf16 storage")
    xs = x[a_rows] if a_rows is not None else x
    if exact:  # (on the table's rows: a gather repeats rows on purpose)
        _reference_is_sensitive(x.astype(np.float64) @ w64.T, x.astype(np.float64), w64)

    def call():
        if epi == QKV:
            return ctx.op_gemm(epi, x, a_rows=a_rows, norm=norm, eps=eps, qkv=dict(q), **w_dev, **kw)
        return ctx.op_gemm(epi, x, a_rows=a_rows, norm=norm, eps=eps, c=c0, res_src=res_src, res_rows=res_rows,
                           **w_dev, **kw)

    what = case.id
    c0 = res_src = res_rows = None
    if epi == QKV:
        g = case.geo
        H, KVH, HD = g["H"], g["KVH"], g["HD"]
        L, sp = case.L, case.start_pos
        B, Smax = M // L, sp + L + case.tail
        cos, sin = synthetic_rope(Smax, HD // 2) if exact else real_rope(Smax, HD)
        ck0, cv0 = l3hip.gemm_sentinel((B, KVH, Smax, HD), 3), l3hip.gemm_sentinel((B, KVH, Smax, HD), 4)
        col_base = H * HD if case.col_base else 0
        q_scale = 0.25 if exact else 0.18033688
        n_end = H * HD if case.q_only else N  # q-only: the first H * HD rows of the weight
        w_dev = dict(w=w_dev["w"][col_base:n_end])
        q = dict(L=L, start_pos=sp, H=H, KVH=KVH, HD=HD, Smax=Smax, q_scale=q_scale, rope_cos=cos, rope_sin=sin,
                 cache_k=ck0, cache_v=cv0, col_base=col_base)
        r = ref.ref_qkv(x, w64[col_base:n_end], cos, sin, L=L, start_pos=sp, H=H, KVH=KVH, HD=HD, q_scale=q_scale,
                        col_base=col_base, norm=norm, eps=eps, a_rows=a_rows)
        out = call()
        route = out["route"]
        if check_route:
            _check_route(route, case)
        want = {"q_out": np.concatenate([l3hip.gemm_sentinel((M, H * HD), 5), l3hip.gemm_sentinel((1, H * HD), 7)]),
                "cache_k": np.concatenate([ck0, l3hip.gemm_sentinel((1, KVH, Smax, HD), 8)]),
                "cache_v": np.concatenate([cv0, l3hip.gemm_sentinel((1, KVH, Smax, HD), 9)])}
        owned = {k: np.zeros(v.shape, bool) for k, v in want.items()}
        val = {k: np.zeros(v.shape) for k, v in want.items()}
        bnd = {k: np.zeros(v.shape) for k, v in want.items()}
        if not col_base:
            owned["q_out"][:M] = True
            val["q_out"][:M], bnd["q_out"][:M] = r["q"], r["q_bound"]
        for name, key in (("cache_k", "k"), ("cache_v", "v")):
            if r[key] is None:
                continue
            owned[name][:B, :, sp:sp + L] = True
            val[name][:B, :, sp:sp + L], bnd[name][:B, :, sp:sp + L] = r[key], r[key + "_bound"]
        for name in want:
            got = out[name]
            if exact:
                full = np.where(owned[name], val[name].astype(np.float32), want[name])
                assert np.array_equal(full[owned[name]].astype(np.float64), val[name][owned[name]])  # fp32 holds it
                _same_bits(got, full, (what, name))
            else:
                _same_bits(np.where(owned[name], 0, got), np.where(owned[name], 0, want[name]), (what, name, "untouched"))
                _within(np.where(owned[name], got, 0), val[name], bnd[name], (route["family"], "random"), (what, name))
        if not exact:
            again = call()
            for name in want:
                assert np.array_equal(again[name].view(np.uint32), out[name].view(np.uint32)), (what, name, "rerun")
        return route

    ldc = N // 2 if epi == SWIGLU else N
    guard = l3hip.gemm_sentinel((1, ldc), 7)
    if epi == RESID:
        resid = (rng.integers(-8, 9, (M, ldc)) if exact else rng.standard_normal((M, ldc))).astype(np.float32)
        if case.gather:
            res_src = (rng.integers(-8, 9, (M + 4, ldc)) if exact else rng.standard_normal((M + 4, ldc))).astype(np.float32)
            res_rows = rng.integers(0, M + 4, M).astype(np.int32)
            res_rows[:2] = (M + 3, 0)
            c0 = None  # the sentinel: C is written, never read
            want64, bound = ref.ref_resid(x, w64, res_src, res_rows=res_rows)
        else:
            c0 = resid
            want64, bound = ref.ref_resid(x, w64, resid)
        kind = "random"
    elif epi == SWIGLU:
        want64, bound, gpre = ref.ref_swiglu(x, w64[:N // 2], w64[N // 2:], norm=norm, eps=eps, a_rows=a_rows)
        kind = "random"
        if exact:
            assert np.abs(gpre).max() <= 32
            bound = ref.swiglu_own_bound(gpre, xs.astype(np.float64) @ w64[N // 2:].T * (0.5 if norm else 1.0))
            kind = "swiglu exact"
    else:
        want64, bound = ref.ref_store(x, w64, norm=norm, eps=eps, a_rows=a_rows)
        kind = "random"
    out = call()
    route = out["route"]
    if check_route:
        _check_route(route, case)
    got = out["c"]
    _same_bits(got[M:], guard, (what, "guard"))
    if exact and epi != SWIGLU:
        _same_bits(got[:M], want64.astype(np.float32), what)
    else:
        _within(got[:M], want64, bound, (route["family"], kind), what)
    if not exact:
        assert np.array_equal(call()["c"].view(np.uint32), got.view(np.uint32)), (what, "rerun")
    return route


def _check_route(route, case):
    assert route["launches"] == 1, (case.id, route)
    for k, v in case.expect.items():
        assert route[k] == v, (case.id, k, v, route)


def params(cases):
    ids = [c.id for c in cases]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    return pytest.mark.parametrize("case", cases, ids=ids)


# ---- the weight-streaming GEMV, fp32 ---------------------------------------------------------------

def gemv_cases(bf16):
    fam = "gemv_bf16" if bf16 else "gemv"
    extra = dict(bf16=True) if bf16 else {}
    epis = E3 if bf16 else E4
    # lanes per unit from the 16-byte pieces of a W row: K / 4 floats, or K / 8 with bf16
    lanes = (lambda K: 16 if K // 8 <= 128 else 32 if K // 8 <= 256 else 64) if bf16 else \
            (lambda K: 16 if K // 4 <= 128 else 32 if K // 4 <= 256 else 64)
    out = []
    for K in (288, 1024, 2048):  # a small weight: one row per block, a grid row per row of A
        for M in (1, 3, 8):
            for e in epis:
                out.append(Case(fam, e, M, K, size="small", L=1 if M == 3 else None, **extra,
                                expect=dict(family=fam, rows_per_block=1, lanes_per_unit=lanes(K), nt=0, row_blocks=M)))
    # past the threshold: 2-, 4- and 8-row blocks; the last four at 16 / 32 lanes per unit
    for M, K, mr in ((2, 4096, 2), (3, 4096, 4), (4, 4096, 4), (5, 2048, 8), (8, 2048, 8),
                     (2, 288, 2), (4, 1024, 4), (8, 1024, 8), (7, 288, 8)):
        for e in epis:
            out.append(Case(fam, e, M, K, size="big", **extra,
                            expect=dict(family=fam, rows_per_block=mr, lanes_per_unit=lanes(K), nt=0, row_blocks=1)))
    # heads of 24 columns (no multiple of 16) on the pair-wise QKV epilogue
    out.append(Case(fam + "_hd24", QKV, 3, 1024, geo=G144, L=1, **extra, expect=dict(family=fam, rows_per_block=1)))
    out.append(Case(fam + "_hd24", QKV, 4, 4096, geo=G144, **extra, expect=dict(family=fam, rows_per_block=1)))
    return out


@params(gemv_cases(False))
def test_gemv(ctx, case):
    run(ctx, case)


@pytest.mark.parametrize("epi", E4, ids=[EPI_NAME[e] for e in E4])
def test_gemv_nontemporal(ctx, epi):
    """One row against a 64 MB weight: the non-temporal form (the only 64 MB cases of this module)."""
    run(ctx, Case("gemv_nt", epi, 1, 4096, size="nt",
                  expect=dict(family="gemv", rows_per_block=1, lanes_per_unit=64, nt=1, row_blocks=1)))


# ---- 5 - 8 rows at K = 4096: past the GEMV's 64 KB of staged rows -----------------------------------

def small_m_tile(epi):
    """The small-M tile of launch_gemm's final switch: 16 x 128 (BK 32) for the fused epilogues;
    EPI_STORE's own table has 32 x 128 (BK 16, gemm_store_config 1) at up to 32 rows."""
    return dict(family="tiled", bm=32, bn=128, bk=16) if epi == STORE else dict(family="tiled", bm=16, bn=128, bk=32)


@params([Case("rows5to8", e, M, 4096, size=size, expect=small_m_tile(e))
         for M, size in ((5, "small"), (8, "big")) for e in E4])
def test_five_to_eight_rows_long_k_take_the_small_m_tile(ctx, case):
    run(ctx, case)


# ---- skinny ----------------------------------------------------------------------------------------

def skinny_cases():
    out = []
    for M in (9, 16, 17, 256):
        for e in E4:
            out.append(Case("skinny", e, M, 1024, size="small", expect=dict(family="skinny", tn=2 if e == SWIGLU else 1)))
    for e in E4:  # a speculative chunk
        out.append(Case("skinny_forced", e, 2, 1024, size="small", force_skinny=True,
                        expect=dict(family="skinny", tn=2 if e == SWIGLU else 1)))
    for M in (257, 300):  # past 256 rows QKV and the residual epilogues take 2-tile columns
        for e in E4:
            out.append(Case("skinny_forced", e, M, 288, size="small", force_skinny=True,
                            expect=dict(family="skinny", tn=1 if e == STORE else 2)))
    return out


@params(skinny_cases())
def test_skinny(ctx, case):
    run(ctx, case)


# ---- split-K ---------------------------------------------------------------------------------------

def need_per(c):
    return c.M * c.N + c.M  # floats per slice (launch_split_cfg)


def splitk_cases():
    out = []
    for M, K, bm in ((9, 2048, 16), (16, 4096, 16), (17, 4096, 64), (64, 2048, 64), (65, 2048, 128), (200, 4096, 128)):
        for e in E4:
            c = Case("splitk", e, M, K, size="big", expect=dict(family="splitk", bm=bm, bn=128, bk=32))
            c.route["ws_floats"] = 16 * need_per(c)
            out.append(c)
    return out


@params(splitk_cases())
def test_splitk(ctx, case):
    route = run(ctx, case)
    assert route["s"] in (2, 4, 8, 16), route


@pytest.mark.parametrize("epi", E4, ids=[EPI_NAME[e] for e in E4])
def test_splitk_workspace_limits_the_slices(ctx, epi):
    """A workspace for two slices but not four: S = 2.  One below two slices: no split, the tiled
    kernel, the same values."""
    c = Case("splitk_s2", epi, 16, 4096, size="big", expect=dict(family="splitk", bm=16, s=2))
    c.route["ws_floats"] = 4 * need_per(c) - 1
    run(ctx, c)
    c = Case("splitk_none", epi, 16, 4096, size="big", expect=small_m_tile(epi))
    c.route["ws_floats"] = 2 * need_per(c) - 1
    run(ctx, c)


def test_splitk_is_not_taken_with_col_base(ctx):
    """The finish kernel's QKV epilogue has no col_base: a K / V-only launch keeps the tiles."""
    c = Case("splitk_colbase", QKV, 64, 4096, geo=G1152, col_base=True, expect=dict(family="tiled", bm=128, bn=128, bk=16))
    c.route["ws_floats"] = 16 * need_per(c)
    run(ctx, c)


# ---- tiled, no workspace: every launch<...> line of the final switch ---------------------------------

def tiled_cases():
    T = lambda bm, bn, bk, **k: dict(family="tiled", bm=bm, bn=bn, bk=bk, **k)  # noqa: E731
    out = []
    for M in (257, 300):  # a partial last row tile
        out += [
            Case("tiled", QKV, M, 1024, geo=G384, expect=T(128, 96, 16)),     # N % 96 == 0, K <= 1024
            Case("tiled", QKV, M, 288, geo=G256, expect=T(128, 128, 16)),
            Case("tiled", RESID, M, 288, N=192, expect=T(64, 96, 32)),        # N % 96 == 0, K <= 512
            Case("tiled", RESID, M, 1024, N=192, expect=T(128, 96, 32)),
            Case("tiled", RESID, M, 1024, N=260, expect=T(128, 128, 32)),
            Case("tiled", SWIGLU, M, 288, N=288, expect=T(128, 128, 16)),
            Case("tiled", STORE, M, 1024, N=260, expect=T(128, 128, 16, stages=4)),
        ]
    for e in E4:  # the small-M tile past the GEMV: 9 .. 32 rows against a weight past the threshold
        out.append(Case("tiled_small_m", e, 20, 2048, size="big", expect=small_m_tile(e)))
    out += [
        Case("tiled_store", STORE, 50, 2048, size="big", expect=T(64, 128, 16)),            # gemm_store_config 2
        Case("tiled_store", STORE, 200, 2048, size="big", expect=T(256, 64, 16, stages=3)),  # one 256-row panel
        # group_m: 5 row tiles in groups of 4 (K >= 1024, past the small-M tile)
        Case("tiled_group", SWIGLU, 600, 1024, N=288, expect=T(128, 128, 16, group_m=4)),
        Case("tiled_group", QKV, 600, 1024, geo=G256, expect=T(128, 128, 16, group_m=4)),
        Case("tiled_group", QKV, 600, 1024, geo=G384, L=200, expect=T(128, 96, 16, group_m=4)),
        Case("tiled_nogroup", SWIGLU, 600, 288, N=288, expect=T(128, 128, 16, group_m=0)),
    ]
    for cfg, (bm, bn) in ((1, (32, 128)), (2, (64, 128)), (3, (128, 128))):  # scoring's fixed configurations
        out.append(Case(f"tiled_forced{cfg}", STORE, 4, 1024, size="small", force_tiled=cfg, expect=T(bm, bn, 16)))
    out.append(Case("tiled_forced3", STORE, 200, 1024, size="small", force_tiled=3, expect=T(128, 128, 16)))
    return out


@params(tiled_cases())
def test_tiled(ctx, case):
    run(ctx, case)


# ---- EPI_QKV geometry on the tiled, skinny and split-K routes ---------------------------------------

def geometry_cases():
    out = []
    routes = (("tiled", 4096, {}, dict(family="tiled")), ("skinny", 1024, {}, dict(family="skinny", tn=1)),
              ("splitk", 4096, dict(ws=True), dict(family="splitk")))
    for rname, K, kw, expect in routes:
        for geo in (G192, G512, G144):  # GQA 4:1 and 2:1, HD 32 / 64 / 24
            for L in (63, 64, 65):      # qkv_fast switches on at 64; 128-row tiles straddle sequences
                out.append((Case(f"geo_{rname}_L{L}", QKV, 3 * L, K, geo=geo, L=L, expect=expect), kw))
        out.append((Case(f"geo_{rname}_decode", QKV, 40, K, geo=G512, L=1, start_pos=5, tail=0, expect=expect), kw))
        out.append((Case(f"geo_{rname}_lastslot", QKV, 66, K, geo=G192, L=33, start_pos=31, tail=0, expect=expect), kw))
    for c, kw in out:
        if kw.get("ws"):
            c.route["ws_floats"] = 16 * need_per(c)
    return [c for c, _ in out]


@params(geometry_cases())
def test_qkv_geometry(ctx, case):
    run(ctx, case)


def colbase_cases():
    return [
        Case("colbase_skinny", QKV, 64, 1024, geo=G256, col_base=True, expect=dict(family="skinny", tn=1)),
        Case("colbase_skinny", QKV, 300, 288, geo=G256, col_base=True, L=100, force_skinny=True,
             expect=dict(family="skinny", tn=2)),
        Case("colbase_tiled", QKV, 300, 1024, geo=G256, col_base=True, L=100, expect=dict(family="tiled", bm=128, bn=128)),
        Case("colbase_tiled", QKV, 300, 1024, geo=G512, col_base=True, L=75, expect=dict(family="tiled", bm=128)),
        Case("colbase_tiled", QKV, 20, 4096, geo=G144, col_base=True, expect=dict(family="tiled", bm=16, bn=128)),
        Case("colbase_x6", QKV, 300, 1024, geo=G256, col_base=True, L=100, x6=True, expect=dict(family="x6", bm=128, bn=128)),
        Case("colbase_x6", QKV, 195, 4096, geo=G512, col_base=True, L=65, x6=True, expect=dict(family="x6")),
        # the other half of a pruned last block: q alone for one row per sequence, forced skinny
        Case("q_only_skinny", QKV, 5, 1024, geo=G256, q_only=True, L=1, start_pos=7, tail=0, force_skinny=True,
             expect=dict(family="skinny", tn=1)),
        Case("q_only_skinny", QKV, 40, 4096, geo=G512, q_only=True, L=1, start_pos=7, tail=0, force_skinny=True,
             expect=dict(family="skinny", tn=1)),
        Case("q_only_rows_bf16", QKV, 5, 1024, geo=G144, q_only=True, L=1, force_skinny=True, bf16=True, wb_rows=64,
             expect=dict(family="rows_bf16", mt=1)),
    ]


@params(colbase_cases())
def test_qkv_col_base(ctx, case):
    """A K / V-only launch: W starts at row H * HD, and all of q_out stays as it was; a q-only launch
    (N = H * HD) leaves both caches as they were."""
    run(ctx, case)


# ---- x6 --------------------------------------------------------------------------------------------

def x6_cases():
    X = lambda bm, bn, waves: dict(family="x6", bm=bm, bn=bn, waves=waves)  # noqa: E731
    out = []
    for M in (33, 128, 257):
        out += [
            Case("x6", SWIGLU, M, 2048, size="big", x6=True, expect=X(128, 128, 8)),
            Case("x6", QKV, M, 2048, size="big", x6=True, expect=X(128, 128, 4)),
            Case("x6", QKV, M, 4096, geo=G144, x6=True, expect=X(128, 128, 4)),
            Case("x6", RESID, M, 512, N=8256, x6=True, expect=X(128, 96, 8)),     # N % 96 == 0, K <= 512
            Case("x6", RESID, M, 2048, N=2112, x6=True, expect=X(128, 96, 4)),    # N % 96 == 0
            Case("x6", RESID, M, 2048, N=2052, x6=True, expect=X(128, 128, 4)),
        ]
    for e in E3:  # up to 32 rows keep the fp32 small-M tile
        out.append(Case("x6_small_m", e, 20, 2048, size="big", x6=True, expect=small_m_tile(e)))
    out.append(Case("x6_store", STORE, 128, 2048, size="big", x6=True, expect=dict(family="tiled", bm=128, bn=128)))
    return out


@params(x6_cases())
def test_x6(ctx, case):
    run(ctx, case)


# ---- bf16 weight storage ---------------------------------------------------------------------------

@params(gemv_cases(True))
def test_gemv_bf16(ctx, case):
    run(ctx, case)


def rows_bf16_cases():
    out = []
    for M in (2, 16, 17, 32, 33, 64):
        mt = 1 if M <= 16 else 2 if M <= 32 else 4
        R = lambda waves, tn: dict(family="rows_bf16", mt=mt, waves=waves, tn=tn, nt=0)  # noqa: E731
        kw = dict(bf16=True, wb_rows=64)
        out += [
            Case("rows_bf16", RESID, M, 288, N=100, expect=R(8, 1), **kw),          # 7 blocks: eight waves
            Case("rows_bf16", RESID, M, 288, N=8260, expect=R(4, 1), **kw),         # 517 blocks: four waves
            Case("rows_bf16", QKV, M, 1024, geo=G256, expect=R(8, 1), **kw),
            Case("rows_bf16", QKV, M, 288, geo=G8320, expect=R(4, 1), **kw),        # 520 blocks
            Case("rows_bf16", QKV, M, 2048, geo=G144, expect=R(8, 1), **kw),        # heads of 24 columns
            # two column tiles (gate / up); four row tiles of them keep four waves
            Case("rows_bf16", SWIGLU, M, 1024, N=288, expect=R(4 if mt == 4 else 8, 2), **kw),
            Case("rows_bf16", SWIGLU, M, 288, N=16416, expect=R(4, 2), **kw),       # 513 blocks
        ]
    return out


@params(rows_bf16_cases())
def test_rows_bf16(ctx, case):
    run(ctx, case)


def rows_bf16_kept_cases():
    kw = dict(bf16=True)
    return [
        Case("kept_wb_rows", RESID, 16, 1024, size="small", wb_rows=8, expect=dict(family="skinny"), **kw),
        Case("kept_wb_rows", QKV, 3, 1024, size="small", wb_rows=2, expect=dict(family="gemv_bf16"), **kw),
        Case("kept_min_bytes", SWIGLU, 16, 1024, size="small", wb_rows=64, wb_min_bytes=1 << 30,
             expect=dict(family="skinny", tn=2), **kw),
        Case("kept_force_tiled", STORE, 16, 1024, size="small", wb_rows=64, force_tiled=2,
             expect=dict(family="tiled", bm=64, bn=128), **kw),
        Case("kept_x6", RESID, 40, 2048, size="big", wb_rows=64, x6=True, expect=dict(family="x6"), **kw),
        Case("kept_x6", QKV, 40, 2048, size="big", wb_rows=64, x6=True, expect=dict(family="x6"), **kw),
        Case("taken_x6_small_m", SWIGLU, 20, 2048, size="big", wb_rows=64, x6=True, expect=dict(family="rows_bf16", mt=2), **kw),
    ]


@params(rows_bf16_kept_cases())
def test_rows_bf16_leaves_what_it_must_not_take(ctx, case):
    run(ctx, case)


# ---- gathers ---------------------------------------------------------------------------------------

def gather_cases():
    """a_rows (EPI_SWIGLU / EPI_QKV) and res_src / res_rows (EPI_RESID) on one shape per family; every
    family's kernels read A through a_row() and the residual through res_row() (kernels.h)."""
    out = []
    for e in E3:
        g = dict(gather=True)
        out += [
            Case("gather_gemv", e, 3, 1024, size="small", expect=dict(family="gemv", rows_per_block=1), **g),
            Case("gather_gemv4", e, 4, 4096, size="big", expect=dict(family="gemv", rows_per_block=4), **g),
            Case("gather_skinny", e, 17, 1024, size="small", expect=dict(family="skinny"), **g),
            Case("gather_tiled", e, 300, 1024, size="small", expect=dict(family="tiled"), **g),
            Case("gather_x6", e, 128, 2048, size="big", x6=True, expect=dict(family="x6"), **g),
            Case("gather_gemv_bf16", e, 3, 1024, size="small", bf16=True, expect=dict(family="gemv_bf16"), **g),
            Case("gather_rows_bf16", e, 17, 1024, size="small", bf16=True, wb_rows=64, expect=dict(family="rows_bf16"), **g),
        ]
        c = Case("gather_splitk", e, 17, 4096, size="big", expect=dict(family="splitk"), **g)
        c.route["ws_floats"] = 16 * need_per(c)
        out.append(c)
    return out


@params(gather_cases())
def test_gathers(ctx, case):
    run(ctx, case)


# ---- refusals --------------------------------------------------------------------------------------

def test_refusals(ctx):
    """The error returns of launch_gemm this entry can reach: each raises, nothing stands in."""
    x = np.ones((4, 48), np.float32)
    with pytest.raises(RuntimeError, match="refused"):  # K not a multiple of 32
        ctx.op_gemm(STORE, x, np.ones((8, 48), np.float32))
    x = np.ones((4, 64), np.float32)
    with pytest.raises(RuntimeError, match="refused"):  # SwiGLU pairs 16-row groups
        ctx.op_gemm(SWIGLU, x, np.ones((48, 64), np.float32))
    with pytest.raises(RuntimeError, match="refused"):  # the GEMV has no col_base
        g = G256
        cos, sin = synthetic_rope(4, g["HD"] // 2)
        cache = l3hip.gemm_sentinel((4, g["KVH"], 4, g["HD"]), 3)
        ctx.op_gemm(QKV, x, np.ones((2 * g["KVH"] * g["HD"], 64), np.float32),
                    qkv=dict(L=1, start_pos=0, Smax=4, q_scale=1.0, rope_cos=cos, rope_sin=sin, cache_k=cache,
                             cache_v=cache, col_base=g["H"] * g["HD"], **g))
    with pytest.raises(RuntimeError, match="refused"):  # fixed tiled configurations are EPI_STORE's
        ctx.op_gemm(RESID, x, np.ones((8, 64), np.float32), c=np.zeros((4, 8), np.float32), force_tiled=2)
    with pytest.raises(RuntimeError, match="refused"):
        ctx.op_gemm(STORE, x, np.ones((8, 64), np.float32), force_tiled=4)
    # and the entry's own checks: slots past the cache never reach a kernel
    with pytest.raises(RuntimeError, match="outside the cache"):
        g = G256
        cos, sin = synthetic_rope(4, g["HD"] // 2)
        cache = l3hip.gemm_sentinel((4, g["KVH"], 4, g["HD"]), 3)
        ctx.op_gemm(QKV, x, np.ones((qn(g), 64), np.float32),
                    qkv=dict(L=1, start_pos=4, Smax=4, q_scale=1.0, rope_cos=cos, rope_sin=sin, cache_k=cache,
                             cache_v=cache, **g))


# ---- random values: one pass per family ------------------------------------------------------------

def random_cases():
    out = []
    for e in E4:
        out += [
            Case("rand_gemv", e, 3, 2048, size="small", expect=dict(family="gemv")),
            Case("rand_gemv8", e, 8, 2048, size="big", expect=dict(family="gemv", rows_per_block=8)),
            Case("rand_skinny", e, 100, 1024, size="small", expect=dict(family="skinny")),
            Case("rand_tiled", e, 300, 1024, size="small", expect=dict(family="tiled")),
        ]
        c = Case("rand_splitk", e, 100, 4096, size="big", expect=dict(family="splitk"))
        c.route["ws_floats"] = 16 * need_per(c)
        out.append(c)
    for e in E3:
        out += [
            Case("rand_x6", e, 130, 2048, size="big", x6=True, expect=dict(family="x6")),
            Case("rand_gemv_bf16", e, 3, 2048, size="small", bf16=True, norm_w=True, expect=dict(family="gemv_bf16")),
            Case("rand_rows_bf16", e, 40, 1024, size="small", bf16=True, norm_w=True, wb_rows=64,
                 expect=dict(family="rows_bf16", mt=4)),
        ]
    return out


@params(random_cases())
def test_random_values_within_the_accumulation_bound(ctx, case):
    run(ctx, case, mode="rand")
