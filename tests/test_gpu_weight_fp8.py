"""fp8 e4m3 weight storage for the 1-64-row decode kernels (DESIGN.md "fp8 weight storage";
l3_set_weight_fp8, the F8 forms of gemv_kernel and gemm_rows_bf16_kernel, misc.hip
to_fp8_rows_kernel).

The format's host restatement (utils.quant_fp8_rows / round_fp8_rows / fp8_e4m3_table) is pinned
against torch in test_weight_fp8_cpu.py; here it is the reference of the kernels.  The reference of
every model comparison is the float64 oracle run on weights whose matrix kinds went through
utils.round_fp8_rows — never the library.  Bars are the project's: "sharp" weights, logits within
atol 1e-4 + rtol 2e-4, greedy ids exact after asserting, on the oracle alone, a top-1 / top-2 margin
of at least 1e-3 at every step.  Every model has non-unit norm weights (1 + 0.25 N(0, 1)).  The
models are far below the default min_bytes of the rows kernel, so they set
set_weight_bf16_rows(64, 0); L3_DECODE_PERSIST=0 except in the test about the persistent step."""

import dataclasses
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import l3hip
import llama3
import llama3_oracle as orc
import spec_ref
import synth
import utils
from config import ModelArgs

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHECK_LIB = os.path.join(os.path.dirname(HERE), "llama3.np_amd", "csrc", "libllama3hip_check.so")
MARGIN = 1e-3
ENV_KEYS = ("L3_WEIGHT_BF16", "L3_WEIGHT_FP8", "L3_WEIGHT_BF16_ROWS", "L3_WEIGHT_BF16_MIN_BYTES", "L3_FP8_NT_MB")
TABLE = utils.fp8_e4m3_table()


def is_matrix(name):
    return name.endswith("_proj.weight") or name == "lm_head.weight"


def make_weights(args, hidden, seed=31):
    """synth's sharp weights with non-unit norm weights."""
    w = synth.make_weights(args, hidden, seed=seed, preset="sharp")
    rng = np.random.default_rng(5)
    for k in sorted(w):
        if not is_matrix(k) and k != "model.embed_tokens.weight":
            w[k] = (1 + 0.25 * rng.standard_normal(w[k].shape)).astype(np.float32)
    return w


def rounded(w):
    return {k: utils.round_fp8_rows(v) if is_matrix(k) else v for k, v in w.items()}


def f64(w):
    return {k: np.asarray(v, np.float64) for k, v in w.items()}


def fp8_bytes(args, hidden):
    D, H, KVH = args.dim, args.n_heads, args.kv_heads
    HD = D // H
    per_layer = (H + 2 * KVH) * HD * (D + 4) + D * (H * HD + 4) + 2 * hidden * (D + 4) + D * (hidden + 4)
    return args.n_layers * per_layer + args.vocab_size * (D + 4)  # a byte per element, four per row


def oracle_loop(w64, args, prompt, total):
    """The reference schedule (prefill at 0, step i >= 1 at pos = L + i) on the oracle: ids
    [B, steps], each step's logits rows, and the least top-1 / top-2 margin over all of them."""
    m = orc.OracleModel(w64, dataclasses.replace(args, max_batch_size=prompt.shape[0]))
    L = prompt.shape[1]
    ids, rows, nxt, margin = [], [], None, np.inf
    for i, pos in enumerate(range(L, total)):
        lg = m(prompt if i == 0 else nxt, 0 if i == 0 else pos)[:, -1, :]
        top = np.partition(lg, -2, axis=-1)[:, -2:]
        margin = min(margin, float((top[:, 1] - top[:, 0]).min()))
        nxt = lg.argmax(-1, keepdims=True)
        ids.append(nxt[:, 0].copy())
        rows.append(lg)
    return np.stack(ids, axis=1), rows, margin


def close(got, want, what=""):
    got = np.asarray(got, np.float64).reshape(np.shape(want))
    err = np.abs(got - want)
    print(f"{what}: max-abs {err.max():.3e} (|logit| up to {np.abs(want).max():.1f})")
    assert np.all(err <= 1e-4 + 2e-4 * np.abs(want)), (what, float(err.max()))


# name -> (args, hidden): tiny HD 16 / n_rep 2; the stories15M shape (HD 48, six layers, K = 288:
# not a multiple of 64); one layer of HD 128 / n_rep 4
SHAPES = {
    "tiny": (synth.tiny(12), synth.TINY_HIDDEN),
    "stories": (ModelArgs(max_batch_size=12, max_seq_len=64), synth.STORIES15M_HIDDEN),
    "gqa": (ModelArgs(dim=512, n_layers=1, n_heads=4, n_kv_heads=1, vocab_size=1024, max_seq_len=96,
                      max_batch_size=12), 256),
}
# prompt seeds whose every greedy step keeps the top-1 margin on the rounded-weight oracle (found on
# the CPU, asserted by each test before it compares ids)
PROMPT_SEED = {"tiny": 8, "stories": 7, "gqa": 7}
STEP_LAUNCHES = {name: 4 * a.n_layers + 1 for name, (a, _) in SHAPES.items()}


class Case:
    """One model: the weights, the rounded-weight oracle's results (made once, never changed) and
    the fp8-e4m3-round model under test, the rows kernel on for every weight."""

    def __init__(self, name, build=True):
        self.name = name
        self.args, self.hidden = SHAPES[name]
        self.w = make_weights(self.args, self.hidden)
        self.wr = rounded(self.w)
        self.w64 = f64(self.wr)
        rng = np.random.default_rng(PROMPT_SEED[name])
        V = self.args.vocab_size
        self.p5 = rng.integers(0, V, (1, 5))
        self.p40 = rng.integers(0, V, (1, 40))
        self.pB = rng.integers(0, V, (12, 5))
        self.rag = [rng.integers(0, V, n) for n in (1, 3, 7, 2, 5)]
        self.spec = [rng.integers(0, V, n) for n in (4, 2, 6, 3)]
        self._memo = {}
        self.model = None
        if build:
            self.model = llama3.Llama(self.w, self.args, device=0, weight_dtype="fp8-e4m3-round")
            self.model.context.set_weight_bf16_rows(64, 0)

    def oracle(self, key, prompt, total):
        if key not in self._memo:
            self._memo[key] = oracle_loop(self.w64, self.args, prompt, total)
        return self._memo[key]

    def alone(self, prompt, total):
        """ids and least margin of one row alone on a zeroed cache."""
        ids, _, mg = self.oracle(("alone", tuple(int(t) for t in prompt), total), np.asarray(prompt)[None], total)
        return ids[0], mg

    def info(self):
        return self.model.context.weight_fp8_info()


_cases = {}


@pytest.fixture
def env(monkeypatch):
    monkeypatch.setenv("L3_DECODE_PERSIST", "0")
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture
def case(request, env):
    name = request.param
    if name not in _cases:
        _cases[name] = Case(name)
    c = _cases[name]
    c.model.context.reset_cache()
    c.model.set_sampling(0.0)
    c.model.context.set_weight_bf16_rows(64, 0)
    return c


@pytest.fixture(scope="module")
def ctx():
    return l3hip.op_context(0)


def _bits(a):
    return np.ascontiguousarray(np.array(a, np.float32)).view(np.uint32)


# ---- 1. the decode, exhaustive ---------------------------------------------------------------------

def test_decode_of_every_code_is_bitwise(ctx):
    """One-hot x returns W_q[n, k] itself: all 254 non-NaN codes (K = 288 holds them, the rest
    repeats), under row scales 2^-20, 2^-5, 1 and 2^7, equal to scale * table[code] bit for bit (-0 arrives
    as +0: it is added to an accumulator that starts at +0; its sign is pinned by the conversion
    test) — this pins the scale operand of v_cvt_scalef32_pk_f32_fp8 on the card."""
    K, N = 288, 8
    valid = np.array([c for c in range(256) if c & 0x7F != 0x7F], np.uint8)
    assert len(valid) == 254
    codes = np.stack([np.roll(np.resize(valid, K), 37 * n) for n in range(N)])  # every code at several byte positions
    scale = np.array([2.0 ** -20, 2.0 ** -5, 1.0, 2.0 ** 7] * 2, np.float32)
    want = (TABLE[codes].astype(np.float64) * scale.astype(np.float64)[:, None]).astype(np.float32)
    assert np.array_equal(want.astype(np.float64), TABLE[codes].astype(np.float64) * scale[:, None])  # exact
    want = want + np.float32(0)  # code 0x80: the accumulator starts at +0, and +0 + -0 = +0
    eye = np.eye(K, dtype=np.float32)
    got = np.concatenate([ctx.op_linear_fp8(eye[r:r + 8], codes, scale) for r in range(0, K, 8)]).T  # [N, K]
    bad = np.argwhere(_bits(got) != _bits(want))
    assert bad.size == 0, ("gemv", bad[:4], [hex(codes[tuple(b)]) for b in bad[:4]], got[tuple(bad[0])], want[tuple(bad[0])])
    for r0, rows in ((0, 64), (64, 64), (128, 64), (192, 64), (256, 32)):
        got = ctx.op_linear_fp8_rows(eye[r0:r0 + rows], codes, scale).T
        bad = np.argwhere(_bits(got) != _bits(want[:, r0:r0 + rows]))
        assert bad.size == 0, ("rows", r0, bad[:4], got[tuple(bad[0])], want[:, r0:][tuple(bad[0])])


def test_operands_are_checked_on_the_host(ctx):
    x = np.zeros((2, 64), np.float32)
    codes = np.zeros((8, 64), np.uint8)
    one = np.ones(8, np.float32)
    for fn in (ctx.op_linear_fp8, ctx.op_linear_fp8_rows):
        for nan in (0x7F, 0xFF):
            bad = codes.copy()
            bad[3, 5] = nan
            with pytest.raises(RuntimeError, match="row 3, column 5"):
                fn(x, bad, one)
        for s in (3.0, 0.0, -1.0, np.inf, 1e-45):
            sc = one.copy()
            sc[6] = s
            with pytest.raises(RuntimeError, match=r"scale\[6\].*power of two"):
                fn(x, codes, sc)
        with pytest.raises(RuntimeError, match="multiple of 32"):
            fn(np.zeros((2, 40), np.float32), np.zeros((8, 40), np.uint8), one)
        with pytest.raises(RuntimeError, match="multiple of 4"):
            fn(x, np.zeros((6, 64), np.uint8), np.ones(6, np.float32))
    with pytest.raises(RuntimeError, match="rows"):
        ctx.op_linear_fp8(np.zeros((9, 64), np.float32), codes, one)
    with pytest.raises(RuntimeError, match="not a shape"):
        ctx.op_linear_fp8(np.zeros((1, 16416), np.float32), np.zeros((4, 16416), np.uint8), np.ones(4, np.float32))
    for rows in (1, 65):
        with pytest.raises(RuntimeError, match="rows"):
            ctx.op_linear_fp8_rows(np.zeros((rows, 64), np.float32), codes, one)


# ---- 2. the conversion -----------------------------------------------------------------------------

def test_conversion_kernel_is_quant_fp8_rows(ctx):
    from test_weight_fp8_cpu import case_rows

    rng = np.random.default_rng(2)
    x = np.concatenate([case_rows(288), rng.standard_normal((301, 288)).astype(np.float32),
                        (rng.standard_normal((64, 288)) * np.exp(rng.uniform(-60, 60, (64, 1)))).astype(np.float32)])
    codes, scale, n = ctx.op_to_fp8_rows(x)
    wc, ws = utils.quant_fp8_rows(x)
    assert codes.dtype == np.uint8 and np.array_equal(scale.view(np.uint32), ws.view(np.uint32))
    bad = np.argwhere(codes != wc)
    assert bad.size == 0, (bad[:4], codes[tuple(bad[0])], wc[tuple(bad[0])], x[tuple(bad[0])])
    want_n = int(np.sum(utils.round_fp8_rows(x).view(np.uint32) != x.view(np.uint32)))
    assert n == want_n and n > 50000
    exact = utils.round_fp8_rows(x)
    c2, s2, n2 = ctx.op_to_fp8_rows(exact)
    assert n2 == 0 and np.array_equal((TABLE[c2] * s2[:, None]).view(np.uint32), exact.view(np.uint32))
    nudged = exact.copy()
    nudged[20, 11] = np.nextafter(nudged[20, 11], np.float32(np.inf))
    assert ctx.op_to_fp8_rows(nudged)[2] == 1
    with pytest.raises(RuntimeError, match="not finite"):
        ctx.op_to_fp8_rows(np.array([[1.0, np.nan, 0.0, 0.0]], np.float32))


# ---- 3. the kernels, integer-exact -----------------------------------------------------------------

INT_CODES = {v: int(np.flatnonzero(TABLE == v)[0 if v >= 0 else -1]) for v in range(-8, 9)}
INT_CODES[0] = 0


def _int_w(rng, N, K):
    """Codes of the integers in [-8, 8] (made as uint8 directly: no fp32 copy on the host) and
    power-of-two row scales that differ between rows."""
    lut = np.array([INT_CODES[v] for v in range(-8, 9)], np.uint8)
    codes = lut[rng.integers(0, 17, (N, K), dtype=np.uint8)]
    scale = (2.0 ** ((np.arange(N) * 3) % 5 - 2)).astype(np.float32)
    return codes, scale


def _int_x(rng, rows, K, norm):
    """Small integers: every product and every partial sum of a row is its scale times an integer
    below 2^24, so fp32 is exact in any order; with the norm, x = +-2 and eps = 0 make 1 / rms(x)
    exactly 0.5."""
    x = (rng.choice([-2.0, 2.0], (rows, K)) if norm else rng.integers(-4, 5, (rows, K))).astype(np.float32)
    g = rng.choice([-2.0, -1.0, 1.0, 2.0, 3.0], K).astype(np.float32) if norm else None
    assert np.abs(x).max() * (3 if norm else 1) * 8 * K < 2 ** 24
    return x, g


def _want(x, g, codes, scale):
    wi = TABLE[codes].astype(np.float64)  # integers: the float64 product is exact
    xi = (x * g if g is not None else x).astype(np.float64)
    y = (xi @ wi.T) * scale.astype(np.float64)
    out = (y * (0.5 if g is not None else 1.0)).astype(np.float32)
    assert np.array_equal(out.astype(np.float64), y * (0.5 if g is not None else 1.0))
    return out


def _check_exact(fn, x, g, codes, scale, what):
    want = _want(x, g, codes, scale)
    if want.shape[1] > 4 and x.shape[1] > 32:  # on the reference alone: a wrong row, column or k piece shows
        assert len({r.tobytes() for r in want}) == want.shape[0]
        for sl in (slice(0, -8), slice(8, None)):
            assert np.all(np.any(_want(x[:, sl], None if g is None else g[sl], codes[:, sl], scale) != want, axis=1))
    got = fn(x, codes, scale, g, 0.0)
    bad = np.argwhere(_bits(got) != _bits(want))
    assert bad.size == 0, (what, bad[:4], got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("K", [32, 288, 544, 1056, 4096, 8160])
def test_gemv_integer_exact(ctx, K):
    """op_linear_fp8 == integer arithmetic bitwise.  K: one piece per lane, a partly filled round
    and several rounds at each lane count; K = 8160 only fits the row-staging LDS up to two rows.
    N: one, a partly filled and many blocks.  rows 1-8: every rows-per-block form."""
    rng = np.random.default_rng(K)
    n0 = ctx.weight_fp8_info()["gemv_launches"]
    for N in (4, 100, 2052):
        codes, scale = _int_w(rng, N, K)
        for rows in ((1, 2) if K == 8160 else range(1, 9)):
            for norm in (False, True):
                x, g = _int_x(rng, rows, K, norm)
                _check_exact(ctx.op_linear_fp8, x, g, codes, scale, (K, N, rows, norm))
    assert ctx.weight_fp8_info()["gemv_launches"] > n0
    y, route = ctx.op_linear_fp8(x, codes, scale, route=True)
    assert route["family"] == "gemv_fp8" and route["nt"] == 0


ROWS = (2, 3, 8, 9, 16, 17, 31, 32, 33, 64)


@pytest.mark.parametrize("K", [32, 288, 4096, 14336])
def test_rows_kernel_integer_exact(ctx, K):
    """op_linear_fp8_rows == integer arithmetic bitwise.  rows: one, two and four row tiles, both
    sides of each tile edge.  K: one k-block (most waves idle), uneven wave shares (288 = 9
    k-blocks), the two Llama K.  N: below one tile, a partly filled last tile, many blocks."""
    rng = np.random.default_rng(K)
    n0 = ctx.weight_fp8_info()["rows_launches"]
    calls = 0
    for N in (4, 100, 2052):
        codes, scale = _int_w(rng, N, K)
        for rows in ROWS:
            for norm in (False, True):
                x, g = _int_x(rng, rows, K, norm)
                _check_exact(ctx.op_linear_fp8_rows, x, g, codes, scale, (K, N, rows, norm))
                calls += 1
    assert ctx.weight_fp8_info()["rows_launches"] == n0 + calls
    y, route = ctx.op_linear_fp8_rows(x, codes, scale, route=True)
    assert route["family"] == "rows_fp8" and route["mt"] == 4 and route["nt"] == 0


def test_nontemporal_forms_integer_exact(ctx):
    """The smallest N * K that crosses the non-temporal threshold (64 MiB of stored codes) at
    K = 4096: N = 16384 — the GEMV's one-row NT form (256 pieces of 16 codes: 32 lanes per unit) and the rows kernel's four-wave NT form (1024
    blocks); the route reports say so."""
    rng = np.random.default_rng(99)
    K, N = 4096, 16384
    assert N * K == 64 << 20
    codes, scale = _int_w(rng, N, K)
    for norm in (False, True):
        x, g = _int_x(rng, 1, K, norm)
        _check_exact(ctx.op_linear_fp8, x, g, codes, scale, ("gemv nt", norm))
    assert ctx.op_linear_fp8(x, codes, scale, route=True)[1] == {
        "family": "gemv_fp8", "rows_per_block": 1, "lanes_per_unit": 32, "nt": 1, "row_blocks": 1}
    x, g = _int_x(rng, 17, K, True)
    _check_exact(ctx.op_linear_fp8_rows, x, g, codes, scale, "rows nt")
    assert ctx.op_linear_fp8_rows(x, codes, scale, route=True)[1] == {
        "family": "rows_fp8", "mt": 2, "waves": 4, "nt": 1, "tn": 1}
    # one row fewer: below the threshold, plain loads
    assert ctx.op_linear_fp8(x[:1], codes[:-4], scale[:-4], route=True)[1]["nt"] == 0


# ---- 4. the kernels, random values -----------------------------------------------------------------

@pytest.mark.parametrize("rows,K,N", [(1, 4096, 2052), (5, 1056, 100), (3, 4096, 2052), (33, 4096, 2052),
                                      (64, 14336, 100), (9, 288, 100)])
def test_kernels_random_values(ctx, rows, K, N):
    """Against the float64 product of the same W_q: the error is at most twice that of op_linear
    (the fp32 kernels) on W_q with the same x, and a second call is bitwise equal."""
    rng = np.random.default_rng(rows * 1000 + N)
    x = rng.standard_normal((rows, K)).astype(np.float32)
    codes, scale = utils.quant_fp8_rows((rng.standard_normal((N, K)) * 0.05 * np.exp(rng.uniform(-2, 2, (N, 1)))))
    wq = TABLE[codes] * scale[:, None]
    want = x.astype(np.float64) @ wq.astype(np.float64).T
    err32 = float(np.abs(ctx.op_linear(x, wq) - want).max())
    fns = ([("gemv", ctx.op_linear_fp8)] if rows <= 8 else []) + ([("rows", ctx.op_linear_fp8_rows)] if rows >= 2 else [])
    g = (1 + 0.25 * rng.standard_normal(K)).astype(np.float32)
    x64 = x.astype(np.float64)
    wantn = (x64 / np.sqrt((x64 ** 2).mean(-1, keepdims=True) + 1e-5) * g) @ wq.astype(np.float64).T
    for name, fn in fns:
        got = fn(x, codes, scale)
        err = float(np.abs(got - want).max())
        print(f"rows {rows} K {K} N {N}: fp8 {name} kernel max-abs {err:.3e}, fp32 op_linear {err32:.3e}")
        assert err <= 2 * err32
        assert np.array_equal(_bits(got), _bits(fn(x, codes, scale)))
        gotn = fn(x, codes, scale, g, 1e-5)
        print(f"  with the norm: max-abs {np.abs(gotn - wantn).max():.3e} (|y| up to {np.abs(wantn).max():.1f})")
        assert np.all(np.abs(gotn - wantn) <= 1e-4 + 2e-4 * np.abs(wantn))


# ---- 5. models ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["tiny", "stories", "gqa"], indirect=True)
def test_model_logits_match_the_rounded_oracle(case):
    m, args = case.model, case.args
    info0 = case.info()
    assert info0["mode"] == 2 and info0["bytes"] == fp8_bytes(args, case.hidden)
    assert m.context.weight_bf16_info()["mode"] == 0 and m.context.weight_bf16_info()["bytes"] == 0
    ids, rows, _ = case.oracle("b1_short", case.p5, 5 + 4)
    got5 = np.array(m(case.p5, 0))[:, 0]
    close(got5, rows[0], f"{case.name} prefill of 5 (rows kernel)")
    # every projection of the five rows but the pruned last layer's (split_rows); the lm_head has one row
    pruned = 3 if args.n_layers > 1 else 0
    assert case.info()["rows_launches"] == info0["rows_launches"] + STEP_LAUNCHES[case.name] - 1 - pruned
    g0 = case.info()["gemv_launches"]
    for i in range(1, 4):  # eager decode steps on the reference's schedule, fed the oracle's ids
        close(m(ids[:, i - 1:i], 5 + i)[:, 0], rows[i], f"{case.name} decode step {i}")
    assert case.info()["gemv_launches"] > g0
    m.context.reset_cache()
    want40 = orc.OracleModel(case.w64, dataclasses.replace(args, max_batch_size=1))(case.p40, 0)[:, -1, :]
    close(m(case.p40, 0)[:, 0], want40, f"{case.name} prefill of 40")
    m.context.reset_cache()
    m.context.set_weight_bf16_rows(0)  # ... and on the fp32 kernels, which read the rounded fp32 copies
    r0 = case.info()["rows_launches"]
    close(m(case.p40, 0)[:, 0], want40, f"{case.name} prefill of 40 (rounded fp32 copies)")
    assert case.info()["rows_launches"] == r0
    m.context.reset_cache()
    close(m(case.p5, 0)[:, 0], rows[0], f"{case.name} prefill of 5 (GEMV)")
    assert case.info()["rows_launches"] == r0
    # the unquantised model is another model: far outside the bar
    plain = llama3.Llama(case.w, args, device=0)
    assert plain.context.weight_fp8_info() == {"mode": 0, "bytes": 0, "gemv_launches": 0, "rows_launches": 0}
    d5 = np.abs(np.array(plain(case.p5, 0))[:, 0] - rows[0])
    over = float((d5 / (1e-4 + 2e-4 * np.abs(rows[0]))).max())
    print(f"{case.name}: unquantised vs quantised logits differ by {d5.max():.3e}: {over:.0f} times the bar")
    assert over > 10
    assert plain.context.weight_fp8_info()["gemv_launches"] == 0


@pytest.mark.parametrize("B", [1, 3, 12])
@pytest.mark.parametrize("case", ["tiny", "stories", "gqa"], indirect=True)
def test_greedy_ids_to_the_last_slot(case, B):
    """generate / generate_all to the last cache slot: the captured graph of GEMV launches at B = 1
    (folded argmax, kv_bak, O-proj parts), the captured batched step on the rows kernel at 3 and 12
    (at 3 its QKV keeps the undo slots, kv_bak, which the rows kernel does not take: the GEMV)."""
    total = case.args.max_seq_len
    prompt = case.p5 if B == 1 else case.pB[:B]
    want, _, margin = case.oracle(f"b{B}_full", prompt, total)
    print(f"{case.name} B={B}: min top-1 margin {margin:.3e} over {want.shape[1]} steps")
    assert margin >= MARGIN
    m = case.model
    i0 = case.info()
    assert np.array_equal(m.generate_all(prompt, total), want)
    i1 = case.info()
    assert i1["rows_launches"] > i0["rows_launches"]  # (B = 1: the five-row prefill)
    assert (i1["gemv_launches"] > i0["gemv_launches"]) == (B <= 8)
    assert m.context.decode_stats()["graph_steps"] > 0 and not m.context.decode_persistent()
    m.context.reset_cache()
    assert np.array_equal(np.concatenate(list(m.generate(prompt, total)), axis=1), want)


@pytest.mark.parametrize("case", ["tiny", "gqa"], indirect=True)
def test_generate_ragged_with_a_stop_id(case):
    max_new = 24
    rows, margin = [], np.inf
    for p in case.rag:  # the reference: each row alone on a zeroed cache
        ids, mg = case.alone(p, max_new)
        rows.append(ids)
        margin = min(margin, mg)
    assert margin >= MARGIN
    stop = int(rows[1][6])
    want = []
    for r in rows:
        hit = np.flatnonzero(r == stop)
        want.append(r[:hit[0] + 1] if hit.size else r)
    assert len(want[1]) <= 7 < len(rows[1])
    n0 = case.info()["rows_launches"]
    got = case.model.generate_ragged(case.rag, max_new, stop_ids=[stop])
    for b, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (b, g, w)
    assert case.info()["rows_launches"] > n0


@pytest.mark.parametrize("case", ["tiny", "gqa"], indirect=True)
def test_extend_ragged_two_row_chunk(case):
    """Two rows continue with one token each at different positions: a 2-row chunk."""
    rng = np.random.default_rng(23)
    V = case.args.vocab_size
    prompts = [rng.integers(0, V, 3), rng.integers(0, V, 6)]
    chunks = [rng.integers(0, V, 1), rng.integers(0, V, 1)]
    m = case.model
    m.forward_ragged(prompts)
    n0 = case.info()["rows_launches"]
    got = np.array(m.extend_ragged(chunks, [3, 6]))[:, 0]
    assert case.info()["rows_launches"] == n0 + STEP_LAUNCHES[case.name]
    oracle = orc.OracleModel(case.w64, dataclasses.replace(case.args, max_batch_size=1))
    for b in range(2):
        want = oracle(np.concatenate([prompts[b], chunks[b]])[None], 0)[:, -1, :]
        close(got[b:b + 1], want, f"{case.name} extend row {b}")


@pytest.mark.parametrize("case", ["tiny", "gqa"], indirect=True)
def test_speculative_generation(case):
    """draft_len 3 at B = 4 (chunks of 16 rows): ids equal to the plain call's and the oracle's; the
    lookup is each row's true continuation with every seventh id wrong."""
    max_new = 28
    V = case.args.vocab_size
    truth = []
    for p in case.spec:
        ids, mg = case.alone(p, max_new)
        assert mg >= MARGIN
        truth.append(ids)
    lookup = []
    for t in truth:
        bad = np.array(t, np.int64)
        bad[5::7] = (bad[5::7] + 1) % V
        lookup.append(bad)
    m = case.model
    plain = m.generate_ragged(case.spec, max_new)
    m.context.reset_cache()
    n0 = case.info()["rows_launches"]
    got, stats = m.generate_ragged_spec(case.spec, max_new, speculate=dict(draft_len=3, ngram_max=3, lookup=lookup))
    assert case.info()["rows_launches"] > n0
    for b in range(4):
        sim = spec_ref.simulate(lookup[b], case.spec[b], truth[b], 3, 3, 1)
        assert np.array_equal(plain[b], truth[b]) and np.array_equal(got[b], plain[b]), b
        assert (int(stats["row_steps"][b]), int(stats["drafted"][b]), int(stats["accepted"][b])) == tuple(sim[1:]), b
    assert stats["accepted"].sum() > 0 and stats["drafted"].sum() > stats["accepted"].sum()


def test_persistent_step_reads_the_same_model(monkeypatch):
    """Default environment: the stories-shape batch-1 step is the persistent kernel, which reads
    the rounded fp32 copies — the same ids as the oracle's."""
    for k in ENV_KEYS + ("L3_DECODE_PERSIST",):
        monkeypatch.delenv(k, raising=False)
    c = _cases.get("stories") or Case("stories")
    _cases["stories"] = c
    want, _, margin = c.oracle("b1_full", c.p5, c.args.max_seq_len)
    assert margin >= MARGIN
    m = llama3.Llama(c.w, c.args, device=0, weight_dtype="fp8-e4m3-round")
    assert np.array_equal(m.generate_all(c.p5, c.args.max_seq_len), want)
    assert m.context.decode_persistent()


# ---- 6. dispatch and mode edges ----------------------------------------------------------------------

def _manual_context(w, args, hidden):
    """A context and a function that uploads ``w`` to it, as Llama.__init__ does."""
    ctx = l3hip.Context(llama3._dims(args, hidden, args.n_layers, args.vocab_size), 0)
    kinds = {"self_attn.q_proj": l3hip.W_Q, "self_attn.k_proj": l3hip.W_K, "self_attn.v_proj": l3hip.W_V,
             "self_attn.o_proj": l3hip.W_O, "mlp.gate_proj": l3hip.W_GATE, "mlp.up_proj": l3hip.W_UP,
             "mlp.down_proj": l3hip.W_DOWN, "input_layernorm": l3hip.W_ATTN_NORM,
             "post_attention_layernorm": l3hip.W_FFN_NORM}

    def upload():
        ctx.upload(0, l3hip.W_EMBED, w["model.embed_tokens.weight"])
        for i in range(args.n_layers):
            for n, kind in kinds.items():
                ctx.upload(i, kind, w[f"model.layers.{i}.{n}.weight"])
        ctx.upload(0, l3hip.W_FINAL_NORM, w["model.norm.weight"])
        ctx.upload(0, l3hip.W_LM_HEAD, w["lm_head.weight"])

    return ctx, upload


def test_mode_0_is_a_context_never_given_the_setting(env):
    args, hidden = SHAPES["tiny"]
    w = make_weights(args, hidden)
    ids = np.random.default_rng(7).integers(0, args.vocab_size, (3, 5))
    step = np.random.default_rng(8).integers(0, args.vocab_size, (3, 1))
    plain = llama3.Llama(w, args, device=0)
    base = np.concatenate([_bits(plain(ids, 0)), _bits(plain(step, 5))], axis=1)
    ctx, upload = _manual_context(w, args, hidden)
    ctx.set_weight_fp8(2)
    ctx.set_weight_fp8(0)
    ctx.set_weight_bf16_rows(64, 0)
    upload()
    ctx.finalize()
    got = np.concatenate([_bits(ctx.forward(ids, 0)), _bits(ctx.forward(step, 5))], axis=1)
    assert np.array_equal(got.reshape(base.shape), base)
    assert ctx.weight_fp8_info() == {"mode": 0, "bytes": 0, "gemv_launches": 0, "rows_launches": 0}


def test_exact_mode(env):
    args, hidden = SHAPES["tiny"]
    w = make_weights(args, hidden)
    wr = rounded(w)
    prompt = np.random.default_rng(7).integers(0, args.vocab_size, (3, 5))

    def run(weights, dtype, rows=64):
        model = llama3.Llama(weights, args, device=0, weight_dtype=dtype)
        model.context.set_weight_bf16_rows(rows, 0)
        out = [_bits(model(prompt, 0))]
        out.append(_bits(model(out[0].view(np.float32)[:, 0].argmax(-1)[:, None], 5)))
        out.append(_bits(model(out[1].view(np.float32)[:1, 0].argmax(-1)[:, None], 6)))  # one row: the GEMV
        info = model.context.weight_fp8_info()
        if dtype:
            assert info["gemv_launches"] > 0 and (info["rows_launches"] > 0) == (rows > 0)
        return np.concatenate(out, axis=0), info

    a, info = run(wr, "fp8-e4m3")
    assert info["mode"] == 1
    b, _ = run(wr, "fp8-e4m3-round")
    assert np.array_equal(a, b)  # bitwise
    c, _ = run(w, "fp8-e4m3-round")
    assert np.array_equal(a, c)  # rounding on the device is round_fp8_rows
    # the fp32 kernels on W_q: the same model to fp32 rounding
    fp32, _ = run(wr, None, rows=0)
    tol = 1e-4 + 2e-4 * np.abs(fp32.view(np.float32).astype(np.float64))
    assert np.all(np.abs(a.view(np.float32).astype(np.float64) - fp32.view(np.float32)) <= tol)
    # one element one ulp off: refused, naming the tensor; the process goes on
    name = "model.layers.1.mlp.up_proj.weight"
    bad = dict(wr)
    bad[name] = wr[name].copy()
    bad[name][37, 11] = np.nextafter(bad[name][37, 11], np.float32(np.inf))
    with pytest.raises(ValueError, match=r"model\.layers\.1\.mlp\.up_proj\.weight \(layer 1, kind 6\) has 1 elements"):
        llama3.Llama(bad, args, device=0, weight_dtype="fp8-e4m3")
    bad2 = dict(wr)
    bad2["lm_head.weight"] = w["lm_head.weight"]
    with pytest.raises(ValueError, match=r"lm_head\.weight"):
        llama3.Llama(bad2, args, device=0, weight_dtype="fp8-e4m3")
    # a non-finite element fails both modes, by name
    bad3 = dict(wr)
    bad3["model.layers.0.self_attn.k_proj.weight"] = wr["model.layers.0.self_attn.k_proj.weight"].copy()
    bad3["model.layers.0.self_attn.k_proj.weight"][3, 3] = np.inf
    for dtype in ("fp8-e4m3", "fp8-e4m3-round"):
        with pytest.raises(ValueError, match=r"model\.layers\.0\.self_attn\.k_proj\.weight.*not finite"):
            llama3.Llama(bad3, args, device=0, weight_dtype=dtype)
    # the nudged arrays still load rounded
    e, _ = run(bad, "fp8-e4m3-round")
    assert np.array_equal(e, a)


def test_max_rows_0_leaves_multi_row_launches_on_the_fp32_routes(env):
    """Twelve rows (past the GEMV's eight) with the rows kernel off: every launch of a 12 x 5
    prefill and of a 12-row decode step runs the fp32 kernels on the rounded fp32 copies — the bits
    of an fp32 model given W_q."""
    args, hidden = SHAPES["tiny"]
    w = make_weights(args, hidden)
    ids = np.random.default_rng(7).integers(0, args.vocab_size, (12, 5))
    step = np.random.default_rng(8).integers(0, args.vocab_size, (12, 1))
    fp32 = llama3.Llama(rounded(w), args, device=0)
    base = np.concatenate([_bits(fp32(ids, 0)), _bits(fp32(step, 5))], axis=1)
    m = llama3.Llama(w, args, device=0, weight_dtype="fp8-e4m3-round")
    m.context.set_weight_bf16_rows(0)
    assert np.array_equal(np.concatenate([_bits(m(ids, 0)), _bits(m(step, 5))], axis=1), base)
    info = m.context.weight_fp8_info()
    assert info["rows_launches"] == 0 and info["gemv_launches"] == 0 and info["bytes"] > 0
    m.context.set_weight_bf16_rows(64, 0)
    m.context.reset_cache()
    got = np.concatenate([_bits(m(ids, 0)), _bits(m(step, 5))], axis=1)
    assert m.context.weight_fp8_info()["rows_launches"] > 0 and not np.array_equal(got, base)
    want = base.view(np.float32).astype(np.float64)
    assert np.all(np.abs(got.view(np.float32) - want) <= 1e-4 + 2e-4 * np.abs(want))


def test_exact_mode_failure_leaves_the_context_usable(env):
    args, hidden = SHAPES["tiny"]
    w = make_weights(args, hidden)
    ctx, upload = _manual_context(w, args, hidden)
    ctx.set_weight_fp8(1)
    upload()
    with pytest.raises(RuntimeError, match=r"model\.layers\.0\.self_attn\.q_proj\.weight \(layer 0, kind 1\)"):
        ctx.finalize()
    assert ctx.weight_fp8_info() == {"mode": 1, "bytes": 0, "gemv_launches": 0, "rows_launches": 0}
    ctx.set_weight_fp8(2)
    ctx.finalize()
    ids = np.random.default_rng(7).integers(0, args.vocab_size, (1, 5))
    want = orc.OracleModel(f64(rounded(w)), dataclasses.replace(args, max_batch_size=1))(ids, 0)[:, -1, :]
    close(ctx.forward(ids, 0), want, "finalized again in round mode")
    with pytest.raises(RuntimeError, match="already finalized"):
        ctx.set_weight_fp8(0)


def test_one_compact_copy_per_context(env, monkeypatch):
    args, hidden = SHAPES["tiny"]
    dims = llama3._dims(args, hidden, 0, 0)
    c = l3hip.Context(dims, 0)
    c.set_weight_bf16(2)
    with pytest.raises(RuntimeError, match="l3_set_weight_fp8: bf16 weight storage is set"):
        c.set_weight_fp8(1)
    c.set_weight_bf16(0)
    c.set_weight_fp8(1)
    with pytest.raises(RuntimeError, match="l3_set_weight_bf16: fp8 weight storage is set"):
        c.set_weight_bf16(2)
    c.set_weight_bf16(0)  # off is always taken
    assert c.weight_fp8_info()["mode"] == 1 and c.weight_bf16_info()["mode"] == 0
    with pytest.raises(RuntimeError, match="mode 3"):
        c.set_weight_fp8(3)
    # the environment sets the mode of new contexts; both at once is an error at l3_create
    monkeypatch.setenv("L3_WEIGHT_FP8", "2")
    assert l3hip.Context(dims, 0).weight_fp8_info()["mode"] == 2
    monkeypatch.setenv("L3_WEIGHT_BF16", "1")
    with pytest.raises(RuntimeError, match="L3_WEIGHT_BF16 and L3_WEIGHT_FP8"):
        l3hip.Context(dims, 0)


def test_group_member_is_refused(env, monkeypatch):
    monkeypatch.setenv("L3_GROUP_VIRTUAL", "1")
    monkeypatch.setenv("L3_WEIGHT_FP8", "2")
    args, hidden = SHAPES["tiny"]
    dims = llama3._dims(args, hidden, args.n_layers, args.vocab_size)
    grp = l3hip.Group(dims, [0, 0])
    for mem in grp.members:
        assert mem.weight_fp8_info()["mode"] == 0
        with pytest.raises(RuntimeError, match="multi-device"):
            mem.set_weight_fp8(1)
        mem.set_weight_fp8(0)
    grp.close()
    one = l3hip.Group(dims, [0])
    assert one.members[0].weight_fp8_info()["mode"] == 2
    one.close()


@pytest.mark.parametrize("case", ["tiny"], indirect=True)
def test_a_change_of_the_rows_setting_recaptures(case):
    m, ctx = case.model, case.model.context
    total = 5 + 20
    want, _, margin = case.oracle("b3_recapture", case.pB[:3], total)
    assert margin >= MARGIN
    ctx.set_weight_bf16_rows(0)
    ctx.set_weight_bf16_rows(64)  # a change: whatever an earlier test captured is dropped
    n0 = case.info()["rows_launches"]
    assert np.array_equal(m.generate_all(case.pB[:3], total), want)
    n1 = case.info()["rows_launches"]
    assert n1 > n0
    ctx.reset_cache()
    assert np.array_equal(m.generate_all(case.pB[:3], total), want)  # replays: nothing is captured again
    prefill = case.info()["rows_launches"] - n1
    assert 0 < prefill < n1 - n0
    ctx.set_weight_bf16_rows(0)
    ctx.reset_cache()
    n2 = case.info()["rows_launches"]
    assert np.array_equal(m.generate_all(case.pB[:3], total), want)
    assert case.info()["rows_launches"] == n2  # captured again, without the rows kernel
    ctx.set_weight_bf16_rows(64)
    ctx.reset_cache()
    assert np.array_equal(m.generate_all(case.pB[:3], total), want)
    assert case.info()["rows_launches"] - n2 == n1 - n0  # ... and again with it


# ---- 7. the check build ------------------------------------------------------------------------------

def test_check_build_records_no_violation(env):
    if not os.path.exists(CHECK_LIB):
        pytest.skip(f"{CHECK_LIB} missing")
    envv = dict(os.environ, L3_LIB_PATH=CHECK_LIB, L3_DECODE_PERSIST="0")
    r = subprocess.run([sys.executable, os.path.join(HERE, "weight_fp8_checks_workload.py")], env=envv,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["enabled"] is True and out["rows_launches"] > 0 and out["gemv_launches"] > 0
    assert out["counts"] == {"kv_slot": 0, "attn_keys": 0, "token_id": 0}
    c = _cases.get("tiny") or Case("tiny")
    _cases["tiny"] = c
    total = c.args.max_seq_len
    want, _, margin = c.oracle("b12_full", c.pB, total)
    assert margin >= MARGIN
    assert out["generate_all"] == want.tolist()
    want1, _, margin = c.oracle("b1_full", c.p5, total)
    assert margin >= MARGIN and out["generate_b1"] == want1.tolist()
    for b, p in enumerate(c.rag):
        ids, mg = c.alone(p, total)
        assert mg >= MARGIN and out["ragged"][b] == ids.tolist(), b
