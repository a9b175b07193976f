"""bf16 weight storage for 2-64 rows (DESIGN.md "bf16 weight storage for 2-64 rows";
l3_set_weight_bf16_rows, gemm_rows_bf16_kernel).

As in test_gpu_weight_bf16.py the reference of every model comparison is the float64 oracle run on
weights whose matrix kinds went through utils.round_bf16, the bars are atol 1e-4 + rtol 2e-4 on
logits and exact greedy ids (after asserting a top-1 margin of 1e-3 on the oracle alone), and every
model has non-unit norm weights.  The models are far below the default min_bytes, so every model
under test sets set_weight_bf16_rows(64, 0); L3_DECODE_PERSIST=0 throughout.

Measured on an MI355X (section 2, printed by the test): see DESIGN.md."""

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
from test_gpu_weight_bf16 import MARGIN, close, f64, make_weights, oracle_loop, rounded

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHECK_LIB = os.path.join(os.path.dirname(HERE), "llama3.np_amd", "csrc", "libllama3hip_check.so")
DEFAULTS = {"max_rows": 32, "min_bytes": 32 << 20, "launches": 0}  # the documented defaults

# tiny: HD 16 / n_rep 2, two layers (17 rows: one past a max_rows of 16); gqa: one layer of HD 128 /
# n_rep 4 (test_gpu_weight_bf16.py's shapes with more batch rows)
SHAPES = {
    "tiny": (synth.tiny(17), synth.TINY_HIDDEN),
    "gqa": (ModelArgs(dim=512, n_layers=1, n_heads=4, n_kv_heads=1, vocab_size=1024, max_seq_len=96,
                      max_batch_size=12), 256),
}
# projection launches of one step: q|k|v, o, gate|up, down per layer and the lm_head
STEP_LAUNCHES = {name: 4 * a.n_layers + 1 for name, (a, _) in SHAPES.items()}


class Case:
    """One model: the weights, the rounded-weight oracle's results (made once, never changed) and
    the bf16-round model under test with the rows kernel on for every weight."""

    def __init__(self, name):
        self.name = name
        self.args, self.hidden = SHAPES[name]
        self.w = make_weights(self.args, self.hidden)
        self.w64 = f64(rounded(self.w))
        rng = np.random.default_rng(8)  # (a seed whose 12 rows keep the top-1 margin to the last slot)
        self.pB = rng.integers(0, self.args.vocab_size, (12, 5))
        self._memo = {}
        self.model = llama3.Llama(self.w, self.args, device=0, weight_dtype="bf16-round")
        self.model.context.set_weight_bf16_rows(64, 0)

    def oracle(self, key, prompt, total):
        if key not in self._memo:
            self._memo[key] = oracle_loop(self.w64, dataclasses.replace(self.args, max_batch_size=prompt.shape[0]),
                                          prompt, total)
        return self._memo[key]

    def alone(self, prompt, total):
        """ids and least margin of one row alone on a zeroed cache."""
        key = ("alone", tuple(int(t) for t in prompt), total)
        if key not in self._memo:
            ids, _, mg = oracle_loop(self.w64, dataclasses.replace(self.args, max_batch_size=1),
                                     np.asarray(prompt)[None], total)
            self._memo[key] = (ids[0], mg)
        return self._memo[key]

    def launches(self):
        return self.model.context.weight_bf16_rows_info()["launches"]


_cases = {}


@pytest.fixture
def env(monkeypatch):
    monkeypatch.setenv("L3_DECODE_PERSIST", "0")
    for k in ("L3_WEIGHT_BF16", "L3_WEIGHT_BF16_ROWS", "L3_WEIGHT_BF16_MIN_BYTES"):
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


# ---- 1. the kernel, integer-exact ----------------------------------------------------------------

ROWS = (2, 3, 8, 9, 16, 17, 31, 32, 33, 64)


def _int_x(rng, rows, K, norm):
    """Small integers: every product and every partial sum is an integer below 2^24, so fp32 is
    exact in any order; with the norm, x = +-2 and eps = 0 make 1 / rms(x) exactly 0.5."""
    x = (rng.choice([-2.0, 2.0], (rows, K)) if norm else rng.integers(-4, 5, (rows, K))).astype(np.float32)
    g = rng.choice([-2.0, -1.0, 1.0, 2.0, 3.0], K).astype(np.float32) if norm else None
    assert np.abs(x).max() * (3 if norm else 1) * 4 * K < 2 ** 24
    return x, g


def _want(x, g, w):
    return (((x * g) @ w.T) * np.float32(0.5) if g is not None else x @ w.T).astype(np.float32)


def _check_exact(ctx, x, g, w, wb, what):
    want = _want(x, g, w)
    if want.shape[1] > 4 and x.shape[1] > 32:  # on the reference alone: a wrong row, column or k piece shows
        assert len({r.tobytes() for r in want}) == want.shape[0]
        xg = x * g if g is not None else x
        s = np.float32(0.5) if g is not None else np.float32(1)
        for sl in (slice(0, -8), slice(8, None)):
            assert np.all(np.any((xg[:, sl] @ w[:, sl].T) * s != want, axis=1))
    got = ctx.op_linear_bf16_rows(x, wb, g, 0.0)
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (what, bad[:4], got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("K", [32, 288, 4096, 14336])
def test_kernel_integer_exact(ctx, K):
    """op_linear_bf16_rows == NumPy bitwise.  rows: one, two and four row tiles, both sides of each
    tile edge, clamped rows.  K: one piece per lane (most waves idle), uneven wave shares, the two
    Llama K.  N: below one tile, a partly filled last tile, many blocks."""
    rng = np.random.default_rng(K)
    n0 = ctx.weight_bf16_rows_info()["launches"]
    calls = 0
    for N in (4, 100, 2052):
        w = rng.integers(-4, 5, (N, K)).astype(np.float32)
        wb = utils.bf16_bits(w)
        assert np.array_equal(utils.round_bf16(w), w)
        for rows in ROWS:
            for norm in (False, True):
                x, g = _int_x(rng, rows, K, norm)
                _check_exact(ctx, x, g, w, wb, (K, N, rows, norm))
                calls += 1
    assert ctx.weight_bf16_rows_info()["launches"] == n0 + calls


@pytest.mark.parametrize("N", [8192, 8256])
def test_kernel_integer_exact_nontemporal(ctx, N):
    """A bf16 weight of at least 64 MB: the non-temporal loads, on the eight-wave blocks (N / 16 = 512
    blocks) and on the four-wave blocks (516)."""
    rng = np.random.default_rng(N)
    K = 4096
    w = rng.integers(-4, 5, (N, K)).astype(np.float32)
    wb = utils.bf16_bits(w)
    assert w.size * 2 >= 64 << 20
    for rows, norm in ((2, True), (17, False), (64, True)):
        x, g = _int_x(rng, rows, K, norm)
        _check_exact(ctx, x, g, w, wb, (N, rows, norm))


def test_kernel_integer_exact_four_wave_blocks(ctx):
    """More than 512 blocks below the non-temporal threshold: the four-wave form with plain loads."""
    rng = np.random.default_rng(5)
    N, K = 8256, 288
    w = rng.integers(-4, 5, (N, K)).astype(np.float32)
    wb = utils.bf16_bits(w)
    for rows in (3, 17, 33, 64):
        for norm in (False, True):
            x, g = _int_x(rng, rows, K, norm)
            _check_exact(ctx, x, g, w, wb, (rows, norm))


def test_kernel_refuses_other_shapes(ctx):
    w = np.zeros((8, 64), np.uint16)
    for rows in (1, 65):
        with pytest.raises(RuntimeError, match="rows"):
            ctx.op_linear_bf16_rows(np.zeros((rows, 64), np.float32), w)
    with pytest.raises(RuntimeError, match="multiple of 32"):
        ctx.op_linear_bf16_rows(np.zeros((2, 40), np.float32), np.zeros((8, 40), np.uint16))
    with pytest.raises(RuntimeError, match="multiple of 4"):
        ctx.op_linear_bf16_rows(np.zeros((2, 64), np.float32), np.zeros((6, 64), np.uint16))


# ---- 2. the kernel, random values ------------------------------------------------------------------

@pytest.mark.parametrize("rows,K,N", [(3, 4096, 2052), (33, 4096, 2052), (64, 14336, 100), (9, 288, 100)])
def test_kernel_random_values(ctx, rows, K, N):
    """Against the float64 product of the same bf16 values: the error is at most twice that of
    op_linear (the fp32 kernels) on float(w) with the same x, and a second call is bitwise equal."""
    rng = np.random.default_rng(rows * 1000 + N)
    x = rng.standard_normal((rows, K)).astype(np.float32)
    w = utils.round_bf16((rng.standard_normal((N, K)) * 0.05).astype(np.float32))
    want = x.astype(np.float64) @ w.astype(np.float64).T
    got = ctx.op_linear_bf16_rows(x, utils.bf16_bits(w))
    err = float(np.abs(got - want).max())
    err32 = float(np.abs(ctx.op_linear(x, w) - want).max())
    print(f"rows {rows} K {K} N {N}: bf16 rows kernel max-abs {err:.3e}, fp32 op_linear {err32:.3e}")
    assert err <= 2 * err32
    again = ctx.op_linear_bf16_rows(x, utils.bf16_bits(w))
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))
    # with the norm: the RMSNorm of the float64 x
    g = (1 + 0.25 * rng.standard_normal(K)).astype(np.float32)
    x64 = x.astype(np.float64)
    wantn = (x64 / np.sqrt((x64 ** 2).mean(-1, keepdims=True) + 1e-5) * g) @ w.astype(np.float64).T
    gotn = ctx.op_linear_bf16_rows(x, utils.bf16_bits(w), g, 1e-5)
    errn = float(np.abs(gotn - wantn).max())
    print(f"  with the norm: max-abs {errn:.3e} (|y| up to {np.abs(wantn).max():.1f})")
    assert np.all(np.abs(gotn - wantn) <= 1e-4 + 2e-4 * np.abs(wantn))


# ---- 3. the model, every epilogue ------------------------------------------------------------------

@pytest.mark.parametrize("B", [3, 12])
@pytest.mark.parametrize("case", ["tiny", "gqa"], indirect=True)
def test_eager_batched_decode_logits(case, B):
    """A prefill of B x 5 rows (15 and 60 rows: one and four row tiles, the pruned last layer's
    force_skinny launches) and eager decode steps of B rows, fed the oracle's ids."""
    m = case.model
    n0, g0 = case.launches(), m.context.weight_bf16_info()["gemv_launches"]
    ids, rows, _ = case.oracle(f"b{B}_short", case.pB[:B], 5 + 4)
    close(np.array(m(case.pB[:B], 0))[:, 0], rows[0], f"{case.name} B={B} prefill of 5")
    assert case.launches() > n0
    for i in range(1, 4):
        n1 = case.launches()
        close(m(ids[:, i - 1:i], 5 + i)[:, 0], rows[i], f"{case.name} B={B} decode step {i}")
        assert case.launches() == n1 + STEP_LAUNCHES[case.name]
    assert m.context.weight_bf16_info()["gemv_launches"] == g0  # no launch on the GEMV


@pytest.mark.parametrize("case", ["tiny", "gqa"], indirect=True)
def test_generate_all_batched_to_the_last_slot(case):
    """The captured batched step (QKV with pos_dev, every epilogue) to the last cache slot."""
    total = case.args.max_seq_len
    want, _, margin = case.oracle("b12_full", case.pB, total)
    print(f"{case.name}: min top-1 margin {margin:.3e} over {want.shape[1]} steps")
    assert margin >= MARGIN
    n0 = case.launches()
    assert np.array_equal(case.model.generate_all(case.pB, total), want)
    assert case.launches() > n0
    assert case.model.context.decode_stats()["graph_steps"] > 0


@pytest.mark.parametrize("case", ["tiny", "gqa"], indirect=True)
def test_generate_ragged_with_a_stop_id(case):
    lens, max_new = (1, 2, 3, 4, 5, 6, 7, 3, 1, 5), 24
    rng = np.random.default_rng(18)
    prompts = [rng.integers(0, case.args.vocab_size, n) for n in lens]
    rows, margin = [], np.inf
    for p in prompts:  # the reference: each row alone on a zeroed cache
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
    n0 = case.launches()
    got = case.model.generate_ragged(prompts, max_new, stop_ids=[stop])
    for b, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (b, g, w)
    assert case.launches() > n0


@pytest.mark.parametrize("case", ["tiny", "gqa"], indirect=True)
def test_extend_ragged_logits(case):
    """Two rows continue with five tokens each at different positions (a 10-row chunk)."""
    rng = np.random.default_rng(23)
    V = case.args.vocab_size
    prompts = [rng.integers(0, V, 3), rng.integers(0, V, 6)]
    chunks = [rng.integers(0, V, 5), rng.integers(0, V, 5)]
    m = case.model
    m.forward_ragged(prompts)
    n0 = case.launches()
    got = np.array(m.extend_ragged(chunks, [3, 6]))[:, 0]
    assert case.launches() > n0
    oracle = orc.OracleModel(case.w64, dataclasses.replace(case.args, max_batch_size=1))
    for b in range(2):
        want = oracle(np.concatenate([prompts[b], chunks[b]])[None], 0)[:, -1, :]
        close(got[b:b + 1], want, f"{case.name} extend row {b}")


@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("case", ["tiny", "gqa"], indirect=True)
def test_speculative_generation(case, B):
    """draft_len 3: chunks of 4 rows at B = 1 (the force_skinny route) and of 16 rows at B = 4; the
    lookup is each row's true continuation with every seventh id wrong, so drafts are accepted and
    rejected."""
    lens, max_new = (4, 2, 6, 3)[:B], 28
    rng = np.random.default_rng(29)
    V = case.args.vocab_size
    prompts = [rng.integers(0, V, n) for n in lens]
    truth = []
    for p in prompts:
        ids, mg = case.alone(p, max_new)
        assert mg >= MARGIN
        truth.append(ids)
    lookup = []
    for t in truth:
        bad = np.array(t, np.int64)
        bad[5::7] = (bad[5::7] + 1) % V
        lookup.append(bad)
    m = case.model
    step = STEP_LAUNCHES[case.name]
    n0 = case.launches()
    m.forward_ragged(prompts)  # the ragged prefill alone (its lm_head has one row per sequence)
    prefill = case.launches() - n0
    assert 0 < prefill <= step
    m.context.reset_cache()
    n0 = case.launches()
    plain = m.generate_ragged(prompts, max_new)
    n1 = case.launches()
    # one row decodes on the GEMV: only the prefill is on the rows kernel
    assert n1 - n0 == prefill if B == 1 else n1 - n0 > prefill
    m.context.reset_cache()
    got, stats = m.generate_ragged_spec(prompts, max_new, speculate=dict(draft_len=3, ngram_max=3, lookup=lookup))
    sim = [spec_ref.simulate(lookup[b], prompts[b], truth[b], 3, 3, 1) for b in range(B)]
    # every iteration's chunk (4 rows at B = 1: the force_skinny route) ran every projection on the
    # rows kernel: the prefill, then one launch per projection and iteration, the iterations those
    # of the row that ran longest
    iters = max(r[1] for r in sim)
    print(f"{case.name} B={B}: {case.launches() - n1} launches, prefill {prefill}, {iters} iterations of {step}")
    assert case.launches() - n1 == prefill + iters * step
    for b in range(B):
        assert np.array_equal(plain[b], truth[b]) and np.array_equal(got[b], plain[b]), b
        assert (int(stats["row_steps"][b]), int(stats["drafted"][b]), int(stats["accepted"][b])) == tuple(sim[b][1:]), b
    assert stats["accepted"].sum() > 0 and stats["drafted"].sum() > stats["accepted"].sum()


# ---- 4. dispatch edges -----------------------------------------------------------------------------

def _bits(a):
    return np.ascontiguousarray(np.array(a, np.float32)).view(np.uint32)


def test_off_is_the_context_without_the_setting(env):
    args, hidden = SHAPES["tiny"]
    w = make_weights(args, hidden)
    ids = np.random.default_rng(7).integers(0, args.vocab_size, (3, 5))
    step = np.random.default_rng(8).integers(0, args.vocab_size, (3, 1))

    def run(model):
        return np.concatenate([_bits(model(ids, 0)), _bits(model(step, 5))], axis=1)

    never = llama3.Llama(w, args, device=0, weight_dtype="bf16-round")
    assert never.context.weight_bf16_rows_info() == DEFAULTS
    base = run(never)
    assert never.context.weight_bf16_rows_info() == DEFAULTS  # tiny weights: below the default min_bytes
    off = llama3.Llama(w, args, device=0, weight_dtype="bf16-round")
    off.context.set_weight_bf16_rows(64, 0)
    off.context.set_weight_bf16_rows(0)
    assert off.context.weight_bf16_rows_info() == {"max_rows": 0, "min_bytes": 0, "launches": 0}
    assert np.array_equal(run(off), base)
    assert off.context.weight_bf16_rows_info()["launches"] == 0
    # on: another kernel, the same model
    on = llama3.Llama(w, args, device=0, weight_dtype="bf16-round")
    on.context.set_weight_bf16_rows(64, 0)
    got = run(on).view(np.float32).astype(np.float64)
    want = base.view(np.float32).astype(np.float64)
    assert on.context.weight_bf16_rows_info()["launches"] > 0
    assert np.all(np.abs(got - want) <= 1e-4 + 2e-4 * np.abs(want))
    # None keeps a value; the environment sets both for new contexts
    on.context.set_weight_bf16_rows(None, 4096)
    assert on.context.weight_bf16_rows_info()["max_rows"] == 64
    on.context.set_weight_bf16_rows(8)
    assert on.context.weight_bf16_rows_info()["min_bytes"] == 4096
    for bad in ((1, None), (65, None), (-2, None), (None, -2)):
        with pytest.raises(RuntimeError, match="max_rows|min_bytes"):
            on.context.set_weight_bf16_rows(*bad)


def test_environment_sets_the_defaults(env, monkeypatch):
    args, hidden = SHAPES["tiny"]
    dims = llama3._dims(args, hidden, 0, 0)
    monkeypatch.setenv("L3_WEIGHT_BF16_ROWS", "16")
    monkeypatch.setenv("L3_WEIGHT_BF16_MIN_BYTES", "12345")
    assert l3hip.Context(dims, 0).weight_bf16_rows_info() == {"max_rows": 16, "min_bytes": 12345, "launches": 0}
    # values out of range and text that is not a number are ignored, not read as 0
    for rows, mb in (("abc", "abc"), ("1", "-5"), ("65", "12x"), ("8 rows", "1e6"), ("", "")):
        monkeypatch.setenv("L3_WEIGHT_BF16_ROWS", rows)
        monkeypatch.setenv("L3_WEIGHT_BF16_MIN_BYTES", mb)
        assert l3hip.Context(dims, 0).weight_bf16_rows_info() == DEFAULTS, (rows, mb)
    monkeypatch.setenv("L3_WEIGHT_BF16_ROWS", "0")
    monkeypatch.setenv("L3_WEIGHT_BF16_MIN_BYTES", "0")
    assert l3hip.Context(dims, 0).weight_bf16_rows_info() == {"max_rows": 0, "min_bytes": 0, "launches": 0}


def test_batch_split_stays_bit_identical(env):
    """l3_set_batch_split's contract with the rows kernel on for every weight: 17 sequences of 40
    tokens run whole (a pruned last layer and an lm_head of 17 rows: two row tiles) and as parts of
    8 and 9 sequences (one row tile each) give the same bits, because launches whose M is a part's
    share of the rows stay off the kernel, and the lm_head runs once on the whole batch."""
    args, hidden = SHAPES["tiny"]
    w = make_weights(args, hidden)
    ids = np.random.default_rng(41).integers(0, args.vocab_size, (17, 40))
    out = {}
    for parts in (1, 2):
        m = llama3.Llama(w, args, device=0, weight_dtype="bf16-round")
        m.context.set_weight_bf16_rows(64, 0)
        m.context.set_batch_split(parts, 1)
        out[parts] = _bits(m(ids, 0))
        out[parts, "launches"] = m.context.weight_bf16_rows_info()["launches"]
    assert np.array_equal(out[1], out[2])
    # the lm_head (17 rows, once) is on the rows kernel in both; the layers (680 or 320 / 360 rows)
    # and the pruned last layer (split_rows) are not
    assert out[1, "launches"] == 1 and out[2, "launches"] == 1


@pytest.mark.parametrize("case", ["tiny"], indirect=True)
def test_row_and_byte_thresholds(case):
    m, ctx, args = case.model, case.model.context, case.args
    rng = np.random.default_rng(11)
    step = STEP_LAUNCHES["tiny"]

    def run(B, pos):
        n0, g0 = case.launches(), ctx.weight_bf16_info()["gemv_launches"]
        m(rng.integers(0, args.vocab_size, (B, 1)), pos)
        return case.launches() - n0, ctx.weight_bf16_info()["gemv_launches"] - g0

    ctx.set_weight_bf16_rows(16, 0)
    assert run(17, 0)[0] == 0  # past max_rows: no launch of the rows kernel
    assert run(16, 1)[0] == step and run(2, 2)[0] == step
    rows1, gemv1 = run(1, 3)  # one row: the GEMV, never the rows kernel
    assert rows1 == 0 and gemv1 > 0
    # min_bytes is inclusive: the tiny wo is 64 x 64 bf16 = 8192 bytes, the smallest tensor
    wo = args.dim * args.dim * 2
    sizes = [(args.dim + 2 * (args.dim // args.n_heads) * args.kv_heads) * args.dim * 2, wo,
             2 * case.hidden * args.dim * 2, args.dim * case.hidden * 2]
    assert min(sizes) == wo == 8192 and args.vocab_size * args.dim * 2 > wo
    ctx.set_weight_bf16_rows(64, wo)
    assert run(3, 4)[0] == step
    ctx.set_weight_bf16_rows(64, wo + 1)
    assert run(3, 5)[0] == step - args.n_layers  # every tensor but the two wo
    ctx.set_weight_bf16_rows(64, sizes[0] + 1)   # past wqkv too: gate|up, down, lm_head
    assert run(3, 6)[0] == 2 * args.n_layers + 1


def test_mode_0_takes_no_effect(env):
    args, hidden = SHAPES["tiny"]
    w = make_weights(args, hidden)
    ids = np.random.default_rng(7).integers(0, args.vocab_size, (3, 5))
    plain = llama3.Llama(w, args, device=0)
    base = _bits(plain(ids, 0))
    fp32 = llama3.Llama(w, args, device=0)
    fp32.context.set_weight_bf16_rows(64, 0)
    assert np.array_equal(_bits(fp32(ids, 0)), base)
    assert fp32.context.weight_bf16_rows_info() == {"max_rows": 64, "min_bytes": 0, "launches": 0}


def test_group_member_is_refused(env, monkeypatch):
    monkeypatch.setenv("L3_GROUP_VIRTUAL", "1")
    args, hidden = SHAPES["tiny"]
    dims = llama3._dims(args, hidden, args.n_layers, args.vocab_size)
    grp = l3hip.Group(dims, [0, 0])
    for mem in grp.members:
        with pytest.raises(RuntimeError, match="multi-device"):
            mem.set_weight_bf16_rows(8, 0)
    grp.close()
    one = l3hip.Group(dims, [0])
    one.members[0].set_weight_bf16_rows(8, 0)
    one.close()


@pytest.mark.parametrize("case", ["tiny"], indirect=True)
def test_a_change_recaptures_the_decode_steps(case):
    m, ctx = case.model, case.model.context
    total = 5 + 20
    want, _, margin = case.oracle("b3_recapture", case.pB[:3], total)
    assert margin >= MARGIN
    ctx.set_weight_bf16_rows(0)
    ctx.set_weight_bf16_rows(64)  # a change: whatever an earlier test captured is dropped
    n0 = case.launches()
    assert np.array_equal(m.generate_all(case.pB[:3], total), want)
    n1 = case.launches()
    assert n1 > n0
    ctx.reset_cache()
    assert np.array_equal(m.generate_all(case.pB[:3], total), want)  # replays: nothing is captured again
    prefill = case.launches() - n1
    assert 0 < prefill < n1 - n0
    ctx.set_weight_bf16_rows(0)
    ctx.reset_cache()
    n2 = case.launches()
    assert np.array_equal(m.generate_all(case.pB[:3], total), want)
    assert case.launches() == n2  # captured again, without the rows kernel
    ctx.set_weight_bf16_rows(64)
    ctx.reset_cache()
    assert np.array_equal(m.generate_all(case.pB[:3], total), want)
    assert case.launches() - n2 == n1 - n0  # ... and again with it


# ---- 5. exact mode -----------------------------------------------------------------------------------

def test_exact_mode_is_round_mode_bitwise(env):
    args, hidden = SHAPES["tiny"]
    wr = rounded(make_weights(args, hidden))
    prompt = np.random.default_rng(7).integers(0, args.vocab_size, (3, 5))

    def run(dtype):
        model = llama3.Llama(wr, args, device=0, weight_dtype=dtype)
        model.context.set_weight_bf16_rows(64, 0)
        out = [_bits(model(prompt, 0))]
        out.append(_bits(model(out[0].view(np.float32)[:, 0].argmax(-1)[:, None], 5)))
        assert model.context.weight_bf16_rows_info()["launches"] > 0
        return np.concatenate(out, axis=1)

    assert np.array_equal(run("bf16"), run("bf16-round"))


# ---- 6. the check build ------------------------------------------------------------------------------

def test_check_build_records_no_violation(env):
    if not os.path.exists(CHECK_LIB):
        pytest.skip(f"{CHECK_LIB} missing")
    envv = dict(os.environ, L3_LIB_PATH=CHECK_LIB, L3_DECODE_PERSIST="0")
    r = subprocess.run([sys.executable, os.path.join(HERE, "weight_bf16_rows_checks_workload.py")], env=envv,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["enabled"] is True and out["launches"] > 0
    assert out["counts"] == {"kv_slot": 0, "attn_keys": 0, "token_id": 0}
    c = _cases.get("tiny") or Case("tiny")
    _cases["tiny"] = c
    total = c.args.max_seq_len
    want, _, margin = c.oracle("b12_full", c.pB, total)
    assert margin >= MARGIN
    assert out["generate_all"] == want.tolist()
    assert all(len(r) == total - n for r, n in zip(out["ragged"], out["ragged_lens"]))
