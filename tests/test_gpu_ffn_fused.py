"""The fused FFN kernel (ffn_fused.h; l3_set_ffn_fused) against the gate|up and down launches it
replaces.

The kernel keeps each row's residual panel and SwiGLU output in registers and runs every MFMA
chain, the row factor, SwiGLU and the residual add in the order of the two tiled fp32 launches, so
its output must be bit-identical to theirs: the kernel-level tests compare ``fused=True`` with
``fused=False`` of ``l3_op_ffn_block_host`` by ``np.array_equal``, the model-level ones the same
calls on fresh models with the path on and off.  The pair itself is checked once against a float64
restatement with the bound tests/test_gpu_gemm_routes.py applies to the tiled fp32 routes
(gemm_epi_ref: the worst case K 2^-24 |x| @ |w|.T of a K-term sum, carried through SwiGLU and into
down's input).

Two of the planned shapes cannot reach the pair as planned.  The tiled down kernel stages hidden in
whole 32-deep k-tiles and ``launch_gemm`` refuses any other K, so at hidden 16 and 48 the pair arm
of ``l3_op_ffn_block_host`` appends 16 zero hidden units (zero gate / up rows, zero down columns):
they give silu(0) * 0 = 0 and add exact zeros at the end of every down sum, so the pair's result
is what hidden 16 / 48 would give and the fused kernel runs the planned, unpadded shapes.  And
``l3_create`` refuses a model whose hidden size is not a multiple of 32, so the model-level tests
use hidden 64 (four stages, each buffer reused) where 48 was planned.
"""

import os
import tempfile

import numpy as np
import pytest

import gemm_epi_ref as ref
import l3hip
import llama3
import synth
from config import ModelArgs
from gemm_epi_ref import U

pytestmark = pytest.mark.gpu

DIM = 288
EPS = 1e-6  # l3hip.op_context's norm_eps


@pytest.fixture(scope="module")
def ctx():
    return l3hip.op_context(0)


def _operands(rows, hidden, seed, dim=DIM):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, dim)).astype(np.float32)
    x[rows // 2] = 0.0  # one all-zero row: sum of squares 0, row factor 1 / sqrt(eps)
    wg, wu = (0.05 * rng.standard_normal((2, hidden, dim))).astype(np.float32)
    wd = (0.05 * rng.standard_normal((dim, hidden))).astype(np.float32)
    return x, wg, wu, wd


# rows: 257 the last block owns one row, 300 a partial last block, 384 whole blocks (a block owns
# 128 rows or, in the narrower tuning shapes, 64); hidden: 16 one stage and no refill, 32 each
# buffer once, 48 a buffer reused, 768 the product shape (once, at rows 300)
SHAPES = [(r, h) for r in (257, 300, 384) for h in (16, 32, 48)] + [(300, 768)]


@pytest.mark.parametrize("norm", [True, False], ids=["norm", "plain"])
@pytest.mark.parametrize("rows,hidden", SHAPES)
def test_fused_equals_pair(ctx, rows, hidden, norm):
    x, wg, wu, wd = _operands(rows, hidden, seed=rows * 1000 + hidden)
    pair = ctx.op_ffn_block(x, wg, wu, wd, norm, fused=False)
    fused = ctx.op_ffn_block(x, wg, wu, wd, norm, fused=True)
    assert np.isfinite(pair).all()
    assert not np.array_equal(pair, x)  # the FFN term is there
    bad = np.argwhere(fused != pair)
    assert bad.size == 0, (len(bad), bad[:4].tolist(), fused[tuple(bad[0])], pair[tuple(bad[0])])
    # a second launch gives the same bits
    assert np.array_equal(ctx.op_ffn_block(x, wg, wu, wd, norm, fused=True), fused)


def test_pair_against_float64(ctx):
    """The two launches at (300, 48) with the norm against float64, bound as for the tiled fp32
    EPI_SWIGLU and EPI_RESID routes: SwiGLU's bound on hidden goes through |wd| into the output
    beside down's own K-term sum and the residual add's rounding."""
    rows, hidden = 300, 48
    x, wg, wu, wd = _operands(rows, hidden, seed=7)
    got = ctx.op_ffn_block(x, wg, wu, wd, True, fused=False)
    hid, bh, _ = ref.ref_swiglu(x, wg, wu, norm=True, eps=EPS)
    wd64 = np.abs(wd.astype(np.float64))
    want = x.astype(np.float64) + hid @ wd.astype(np.float64).T
    bound = bh @ wd64.T + hidden * U * ((np.abs(hid) + bh) @ wd64.T) + U * np.abs(want)
    err = np.abs(got.astype(np.float64) - want)
    nz = bound > 0  # (the all-zero row: both sides exactly 0)
    print(f"\n[ffn block] worst error / bound: {float((err[nz] / bound[nz]).max()):.4f}")
    over = np.argwhere(err > bound)
    assert over.size == 0, (len(over), over[:4].tolist(), err[tuple(over[0])], bound[tuple(over[0])])


@pytest.mark.parametrize("rows,dim,hidden", [(300, 256, 32), (300, 288, 24), (256, 288, 32)],
                         ids=["dim256", "hidden24", "rows256"])
def test_refusals(ctx, rows, dim, hidden):
    """Shapes the fused kernel does not take are errors, never the pair in its place."""
    x, wg, wu, wd = _operands(rows, hidden, seed=1, dim=dim)
    with pytest.raises(RuntimeError):
        ctx.op_ffn_block(x, wg, wu, wd, True, fused=True)


# ---- model level ---------------------------------------------------------------------------------

HIDDEN = 64
VS = 320
B, L = 3, 100


@pytest.fixture(scope="module")
def tmp():
    with tempfile.TemporaryDirectory() as d:
        yield d


def _args(batch=B):
    return ModelArgs(dim=DIM, n_layers=2, n_heads=6, n_kv_heads=6, vocab_size=VS, max_seq_len=256,
                     max_batch_size=batch)


@pytest.fixture(scope="module")
def weights(tmp):
    path = os.path.join(tmp, "ffn.npz")
    synth.save_npz(path, synth.make_weights(_args(), HIDDEN, seed=3, preset="sharp"))
    return path


def _model(path, on, batch=B, **kw):
    m = llama3.Llama(path, _args(batch), **kw)
    m.context.set_ffn_fused(on)
    m.context.kernel_timing(True, ["ffn"])
    return m


def _counts(m):
    st = m.context.kernel_stats()
    return st["ffn"][1], st["gateup"][1], st["down"][1]


def _run_both(path, fn, batch=B, expect_fused=True):
    outs = []
    for on in (True, False):
        m = _model(path, on, batch)
        outs.append(fn(m))
        assert (_counts(m)[0] > 0) == (on and expect_fused)
    for k, (a, b) in enumerate(zip(*outs)):
        assert np.array_equal(a, b), f"output {k}: fused path differs from the two launches"


def test_model_prefill_chunk_decode_score(weights):
    """Logits of B 3 x L 100 at 0, of a second chunk of 90 at 100, four greedy decode steps over
    every slot both wrote, and the scores of every position: on == off bit for bit."""
    rng = np.random.default_rng(5)
    ids, ids2 = rng.integers(0, VS, (B, L)), rng.integers(0, VS, (B, 90))

    def fn(m):
        outs = [np.array(m(ids, 0)), np.array(m(ids2, L))]
        pos = L + 90
        for _ in range(4):
            nxt = outs[-1][:, -1].argmax(-1)[:, None]
            outs.append(np.array(m(nxt, pos)))
            pos += 1
        lp, am = m.score(ids, np.roll(ids, -1, axis=1), 0, return_argmax=True)
        return outs + [np.array(lp), np.array(am)]

    _run_both(weights, fn)


def test_model_last_layer_all_rows(weights):
    ids = np.random.default_rng(6).integers(0, VS, (B, L))

    def fn(m):
        m.context.set_last_layer_rows(True)
        return [np.array(m(ids, 0))]

    _run_both(weights, fn)


def test_model_batch_split(weights):
    """B 6 x L 100 as one part of 600 rows and as two of 300, fused on and off: all four equal."""
    ids = np.random.default_rng(7).integers(0, VS, (6, L))
    outs = []
    for on in (True, False):
        for parts in (1, 2):
            m = _model(weights, on, batch=6)
            m.context.set_batch_split(parts, 257)
            outs.append(np.array(m(ids, 0)))
            assert (_counts(m)[0] > 0) == on
    for o in outs[1:]:
        assert np.array_equal(o, outs[0])


def test_model_ragged_forward(weights):
    rng = np.random.default_rng(8)
    prompts = [rng.integers(0, VS, n) for n in (100, 37, 1)]
    _run_both(weights, lambda m: [np.array(m.forward_ragged(prompts))])


def test_accounting(weights):
    """A 2-layer all-rows forward: ffn, gateup and down count 2 each and gateup + down == ffn in
    ms; x6, bf16 or fp8 weights, or the knob off, leave the ffn count at 0."""
    ids = np.random.default_rng(9).integers(0, VS, (B, L))
    m = llama3.Llama(weights, _args())
    m.context.set_last_layer_rows(True)
    for names in (["ffn"], ["gateup"], ["down"], None):
        m.context.kernel_timing(True, names)
        m(ids, 0)
        st = m.context.kernel_stats()
        assert (st["ffn"][1], st["gateup"][1], st["down"][1]) == (2, 2, 2), names
        assert st["ffn"][0] > 0
        assert abs(st["gateup"][0] + st["down"][0] - st["ffn"][0]) <= 1e-9 * st["ffn"][0]
        assert abs(st["gateup"][0] - 2 * st["down"][0]) <= 1e-9 * st["ffn"][0]
    m.context.kernel_timing(True, ["qkv"])  # none of the three bits: no timer
    m(ids, 0)
    assert _counts(m) == (0, 0, 0)

    def off_counts(m):
        m.context.set_last_layer_rows(True)
        m.context.kernel_timing(True, None)
        m(ids, 0)
        return _counts(m)

    m = llama3.Llama(weights, _args())
    m.context.set_ffn_fused(False)
    assert off_counts(m) == (0, 2, 2)
    m = llama3.Llama(weights, _args())
    m.context.set_gemm_x6(True)
    assert off_counts(m) == (0, 2, 2)
    for dtype in ("bf16-round", "fp8-e4m3-round"):
        m = llama3.Llama(weights, _args(), weight_dtype=dtype)
        assert off_counts(m) == (0, 2, 2), dtype
