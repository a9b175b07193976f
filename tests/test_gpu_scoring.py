"""Teacher-forced scoring on the device (gemm_kernel.h lse_rows epilogue, score.hip combine,
l3_score_host / l3_op_linear_logprob_host) against the rule restated in scoring_ref.py: the op
against float64, the padding and range edges, the row chunking, the model against the oracle, the
call as a forward, and the refusals.

Bounds.  OP_BOUND is 4x the worst |logprob| / |lse| difference measured on the MI355X over the
shapes of test_op_against_float64 (the kernel is deterministic; the factor covers other seeds):
measured 1.33e-6 (K = 32) and 1.43e-6 (K = 288), both at 257 x 2000 (three ulps of an lse near
7.6).  LOGIT_BOUND is the fp32 product's error bound for these inputs, K * 2^-24 * sum |x_i w_i| ~
288 * 6e-8 * 0.64 = 1.1e-5 per logit, two logits per margin.  The model tests carry the project's 1e-4 logit tolerance twice (|dz_t| + |dlse|).
"""

import numpy as np
import pytest

import l3hip
import llama3
import llama3_oracle as orc
import scoring_ref as ref
import synth

pytestmark = pytest.mark.gpu

OP_BOUND = 4 * 1.434e-6
LOGIT_BOUND = 2e-5
MODEL_BOUND = 2e-4

ROWS = (1, 15, 17, 33, 65, 129, 257)
COLS = (4, 60, 64, 68, 132, 260, 2000)


@pytest.fixture(scope="module")
def ctx():
    c = l3hip.op_context(0)
    yield c
    c.set_score_workspace(0)


def _targets(rng, rows, N):
    """random columns, with 0, N - 1, the first column of the last (partial) tile and -1 among them"""
    t = rng.integers(0, N, rows).astype(np.int32)
    for i, v in enumerate((0, N - 1, (N - 1) // 64 * 64, -1)):
        if i < rows:
            t[(i * 7) % rows] = v
    return t


@pytest.mark.parametrize("K", [32, 288])
def test_op_against_float64(ctx, K):
    rng = np.random.default_rng(2000 + K)
    worst_lp = worst_lse = 0.0
    skipped = total = 0
    for rows in ROWS:
        for N in COLS:
            x = (rng.standard_normal((rows, K)) / np.sqrt(K)).astype(np.float32)
            w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
            t = _targets(rng, rows, N)
            lp, lse, am = ctx.op_linear_logprob(x, w, t)
            assert lp.shape == lse.shape == am.shape == (rows,)
            assert lp.dtype == lse.dtype == np.float32 and am.dtype == np.int32
            # argmax against the float64 product of the same inputs
            z64 = x.astype(np.float64) @ w.astype(np.float64).T
            _, _, am64, margin = ref.logprobs64(z64, t)
            clear = margin > LOGIT_BOUND
            skipped += int((~clear).sum())
            total += rows
            assert (am[clear] == am64[clear]).all(), (rows, N)
            # the reduction against float64 on the device's own fp32 logits
            z = ctx.op_linear(x, w)
            lp64, lse64, _, _ = ref.logprobs64(z, t)
            d_lp = float(np.max(np.abs(lp - lp64)))
            d_lse = float(np.max(np.abs(lse - lse64)))
            worst_lp, worst_lse = max(worst_lp, d_lp), max(worst_lse, d_lse)
            assert (lp[t < 0] == 0.0).all()
            assert d_lp <= OP_BOUND and d_lse <= OP_BOUND, (rows, N, d_lp, d_lse)
    print(f"K {K}: worst |logprob - f64| {worst_lp:.3e}, worst |lse - f64| {worst_lse:.3e}, "
          f"argmax rows under the margin {skipped} of {total}")
    assert skipped <= 0.02 * total


def _ulp(v):
    return float(np.spacing(np.float32(abs(v))))


def test_padding_and_range_edges(ctx):
    K = 32
    ones = np.ones((5, K), np.float32)
    # every logit -50 (exact): a padded column counted as 0 would move lse by about 50
    N = 68
    w = np.full((N, K), -50.0 / 32, np.float32)
    t = np.array([0, 67, 64, -1, 3], np.int32)
    lp, lse, am = ctx.op_linear_logprob(ones, w, t)
    lp64, lse64, am64, _ = ref.logprobs64(np.full((5, N), -50.0), t)
    assert np.max(np.abs(lse - lse64)) <= 4 * _ulp(50.0)
    assert np.max(np.abs(lp - lp64)) <= 4 * _ulp(50.0)
    assert (am == 0).all() and lp[3] == 0.0
    # logits of magnitude 1e3 (integers: exact in every kernel): the maximum is subtracted
    rng = np.random.default_rng(11)
    N = 260
    w = np.repeat(rng.integers(-32, 33, (N, 1)), K, axis=1).astype(np.float32)
    z = np.repeat(32.0 * w[None, :, 0].astype(np.float64), 5, axis=0)
    t = np.array([int(np.argmax(z[0])), 259, 256, -1, 1], np.int32)
    lp, lse, am = ctx.op_linear_logprob(ones, w, t)
    lp64, lse64, am64, _ = ref.logprobs64(z, t)
    assert np.isfinite(lse).all() and np.isfinite(lp).all()
    assert np.max(np.abs(lse - lse64)) <= 4 * _ulp(1024.0)
    assert np.max(np.abs(lp - lp64)) <= 8 * _ulp(1024.0)
    assert (am == am64).all()
    # one whole 64-column tile of -inf among finite ones
    N = 132
    w = (rng.standard_normal((N, K)) / 8).astype(np.float32)
    w[64:128] = -np.inf
    t = np.array([0, 131, 128, 70, -1], np.int32)
    lp, lse, am = ctx.op_linear_logprob(ones, w, t)
    z = ctx.op_linear(ones, w)
    assert np.isneginf(z[:, 64:128]).all() and np.isfinite(z[:, :64]).all()
    lp64, lse64, am64, _ = ref.logprobs64(z, t)
    assert np.isfinite(lse).all()
    assert np.max(np.abs(lse - lse64)) <= OP_BOUND
    assert np.isneginf(lp[3]) and lp[4] == 0.0
    keep = [0, 1, 2]
    assert np.max(np.abs(lp[keep] - lp64[keep])) <= OP_BOUND
    assert (am == am64).all()
    # every column -inf: NaN (no target: still 0.0)
    w = np.full((N, K), -np.inf, np.float32)
    lp, lse, am = ctx.op_linear_logprob(ones, w, t)
    assert np.isnan(lp[:4]).all() and lp[4] == 0.0
    assert (am == 0).all()
    # NaN columns: NaN, and the argmax is the first of them
    w = (rng.standard_normal((N, K)) / 8).astype(np.float32)
    w[100] = np.nan
    w[70] = np.nan
    lp, lse, am = ctx.op_linear_logprob(ones, w, t)
    assert np.isnan(lp[:4]).all() and np.isnan(lse).all() and lp[4] == 0.0
    assert (am == 70).all()
    # a +inf maximum: NaN
    w = (rng.standard_normal((N, K)) / 8).astype(np.float32)
    w[129] = np.inf
    lp, lse, am = ctx.op_linear_logprob(ones, w, t)
    assert np.isnan(lp[:4]).all() and (am == 129).all()
    # target N: an error return, and a correct call straight after it succeeds
    w = (rng.standard_normal((N, K)) / 8).astype(np.float32)
    with pytest.raises(RuntimeError, match="target"):
        ctx.op_linear_logprob(ones, w, np.array([0, 1, N, 2, 3], np.int32))
    with pytest.raises(RuntimeError, match="target"):
        ctx.op_linear_logprob(ones, w, np.array([0, 1, -2, 2, 3], np.int32))
    lp, lse, am = ctx.op_linear_logprob(ones, w, t)
    lp64, _, _, _ = ref.logprobs64(ctx.op_linear(ones, w), t)
    assert np.max(np.abs(lp - lp64)) <= OP_BOUND


def test_chunking_is_invisible(ctx):
    rows, N, K = 1300, 2000, 64
    rng = np.random.default_rng(12)
    x = (rng.standard_normal((rows, K)) / np.sqrt(K)).astype(np.float32)
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    t = _targets(rng, rows, N)
    per_row = 16 * ((N + 63) // 64)
    out = []
    try:
        for nbytes in (256 * per_row, 256 * per_row, 768 * per_row, 0):  # 5 chunks + 20 rows; 768 + 532; one
            ctx.set_score_workspace(nbytes)
            out.append(ctx.op_linear_logprob(x, w, t))
        for got in out[1:]:
            for a, b in zip(out[0], got):
                np.testing.assert_array_equal(a.view(np.int32), b.view(np.int32))
        lp64, _, _, _ = ref.logprobs64(ctx.op_linear(x, w), t)
        assert np.max(np.abs(out[0][0] - lp64)) <= OP_BOUND
        # below one 256-row chunk: refused, by the setter (the context's own vocabulary) or by the
        # call (this N)
        with pytest.raises(RuntimeError, match="256"):
            ctx.set_score_workspace(100)
        with pytest.raises(RuntimeError, match="256"):
            ctx.set_score_workspace(256 * per_row - 16)
            ctx.op_linear_logprob(x, w, t)
    finally:
        ctx.set_score_workspace(0)
    got = ctx.op_linear_logprob(x, w, t)
    for a, b in zip(out[0], got):
        np.testing.assert_array_equal(a.view(np.int32), b.view(np.int32))


def _model_case(name):
    if name == "stories15m":
        args, hidden, preset, B, L = synth.stories15m(2), synth.STORIES15M_HIDDEN, "sharp", 2, 40
    else:
        args, hidden, preset, B, L = synth.tiny(4), synth.TINY_HIDDEN, name, 4, 33
    w = synth.make_weights(args, hidden, seed=0, preset=preset)
    ids = np.random.default_rng(7).integers(0, args.vocab_size, (B, L))
    return args, w, ids


@pytest.mark.parametrize("name", ["default", "sharp", "stories15m"])
def test_model_against_the_oracle(name):
    args, w, ids = _model_case(name)
    B, L = ids.shape
    z = ref.all_logits(orc.OracleModel(w, args), ids, 0)
    model = llama3.Llama(w, args, device=0)
    # next-token scores inside the sequence
    got = model.score(ids)
    assert got.shape == (B, L - 1) and got.dtype == np.float32
    want, _, _, _ = ref.logprobs64(z[:, :-1], ids[:, 1:])
    d = float(np.max(np.abs(got - want)))
    # explicit targets: every position, and the greedy ids
    tg = np.concatenate([ids[:, 1:], ids[:, :1]], axis=1)
    tg[0, 3] = -1
    got2, am = model.score(ids, tg, 0, return_argmax=True)
    assert got2.shape == (B, L) and am.shape == (B, L) and am.dtype == np.int64
    want2, _, am64, margin = ref.logprobs64(z, tg)
    d2 = float(np.max(np.abs(got2 - want2)))
    clear = margin >= MODEL_BOUND
    print(f"{name}: max |logprob - oracle| {d:.3e} / {d2:.3e}; logprobs {want.min():.2f} .. {want.max():.2f}; "
          f"argmax positions under the margin {int((~clear).sum())} of {clear.size}")
    assert d <= MODEL_BOUND and d2 <= MODEL_BOUND
    assert got2[0, 3] == 0.0
    np.testing.assert_array_equal(got2[:, :-1][tg[:, :-1] >= 0], got[tg[:, :-1] >= 0])
    assert (~clear).sum() <= 0.02 * clear.size
    assert (am[clear] == am64[clear]).all()
    # negative ids wrap as the embedding wraps them, as targets too
    neg = ids.copy()
    neg[:, 1::2] -= args.vocab_size
    np.testing.assert_array_equal(model.score(neg), got)


def test_it_is_a_forward():
    args, w, ids = _model_case("default")
    ids = ids[:, :32]
    B, L = ids.shape
    rng = np.random.default_rng(8)
    nxt = rng.integers(0, args.vocab_size, (B, 3))
    tg = rng.integers(0, args.vocab_size, (B, L))
    a, b = llama3.Llama(w, args, device=0), llama3.Llama(w, args, device=0)
    # the cache after a score is the cache after a forward
    full = a.score(ids, tg)
    b(ids, 0)
    np.testing.assert_array_equal(np.array(a(nxt, L)), np.array(b(nxt, L)))
    # two halves against one piece (the chunked-prefill tolerance)
    h = L // 2
    halves = np.concatenate([a.score(ids[:, :h], tg[:, :h], 0), a.score(ids[:, h:], tg[:, h:], h)], axis=1)
    assert float(np.max(np.abs(halves - full))) <= 1e-5
    # the last column against log_softmax of the forward's logits
    logits = np.array(b(ids, 0))[:, 0].astype(np.float64)
    want, _, _, _ = ref.logprobs64(logits, tg[:, -1])
    assert float(np.max(np.abs(full[:, -1] - want))) <= MODEL_BOUND
    # the last-layer setting is neither used nor changed: with every row through the last block
    # the forward gives what it gave, and the score is the same bits
    b.context.set_last_layer_rows(True)
    all_rows = np.array(b(ids, 0))
    np.testing.assert_array_equal(b.score(ids, tg), full)
    np.testing.assert_array_equal(np.array(b(ids, 0)), all_rows)
    b.context.set_last_layer_rows(False)
    pruned = np.array(b(ids, 0))
    b.score(ids, tg)
    np.testing.assert_array_equal(np.array(b(ids, 0)), pruned)


def test_score_between_two_generate_calls():
    args, w, ids = _model_case("sharp")
    prompt = ids[:1, :5]
    model = llama3.Llama(w, args, device=0)
    want = np.concatenate(list(model.generate(prompt, 30)), axis=1)
    gen = model.generate(prompt, 30)
    first = [next(gen) for _ in range(4)]  # the device now runs ahead of the consumer
    # (scored over the prompt's own slots: the reference's generate never writes slot L, and a
    # longer text here would fill that slot for the second generate as any forward would)
    s1 = model.score(ids[:2, :5])
    rest = np.concatenate(list(model.generate(prompt, 30)), axis=1)
    np.testing.assert_array_equal(np.concatenate(first, axis=1), want[:, :4])
    np.testing.assert_array_equal(rest, want)
    np.testing.assert_array_equal(model.score(ids[:2, :5]), s1)


def test_refusals(monkeypatch):
    args, w, ids = _model_case("default")
    model = llama3.Llama(w, args, device=0)
    with pytest.raises(ValueError):
        model.score(ids, ids[:, :-1])
    with pytest.raises(ValueError):
        model.score(ids[0])
    with pytest.raises(RuntimeError, match="target"):
        model.score(ids, np.full(ids.shape, args.vocab_size))
    assert model.score(ids).shape == (ids.shape[0], ids.shape[1] - 1)  # and a correct call succeeds
    monkeypatch.setenv("L3_GROUP_VIRTUAL", "1")
    grp = llama3.Llama(w, args, devices=[0, 0])
    with pytest.raises(NotImplementedError):
        grp.score(ids)
    with pytest.raises(RuntimeError, match="multi-device"):
        grp.context.score(ids[:2], ids[:2], 0)
