"""bf16 weight storage for the weight-streaming decode GEMVs (DESIGN.md "bf16 weight storage";
l3_set_weight_bf16, gemv_kernel's WB form, misc.hip to_bf16_kernel).

The reference of every comparison is the oracle (oracle/llama3_oracle.py, float64) run on weights
whose eight matrix kinds went through utils.round_bf16 — never the library.  Bars are the
project's: "sharp" weights, logits within atol 1e-4 + rtol 2e-4, greedy ids exact.  Every model
has non-unit norm weights (1 + 0.25 N(0, 1)): with synth's all-ones norms a missing or misplaced
norm multiply on the activations would not show.  Every id comparison first asserts, on the oracle
alone, that each step's top-1 / top-2 margin is at least 1e-3 (ten times the logit bar).

All model runs set L3_DECODE_PERSIST=0 (the graph of GEMV launches), except the one test that is
about the persistent step."""

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
import sampling_ref as ref
import synth
import utils
from config import ModelArgs

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHECK_LIB = os.path.join(os.path.dirname(HERE), "llama3.np_amd", "csrc", "libllama3hip_check.so")
MARGIN = 1e-3


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
    return {k: utils.round_bf16(v) if is_matrix(k) else v for k, v in w.items()}


def f64(w):
    return {k: np.asarray(v, np.float64) for k, v in w.items()}


def bf16_bytes(args, hidden):
    D, H, KVH = args.dim, args.n_heads, args.kv_heads
    HD = D // H
    per_layer = (H + 2 * KVH) * HD * D + D * H * HD + 3 * hidden * D
    return 2 * (args.n_layers * per_layer + args.vocab_size * D)


def oracle_loop(w64, args, prompt, total):
    """The reference schedule (prefill at 0, step i >= 1 at pos = L + i) on the oracle: ids
    [B, steps], each step's logits rows, and the least top-1 / top-2 margin over all of them."""
    m = orc.OracleModel(w64, args)
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


# name -> (args, hidden): tiny HD 16 / n_rep 2; the stories15M shape (HD 48, six layers); one
# layer of HD 128 / n_rep 4 (test_gpu_ragged.py's)
SHAPES = {
    "tiny": (synth.tiny(8), synth.TINY_HIDDEN),
    "stories": (ModelArgs(max_batch_size=8, max_seq_len=64), synth.STORIES15M_HIDDEN),
    "gqa": (ModelArgs(dim=512, n_layers=1, n_heads=4, n_kv_heads=1, vocab_size=1024, max_seq_len=96,
                      max_batch_size=8), 256),
}


class Case:
    """One model: the weights, the rounded-weight oracle's results (made once, never changed) and
    the bf16-round model under test."""

    def __init__(self, name):
        self.name = name
        self.args, self.hidden = SHAPES[name]
        self.w = make_weights(self.args, self.hidden)
        self.wr = rounded(self.w)
        self.w64 = f64(self.wr)
        rng = np.random.default_rng(7)
        self.p5 = rng.integers(0, self.args.vocab_size, (1, 5))
        self.p40 = rng.integers(0, self.args.vocab_size, (1, 40))
        self.pB = rng.integers(0, self.args.vocab_size, (8, 5))
        self._memo = {}
        self.model = llama3.Llama(self.w, self.args, device=0, weight_dtype="bf16-round")

    def oracle(self, key, prompt, total):
        if key not in self._memo:
            self._memo[key] = oracle_loop(self.w64, self.args, prompt, total)
        return self._memo[key]


_cases = {}


@pytest.fixture
def case(request, monkeypatch):
    monkeypatch.setenv("L3_DECODE_PERSIST", "0")
    monkeypatch.delenv("L3_WEIGHT_BF16", raising=False)
    name = request.param
    if name not in _cases:
        _cases[name] = Case(name)
    c = _cases[name]
    c.model.context.reset_cache()
    c.model.set_sampling(0.0)
    return c


@pytest.fixture(scope="module")
def ctx():
    return l3hip.op_context(0)


# ---- 1. the kernel, integer-exact ----------------------------------------------------------------

def _int_case(rng, rows, K, N, norm):
    """Small integers: every product and every partial sum is an integer below 2^24, so fp32 is
    exact in any order; with the norm, x = +-2 and eps = 0 make 1 / rms(x) exactly 0.5."""
    x = (rng.choice([-2.0, 2.0], (rows, K)) if norm else rng.integers(-4, 5, (rows, K))).astype(np.float32)
    w = rng.integers(-4, 5, (N, K)).astype(np.float32)
    g = rng.choice([-2.0, -1.0, 1.0, 2.0, 3.0], K).astype(np.float32) if norm else None
    want = ((x * g) @ w.T) * np.float32(0.5) if norm else x @ w.T
    assert np.abs(x).max() * (3 if norm else 1) * 4 * K < 2 ** 24
    return x, w, g, want.astype(np.float32)


def _shows_wrong_indexing(x, w, g, want):
    """On the reference alone: no two rows of the expected result are equal, no two columns either
    (from four rows on: 2052 single numbers of a few hundred in magnitude cannot all differ), and
    dropping the last 8 k, or the first, changes every row — a wrong row, a wrong unit, a wrong
    piece or a wrong tail predicate cannot give the expected matrix."""
    assert len({r.tobytes() for r in want}) == want.shape[0]
    if want.shape[0] >= 4:
        assert len({c.tobytes() for c in want.T}) == want.shape[1]
    xg = x * g if g is not None else x
    s = np.float32(0.5) if g is not None else np.float32(1)
    for sl in (slice(0, -8), slice(8, None)):
        if x.shape[1] > 8:
            assert np.all(np.any((xg[:, sl] @ w[:, sl].T) * s != want, axis=1))


@pytest.mark.parametrize("K", [32, 288, 544, 1056, 4096, 8160])
def test_kernel_integer_exact(ctx, K):
    """op_linear_bf16 == NumPy exactly.  K: one piece per lane, a partly filled round and several
    rounds at each lane count (16 lanes up to K = 1024, 32 up to 2048, then 64); K = 8160 (two
    chunks of 8 pieces, the second partly filled) only fits the row-staging LDS up to two rows.
    N: one, a partly filled and many blocks.  rows: 1 / 2 / 4 / 8 per block where N * K is past
    4 M elements, else one row per block and the rows in grid.y."""
    rng = np.random.default_rng(K)
    for N in (4, 100, 2052):
        for rows in ((1, 2) if K == 8160 else (1, 2, 3, 4, 8)):
            for norm in (False, True):
                x, w, g, want = _int_case(rng, rows, K, N, norm)
                if N > 4 and K > 32:
                    _shows_wrong_indexing(x, w, g, want)
                wb = utils.bf16_bits(w)
                assert np.array_equal(utils.round_bf16(w), w)
                got = ctx.op_linear_bf16(x, wb, g, 0.0)
                bad = np.argwhere(got != want)
                assert bad.size == 0, (K, N, rows, norm, bad[:4], got[tuple(bad[0])], want[tuple(bad[0])])


def test_kernel_integer_exact_nontemporal(ctx):
    """The NT instantiation: one row, 64 lanes per unit (K = 4096) and a bf16 weight of 64 MB."""
    rng = np.random.default_rng(99)
    for norm in (False, True):
        x, w, g, want = _int_case(rng, 1, 4096, 8192, norm)
        assert w.size * 2 >= 64 << 20
        assert np.array_equal(ctx.op_linear_bf16(x, utils.bf16_bits(w), g, 0.0), want)


def test_kernel_refuses_other_shapes(ctx):
    x = np.zeros((9, 64), np.float32)
    w = np.zeros((8, 64), np.uint16)
    with pytest.raises(RuntimeError, match="rows"):
        ctx.op_linear_bf16(x, w)
    with pytest.raises(RuntimeError, match="multiple of 32"):
        ctx.op_linear_bf16(np.zeros((1, 40), np.float32), np.zeros((8, 40), np.uint16))
    with pytest.raises(RuntimeError, match="multiple of 4"):
        ctx.op_linear_bf16(np.zeros((1, 64), np.float32), np.zeros((6, 64), np.uint16))
    with pytest.raises(RuntimeError, match="not a shape"):
        ctx.op_linear_bf16(np.zeros((1, 16416), np.float32), np.zeros((4, 16416), np.uint16))


# ---- 2. the conversion ---------------------------------------------------------------------------

def test_conversion_kernel_is_round_bf16(ctx):
    from test_weight_bf16_cpu import edge_values

    rng = np.random.default_rng(2)
    exact = utils.round_bf16(rng.standard_normal(777).astype(np.float32))
    x = np.concatenate([edge_values(), rng.standard_normal(100003).astype(np.float32), exact,
                        rng.integers(0, 2 ** 32, 5000, dtype=np.uint64).astype(np.uint32).view(np.float32)])
    got, n = ctx.op_to_bf16(x)
    assert got.dtype == np.uint16 and np.array_equal(got, utils.bf16_bits(x))
    want_n = int(np.sum((utils.round_bf16(x).view(np.uint32) != x.view(np.uint32)) & ~np.isnan(x)))
    assert n == want_n and n > 50000
    got, n = ctx.op_to_bf16(exact.reshape(7, 111))
    assert n == 0 and got.shape == (7, 111)
    assert np.array_equal(got.astype(np.uint32) << 16, exact.reshape(7, 111).view(np.uint32))
    assert ctx.op_to_bf16(np.array([np.nan, -0.0, np.inf], np.float32))[1] == 0


# ---- 3. model logits -------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["tiny", "stories", "gqa"], indirect=True)
def test_model_logits_match_the_rounded_oracle(case):
    m, args = case.model, case.args
    info0 = m.context.weight_bf16_info()
    assert info0["mode"] == 2 and info0["bytes"] == bf16_bytes(args, case.hidden)
    ids, rows, _ = case.oracle("b1_short", case.p5, 5 + 4)
    got5 = np.array(m(case.p5, 0))[:, 0]
    close(got5, rows[0], f"{case.name} prefill of 5 (GEMV)")
    for i in range(1, 4):  # eager decode steps on the reference's schedule, fed the oracle's ids
        close(m(ids[:, i - 1:i], 5 + i)[:, 0], rows[i], f"{case.name} decode step {i}")
    assert m.context.weight_bf16_info()["gemv_launches"] > info0["gemv_launches"]
    m.context.reset_cache()
    want40 = orc.OracleModel(case.w64, args)(case.p40, 0)[:, -1, :]
    close(m(case.p40, 0)[:, 0], want40, f"{case.name} prefill of 40 (rounded fp32 copies)")
    # the unrounded model is another model: far outside the bar on both paths
    plain = llama3.Llama(case.w, args, device=0)
    assert plain.context.weight_bf16_info() == {"mode": 0, "bytes": 0, "gemv_launches": 0}
    d5 = float(np.abs(np.array(plain(case.p5, 0))[:, 0] - got5).max())
    plain.context.reset_cache()
    plain40 = np.array(plain(case.p40, 0))[:, 0]
    d40 = float(np.abs(plain40 - want40).max())
    # ... and the right one: the unrounded oracle's (non-unit norm weights folded into every row
    # of the fp32 tensors, a 32000-row lm_head included)
    close(plain40, orc.OracleModel(f64(case.w), args)(case.p40, 0)[:, -1, :], f"{case.name} fp32 prefill of 40")
    print(f"{case.name}: unrounded vs rounded logits differ by {d5:.3e} (5 tokens), {d40:.3e} (40)")
    assert d5 > 1e-3 and d40 > 1e-3
    assert plain.context.weight_bf16_info()["gemv_launches"] == 0


# ---- 4. greedy ids ---------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["tiny", "stories", "gqa"], indirect=True)
def test_greedy_ids_b1_to_the_last_slot(case):
    """The captured graph (folded argmax where the vocabulary is small, kv_bak, O-proj parts)."""
    total = case.args.max_seq_len
    want, _, margin = case.oracle("b1_full", case.p5, total)
    print(f"{case.name}: min top-1 margin {margin:.3e} over {want.shape[1]} steps")
    assert margin >= MARGIN
    m = case.model
    n0 = m.context.weight_bf16_info()["gemv_launches"]
    lazy = np.concatenate(list(m.generate(case.p5, total)), axis=1)
    assert np.array_equal(lazy, want)
    assert not m.context.decode_persistent() and m.context.decode_stats()["graph_steps"] > 0
    m.context.reset_cache()
    assert np.array_equal(m.generate_all(case.p5, total), want)
    assert m.context.weight_bf16_info()["gemv_launches"] > n0


@pytest.mark.parametrize("B", [3, 8])
@pytest.mark.parametrize("case", ["tiny", "stories", "gqa"], indirect=True)
def test_greedy_ids_batched(case, B):
    total = 5 + 12
    want, _, margin = case.oracle(f"b{B}", case.pB[:B], total)
    print(f"{case.name} B={B}: min top-1 margin {margin:.3e}")
    assert margin >= MARGIN
    assert np.array_equal(case.model.generate_all(case.pB[:B], total), want)
    case.model.context.reset_cache()
    assert np.array_equal(np.concatenate(list(case.model.generate(case.pB[:B], total)), axis=1), want)


@pytest.mark.parametrize("case", ["tiny", "gqa"], indirect=True)
def test_generate_ragged_with_a_stop_id(case):
    lens, max_new = (1, 3, 7), 24
    rng = np.random.default_rng(17)
    prompts = [rng.integers(0, case.args.vocab_size, n) for n in lens]
    one = dataclasses.replace(case.args, max_batch_size=1)
    rows, margin = [], np.inf
    for p in prompts:  # the reference: each row alone on a zeroed cache
        ids, _, mg = oracle_loop(case.w64, one, p[None], max_new)
        rows.append(ids[0])
        margin = min(margin, mg)
    assert margin >= MARGIN
    stop = int(rows[1][6])  # row 1 emits it at its 7th token at the latest
    want = []
    for r in rows:
        hit = np.flatnonzero(r == stop)
        want.append(r[:hit[0] + 1] if hit.size else r)
    assert len(want[1]) <= 7 < len(rows[1])
    got = case.model.generate_ragged(prompts, max_new, stop_ids=[stop])
    for b, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (b, g, w)


@pytest.mark.parametrize("case", ["tiny", "gqa"], indirect=True)
def test_sampling_against_the_rounded_oracle(case):
    """The sampled ids of generate_all, teacher-forced through the rounded-weight oracle and judged
    by sampling_ref's rule on its float64 logits (test_gpu_sampling.py's bound); the same ids from
    eager stepping."""
    T, k, p, seed, new, B = 0.9, 0, 0.95, 4321, 12, 3
    m, prompt = case.model, case.pB[:B]
    m.set_sampling(T, k, p, seed)
    ids = m.generate_all(prompt, 5 + new)
    oracle = orc.OracleModel(case.w64, case.args)
    tol = ref.TOL + 4e-4 / T
    for i in range(new):
        logits = oracle(prompt if i == 0 else ids[:, i - 1:i], 0 if i == 0 else 5 + i)[:, -1, :]
        pos = 4 if i == 0 else 5 + i
        for b in range(B):
            d = ref.distance(logits[b], T, k, p, l3hip.sample_uniform(seed, b, pos), int(ids[b, i]))
            assert d <= tol, (i, b, int(ids[b, i]), d)
    m.context.reset_cache()
    eager, nxt = [], None
    for i, pos in enumerate(range(5, 5 + new)):
        nxt, _ = m.context.greedy_step(prompt if i == 0 else nxt.reshape(-1, 1), 0 if i == 0 else pos, want_logits=True)
        eager.append(nxt.copy())
    assert np.array_equal(np.stack(eager, axis=1), ids)
    m.set_sampling(0.0)


# ---- 5. a 64 MB lm_head ----------------------------------------------------------------------------

def test_large_lm_head(monkeypatch):
    """One layer, dim 512, vocabulary 65536: the lm_head's bf16 copy is 64 MB (the non-temporal
    threshold; with K = 512 its lanes take the 16-lane form, so the NT instantiation itself is
    pinned by test_kernel_integer_exact_nontemporal)."""
    monkeypatch.setenv("L3_DECODE_PERSIST", "0")
    args = ModelArgs(dim=512, n_layers=1, n_heads=4, n_kv_heads=1, vocab_size=65536, max_seq_len=16,
                     max_batch_size=1)
    w = make_weights(args, 256, seed=33)
    w64 = f64(rounded(w))
    m = llama3.Llama(w, args, device=0, weight_dtype="bf16-round")
    assert m.context.weight_bf16_info()["bytes"] == bf16_bytes(args, 256) and 65536 * 512 * 2 == 64 << 20
    prompt = np.random.default_rng(3).integers(0, args.vocab_size, (1, 3))
    ids, rows, _ = oracle_loop(w64, args, prompt, 3 + 5)
    close(m(prompt, 0)[:, 0], rows[0], "vocab 65536 prefill of 3")
    for i in range(1, 5):
        close(m(ids[:, i - 1:i], 3 + i)[:, 0], rows[i], f"vocab 65536 decode step {i}")


# ---- 6. exact mode -----------------------------------------------------------------------------------

def test_exact_mode(monkeypatch):
    monkeypatch.setenv("L3_DECODE_PERSIST", "0")
    args, hidden = SHAPES["tiny"]
    w = make_weights(args, hidden)
    wr = rounded(w)
    prompt = np.random.default_rng(7).integers(0, args.vocab_size, (2, 5))

    def run(model):
        out = [np.array(model(prompt, 0))]
        out.append(np.array(model(out[0][:, 0].argmax(-1)[:, None], 6)))
        return np.concatenate(out)

    exact = llama3.Llama(wr, args, device=0, weight_dtype="bf16")
    assert exact.context.weight_bf16_info()["mode"] == 1
    a = run(exact)
    assert exact.context.weight_bf16_info()["gemv_launches"] > 0
    b = run(llama3.Llama(wr, args, device=0, weight_dtype="bf16-round"))
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))  # bitwise
    # a bf16-native checkpoint: the fp32 path's results to fp32 rounding
    fp32 = run(llama3.Llama(wr, args, device=0))
    assert np.all(np.abs(a.astype(np.float64) - fp32) <= 1e-4 + 2e-4 * np.abs(fp32))
    # one element one ulp off: refused, naming the tensor; the process goes on
    name = "model.layers.1.mlp.up_proj.weight"
    bad = dict(wr)
    bad[name] = wr[name].copy()
    bad[name][37, 11] = np.nextafter(bad[name][37, 11], np.float32(np.inf))
    with pytest.raises(ValueError, match=r"model\.layers\.1\.mlp\.up_proj\.weight.* 1 elements"):
        llama3.Llama(bad, args, device=0, weight_dtype="bf16")
    bad2 = dict(wr)
    bad2["lm_head.weight"] = w["lm_head.weight"]
    with pytest.raises(ValueError, match=r"lm_head\.weight"):
        llama3.Llama(bad2, args, device=0, weight_dtype="bf16")
    # the same arrays still load rounded, and an fp32 model still builds and runs
    c = run(llama3.Llama(bad, args, device=0, weight_dtype="bf16-round"))
    assert np.array_equal(c.view(np.uint32), a.view(np.uint32))
    again = run(llama3.Llama(wr, args, device=0))
    assert np.array_equal(again.view(np.uint32), fp32.view(np.uint32))


def test_exact_mode_failure_leaves_the_context_usable():
    """l3_finalize fails in exact mode, the mode is changed, the same context finalizes and runs."""
    args, hidden = SHAPES["tiny"]
    w = make_weights(args, hidden)
    ctx, upload = _manual_context(w, args, hidden)
    ctx.set_weight_bf16(1)
    upload()
    with pytest.raises(RuntimeError, match=r"model\.layers\.0\.self_attn\.q_proj\.weight \(layer 0, kind 1\)"):
        ctx.finalize()
    assert ctx.weight_bf16_info() == {"mode": 1, "bytes": 0, "gemv_launches": 0}
    ctx.set_weight_bf16(2)
    ctx.finalize()
    ids = np.random.default_rng(7).integers(0, args.vocab_size, (1, 5))
    want = orc.OracleModel(f64(rounded(w)), args)(ids, 0)[:, -1, :]
    close(ctx.forward(ids, 0), want, "finalized again in round mode")
    with pytest.raises(RuntimeError, match="already finalized"):
        ctx.set_weight_bf16(0)


# ---- 7. consistency and state ------------------------------------------------------------------------

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


def test_persistent_step_reads_the_same_model(monkeypatch):
    """Default environment: the stories-shape batch-1 step is the persistent kernel, which reads
    the rounded fp32 copies — the same ids as the oracle's."""
    monkeypatch.delenv("L3_DECODE_PERSIST", raising=False)
    args, hidden = SHAPES["stories"]
    w = make_weights(args, hidden)
    prompt = np.random.default_rng(7).integers(0, args.vocab_size, (1, 5))
    want, _, margin = oracle_loop(f64(rounded(w)), args, prompt, 40)
    assert margin >= MARGIN
    m = llama3.Llama(w, args, device=0, weight_dtype="bf16-round")
    assert np.array_equal(m.generate_all(prompt, 40), want)
    assert m.context.decode_persistent()


def test_state_and_determinism(monkeypatch):
    monkeypatch.setenv("L3_DECODE_PERSIST", "0")
    args, hidden = SHAPES["tiny"]
    w = make_weights(args, hidden)
    ids = np.random.default_rng(7).integers(0, args.vocab_size, (3, 5))
    m = llama3.Llama(w, args, device=0, weight_dtype="bf16-round")
    a = np.array(m(ids, 0))
    m.context.reset_cache()
    assert np.array_equal(a.view(np.uint32), np.array(m(ids, 0)).view(np.uint32))
    with pytest.raises(RuntimeError, match="already finalized"):
        m.context.set_weight_bf16(0)
    with pytest.raises(RuntimeError, match="mode 3"):
        l3hip.Context(llama3._dims(args, hidden, 0, 0), 0).set_weight_bf16(3)
    # mode 0 set explicitly is not calling the setter at all, bit for bit
    plain = llama3.Llama(w, args, device=0)
    assert plain.context.weight_bf16_info() == {"mode": 0, "bytes": 0, "gemv_launches": 0}
    base = np.array(plain(ids, 0))
    ctx, upload = _manual_context(w, args, hidden)
    ctx.set_weight_bf16(2)
    ctx.set_weight_bf16(0)
    upload()
    ctx.finalize()
    assert np.array_equal(np.array(ctx.forward(ids, 0)).view(np.uint32), base[:, 0].view(np.uint32))
    assert ctx.weight_bf16_info() == {"mode": 0, "bytes": 0, "gemv_launches": 0}
    # the environment variable sets the mode of new contexts
    monkeypatch.setenv("L3_WEIGHT_BF16", "2")
    env = llama3.Llama(w, args, device=0)
    assert env.context.weight_bf16_info()["mode"] == 2
    assert np.array_equal(np.array(env(ids, 0)).view(np.uint32), a.view(np.uint32))


def test_multi_device_group_is_refused(monkeypatch):
    """A member of a multi-device group takes no bf16 mode (two members sharing device 0), and
    L3_WEIGHT_BF16 does not reach the members of such a group; a group of one may have it."""
    monkeypatch.setenv("L3_GROUP_VIRTUAL", "1")
    monkeypatch.setenv("L3_WEIGHT_BF16", "2")
    args, hidden = SHAPES["tiny"]
    dims = llama3._dims(args, hidden, args.n_layers, args.vocab_size)
    grp = l3hip.Group(dims, [0, 0])
    for m in grp.members:
        assert m.weight_bf16_info()["mode"] == 0
        with pytest.raises(RuntimeError, match="multi-device"):
            m.set_weight_bf16(1)
        m.set_weight_bf16(0)
    grp.close()
    one = l3hip.Group(dims, [0])
    assert one.members[0].weight_bf16_info()["mode"] == 2
    one.members[0].set_weight_bf16(1)
    one.close()


# ---- 8. the check build ------------------------------------------------------------------------------

def test_check_build_records_no_violation():
    assert os.path.exists(CHECK_LIB), f"{CHECK_LIB} missing: __graft_entry__.build() makes it"
    env = dict(os.environ, L3_LIB_PATH=CHECK_LIB, L3_DECODE_PERSIST="0")
    env.pop("L3_WEIGHT_BF16", None)
    r = subprocess.run([sys.executable, os.path.join(HERE, "weight_bf16_checks_workload.py")], env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["enabled"] is True and out["gemv_launches"] > 0 and out["persistent"] is False
    assert out["counts"] == {"kv_slot": 0, "attn_keys": 0, "token_id": 0}
    args, hidden = SHAPES["tiny"]
    prompt = np.random.default_rng(7).integers(0, args.vocab_size, (1, 5))
    want, _, margin = oracle_loop(f64(rounded(make_weights(args, hidden))), args, prompt, args.max_seq_len)
    assert margin >= MARGIN
    assert out["generate"] == want[0].tolist() and out["generate_all"] == want[0].tolist()
