"""Split-KV decode attention of the ragged step (DESIGN.md "Split-KV decode attention";
csrc/ragged.hip attn_decode_split_kernel / attn_decode_combine_kernel, l3_set_ragged_attn_split,
l3_ragged_attn_info, l3_op_attn_decode_ragged_host).

Op level: one launch on plain arrays against the fp64 reference of tests/split_attn_ref.py, with
rows at every position around the 64-key chunk boundaries.  Model level: greedy ids exact against
the oracle run on each row alone ("sharp" weights, as tests/test_gpu_ragged.py), with the split
form forced and on the call the single-pass kernel's LDS limit used to refuse.  Each model's oracle
rows are computed once and shared."""

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
import split_attn_ref as ref
import synth
from config import ModelArgs

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHECK_LIB = os.path.join(os.path.dirname(HERE), "llama3.np_amd", "csrc", "libllama3hip_check.so")

CH = 64
# (HD, n_rep) at KVH = 2: every head-size instantiation class — D4 a power of two or not, one or
# several heads per wave pass (n_rep 8 > the 4 waves), n_rep 1
OP_SHAPES = [(16, 2), (48, 1), (64, 8), (96, 3), (128, 4)]


@pytest.fixture(scope="module")
def ctx():
    return l3hip.op_context(0)


def _run(ctx, inp, s_cap, split):
    return ctx.op_attn_decode_ragged(inp["qkv"], inp["cache_k"], inp["cache_v"], inp["rope_cos"], inp["rope_sin"],
                                     inp["pos"], inp["finished"], inp["n_heads"], s_cap, split)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 1. op level: chunk boundaries -----------------------------------------------------------

@pytest.mark.parametrize("hd,n_rep", OP_SHAPES)
def test_op_matches_the_reference_at_every_chunk_boundary(ctx, hd, n_rep):
    """Measured on an MI355X (max-abs error against fp64: split at CH 64 / single-pass):
      (16, 2) 2.100e-07 / 2.100e-07    (48, 1) 2.112e-07 / 2.112e-07    (64, 8) 2.456e-07 / 2.602e-07
      (96, 3) 2.678e-07 / 3.223e-07    (128, 4) 3.392e-07 / 3.392e-07
    The bound: 1e-5 is the project's kernel-against-kernel bar, the factor 4 allows for the other
    summation order."""
    smax = 256
    inp = ref.make_inputs(hd, n_rep, 2, smax, ref.POSITIONS)
    want, new_k, new_v = ref.reference(inp)
    launches = ctx.ragged_attn_info()["split_launches"]
    out, ck, cv = _run(ctx, inp, smax, CH)
    assert ctx.ragged_attn_info()["split_launches"] == launches + 1
    single, sk, sv = _run(ctx, inp, smax, 0)
    assert ctx.ragged_attn_info()["split_launches"] == launches + 1
    e_split = float(np.abs(out.astype(np.float64) - want).max())
    e_single = float(np.abs(single.astype(np.float64) - want).max())
    print(f"HD {hd} n_rep {n_rep}: split max-abs {e_split:.3e}, single-pass max-abs {e_single:.3e}")
    assert np.isfinite(out).all()  # no poisoned slot was read
    assert e_split <= max(1e-5, 4 * e_single), (e_split, e_single)
    live = len(ref.POSITIONS)
    for b in range(live):
        p = int(inp["pos"][b])
        # slot pos: the RoPE'd k within 1e-6 of the reference, relative to the row's largest
        # element (a rotated pair can cancel, so not element by element); v exactly
        for g in range(2):
            err = float(np.abs(ck[b, g, p].astype(np.float64) - new_k[b, g]).max())
            assert err <= 1e-6 * float(np.abs(new_k[b, g]).max()), (b, g, err)
        assert np.array_equal(cv[b, :, p].astype(np.float64), new_v[b])
        # every other slot bit for bit what went in, NaNs included
        for got, was in ((ck, inp["cache_k"]), (cv, inp["cache_v"])):
            keep = np.ones(smax, bool)
            keep[p] = False
            assert np.array_equal(_bits(got[b][:, keep]), _bits(was[b][:, keep])), b
    # the finished row: zeros out, cache untouched
    assert not out[live:].any()
    assert np.array_equal(_bits(ck[live:]), _bits(inp["cache_k"][live:]))
    assert np.array_equal(_bits(cv[live:]), _bits(inp["cache_v"][live:]))
    # both kernels append the same bits
    assert np.array_equal(_bits(ck), _bits(sk)) and np.array_equal(_bits(cv), _bits(sv))


# ---- 2. independence of the grid, determinism --------------------------------------------------

@pytest.mark.parametrize("hd,n_rep", [(16, 2), (128, 4)])
def test_result_does_not_depend_on_s_cap_and_repeats(ctx, hd, n_rep):
    big = ref.make_inputs(hd, n_rep, 2, 1024, ref.POSITIONS)
    small = dict(big, cache_k=big["cache_k"][:, :, :256], cache_v=big["cache_v"][:, :, :256],
                 rope_cos=big["rope_cos"][:256], rope_sin=big["rope_sin"][:256])
    a, _, _ = _run(ctx, small, 256, CH)
    b, _, _ = _run(ctx, big, 1024, CH)   # 16 chunks in the grid, the same 1 .. 4 of them active
    c, _, _ = _run(ctx, big, 1024, CH)
    d, _, _ = _run(ctx, small, 128, CH)  # rows at pos >= 128 are out of this launch's range: zeros
    assert np.array_equal(_bits(a), _bits(b))
    assert np.array_equal(_bits(b), _bits(c))
    inside = big["pos"] < 128
    assert np.array_equal(_bits(d[inside]), _bits(a[inside])) and not d[~inside].any()
    # another chunk length is another summation order, not another result
    w, _, _ = _run(ctx, small, 256, 128)
    assert float(np.abs(w - a).max()) <= 1e-5


def test_op_refuses_what_no_kernel_takes(ctx):
    inp = ref.make_inputs(128, 8, 1, 1024, (0, 900), n_finished=0)
    with pytest.raises(RuntimeError, match="single-pass kernel needs"):  # 70 688 bytes of LDS
        _run(ctx, inp, 1024, 0)
    for chunk in (63, 96, 8192, 896):  # 896 keys of 8 heads: 66 592 bytes
        with pytest.raises(RuntimeError, match=f"chunk {chunk}"):
            _run(ctx, inp, 1024, chunk)
    with pytest.raises(RuntimeError, match="s_cap"):
        _run(ctx, inp, 1028, CH)
    wide = ref.make_inputs(16, 16, 1, 8, (0,), n_finished=0)
    with pytest.raises(RuntimeError, match="at most 8 query heads per KV head"):
        _run(ctx, wide, 8, CH)
    out, _, _ = _run(ctx, inp, 1024, 832)  # the largest chunk that fits this shape
    assert float(np.abs(out - ref.reference(inp)[0]).max()) <= 1e-5


# ---- models ------------------------------------------------------------------------------------

# name -> (args, hidden, prompt lengths, max_new_tokens)
#   tiny:    HD 16, n_rep 2, Smax 200: run to the last cache slot, positions cross 64, 128, 192
#   stories: the stories15M shape, HD 48, n_rep 1, two chunks
#   gqa:     one layer, HD 128, n_rep 4, Smax 160
#   long:    one layer, HD 128, n_rep 8: the single-pass kernel needs 68 000 bytes of LDS at 940
#            positions, so the call was refused before the split form existed
SHAPES = {
    "tiny": (dataclasses.replace(synth.tiny(4), max_seq_len=200), synth.TINY_HIDDEN, (1, 3, 7, 12), 200),
    "stories": (synth.stories15m(5), synth.STORIES15M_HIDDEN, (2, 9, 9, 17, 33), 100),
    "gqa": (ModelArgs(dim=512, n_layers=1, n_heads=4, n_kv_heads=1, vocab_size=1024, max_seq_len=160,
                      max_batch_size=3), 256, (3, 30, 64), 160),
    "long": (ModelArgs(dim=1024, n_layers=1, n_heads=8, n_kv_heads=1, vocab_size=1024, max_seq_len=960,
                       max_batch_size=3), 256, (860, 880, 900), 940),
    # the shapes of tests/test_gpu_ragged.py, for auto mode
    "tiny64": (synth.tiny(4), synth.TINY_HIDDEN, (1, 3, 7, 12), 64),
    "gqa96": (ModelArgs(dim=512, n_layers=1, n_heads=4, n_kv_heads=1, vocab_size=1024, max_seq_len=96,
                        max_batch_size=3), 256, (3, 30, 64), 96),
}


class Case:
    def __init__(self, name):
        self.args, hidden, self.lens, self.max_new = SHAPES[name]
        self.w = synth.make_weights(self.args, hidden, seed=31, preset="sharp")
        w64 = {k: np.asarray(v, np.float64) for k, v in self.w.items()}
        rng = np.random.default_rng(7)
        self.prompts = [rng.integers(0, self.args.vocab_size, n) for n in self.lens]
        self.model = llama3.Llama(self.w, self.args, device=0)
        one = dataclasses.replace(self.args, max_batch_size=1)
        # the reference: each row alone on a zeroed cache
        self.ids = [orc.greedy_ids(orc.OracleModel(w64, one), p[None], self.max_new)[0] for p in self.prompts]

    def want(self, max_new):
        return [ids[:max(0, max_new - n)] for ids, n in zip(self.ids, self.lens)]


_cases = {}


def _case(name, mode, chunk):
    if name not in _cases:
        _cases[name] = Case(name)
    c = _cases[name]
    c.model.context.reset_cache()
    c.model.set_sampling(0.0)
    c.model.context.set_ragged_attn_split(mode, chunk)
    return c


def _same_rows(got, want):
    assert len(got) == len(want)
    for b, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.int64 and np.array_equal(g, w), (b, g, w)


def _truncate(rows, stops):
    out = []
    for r in rows:
        hit = np.flatnonzero(np.isin(r, stops))
        out.append(r[:hit[0] + 1] if hit.size else r)
    return out


# ---- 3. model level, forced split --------------------------------------------------------------

@pytest.mark.parametrize("name", ["tiny", "stories", "gqa"])
def test_forced_split_greedy_ids_match_each_row_alone(name):
    case = _case(name, 1, CH)
    ctx = case.model.context
    before = ctx.ragged_attn_info()
    assert before["mode"] == 1 and before["chunk"] == CH
    got = case.model.generate_ragged(case.prompts, case.max_new)
    _same_rows(got, case.want(case.max_new))
    assert [g.size for g in got] == [case.max_new - n for n in case.lens]
    info = ctx.ragged_attn_info()
    steps = case.max_new - min(case.lens) - 1  # decode steps after the prefill's token
    assert info["split_launches"] - before["split_launches"] == steps * case.args.n_layers
    n_split = -(-case.max_new // CH)
    hd = case.args.dim // case.args.n_heads
    assert info["workspace_bytes"] >= case.args.max_batch_size * case.args.n_heads * n_split * (hd + 2) * 4


def test_forced_split_stop_ids_and_sampling_on_the_tiny_shape():
    case = _case("tiny", 1, CH)
    m, max_new = case.model, 150
    base = m.generate_ragged(case.prompts, max_new)
    _same_rows(base, case.want(max_new))
    stop = int(base[1][len(base[1]) // 2])  # a token row 1 emits mid-way
    want = _truncate(base, [stop])
    assert want[1].size < base[1].size
    m.context.reset_cache()
    _same_rows(m.generate_ragged(case.prompts, max_new, stop_ids=[stop]), want)
    # sampled: the same seed gives the same ids, and they are sampled
    m.set_sampling(0.8, 40, 0.95, 4321)
    m.context.reset_cache()
    first = m.generate_ragged(case.prompts, max_new)
    m.context.reset_cache()
    _same_rows(m.generate_ragged(case.prompts, max_new), first)
    assert any(not np.array_equal(a, b) for a, b in zip(first, base))
    m.set_sampling(0.0)
    assert m.context.ragged_attn_info()["split_launches"] > 0


# ---- 4. the lifted refusal ---------------------------------------------------------------------

def test_a_call_past_the_single_pass_lds_limit_runs_split():
    """Default settings (auto mode, the default chunk): 8 heads per KV head over 940 positions."""
    case = _case("long", 0, 0)
    ctx = case.model.context
    fresh = llama3.Llama(case.w, case.args, device=0)  # a context nobody configured
    info = fresh.context.ragged_attn_info()
    assert info["mode"] == 0 and info["split_launches"] == 0 and info["workspace_bytes"] == 0
    assert info["chunk"] == 256
    got = fresh.generate_ragged(case.prompts, case.max_new)
    _same_rows(got, case.want(case.max_new))
    assert [g.size for g in got] == [case.max_new - n for n in case.lens]
    info = fresh.context.ragged_attn_info()
    assert info["split_launches"] == case.max_new - min(case.lens) - 1
    assert info["workspace_bytes"] == 3 * 8 * 4 * 130 * 4
    # the chunk in force is clipped to what fits 64 KiB at this shape: 832 keys of 8 heads
    ctx.set_ragged_attn_split(0, 4096)
    assert ctx.ragged_attn_info()["chunk"] == 832
    ctx.set_ragged_attn_split(0, 256)


# ---- 5. auto mode leaves fitting shapes alone --------------------------------------------------

@pytest.mark.parametrize("name", ["tiny64", "gqa96"])
def test_auto_mode_keeps_the_single_pass_kernel_where_it_fits(name):
    case = _case(name, 0, 0)
    ctx = case.model.context
    before = ctx.ragged_attn_info()["split_launches"]
    auto = case.model.generate_ragged(case.prompts, case.max_new)
    assert ctx.ragged_attn_info()["split_launches"] == before
    _same_rows(auto, case.want(case.max_new))
    ctx.reset_cache()
    ctx.set_ragged_attn_split(1, CH)
    forced = case.model.generate_ragged(case.prompts, case.max_new)
    assert ctx.ragged_attn_info()["split_launches"] > before
    _same_rows(forced, auto)
    ctx.set_ragged_attn_split(0, 0)
    assert ctx.ragged_attn_info()["mode"] == 0 and ctx.ragged_attn_info()["chunk"] == CH  # 0 keeps the chunk


# ---- 6. errors ---------------------------------------------------------------------------------

def test_errors_are_reported_before_anything_runs():
    case = _case("tiny64", 0, 0)
    m, ctx = case.model, case.model.context
    probe = np.random.default_rng(19).integers(0, case.args.vocab_size, (2, 6))
    before = np.array(m(probe, 0))
    ctx.reset_cache()
    info = ctx.ragged_attn_info()
    for mode, chunk, match in ((0, 63, "chunk 63"), (0, 8192, "chunk 8192"), (1, 100, "chunk 100"),
                               (2, 0, "mode 2"), (-1, 64, "mode -1")):
        with pytest.raises(RuntimeError, match=match):
            ctx.set_ragged_attn_split(mode, chunk)
    assert ctx.ragged_attn_info() == info  # a refused call changes nothing
    # 16 query heads per KV head: refused by the ragged generate, in both modes, before any launch
    wide_args = ModelArgs(dim=256, n_layers=1, n_heads=16, n_kv_heads=1, vocab_size=512, max_seq_len=32,
                          max_batch_size=2)
    wide = llama3.Llama(synth.make_weights(wide_args, 64, seed=3, preset="sharp"), wide_args, device=0)
    wprobe = probe[:, :4]
    wbefore = np.array(wide(wprobe, 0))
    wide.context.reset_cache()
    for mode in (0, 1):
        wide.context.set_ragged_attn_split(mode, CH)
        with pytest.raises(RuntimeError, match="at most 8 query heads per KV head"):
            wide.generate_ragged([[1, 2, 3], [4]], 20)
    assert wide.context.ragged_attn_info()["split_launches"] == 0
    assert wide.context.ragged_attn_info()["workspace_bytes"] == 0
    assert np.array_equal(np.array(wide(wprobe, 0)), wbefore)
    # nothing was launched: the cache is still zero and a normal forward gives what it gave
    assert np.array_equal(np.array(m(probe, 0)), before)


# ---- check library -----------------------------------------------------------------------------

def test_check_build_records_no_violation():
    assert os.path.exists(CHECK_LIB), f"{CHECK_LIB} missing: __graft_entry__.build() makes it"
    env = dict(os.environ, L3_LIB_PATH=CHECK_LIB)
    r = subprocess.run([sys.executable, os.path.join(HERE, "ragged_split_checks_workload.py")], env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["enabled"] is True
    assert out["workload"] == {"kv_slot": 0, "attn_keys": 0, "token_id": 0}
    assert out["tokens"] > 0 and out["split_launches"] > 0
