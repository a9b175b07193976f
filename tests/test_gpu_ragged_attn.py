"""The ragged attention kernels at kernel level (DESIGN.md "Ragged attention at kernel level";
csrc/ragged.hip attn_decode_ragged_kernel / attn_decode_split_kernel / attn_decode_combine_kernel,
csrc/ragged_extend.hip ragged_extend_append_kernel / attn_extend_ragged_kernel): all 54
instantiations — head size 16 .. 128, both cache element types — at every n_rep in 1 .. 8, launched
on plain arrays through l3_op_attn_decode_ragged(_kv)_host and l3_op_attn_extend_ragged(_kv)_host
against the fp64 reference, the key census and the softmax-state stress inputs of
tests/ragged_attn_ref.py.  tests/test_ragged_attn_cpu.py shows the tables reach every edge."""

import dataclasses
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import kv_bf16_ref as kv
import l3hip
import llama3
import llama3_oracle as orc
import ragged_attn_ref as ref
import synth
from config import ModelArgs

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHECK_LIB = os.path.join(os.path.dirname(HERE), "llama3.np_amd", "csrc", "libllama3hip_check.so")

# the project's kernel-against-fp64 bar for attention (tests/test_gpu_ragged_split.py,
# tests/test_gpu_ragged_extend.py, tests/test_gpu_attn_dense.py)
BOUND = 1e-5
# random, census, and the four stress shapes; the stress kind runs at these n_rep only — one, an odd
# one, one with idle query rows, and the largest — which keeps every head size and every edge and
# a third of the module's wall time
STRESS_N_REPS = (1, 3, 5, 8)


def _kinds(n_rep):
    basic = (("random", None), ("census", None))
    return basic + tuple(("stress", s) for s in ref.STRESS) if n_rep in STRESS_N_REPS else basic


@pytest.fixture(scope="module")
def ctx():
    return l3hip.op_context(0)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a if a.dtype == np.uint16 else a.astype(np.float32, copy=False).view(np.uint32)


def _f64(a):
    return kv.widen(a) if a.dtype == np.uint16 else a.astype(np.float64)


def _typed(inp, kt):
    return ref.to_bf16(inp) if kt == "bf16" else inp


def _check_new_slots(kt, got_k, got_v, want_k, v32, where):
    """the new slots of one row, [KVH, n, HD]: K within 1e-6 of the fp64 RoPE relative to the
    slot's largest element (bf16: a correct rounding given that allowance, kv_bf16_ref.check_a);
    V the input's bits (bf16: their RNE)"""
    big = np.abs(want_k).max(axis=-1, keepdims=True)
    if kt == "bf16":
        assert kv.check_a(kv.widen(got_k), want_k, 1e-6 * big).all(), where
        assert np.array_equal(got_v, kv.to_bits(v32)), where
    else:
        assert (np.abs(got_k.astype(np.float64) - want_k) <= 1e-6 * big).all(), where
        assert np.array_equal(_bits(got_v), _bits(v32)), where


def _census_ok(got, want, where):
    """tests/test_gpu_attn_dense.py test_prefill_table_counts_every_key_once's rule: out * keys
    rounds to the count and lies within 1e-3 of it"""
    bad = np.argwhere(~(np.rint(got) == want) | ~(np.abs(got - want) <= 1e-3))
    assert not bad.size, f"{where}: element {tuple(int(x) for x in bad[0])} counts {got[tuple(bad[0])]!r}, " \
                         f"{int(np.broadcast_to(want, got.shape)[tuple(bad[0])])} expected ({bad.shape[0]} differ)"


# ---- decode ---------------------------------------------------------------------------------------

def _decode(ctx, inp, kt, kind, s_cap, split, where):
    """One launch of a decode batch, every check of its kind.  Returns (error or 0.0, out, k, v)"""
    t = _typed(inp, kt)
    out, ck, cv = ctx.op_attn_decode_ragged(t["qkv"], t["cache_k"], t["cache_v"], t["rope_cos"], t["rope_sin"],
                                            t["pos"], t["finished"], t["n_heads"], s_cap, split)
    assert np.isfinite(out).all(), f"{where}: a poisoned slot was read, or the softmax state overflowed"
    B, kvh, _, hd = ck.shape
    H, live = inp["n_heads"], len(inp["pos"]) - 1
    want, new_k, new_v, _ = ref.decode_reference(inp, kind, (_f64(ck), _f64(cv)) if kt == "bf16" else None)
    # the appended slot, and every other slot — the guard row's cache whole — bit for bit what went in
    was_k, was_v = t["cache_k"].copy(), t["cache_v"].copy()
    v32 = inp["qkv"][:, (H + kvh) * hd:].reshape(B, kvh, hd)
    for b in range(live):
        p = int(inp["pos"][b])
        _check_new_slots(kt, ck[b, :, p:p + 1], cv[b, :, p:p + 1], new_k[b][:, None], v32[b][:, None], (where, b))
        was_k[b, :, p], was_v[b, :, p] = ck[b, :, p], cv[b, :, p]
    assert np.array_equal(_bits(ck), _bits(was_k)) and np.array_equal(_bits(cv), _bits(was_v)), where
    assert not out[live:].any(), f"{where}: the finished row"
    if kind == "census":
        keys = (inp["pos"][:live].astype(np.float64) + 1)[:, None, None]
        _census_ok(out[:live].astype(np.float64).reshape(live, H, hd) * keys, ref.decode_census(inp)[:live, None], where)
        return 0.0, out, ck, cv
    err = float(np.abs(out.astype(np.float64) - want).max())
    assert err <= BOUND, (where, err)
    return err, out, ck, cv


@pytest.mark.parametrize("kt", ref.KTS)
@pytest.mark.parametrize("hd,n_rep", ref.PARAMS)
def test_single_pass(ctx, hd, n_rep, kt):
    """attn_decode_ragged_kernel<HD, KT> at s_cap = Smax = 320, rows at every position of
    ref.single_positions: against fp64 at 1e-5 (random), the exact key census, and the four stress
    shapes at 1e-5.  Measured on an MI355X: DESIGN.md "Ragged attention at kernel level"."""
    worst = {}
    for kind, shape in _kinds(n_rep):
        inp = ref.decode_inputs(hd, n_rep, ref.single_positions(hd), ref.SMAX, kind, shape)
        err, *_ = _decode(ctx, inp, kt, kind, ref.SMAX, 0, (hd, n_rep, kt, kind, shape))
        worst[shape or kind] = err
    print(f"single-pass HD {hd} n_rep {n_rep} {kt}: " + "  ".join(f"{k} {v:.3e}" for k, v in worst.items()))


@pytest.mark.parametrize("kt", ref.KTS)
@pytest.mark.parametrize("hd,n_rep", ref.PARAMS)
def test_split(ctx, hd, n_rep, kt):
    """attn_decode_split_kernel<HD, KT> + attn_decode_combine_kernel<HD> at chunk 64 / s_cap 320,
    chunk 320 / s_cap 384 and chunk 128 / s_cap 320: as test_single_pass; each launch counted by
    split_launches; the random kind's caches bit for bit the single-pass form's."""
    worst = {}
    for chunk, s_cap in ref.SPLITS:
        for kind, shape in _kinds(n_rep):
            inp = ref.decode_inputs(hd, n_rep, ref.split_positions(chunk, s_cap), s_cap, kind, shape)
            before = ctx.ragged_attn_info()["split_launches"]
            err, out, ck, cv = _decode(ctx, inp, kt, kind, s_cap, chunk, (hd, n_rep, kt, chunk, kind, shape))
            assert ctx.ragged_attn_info()["split_launches"] == before + 1
            worst[shape or kind] = max(worst.get(shape or kind, 0.0), err)
            if kind == "random":
                _, single, sk, sv = _decode(ctx, inp, kt, kind, s_cap, 0, (hd, n_rep, kt, chunk, "single-pass"))
                assert ctx.ragged_attn_info()["split_launches"] == before + 1
                assert np.array_equal(_bits(ck), _bits(sk)) and np.array_equal(_bits(cv), _bits(sv)), (hd, n_rep, chunk)
                assert float(np.abs(out - single).max()) <= BOUND
    print(f"split HD {hd} n_rep {n_rep} {kt}: " + "  ".join(f"{k} {v:.3e}" for k, v in worst.items()))


# ---- extend ---------------------------------------------------------------------------------------

def _extend(ctx, inp, kt, kind, where):
    """The two launches of an extend batch, every check of its kind.  Returns (error, out, k, v)"""
    t = _typed(inp, kt)
    out, ck, cv = ctx.op_attn_extend_ragged(t["qkv"], t["cache_k"], t["cache_v"], t["rope_cos"], t["rope_sin"],
                                            t["starts"], t["lens"], t["n_heads"])
    assert np.isfinite(out).all(), f"{where}: a poisoned slot was read, or the softmax state overflowed"
    B, kvh, _, hd = ck.shape
    H, lq = inp["n_heads"], inp["qkv"].shape[1]
    want, new_k, new_v, _ = ref.extend_reference(inp, kind, (_f64(ck), _f64(cv)) if kt == "bf16" else None)
    was_k, was_v = t["cache_k"].copy(), t["cache_v"].copy()
    v32 = inp["qkv"][:, :, (H + kvh) * hd:].reshape(B, lq, kvh, hd).transpose(0, 2, 1, 3)
    for b in range(B):
        st, n = int(inp["starts"][b]), int(inp["lens"][b])
        assert not out[b, n:].any(), f"{where}: pads of row {b}"
        if n:
            _check_new_slots(kt, ck[b, :, st:st + n], cv[b, :, st:st + n], new_k[b], v32[b, :, :n], (where, b))
            was_k[b, :, st:st + n], was_v[b, :, st:st + n] = ck[b, :, st:st + n], cv[b, :, st:st + n]
    assert np.array_equal(_bits(ck), _bits(was_k)) and np.array_equal(_bits(cv), _bits(was_v)), where
    if kind == "census":
        keys = (inp["starts"].astype(np.float64)[:, None] + np.arange(lq)[None, :] + 1)[:, :, None, None]
        got = out.astype(np.float64).reshape(B, lq, H, hd) * keys
        live = np.arange(lq)[None, :] < inp["lens"][:, None]
        _census_ok(np.where(live[:, :, None, None], got, 0.0),
                   np.where(live[:, :, None, None], ref.extend_census(inp)[:, :, None], 0), where)
        return 0.0, out, ck, cv
    err = float(np.abs(out.astype(np.float64) - want).max())
    assert err <= BOUND, (where, err)
    return err, out, ck, cv


@pytest.mark.parametrize("kt", ref.KTS)
@pytest.mark.parametrize("hd,n_rep", ref.PARAMS)
def test_extend(ctx, hd, n_rep, kt):
    """ragged_extend_append_kernel<HD, KT> + attn_extend_ragged_kernel<HD, KT> on the rows of
    ref.extend_pairs (Lq = 2 TQ + 17, TQ = 64 / n_rep): fp64 at 1e-5, the census per query row, the
    stress shapes, pads zero, the new slots and every untouched slot; at n_rep = 1 also Lq = 130,
    three query tiles of 64; and one-token extends against the decode kernel at
    ref.single_positions."""
    worst = {}
    tables = [(ref.extend_pairs(n_rep), ref.lq_of(n_rep), _kinds(n_rep))]
    if n_rep == 1:
        tables.append((ref.LONG_PAIRS, ref.LQ_LONG, _kinds(1)[:3]))
    for pairs, lq, kinds in tables:
        for kind, shape in kinds:
            inp = ref.extend_inputs(hd, n_rep, pairs, lq, kind, shape)
            err, *_ = _extend(ctx, inp, kt, kind, (hd, n_rep, kt, lq, kind, shape))
            worst[shape or kind] = max(worst.get(shape or kind, 0.0), err)
    # a one-token extend is the decode kernel's launch: the same out to 1e-5, the same new V bits
    pos = ref.single_positions(hd)
    pairs = tuple((p, 1) for p in pos) + ((5, 0),)
    inp = ref.extend_inputs(hd, n_rep, pairs, 1)
    fin = np.array([0] * len(pos) + [1], np.int32)
    t = _typed(inp, kt)
    _, e_out, ek, ev = _extend(ctx, inp, kt, "random", (hd, n_rep, kt, "one token"))
    d_out, dk, dv = ctx.op_attn_decode_ragged(t["qkv"][:, 0], t["cache_k"], t["cache_v"], t["rope_cos"],
                                              t["rope_sin"], t["starts"], fin, t["n_heads"], ref.SMAX, 0)
    worst["one-token"] = float(np.abs(e_out[:, 0] - d_out).max())
    assert np.isfinite(d_out).all() and worst["one-token"] <= BOUND, (hd, n_rep, kt, worst)
    assert np.array_equal(_bits(ev), _bits(dv))
    if kt == "bf16":  # the kernels' RoPE may differ in the last fp32 bit, which moves a key that sits on a tie
        diff = np.abs(ek.astype(np.int32) - dk.astype(np.int32))
        assert diff.max() <= 1 and float((diff == 0).mean()) >= 0.99
    else:
        k_err = np.abs(ek.astype(np.float64) - dk.astype(np.float64))
        assert np.array_equal(np.isnan(ek), np.isnan(dk)) and \
            float(np.nanmax(k_err)) <= 1e-6 * float(np.nanmax(np.abs(dk)))
    print(f"extend HD {hd} n_rep {n_rep} {kt}: " + "  ".join(f"{k} {v:.3e}" for k, v in worst.items()))


# ---- stale workspace ------------------------------------------------------------------------------

@pytest.mark.parametrize("kt", ref.KTS)
@pytest.mark.parametrize("hd,n_rep", [(32, 5), (128, 8)])
def test_a_short_launch_does_not_read_what_a_long_one_left(ctx, hd, n_rep, kt):
    """The workspace is never cleared: after a spike_high launch with rows in all five chunks
    (partials with m = 200), a launch whose rows all sit at pos <= 65 — one or two active chunks —
    gives bit for bit what it gives on a fresh context."""
    chunk, s_cap = ref.SPLITS[0]
    long_pos = ref.split_positions(chunk, s_cap)
    assert max(long_pos) // chunk + 1 >= 5
    # the short launch has the long one's batch size, so that its partials land on the same words
    short_pos = tuple((0, 1, 63, 64, 65)[i % 5] for i in range(len(long_pos)))
    short = ref.decode_inputs(hd, n_rep, short_pos, s_cap)
    _decode(ctx, ref.decode_inputs(hd, n_rep, long_pos, s_cap, "stress", "spike_high"), kt, "stress", s_cap, chunk,
            (hd, n_rep, kt, "long"))
    _, got, gk, gv = _decode(ctx, short, kt, "random", s_cap, chunk, (hd, n_rep, kt, "short"))
    _, want, wk, wv = _decode(l3hip.op_context(0), short, kt, "random", s_cap, chunk, (hd, n_rep, kt, "fresh"))
    assert np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(_bits(gk), _bits(wk)) and np.array_equal(_bits(gv), _bits(wv))


# ---- a model at HD = 32 ---------------------------------------------------------------------------

class Hd32:
    """dim 128, 4 heads over 2 KV heads (HD 32, n_rep 2), 320 positions, "sharp" weights; prompts of
    3, 250 and 300 tokens; the oracle's greedy ids of each row alone, to the last slot"""
    LENS, MAX_NEW = (3, 250, 300), 320

    def __init__(self):
        self.args = ModelArgs(dim=128, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=512, max_seq_len=320,
                              max_batch_size=3)
        self.w = synth.make_weights(self.args, 256, seed=31, preset="sharp")
        self.w64 = {k: np.asarray(v, np.float64) for k, v in self.w.items()}
        self.one = dataclasses.replace(self.args, max_batch_size=1)
        rng = np.random.default_rng(7)
        self.prompts = [rng.integers(0, self.args.vocab_size, n) for n in self.LENS]
        self.ids = [orc.greedy_ids(orc.OracleModel(self.w64, self.one), p[None], self.MAX_NEW)[0] for p in self.prompts]
        self.models = {}

    def model(self, kt):
        if kt not in self.models:
            self.models[kt] = llama3.Llama(self.w, self.args, device=0, kv_dtype="bf16" if kt == "bf16" else None)
        m = self.models[kt]
        m.context.reset_cache()
        m.set_sampling(0.0)
        m.context.set_ragged_attn_split(0, 64)
        return m


@pytest.fixture(scope="module")
def hd32():
    return Hd32()


def _ids_ok(case, m, kt, got):
    """fp32 cache: the oracle's ids, exactly.  bf16: each row replayed through the oracle forced to
    the device's own cache (tests/kv_bf16_ref.py), ids equal wherever the top-2 margin is 1e-3"""
    assert [g.size for g in got] == [case.MAX_NEW - n for n in case.LENS]
    for b, g in enumerate(got):
        if kt == "f32":
            assert np.array_equal(g, case.ids[b]), (b, g, case.ids[b])
            continue
        caches = [m.context.cache_read(l, b, 0, case.args.max_seq_len) for l in range(case.args.n_layers)]
        _, steps, margins = kv.replay(kv.ForcedOracle(case.w64, case.one, caches), [(case.prompts[b], 0)], g, case.MAX_NEW)
        close = margins < 1e-3
        assert int(close.sum()) <= math.ceil(g.size / 50), (b, int(close.sum()))
        assert np.array_equal(np.asarray(g)[~close], steps.argmax(-1)[~close]), b


@pytest.mark.parametrize("kt", ref.KTS)
def test_hd32_model_generates_to_the_last_slot(hd32, kt):
    """The head size no model of the suite had: greedy ragged ids to slot 319 — past the
    single-pass score loop's 256 — in auto mode, which must stay on the single-pass kernel; the same
    with the split form forced."""
    m = hd32.model(kt)
    info = m.context.ragged_attn_info()
    assert info["mode"] == 0
    auto = m.generate_ragged(hd32.prompts, hd32.MAX_NEW)
    assert m.context.ragged_attn_info()["split_launches"] == info["split_launches"], "auto mode left the single-pass kernel"
    _ids_ok(hd32, m, kt, auto)
    m.context.reset_cache()
    m.context.set_ragged_attn_split(1, 64)
    forced = m.generate_ragged(hd32.prompts, hd32.MAX_NEW)
    steps = hd32.MAX_NEW - min(hd32.LENS) - 1
    assert m.context.ragged_attn_info()["split_launches"] == info["split_launches"] + steps * hd32.args.n_layers
    _ids_ok(hd32, m, kt, forced)
    m.context.set_ragged_attn_split(0, 64)


@pytest.mark.parametrize("kt", ref.KTS)
def test_hd32_model_extends_in_two_chunks_and_forks(hd32, kt):
    """extend_ragged of each prompt's second part on the first part's cache: the oracle's logits of
    the whole prompt at 1e-4 (bf16: of the oracle forced to the device's cache).  Then
    l3_cache_copy_rows with n_slots 63, 64, 65 (COPY_SLOTS = 64), read back bit for bit."""
    m = hd32.model(kt)
    cuts = [1, 100, 170]
    m.forward_ragged([p[:c] for p, c in zip(hd32.prompts, cuts)])
    lg = m.extend_ragged([p[c:] for p, c in zip(hd32.prompts, cuts)], cuts)
    S, L = hd32.args.max_seq_len, hd32.args.n_layers
    for b, p in enumerate(hd32.prompts):
        if kt == "bf16":
            caches = [m.context.cache_read(l, b, 0, S) for l in range(L)]
            want, _, _ = kv.replay(kv.ForcedOracle(hd32.w64, hd32.one, caches), [(p[:cuts[b]], 0), (p[cuts[b]:], cuts[b])], [], 0)
        else:
            want = orc.OracleModel(hd32.w64, hd32.one)(p[None], 0)[0, -1]
        err = float(np.abs(lg[b, 0].astype(np.float64) - want).max())
        assert err <= 1e-4, (b, err)
    for n_slots in (63, 64, 65):
        before = [m.context.cache_read(l, 0, 0, S) for l in range(L)]
        m.fork_cache(2, [0], n_slots)
        for l in range(L):
            src, dst = m.context.cache_read(l, 2, 0, S), m.context.cache_read(l, 0, 0, S)
            for s, d, was in zip(src, dst, before[l]):
                assert s[:, :n_slots].any() and np.array_equal(_bits(d[:, :n_slots]), _bits(s[:, :n_slots])), (l, n_slots)
                assert np.array_equal(_bits(d[:, n_slots:]), _bits(was[:, n_slots:])), (l, n_slots)
        m.fork_cache(1, [0], 70)  # another history in row 0 before the next fork


# ---- device checks --------------------------------------------------------------------------------

def test_check_build_records_no_violation():
    assert os.path.exists(CHECK_LIB), f"{CHECK_LIB} missing: __graft_entry__.build() makes it"
    env = dict(os.environ, L3_LIB_PATH=CHECK_LIB)
    r = subprocess.run([sys.executable, os.path.join(HERE, "ragged_attn_checks_workload.py")], env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["enabled"] is True
    assert out["workload"] == {"kv_slot": 0, "attn_keys": 0, "token_id": 0}
    assert out["launches"] >= 6 * 2 * 5 and out["split_launches"] >= 6 * 2 * 3
