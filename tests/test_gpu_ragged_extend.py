"""Ragged continuation (DESIGN.md "Ragged continuation"; csrc/ragged_extend.hip,
l3_ragged_extend_host / l3_ragged_generate_from_host / l3_cache_copy_rows /
l3_op_attn_extend_ragged_host): several new tokens per row, each row at its own offset.

Op level: the two launches on plain arrays against the fp64 reference of tests/extend_attn_ref.py,
with (start, len) pairs that straddle every tile edge.  Model level, on the models of
tests/test_gpu_ragged.py with "sharp" weights: the reference for row b is the oracle run on that
row alone with the same sequence of calls — its logits within the project's 1e-4 bar, its greedy
ids exactly.  Each model's oracle rows are computed once and shared by the tests below."""

import dataclasses
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import extend_attn_ref as ref
import l3hip
import llama3
import llama3_oracle as orc
import synth
from config import ModelArgs
from split_attn_ref import POSITIONS
from test_gpu_ragged import SHAPES

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHECK_LIB = os.path.join(os.path.dirname(HERE), "llama3.np_amd", "csrc", "libllama3hip_check.so")

# (HD, n_rep) at KVH = 2, the table of tests/test_gpu_ragged_split.py: 64 / n_rep query tokens per
# workgroup is 32, 64, 8, 21 (one query row idle) and 16
OP_SHAPES = [(16, 2), (48, 1), (64, 8), (96, 3), (128, 4)]


@pytest.fixture(scope="module")
def ctx():
    return l3hip.op_context(0)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 1. op level -------------------------------------------------------------------------------

@pytest.mark.parametrize("hd,n_rep", OP_SHAPES)
def test_op_matches_the_reference_at_every_tile_edge(ctx, hd, n_rep):
    """Measured on an MI355X (max-abs error of out against fp64):
      (16, 2) 5.07e-07    (48, 1) 4.99e-07    (64, 8) 6.55e-07    (96, 3) 7.84e-07    (128, 4) 9.96e-07
    The bound, 1e-5, is the project's kernel-against-reference floor for attention over N(0, 1)
    inputs (tests/test_gpu_ragged_split.py)."""
    inp = ref.make_inputs(hd, n_rep)
    want, want_k, want_v = ref.reference(inp)
    out, ck, cv = ctx.op_attn_extend_ragged(inp["qkv"], inp["cache_k"], inp["cache_v"], inp["rope_cos"],
                                            inp["rope_sin"], inp["starts"], inp["lens"], inp["n_heads"])
    assert out.shape == want.shape and out.dtype == np.float32
    assert np.isfinite(out).all()  # no poisoned slot was read
    err = float(np.abs(out.astype(np.float64) - want).max())
    print(f"HD {hd} n_rep {n_rep}: max-abs {err:.3e}")
    assert err <= 1e-5, err
    for b, (st, n) in enumerate(ref.PAIRS):
        assert not out[b, n:].any(), b  # the pads
        # the new slots: the RoPE'd k within 1e-6 of the reference, relative to the row's largest
        # element (a rotated pair can cancel, so not element by element); v exactly
        for g in range(2):
            for p in range(st, st + n):
                e = float(np.abs(ck[b, g, p].astype(np.float64) - want_k[b, g, p]).max())
                assert e <= 1e-6 * float(np.abs(want_k[b, g, p]).max()), (b, g, p, e)
        assert np.array_equal(cv[b, :, st:st + n].astype(np.float64), want_v[b, :, st:st + n])
        # every other slot bit for bit what went in, NaNs included
        for got, was in ((ck, inp["cache_k"]), (cv, inp["cache_v"])):
            keep = np.ones(ref.SMAX, bool)
            keep[st:st + n] = False
            assert np.array_equal(_bits(got[b][:, keep]), _bits(was[b][:, keep])), b


@pytest.mark.parametrize("hd,n_rep", OP_SHAPES)
def test_one_token_extend_agrees_with_the_decode_kernel(ctx, hd, n_rep):
    inp = ref.make_inputs(hd, n_rep, lq=1, pairs=tuple((p, 1) for p in POSITIONS))
    out, ck, cv = ctx.op_attn_extend_ragged(inp["qkv"], inp["cache_k"], inp["cache_v"], inp["rope_cos"],
                                            inp["rope_sin"], inp["starts"], inp["lens"], inp["n_heads"])
    dec, dk, dv = ctx.op_attn_decode_ragged(inp["qkv"][:, 0], inp["cache_k"], inp["cache_v"], inp["rope_cos"],
                                            inp["rope_sin"], inp["starts"], np.zeros(len(POSITIONS), np.int32),
                                            inp["n_heads"], ref.SMAX, 0)
    err = float(np.abs(out[:, 0] - dec).max())
    print(f"HD {hd} n_rep {n_rep}: extend against decode max-abs {err:.3e}")
    assert np.isfinite(out).all() and err <= 1e-5, err
    assert np.array_equal(_bits(cv), _bits(dv))
    k_err = np.abs(ck.astype(np.float64) - dk.astype(np.float64))
    assert float(np.nanmax(k_err)) <= 1e-6 * float(np.nanmax(np.abs(dk))) and \
        np.array_equal(np.isnan(ck), np.isnan(dk))


def test_op_refuses_what_no_kernel_takes(ctx):
    wide = ref.make_inputs(16, 16, kvh=1, smax=8, lq=2, pairs=((0, 2),))
    with pytest.raises(RuntimeError, match="at most 8 query heads per KV head"):
        ctx.op_attn_extend_ragged(wide["qkv"], wide["cache_k"], wide["cache_v"], wide["rope_cos"], wide["rope_sin"],
                                  wide["starts"], wide["lens"], wide["n_heads"])
    inp = ref.make_inputs(16, 2, smax=8, lq=4, pairs=((0, 2), (3, 4)))
    for starts, lens, match in (([0, 5], [2, 4], r"row 1: positions \[5, 9\) exceed Smax 8"),
                                ([-1, 3], [2, 4], r"starts\[0\] = -1 is negative"),
                                ([0, 3], [5, 4], r"lens\[0\] = 5 outside \[0, 4\]")):
        with pytest.raises(RuntimeError, match=match):
            ctx.op_attn_extend_ragged(inp["qkv"], inp["cache_k"], inp["cache_v"], inp["rope_cos"], inp["rope_sin"],
                                      starts, lens, inp["n_heads"])
    # a row of pads only: zeros out, its cache untouched
    out, ck, cv = ctx.op_attn_extend_ragged(inp["qkv"], inp["cache_k"], inp["cache_v"], inp["rope_cos"],
                                            inp["rope_sin"], [0, 3], [0, 4], inp["n_heads"])
    assert not out[0].any() and np.isfinite(out[1]).all()
    assert np.array_equal(_bits(ck[0]), _bits(inp["cache_k"][0])) and np.array_equal(_bits(cv[0]), _bits(inp["cache_v"][0]))


# ---- models ------------------------------------------------------------------------------------

# name -> (prompt lengths, the per-row cut into two chunks, the cuts into three, max_new_tokens):
# the models of tests/test_gpu_ragged.py; the long runs end at the last cache slot (tiny, gqa)
PLANS = {
    "tiny": ((3, 5, 9, 14), (1, 2, 6, 3), ((1, 2), (1, 3), (2, 7), (5, 6)), 64),
    "stories": ((3, 9, 9, 17, 33), (1, 4, 8, 16, 20), ((1, 2), (3, 5), (1, 2), (6, 16), (17, 18)), 41),
    "gqa": ((3, 30, 64), (1, 17, 33), ((1, 2), (10, 20), (16, 48)), 96),
}


def continued_greedy(model, logits, total, max_new):
    """The reference's loop (llama3.py:310-321) continued from a cache that holds ``total``
    tokens, ``logits`` being those of the last of them: the first id from position total - 1,
    step i >= 1 at total + i, slot total never written."""
    out, nxt = [], None
    for i, pos in enumerate(range(total, max_new)):
        if i:
            logits = model(nxt, pos)
        nxt = logits[:, -1, :].argmax(-1, keepdims=True)
        out.append(int(nxt[0, 0]))
    return np.array(out, np.int64)


class Case:
    def __init__(self, name):
        self.args, hidden, _, _ = SHAPES[name]
        self.lens, self.cuts, self.cuts3, self.max_new = PLANS[name]
        self.w = synth.make_weights(self.args, hidden, seed=31, preset="sharp")
        self.w64 = {k: np.asarray(v, np.float64) for k, v in self.w.items()}
        rng = np.random.default_rng(7)
        self.prompts = [rng.integers(0, self.args.vocab_size, n) for n in self.lens]
        self.first = [p[:c] for p, c in zip(self.prompts, self.cuts)]
        self.second = [p[c:] for p, c in zip(self.prompts, self.cuts)]
        self.model = llama3.Llama(self.w, self.args, device=0)
        self.one = dataclasses.replace(self.args, max_batch_size=1)
        self.logits, self.logits3, self.ids = [], [], []
        for p, c, (c1, c2) in zip(self.prompts, self.cuts, self.cuts3):  # each row alone on a zeroed cache
            m = orc.OracleModel(self.w64, self.one)
            m(p[None, :c], 0)
            lg = m(p[None, c:], c)
            self.logits.append(lg[0, -1])
            self.ids.append(continued_greedy(m, lg, p.size, self.max_new))
            m = orc.OracleModel(self.w64, self.one)
            m(p[None, :c1], 0)
            m(p[None, c1:c2], c1)
            self.logits3.append(m(p[None, c2:], c2)[0, -1])

    def want(self, max_new):
        """row b's first max(0, max_new - len_b) greedy ids (a greedy prefix does not depend on
        where the loop ends)"""
        return [ids[:max(0, max_new - n)] for ids, n in zip(self.ids, self.lens)]

    def prefill_first(self):
        self.model.forward_ragged(self.first)


_cases = {}


@pytest.fixture
def case(request):
    name = request.param
    if name not in _cases:
        _cases[name] = Case(name)
    _cases[name].model.context.reset_cache()
    _cases[name].model.set_sampling(0.0)
    _cases[name].model.context.set_ragged_attn_split(0)
    return _cases[name]


def _same_rows(got, want):
    assert len(got) == len(want)
    for b, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.int64 and np.array_equal(g, w), (b, g, w)


def _padded(rows, fill=0):
    lens = np.array([r.size for r in rows], np.int32)
    ids = np.full((len(rows), int(lens.max())), fill, np.int64)
    for b, r in enumerate(rows):
        ids[b, :r.size] = r
    return ids, lens


# ---- 2. logits -----------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["tiny", "stories", "gqa"], indirect=True)
def test_two_chunks_match_the_oracle(case):
    """Measured on an MI355X (max-abs error of the logits, largest row): 
    tiny 2.4e-06, stories 4.9e-05, gqa 5.7e-05."""
    m, V = case.model, case.args.vocab_size
    case.prefill_first()
    got = m.extend_ragged(case.second, case.cuts)
    assert got.shape == (len(case.lens), 1, V) and got.dtype == np.float32
    for b, want in enumerate(case.logits):
        err = float(np.abs(got[b, 0].astype(np.float64) - want).max())
        print(f"row {b} ({case.cuts[b]} + {case.lens[b] - case.cuts[b]}): max-abs {err:.3e}")
        assert err <= 1e-4, (b, err)
    # the pad entries are never looked at: garbage and out-of-range values change nothing
    _, lens = _padded(case.second)
    for fill in (V - 1, 10 ** 12, -5 * V):
        m.context.reset_cache()
        case.prefill_first()
        junk, _ = _padded(case.second, fill)
        again = np.array(m.context.ragged_extend(junk, lens, case.cuts))
        assert np.array_equal(_bits(again), _bits(got[:, 0])), fill


@pytest.mark.parametrize("case", ["tiny", "stories", "gqa"], indirect=True)
def test_three_chunks_match_the_oracle(case):
    m = case.model
    m.forward_ragged([p[:c1] for p, (c1, _) in zip(case.prompts, case.cuts3)])
    m.extend_ragged([p[c1:c2] for p, (c1, c2) in zip(case.prompts, case.cuts3)], [c1 for c1, _ in case.cuts3])
    got = m.extend_ragged([p[c2:] for p, (_, c2) in zip(case.prompts, case.cuts3)], [c2 for _, c2 in case.cuts3])
    for b, want in enumerate(case.logits3):
        err = float(np.abs(got[b, 0].astype(np.float64) - want).max())
        print(f"row {b} {case.cuts3[b]} of {case.lens[b]}: max-abs {err:.3e}")
        assert err <= 1e-4, (b, err)


# ---- 3. greedy continuation ------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["tiny", "stories", "gqa"], indirect=True)
def test_greedy_continuation_matches_each_row_alone(case):
    m = case.model
    case.prefill_first()
    got = m.generate_ragged(case.second, case.max_new, start_pos=case.cuts)  # tiny, gqa: to the last cache slot
    _same_rows(got, case.want(case.max_new))
    assert [g.size for g in got] == [case.max_new - n for n in case.lens]
    # a row with no budget yields nothing; the others their prefix
    m.context.reset_cache()
    case.prefill_first()
    short = max(case.lens)
    got = m.generate_ragged(case.second, short, start_pos=case.cuts)
    _same_rows(got, case.want(short))
    assert got[-1].size == 0 and got[0].size == short - case.lens[0]
    # through the context: [B, cap] with -1 past each row's tokens
    m.context.reset_cache()
    case.prefill_first()
    ids, lens = _padded(case.second)
    out, n = m.context.ragged_generate(ids, lens, short, starts=case.cuts)
    assert out.shape == (len(lens), short - min(case.lens)) and n.tolist() == [short - x for x in case.lens]
    for b in range(len(lens)):
        assert (out[b, n[b]:] == -1).all() and np.array_equal(out[b, :n[b]], got[b])


@pytest.mark.parametrize("case", ["tiny", "stories", "gqa"], indirect=True)
def test_continuation_on_a_dirtied_cache_zeroes_the_hole(case):
    """A full-length forward first fills slots [0, Lmax) of every row with other tokens' K / V.
    The prefill and the extend overwrite [0, T_b); slot T_b, which the decode steps attend and
    never write, must read as zero again or the ids differ."""
    m = case.model
    rng = np.random.default_rng(11)
    m(rng.integers(0, case.args.vocab_size, (len(case.lens), max(case.lens) + 1)), 0)
    case.prefill_first()
    max_new = min(case.lens) + 12
    _same_rows(m.generate_ragged(case.second, max_new, start_pos=case.cuts), case.want(max_new))


@pytest.mark.parametrize("case", ["tiny", "gqa"], indirect=True)
def test_continuation_with_split_kv_forced(case):
    m = case.model
    m.context.set_ragged_attn_split(1, 64)
    before = m.context.ragged_attn_info()["split_launches"]
    case.prefill_first()
    _same_rows(m.generate_ragged(case.second, case.max_new, start_pos=case.cuts), case.want(case.max_new))
    assert m.context.ragged_attn_info()["split_launches"] > before


def _truncate(rows, stops):
    out = []
    for r in rows:
        hit = np.flatnonzero(np.isin(r, stops))
        out.append(r[:hit[0] + 1] if hit.size else r)
    return out


@pytest.mark.parametrize("case", ["tiny"], indirect=True)
def test_stop_ids_end_a_continued_row(case):
    m, max_new = case.model, 40
    base = case.want(max_new)
    stop = int(base[1][len(base[1]) // 2])  # a token row 1 emits mid-way
    want = _truncate(base, [stop])
    assert want[1].size < base[1].size
    case.prefill_first()
    _same_rows(m.generate_ragged(case.second, max_new, stop_ids=[stop, 10 ** 9], start_pos=case.cuts), want)


SAMPLING = (0.8, 40, 0.95, 4321)


@pytest.mark.parametrize("case", ["tiny"], indirect=True)
def test_sampled_continuation_reproduces_across_cuts_and_calls(case):
    """Rows of equal T_b: a token's uniform is that of (seed, row, position), so the same rows cut
    at other points, and the uncut rows through generate_all, draw the same ids."""
    m, V = case.model, case.args.vocab_size
    prompt = np.random.default_rng(13).integers(0, V, (3, 9))
    total = 31
    m.set_sampling(*SAMPLING)
    want = m.generate_all(prompt, total)
    runs = []
    for cuts in ((2, 5, 8), (7, 1, 4), (2, 5, 8)):
        m.context.reset_cache()
        m.forward_ragged([p[:c] for p, c in zip(prompt, cuts)])
        runs.append(np.stack(m.generate_ragged([p[c:] for p, c in zip(prompt, cuts)], total, start_pos=cuts)))
    assert np.array_equal(runs[0], runs[2]) and np.array_equal(runs[0], runs[1])
    assert np.array_equal(runs[0], want)
    m.set_sampling(0.0)
    m.context.reset_cache()
    m.forward_ragged([p[:4] for p in prompt])
    greedy = np.stack(m.generate_ragged([p[4:] for p in prompt], total, start_pos=[4] * 3))
    assert not np.array_equal(greedy, want)  # it was sampled


# ---- 4. prefix reuse and forks ---------------------------------------------------------------------

@pytest.mark.parametrize("case", ["tiny", "stories", "gqa"], indirect=True)
def test_prefix_equals_concatenation(case):
    m = case.model
    P = 6
    pre = np.random.default_rng(23).integers(0, case.args.vocab_size, P)
    rest = [p[:n] for p, n in zip(case.prompts, (1, 3, 2, 5, 4))]  # suffix lengths differ per row
    max_new = P + 5 + 14
    want = [orc.greedy_ids(orc.OracleModel(case.w64, case.one), np.concatenate([pre, r])[None], max_new)[0]
            for r in rest]
    # a dirty cache: rows 1.. hold other tokens where the prefix is forked to
    m(np.random.default_rng(29).integers(0, case.args.vocab_size, (len(rest), P + 7)), 0)
    _same_rows(m.generate_ragged(rest, max_new, prefix=pre), want)
    # the same by hand: prefill on row 0, fork, generate from the offset
    m.context.reset_cache()
    m(pre[None], 0)
    m.fork_cache(0, range(1, len(rest)), P)
    _same_rows(m.generate_ragged(rest, max_new, start_pos=[P] * len(rest)), want)
    with pytest.raises(ValueError, match="not both"):
        m.generate_ragged(rest, max_new, start_pos=[P] * len(rest), prefix=pre)


@pytest.mark.parametrize("case", ["tiny", "gqa"], indirect=True)
def test_forked_row_equals_its_source(case):
    m, B = case.model, len(case.lens)
    hist = case.prompts[-1][:-3]
    chunk = case.prompts[-1][-3:]
    m(hist[None], 0)  # row 0
    m.fork_cache(0, [B - 1], hist.size)
    got = np.array(m.extend_ragged([chunk] * B, [hist.size] * B))
    assert np.array_equal(_bits(got[0]), _bits(got[B - 1]))
    assert not np.array_equal(_bits(got[0]), _bits(got[1]))  # row 1 has no history: other logits


# ---- 5. errors -------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["tiny"], indirect=True)
def test_errors_are_reported_and_leave_the_context_usable(case, monkeypatch):
    m, c, V = case.model, case.model.context, case.args.vocab_size
    ids, lens = _padded(case.second)  # lens (2, 3, 3, 11), Lmax 11
    starts = np.array(case.cuts, np.int32)

    def bad(match, ids, lens, starts, max_new=20):
        with pytest.raises(RuntimeError, match=match):
            c.ragged_extend(ids, lens, starts)
        with pytest.raises(RuntimeError, match=match):
            c.ragged_generate(ids, lens, max_new, starts=starts)

    zero = lens.copy()
    zero[1] = 0
    bad(r"lens\[1\] = 0 outside \[1, 11\]", ids, zero, starts)
    long = lens.copy()
    long[0] = 12
    bad(r"lens\[0\] = 12 outside \[1, 11\]", ids, long, starts)
    bad("batch 5 exceeds max_batch_size 4", np.zeros((5, 3), np.int64), np.full(5, 3, np.int32), np.zeros(5, np.int32))
    neg = starts.copy()
    neg[2] = -1
    bad(r"starts\[2\] = -1 is negative", ids, lens, neg)
    far = starts.copy()
    far[3] = 54
    bad(r"row 3: positions \[54, 65\) exceed max_seq_len 64", ids, lens, far)
    with pytest.raises(RuntimeError, match="last decode position 64 exceeds max_seq_len 64"):
        c.ragged_generate(ids, lens, 65, starts=starts)
    oob = ids.copy()
    oob[2, 2] = V  # the last real position of row 2 (3 new tokens)
    bad(f"token id {V} out of range for vocab_size {V}", oob, lens, starts)
    lib = l3hip.lib()
    out = np.zeros((4, V), np.float32)
    for args in ((None, l3hip.ptr(lens), l3hip.ptr(starts)), (l3hip.ptr(ids), None, l3hip.ptr(starts)),
                 (l3hip.ptr(ids), l3hip.ptr(lens), None)):
        assert lib.l3_ragged_extend_host(c.handle, *args, 4, 11, l3hip.ptr(out)) != 0
        assert b"l3_ragged_extend_host: null argument" in lib.l3_last_error()
        toks, n = np.zeros((4, 20), np.int64), np.zeros(4, np.int32)
        assert lib.l3_ragged_generate_from_host(c.handle, *args, 4, 11, 20, None, 0, l3hip.ptr(toks), l3hip.ptr(n)) != 0
        assert b"l3_ragged_generate_from_host: null argument" in lib.l3_last_error()
    assert lib.l3_ragged_extend_host(c.handle, l3hip.ptr(ids), l3hip.ptr(lens), l3hip.ptr(starts), 4, 11, None) != 0
    assert b"null argument" in lib.l3_last_error()
    with pytest.raises(ValueError):
        c.ragged_extend(ids, lens, starts[:2])
    # the copy
    for src, dst, n, match in ((4, [1], 3, r"src_row 4 outside \[0, 4\)"), (-1, [1], 3, r"src_row -1 outside"),
                               (0, [1, 4], 3, r"dst_rows\[1\] = 4 outside \[0, 4\)"),
                               (0, [2, 0], 3, r"dst_rows\[1\] is src_row 0"),
                               (0, [1], 65, r"n_slots 65 outside \[0, 64\]"), (0, [1], -1, r"n_slots -1 outside")):
        with pytest.raises(RuntimeError, match=match):
            c.cache_copy_rows(src, dst, n)
    assert lib.l3_cache_copy_rows(c.handle, 0, None, 2, 3) != 0
    assert b"l3_cache_copy_rows: null argument" in lib.l3_last_error()
    # a head shape the ragged attention does not take
    wide = ModelArgs(dim=256, n_layers=1, n_heads=16, n_kv_heads=1, vocab_size=64, max_seq_len=32, max_batch_size=2)
    wm = llama3.Llama(synth.make_weights(wide, 64, seed=3, preset="sharp"), wide, device=0)
    with pytest.raises(RuntimeError, match="at most 8 query heads per KV head"):
        wm.extend_ragged([[1, 2], [3]], [0, 0])
    with pytest.raises(RuntimeError, match="at most 8 query heads per KV head"):
        wm.generate_ragged([[1, 2], [3]], 8, start_pos=[0, 0])
    # a member of a multi-device group
    monkeypatch.setenv("L3_GROUP_VIRTUAL", "1")
    grp = llama3.Llama(case.w, case.args, devices=[0, 0])
    member = grp.group.members[0]
    with pytest.raises(RuntimeError, match="member of a multi-device l3_group"):
        member.ragged_extend(ids[:1], lens[:1], starts[:1])
    with pytest.raises(RuntimeError, match="member of a multi-device l3_group"):
        member.ragged_generate(ids[:1], lens[:1], 20, starts=starts[:1])
    with pytest.raises(RuntimeError, match="member of a multi-device l3_group"):
        member.cache_copy_rows(0, [1], 3)
    with pytest.raises(NotImplementedError):
        grp.extend_ragged(case.second, case.cuts)
    with pytest.raises(NotImplementedError):
        grp.fork_cache(0, [1], 3)
    with pytest.raises(NotImplementedError):  # refused before the prefix is prefilled
        grp.generate_ragged(case.second, 20, prefix=[1, 2, 3])
    # nothing was launched: the cache is still zero, and the ragged calls that follow are exact
    case.prefill_first()
    max_new = min(case.lens) + 10
    _same_rows(m.generate_ragged(case.second, max_new, start_pos=case.cuts), case.want(max_new))


# ---- 6. check library --------------------------------------------------------------------------------

def test_check_build_records_no_violation():
    assert os.path.exists(CHECK_LIB), f"{CHECK_LIB} missing: __graft_entry__.build() makes it"
    env = dict(os.environ, L3_LIB_PATH=CHECK_LIB)
    r = subprocess.run([sys.executable, os.path.join(HERE, "ragged_extend_checks_workload.py")], env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["enabled"] is True
    assert out["workload"] == {"kv_slot": 0, "attn_keys": 0, "token_id": 0}
    assert out["tokens"] > 0 and out["extends"] > 0
