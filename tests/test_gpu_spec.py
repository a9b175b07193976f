"""Speculative decoding with lookup drafts (DESIGN.md "Speculative decoding"; csrc/spec.hip,
l3_ragged_generate_spec_host / l3_ragged_verify_host / l3_op_spec_draft_host).

The drafting rule is tests/spec_ref.py's; the truth for a row is the oracle's greedy ids on that
row alone (the models, prompts and seeds of tests/test_gpu_ragged_extend.py, whose cases are
shared), and the counters are those of spec_ref.simulate replayed on those ids."""

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
from config import ModelArgs
from test_gpu_ragged_extend import SAMPLING, Case, _cases, _padded, _same_rows, _truncate

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHECK_LIB = os.path.join(os.path.dirname(HERE), "llama3.np_amd", "csrc", "libllama3hip_check.so")
DRAFT_LENS = (0, 1, 4, 7, 15)


@pytest.fixture(scope="module")
def ctx():
    return l3hip.op_context(0)


@pytest.fixture
def case(request):
    name = request.param
    if name not in _cases:
        _cases[name] = Case(name)
    c = _cases[name]
    c.model.context.reset_cache()
    c.model.set_sampling(0.0)
    c.model.context.set_ragged_attn_split(0)
    return c


# ---- 1. the draft op --------------------------------------------------------------------------------

SEQ_LENS = (1, 2, 3, 255, 256, 257, 1025, 4097)  # the workgroup's stride edges


def _draft_rows():
    rng = np.random.default_rng(41)
    rows = [rng.integers(0, alphabet, n) for alphabet in (2, 1000) for n in SEQ_LENS]
    uniq = np.arange(100, 400)
    rows.append(np.concatenate([[7], uniq, [7]]))            # n = 1: the only match is at j = 0
    rows.append(np.concatenate([[1, 2, 3], uniq, [1, 2, 3]]))  # n = 3: the only match is at j = 0
    rows.append(np.concatenate([uniq, [9, 9]]))              # n = 1: j = E - 2, the draft clipped at E
    rows.append(np.concatenate([uniq, [4, 4, 4, 4]]))        # n = 3: j = E - 4
    return rows


@pytest.mark.parametrize("n_max", [1, 3, 8])
def test_draft_op_equals_the_reference(ctx, n_max):
    rows = _draft_rows()
    seq, lens = _padded(rows)
    draft_len = 7
    for kk in (0, 1, draft_len):
        for n_min in (1, n_max):
            out, n = ctx.op_spec_draft(seq, lens, np.full(len(rows), kk), draft_len, n_max, n_min)
            assert out.shape == (len(rows), draft_len) and out.dtype == np.int32
            for b, r in enumerate(rows):
                want = spec_ref.draft(r, kk, n_max, n_min)
                assert n[b] == len(want) and out[b, :n[b]].tolist() == want and (out[b, n[b]:] == -1).all(), \
                    (b, kk, n_max, n_min, out[b], want)
    # the hand-made rows find what they were made for
    out, n = ctx.op_spec_draft(seq, lens, np.full(len(rows), draft_len), draft_len, n_max, 1)
    assert out[-4, :n[-4]].tolist() == list(range(100, 107))
    assert out[-3, :n[-3]].tolist() == list(range(100, 107))
    assert out[-2, :n[-2]].tolist() == [9]
    assert out[-1, :n[-1]].tolist() == [4]


def test_draft_op_per_row_limits_and_longest_draft(ctx):
    rng = np.random.default_rng(43)
    rows = [rng.integers(0, 3, n) for n in (40, 41, 300, 2000)]
    rows[2] = np.tile(np.arange(20), 3)  # period 20: the match one period back has 20 tokens after it
    seq, lens = _padded(rows)
    k = np.array([0, 3, 15, 9], np.int32)
    out, n = ctx.op_spec_draft(seq, lens, k, 15, 8, 1)
    for b, r in enumerate(rows):
        want = spec_ref.draft(r, int(k[b]), 8, 1)
        assert out[b, :n[b]].tolist() == want and n[b] == len(want) and (out[b, n[b]:] == -1).all()
    assert n[0] == 0 and out[2].tolist() == list(range(15))


# ---- 2. verify ----------------------------------------------------------------------------------------

def _oracle_chosen(case, b, chunk, start):
    """the oracle's greedy id at every position of ``chunk`` run at ``start`` after row b's prompt"""
    m = orc.OracleModel(case.w64, case.one)
    m(case.prompts[b][None], 0)
    return [int(m(np.array([[t]]), start + i)[0, -1].argmax()) for i, t in enumerate(chunk)]


def _chunks(case, variant):
    """row b's chunk at position T_b + 1 (the reference's schedule): its true continuation, 2 + b
    tokens of it (so the rows differ in length), one position replaced, or one token only"""
    out = []
    for b, ids in enumerate(case.ids):
        n = 1 if variant == "one" else min(2 + b, ids.size - 1)
        c = ids[:n].copy()
        j = {"true": None, "one": None, "first": 0, "middle": n // 2, "last": n - 1}[variant]
        if j is not None:
            c[j] = (c[j] + 1) % case.args.vocab_size
        out.append(c)
    return out


@pytest.mark.parametrize("variant", ["true", "first", "middle", "last", "one"])
@pytest.mark.parametrize("case", ["tiny", "stories", "gqa"], indirect=True)
def test_verify_matches_the_oracle(case, variant):
    m = case.model
    chunks = _chunks(case, variant)
    starts = [n + 1 for n in case.lens]  # rows at different positions in one batch
    m.forward_ragged(case.prompts)
    chosen, n_accept = m.verify_ragged(chunks, starts)
    ids, lens = _padded(chunks)
    raw, _ = m.context.ragged_verify(ids, lens, starts)  # (the same call again: an extend is idempotent)
    for b, c in enumerate(chunks):
        want = _oracle_chosen(case, b, c, starts[b])
        assert chosen[b].dtype == np.int64 and chosen[b].tolist() == want, (b, chosen[b], want)
        assert raw[b, :c.size].tolist() == want and (raw[b, c.size:] == -1).all()
        a = 0
        while a < c.size - 1 and c[a + 1] == want[a]:
            a += 1
        assert n_accept[b] == a, (b, n_accept[b], a)
        if variant == "true":
            assert a == c.size - 1 and want == case.ids[b][1:c.size + 1].tolist()


@pytest.mark.parametrize("case", ["tiny", "gqa"], indirect=True)
def test_verify_leaves_the_cache_as_an_extend_does(case):
    m = case.model
    chunks = _chunks(case, "middle")
    starts = [n + 1 for n in case.lens]
    after = [[int(ids[c.size])] for ids, c in zip(case.ids, chunks)]
    after_at = [s + c.size for s, c in zip(starts, chunks)]
    m.forward_ragged(case.prompts)
    m.verify_ragged(chunks, starts)
    got = np.array(m.extend_ragged(after, after_at))
    m.context.reset_cache()
    m.forward_ragged(case.prompts)
    m.extend_ragged(chunks, starts)
    want = np.array(m.extend_ragged(after, after_at))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---- 3. speculative generation ------------------------------------------------------------------------

def _corrupt(ids, V):
    bad = np.array(ids, np.int64)
    bad[5::7] = (bad[5::7] + 1) % V
    return bad


def _lookup(case, mode):
    if mode == "none":
        return None
    if mode == "true":
        return [ids for ids in case.ids]
    return [_corrupt(ids, case.args.vocab_size) for ids in case.ids]


def _simulate(case, prompts, lookup, want, draft_len, n_max=3, n_min=1, stops=()):
    rows = [spec_ref.simulate([] if lookup is None else lookup[b], prompts[b], want[b], draft_len, n_max, n_min, stops)
            for b in range(len(prompts))]
    return [np.array(r[0], np.int64) for r in rows], np.array([r[1:] for r in rows], np.int64).reshape(-1, 3)


def _check(got, stats, sim_ids, sim_counts):
    _same_rows(got, sim_ids)
    have = np.stack([stats["row_steps"], stats["drafted"], stats["accepted"]], axis=1)
    assert np.array_equal(have, sim_counts), (have.tolist(), sim_counts.tolist())


# recorded from the oracle's ids on the CPU for draft_len 4 (ngram_max 3): per row (row_steps, drafted, accepted)
RECORDED = {
    ("tiny", "none"): {0: (47, 20, 13), 1: (23, 38, 35), 2: (49, 12, 5), 3: (36, 16, 13)},
    ("stories", "true"): {0: (8, 29, 29)},
    ("stories", "bad"): {0: (15, 38, 22)},
    ("gqa", "bad"): {0: (39, 101, 53)},
}


@pytest.mark.parametrize("case,mode", [("tiny", "none"), ("stories", "none"), ("stories", "true"), ("stories", "bad"),
                                       ("gqa", "none"), ("gqa", "true"), ("gqa", "bad")], indirect=["case"])
def test_speculative_ids_and_counters(case, mode, request):
    m, name = case.model, request.node.callspec.params["case"]
    want = case.want(case.max_new)
    plain = m.generate_ragged(case.prompts, case.max_new)  # tiny, gqa: to the last cache slot
    _same_rows(plain, want)
    lookup = _lookup(case, mode)
    for draft_len in DRAFT_LENS:
        m.context.reset_cache()
        sim_ids, sim = _simulate(case, case.prompts, lookup, want, draft_len)
        _same_rows(sim_ids, want)
        got, stats = m.generate_ragged_spec(case.prompts, case.max_new,
                                            speculate=dict(draft_len=draft_len, ngram_max=3, lookup=lookup))
        print(f"{name} {mode} draft_len {draft_len}: {sim.tolist()}")
        _check(got, stats, sim_ids, sim)
        if draft_len == 0:
            assert not sim[:, 1:].any() and sim[:, 0].tolist() == [w.size - 1 for w in want]
            continue
        if mode == "none" and name != "tiny":
            assert not sim[:, 2].any()  # random prompts: nothing repeats
        if mode == "true":
            assert np.array_equal(sim[:, 1], sim[:, 2]) and sim[:, 2].sum() > 0  # every draft accepted
        if (name, mode) == ("tiny", "none") or mode == "bad":
            assert any(0 < a < d for _, d, a in sim.tolist()), sim.tolist()  # accepted and rejected
        if draft_len == 4:
            for b, rec in RECORDED.get((name, mode), {}).items():
                assert tuple(sim[b]) == rec, (b, sim[b], rec)
    if (name, mode) == ("stories", "true"):
        assert tuple(_simulate(case, case.prompts, lookup, want, 7)[1][0]) == (5, 32, 32)
    # through generate_ragged's option: the same list of arrays
    m.context.reset_cache()
    _same_rows(m.generate_ragged(case.prompts, case.max_new, speculate=llama3.Speculate(4, 3, 1, lookup)), want)


@pytest.mark.parametrize("case", ["tiny", "stories"], indirect=True)
def test_a_row_without_budget_and_stop_ids(case):
    m = case.model
    short = max(case.lens)  # the last row has no budget
    got, stats = m.generate_ragged_spec(case.prompts, short, speculate=dict(draft_len=4))
    sim_ids, sim = _simulate(case, case.prompts, None, case.want(short), 4)
    _check(got, stats, sim_ids, sim)
    assert got[-1].size == 0 and stats["row_steps"][-1] == 0
    # stop ids, with every draft right (the lookup is the truth): one lands inside an accepted run
    base = case.want(case.max_new)
    lookup = [ids for ids in case.ids]
    inside = None
    for b, r in enumerate(base):
        for i in range(2, r.size - 1):
            stop = int(r[i])
            ids, steps, _, acc = spec_ref.simulate(lookup[b], case.prompts[b], r, 7, 3, 1, [stop])
            if len(ids) < 1 + steps + acc and int(r[i]) not in r[:i].tolist():
                inside = stop
                break
        if inside is not None:
            break
    assert inside is not None
    stops = [inside, 10 ** 9]
    sim_ids, sim = _simulate(case, case.prompts, lookup, base, 7, stops=stops[:1])
    _same_rows(sim_ids, _truncate(base, stops[:1]))
    m.context.reset_cache()
    got, stats = m.generate_ragged_spec(case.prompts, case.max_new, stop_ids=stops,
                                        speculate=dict(draft_len=7, lookup=lookup))
    _check(got, stats, sim_ids, sim)
    m.context.reset_cache()
    _same_rows(m.generate_ragged(case.prompts, case.max_new, stop_ids=stops), sim_ids)


@pytest.mark.parametrize("case", ["tiny", "gqa"], indirect=True)
def test_continuation_dirty_cache_split_and_prefix(case):
    m, V = case.model, case.args.vocab_size
    want = case.want(case.max_new)
    bad = _lookup(case, "bad")
    # a cache dirtied beforehand, rows cut at different points
    m(np.random.default_rng(11).integers(0, V, (len(case.lens), max(case.lens) + 1)), 0)
    case.prefill_first()
    got, stats = m.generate_ragged_spec(case.second, case.max_new, start_pos=case.cuts,
                                        speculate=dict(draft_len=7, lookup=bad))
    sim_ids, sim = _simulate(case, case.second, bad, want, 7)
    _check(got, stats, sim_ids, sim)
    assert any(0 < a < d for _, d, a in sim.tolist())
    # split-KV forced: the setting belongs to the decode steps, the ids are the same
    m.context.set_ragged_attn_split(1, 64)
    m.context.reset_cache()
    got, stats = m.generate_ragged_spec(case.prompts, case.max_new, speculate=dict(draft_len=4, lookup=bad))
    sim_ids, sim = _simulate(case, case.prompts, bad, want, 4)
    _check(got, stats, sim_ids, sim)
    m.context.set_ragged_attn_split(0)
    # a shared prefix
    P = 6
    pre = np.random.default_rng(23).integers(0, V, P)
    rest = [p[:n] for p, n in zip(case.prompts, (1, 3, 2, 5, 4))]
    max_new = P + 5 + 14
    truth = [orc.greedy_ids(orc.OracleModel(case.w64, case.one), np.concatenate([pre, r])[None], max_new)[0]
             for r in rest]
    look = [_corrupt(t, V) for t in truth]
    m(np.random.default_rng(29).integers(0, V, (len(rest), P + 7)), 0)
    got, stats = m.generate_ragged_spec(rest, max_new, prefix=pre, speculate=dict(draft_len=4, lookup=look))
    sim_ids, sim = _simulate(case, rest, look, truth, 4)
    _check(got, stats, sim_ids, sim)
    with pytest.raises(ValueError, match="not both"):
        m.generate_ragged_spec(rest, max_new, start_pos=[P] * len(rest), prefix=pre)


def test_bf16_rounded_weights_against_generate_ragged():
    case = _cases.get("gqa") or Case("gqa")
    _cases["gqa"] = case
    m = llama3.Llama(case.w, case.args, device=0, weight_dtype="bf16-round")
    want = m.generate_ragged(case.prompts, case.max_new)
    look = [_corrupt(w, case.args.vocab_size) for w in want]
    for draft_len in (4, 15):
        m.context.reset_cache()
        got, stats = m.generate_ragged_spec(case.prompts, case.max_new, speculate=dict(draft_len=draft_len, lookup=look))
        sim_ids, sim = _simulate(case, case.prompts, look, want, draft_len)
        _check(got, stats, sim_ids, sim)
        assert any(0 < a < d for _, d, a in sim.tolist())


# ---- 4. sampling ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["tiny"], indirect=True)
def test_sampled_ids_equal_generate_ragged(case):
    m, V = case.model, case.args.vocab_size
    prompts = [np.random.default_rng(13).integers(0, V, n) for n in (9, 4, 9)]
    total = 31
    m.set_sampling(*SAMPLING)
    want = m.generate_ragged(prompts, total)
    look = [_corrupt(w, V) for w in want]
    for draft_len, lookup in ((4, None), (7, look), (15, want)):
        m.context.reset_cache()
        got, stats = m.generate_ragged_spec(prompts, total, speculate=dict(draft_len=draft_len, lookup=lookup))
        sim_ids, sim = _simulate(case, prompts, lookup, want, draft_len)
        _check(got, stats, sim_ids, sim)
    assert sim[:, 2].sum() > 0
    # a verify draws the same uniforms: the sampled continuation is accepted whole
    m.context.reset_cache()
    m.forward_ragged(prompts)
    chosen, n_accept = m.verify_ragged([w[:6] for w in want], [p.size + 1 for p in prompts])
    assert [c.tolist() for c in chosen] == [w[1:7].tolist() for w in want] and n_accept.tolist() == [5, 5, 5]
    m.set_sampling(0.0)
    m.context.reset_cache()
    greedy = m.generate_ragged(prompts, total)
    assert any(not np.array_equal(g, w) for g, w in zip(greedy, want))  # it was sampled


# ---- 5. errors --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["tiny"], indirect=True)
def test_errors_are_reported_and_leave_the_context_usable(case, ctx, monkeypatch):
    m, c, V = case.model, case.model.context, case.args.vocab_size
    ids, lens = _padded(case.second)  # lens (2, 3, 3, 11), Lmax 11
    starts = np.array(case.cuts, np.int32)

    def bad(match, ids, lens, starts, max_new=20, verify=True, **kw):
        with pytest.raises(RuntimeError, match=match):
            c.ragged_generate_spec(ids, lens, max_new, starts=starts, **kw)
        if verify:
            with pytest.raises(RuntimeError, match=match):
                c.ragged_verify(ids, lens, starts)

    # what the ragged generate calls refuse
    zero = lens.copy()
    zero[1] = 0
    bad(r"lens\[1\] = 0 outside \[1, 11\]", ids, zero, starts)
    bad("batch 5 exceeds max_batch_size 4", np.zeros((5, 3), np.int64), np.full(5, 3, np.int32), np.zeros(5, np.int32))
    neg = starts.copy()
    neg[2] = -1
    bad(r"starts\[2\] = -1 is negative", ids, lens, neg)
    far = starts.copy()
    far[3] = 54
    bad(r"row 3: positions \[54, 65\) exceed max_seq_len 64", ids, lens, far)
    bad("last decode position 64 exceeds max_seq_len 64", ids, lens, starts, max_new=65, verify=False)
    oob = ids.copy()
    oob[2, 2] = V
    bad(f"token id {V} out of range for vocab_size {V}", oob, lens, starts)
    with pytest.raises(RuntimeError, match=r"lens\[0\] = 12 outside \[1, 11\]"):  # without starts too
        c.ragged_generate_spec(ids, np.array([12, 3, 3, 11], np.int32), 20)
    # the ranges
    for kw, match in ((dict(draft_len=16), r"draft_len 16 outside \[0, 15\]"),
                      (dict(draft_len=-1), r"draft_len -1 outside \[0, 15\]"),
                      (dict(ngram_max=9), r"ngram_min 1, ngram_max 9 \(1 <= ngram_min <= ngram_max <= 8\)"),
                      (dict(ngram_min=0), r"ngram_min 0, ngram_max 3"),
                      (dict(ngram_min=4, ngram_max=3), r"ngram_min 4, ngram_max 3")):
        bad(match, ids, lens, starts, verify=False, **kw)
    look = np.zeros((4, 5), np.int64)
    bad(r"lookup_lens\[2\] = 6 outside \[0, 5\]", ids, lens, starts, verify=False, lookup=look, lookup_lens=[0, 5, 6, 1])
    bad(r"lookup_lens\[0\] = -1 outside \[0, 5\]", ids, lens, starts, verify=False, lookup=look,
        lookup_lens=[-1, 5, 5, 1])
    look[1, 4] = V
    bad(rf"lookup id {V} \(row 1, index 4\) outside \[0, {V}\)", ids, lens, starts, verify=False, lookup=look,
        lookup_lens=[0, 5, 5, 1])
    look[1, 4] = -1
    bad(r"lookup id -1 \(row 1, index 4\)", ids, lens, starts, verify=False, lookup=look, lookup_lens=[0, 5, 5, 1])
    c.ragged_generate_spec(ids, lens, 13, starts=starts, lookup=look, lookup_lens=[0, 4, 5, 1])  # past the length: unread
    c.reset_cache()
    # null arguments
    lib = l3hip.lib()
    toks, n = np.zeros((4, 20), np.int64), np.zeros(4, np.int32)
    tail = (4, 11, 20, None, 0, None, None, 0, 4, 3, 1, l3hip.ptr(toks), l3hip.ptr(n), None, None, None)
    for args in ((None, l3hip.ptr(lens), l3hip.ptr(starts)), (l3hip.ptr(ids), None, l3hip.ptr(starts))):
        assert lib.l3_ragged_generate_spec_host(c.handle, *args, *tail) != 0
        assert b"l3_ragged_generate_spec_host: null argument" in lib.l3_last_error()
        assert lib.l3_ragged_verify_host(c.handle, *args, 4, 11, l3hip.ptr(toks), l3hip.ptr(n)) != 0
        assert b"l3_ragged_verify_host: null argument" in lib.l3_last_error()
    assert lib.l3_ragged_verify_host(c.handle, l3hip.ptr(ids), l3hip.ptr(lens), None, 4, 11, l3hip.ptr(toks),
                                     l3hip.ptr(n)) != 0
    assert b"l3_ragged_verify_host: null argument" in lib.l3_last_error()
    assert lib.l3_ragged_verify_host(c.handle, l3hip.ptr(ids), l3hip.ptr(lens), l3hip.ptr(starts), 4, 11, None,
                                     l3hip.ptr(n)) != 0
    assert b"l3_ragged_verify_host: null argument" in lib.l3_last_error()
    assert lib.l3_ragged_generate_spec_host(c.handle, l3hip.ptr(ids), l3hip.ptr(lens), l3hip.ptr(starts), 4, 11, 20,
                                            None, 0, l3hip.ptr(look), None, 5, 4, 3, 1, l3hip.ptr(toks), l3hip.ptr(n),
                                            None, None, None) != 0
    assert b"l3_ragged_generate_spec_host: null argument" in lib.l3_last_error()
    # the draft op
    seq = np.zeros((2, 8), np.int32)
    for args, match in (((seq, [8, 9], [1, 1], 4), r"seq_lens\[1\] = 9 outside \[0, 8\]"),
                        ((seq, [8, 3], [1, 5], 4), r"k\[1\] = 5 outside \[0, 4\]"),
                        ((seq, [8, 3], [1, 1], 16), r"draft_len 16 outside \[0, 15\]"),
                        ((seq, [8, 3], [1, 1], 4, 9), r"ngram_max 9")):
        with pytest.raises(RuntimeError, match=match):
            ctx.op_spec_draft(*args)
    out, n0 = ctx.op_spec_draft(seq, [8, 3], [0, 0], 0)
    assert out.shape == (2, 0) and n0.tolist() == [0, 0]
    # a logits workspace no device holds (2^20 chunk rows x 2^17 logits): refused, nothing allocated
    big = ModelArgs(dim=32, n_layers=1, n_heads=2, n_kv_heads=1, vocab_size=131072, max_seq_len=16384,
                    max_batch_size=64)
    bm = llama3.Llama(synth.make_weights(big, 64, seed=3, preset="sharp"), big, device=0)
    with pytest.raises(RuntimeError, match=r"the speculative workspace \(\d+ bytes: 1048576 chunk rows x 131072 "
                                           r"logits\) could not be allocated"):
        bm.context.ragged_verify(np.zeros((64, 16384), np.int64), np.full(64, 16384, np.int32), np.zeros(64, np.int32))
    chosen, _ = bm.verify_ragged([[1, 2, 3], [4]], [0, 0])
    assert [c.size for c in chosen] == [3, 1]
    del bm
    # a head shape the ragged attention does not take, and a multi-device model
    wide = ModelArgs(dim=256, n_layers=1, n_heads=16, n_kv_heads=1, vocab_size=64, max_seq_len=32, max_batch_size=2)
    wm = llama3.Llama(synth.make_weights(wide, 64, seed=3, preset="sharp"), wide, device=0)
    with pytest.raises(RuntimeError, match="at most 8 query heads per KV head"):
        wm.generate_ragged_spec([[1, 2], [3]], 8)
    with pytest.raises(RuntimeError, match="at most 8 query heads per KV head"):
        wm.verify_ragged([[1, 2], [3]], [0, 0])
    monkeypatch.setenv("L3_GROUP_VIRTUAL", "1")
    grp = llama3.Llama(case.w, case.args, devices=[0, 0])
    member = grp.group.members[0]
    with pytest.raises(RuntimeError, match="member of a multi-device l3_group"):
        member.ragged_generate_spec(ids[:1], lens[:1], 20, starts=starts[:1])
    with pytest.raises(RuntimeError, match="member of a multi-device l3_group"):
        member.ragged_verify(ids[:1], lens[:1], starts[:1])
    with pytest.raises(NotImplementedError):
        grp.generate_ragged(case.second, 20, speculate={})
    with pytest.raises(NotImplementedError):
        grp.verify_ragged(case.second, case.cuts)
    # nothing was launched by the refused calls: a plain generate_ragged gives the right ids
    case.prefill_first()
    max_new = min(case.lens) + 10
    _same_rows(m.generate_ragged(case.second, max_new, start_pos=case.cuts), case.want(max_new))


# ---- 6. check library ---------------------------------------------------------------------------------------

def test_check_build_records_no_violation():
    assert os.path.exists(CHECK_LIB), f"{CHECK_LIB} missing: __graft_entry__.build() makes it"
    env = dict(os.environ, L3_LIB_PATH=CHECK_LIB)
    r = subprocess.run([sys.executable, os.path.join(HERE, "spec_checks_workload.py")], env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["enabled"] is True
    assert out["workload"] == {"kv_slot": 0, "attn_keys": 0, "token_id": 0}
    assert out["tokens"] > 0 and out["accepted"] > 0 and out["drafted"] > out["accepted"]
