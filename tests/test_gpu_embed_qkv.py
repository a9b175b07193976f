"""Layer 0's QKV of a prefill as a table lookup (l3_set_embed_qkv; embed_qkv.h) against the GEMM
it replaces.

The table holds, per token id, what the tiled fp32 QKV kernel's accumulators and row factor give
for an embedding row just before the rotation, and the gather kernel rotates with the epilogues'
arithmetic, so logits, q and every K / V slot must be bit-identical to the GEMM path's on every
entry point: each test runs the same calls on fresh models with the path on and off and compares
with ``np.array_equal``.  The caches are compared through what reads them: a later chunk, a decode
step over every written slot, and scoring of every position.

The plan for these tests also named an "H 4 at D 96 (head size 24)" model, to put the generic
(guarded) QKV epilogue on the GEMM side.  It cannot be built: ``l3_create`` refuses head sizes that
are not multiples of 16.  ``gen60`` below reaches that epilogue with sequences shorter than 64 rows
(the division-free one needs L >= 64), every T = 300 case ends in a partial row tile, which takes
it too, and ``hd32`` adds a head size and the 128 x 128 tile in its place.
"""

import os
import tempfile

import numpy as np
import pytest

import llama3
import llama3_oracle as orc
import synth
from config import ModelArgs

pytestmark = pytest.mark.gpu

ATOL, RTOL = 1e-4, 2e-4  # the project's bar against the oracle (test_gpu_parity._close)
HIDDEN = 256
VS = 600  # 4 full 128-row table tiles and a partial one


def _close(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want)
    assert not (err > ATOL + RTOL * np.abs(want)).any(), f"max-abs {err.max():.3e}"


@pytest.fixture(scope="module")
def tmp():
    with tempfile.TemporaryDirectory() as d:
        yield d


def _args(dim=96, heads=2, kv=1, batch=3):
    return ModelArgs(dim=dim, n_layers=2, n_heads=heads, n_kv_heads=kv, vocab_size=VS, max_seq_len=192,
                     max_batch_size=batch)


def _weights(tmp, args, seed=3):
    w = synth.make_weights(args, HIDDEN, seed=seed, preset="default")
    path = os.path.join(tmp, f"eq_{args.dim}_{args.n_heads}_{args.n_kv_heads}_{args.max_batch_size}_{seed}.npz")
    if not os.path.exists(path):
        synth.save_npz(path, w)
    return w, path


def _model(path, args, on, **kw):
    m = llama3.Llama(path, args)
    m.context.set_embed_qkv(on, **kw)
    return m


def _ids(rng, B, L):
    """Random ids with the vocabulary's ends and repeats (inside a row and across rows)."""
    ids = rng.integers(0, VS, (B, L))
    ids[0, 0], ids[0, 1], ids[-1, -1] = 0, VS - 1, VS - 1
    ids[:, L // 2] = ids[0, 0]
    ids[1 % B, 3:6] = ids[0, 3]
    return ids


def _count(m):
    return m.context.kernel_stats()["embed_qkv"][1]


def _sequence(m, calls):
    """Each (ids, start_pos) call's logits, then the scores of every position of the first call."""
    outs = [np.array(m(ids, pos)) for ids, pos in calls]
    lp, am = m.score(calls[0][0], np.roll(calls[0][0], -1, axis=1), 0, return_argmax=True)
    return outs + [np.array(lp), np.array(am)]


def _on_off(path, args, calls):
    res = []
    for on in (True, False):
        m = _model(path, args, on)
        m.context.kernel_timing(True, ["embed_qkv"])
        res.append(_sequence(m, calls))
        # the prefills and the scoring run the lookup when on; nothing does when off
        assert (_count(m) > 0) == on
    for k, (a, b) in enumerate(zip(*res)):
        assert np.array_equal(a, b), f"output {k}: table path differs from the GEMM path"
    return res[0]


def test_chunks_decode_score_gqa(tmp):
    """B 3 x L 100 at 0 (T = 300: two full row tiles on the division-free epilogue, a partial one,
    sequence wraps inside a wave), B 3 x L 90 at 100 (offset positions), a decode step at 190 over
    every slot both paths wrote, and score() over the first call: on == off bitwise; the table
    path's logits against the oracle."""
    args = _args()
    w, path = _weights(tmp, args)
    rng = np.random.default_rng(11)
    calls = [(_ids(rng, 3, 100), 0), (_ids(rng, 3, 90), 100), (rng.integers(0, VS, (3, 1)), 190)]
    got = _on_off(path, args, calls)
    ref = orc.OracleModel(w, args)
    for (ids, pos), g in zip(calls, got):
        _close(g, ref(ids, pos))


@pytest.mark.parametrize("name,dim,heads,kv,B,L,L2", [
    ("hd16", 64, 4, 2, 3, 100, 90),   # head size 16, two KV heads; N = 128: the 128 x 128 table tile
    ("hd32", 128, 4, 2, 3, 100, 90),  # head size 32, two KV heads; N = 256: the 128 x 128 table tile
    ("gen60", 96, 2, 1, 5, 60, 60),   # L < 64: the generic QKV epilogue on every tile of the GEMM side
])
def test_head_sizes_and_generic_epilogue(tmp, name, dim, heads, kv, B, L, L2):
    """Two chunks and a decode step as above, at other head sizes and on the other QKV tile (the
    first test's N = 192 takes the 128 x 96 one)."""
    args = _args(dim, heads, kv, batch=B)
    _, path = _weights(tmp, args, seed=5)
    rng = np.random.default_rng(dim + L)
    calls = [(_ids(rng, B, L), 0), (_ids(rng, B, L2), L), (rng.integers(0, VS, (B, 1)), L + L2)]
    _on_off(path, args, calls)


def test_batch_split(tmp):
    """B 4 x L 160 as two parts of 320 rows on two streams and as one: split and unsplit, table on
    and off, all four equal (the table is built before the parts fork)."""
    args = _args(batch=4)
    _, path = _weights(tmp, args)
    ids = _ids(np.random.default_rng(7), 4, 160)
    nxt = np.random.default_rng(8).integers(0, VS, (4, 1))
    outs = []
    for on in (True, False):
        for parts in (2, 1):
            m = _model(path, args, on)
            m.context.set_batch_split(parts, 257)
            m.context.kernel_timing(True, ["embed_qkv"])
            outs.append((np.array(m(ids, 0)), np.array(m(nxt, 160))))
            assert _count(m) == (parts if on else 0)
    for o in outs[1:]:
        assert np.array_equal(o[0], outs[0][0]) and np.array_equal(o[1], outs[0][1])


def test_cap_and_x6_keep_the_gemm(tmp):
    """A cap below the table's bytes, and the x6 path, leave the GEMM on (no embed_qkv launch,
    results equal the reference side's); with x6 off again the lookup runs and is bitwise equal."""
    args = _args()
    _, path = _weights(tmp, args)
    ids = _ids(np.random.default_rng(21), 3, 100)
    ref = _model(path, args, False)
    want = np.array(ref(ids, 0))
    ref.context.set_gemm_x6(True)
    want_x6 = np.array(ref(ids, 0))

    table_bytes = VS * (args.n_heads + 2 * args.n_kv_heads) * (args.dim // args.n_heads) * 4
    m = _model(path, args, True, max_bytes=table_bytes - 1)
    m.context.kernel_timing(True, ["embed_qkv"])
    assert np.array_equal(np.array(m(ids, 0)), want) and _count(m) == 0
    m.context.set_embed_qkv(True, max_bytes=table_bytes)  # exactly fits
    assert np.array_equal(np.array(m(ids, 0)), want) and _count(m) == 1

    m = _model(path, args, True)
    m.context.set_gemm_x6(True)
    m.context.kernel_timing(True, ["embed_qkv"])
    assert np.array_equal(np.array(m(ids, 0)), want_x6) and _count(m) == 0
    m.context.set_gemm_x6(False)
    assert np.array_equal(np.array(m(ids, 0)), want) and _count(m) == 1


def test_ragged_forward(tmp):
    """forward_ragged, B 3, Lmax 100, lens (100, 37, 1): on == off bitwise."""
    args = _args()
    _, path = _weights(tmp, args)
    rng = np.random.default_rng(31)
    prompts = [_ids(rng, 1, 100)[0], rng.integers(0, VS, 37), np.array([VS - 1])]
    outs = []
    for on in (True, False):
        m = _model(path, args, on)
        m.context.kernel_timing(True, ["embed_qkv"])
        outs.append(np.array(m.forward_ragged(prompts)))
        assert _count(m) == (1 if on else 0)
    assert np.array_equal(outs[0], outs[1])
