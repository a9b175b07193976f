"""On-device temperature / top-k / top-p sampling (sample.hip, l3_set_sampling) against the rule
restated in sampling_ref.py: the op against the rule, exact top-k sets, a stratified distribution,
the edge rows, device RNG = host RNG, determinism, one seed = one sequence on every decode path,
and the picks judged on the oracle's logits.

A pick is judged by sampling_ref's acceptance rule (D = 2e-4, TOL = 1e-3), never by equality with
a NumPy draw: the device's exp and sums round differently.
"""

import numpy as np
import pytest

import l3hip
import llama3
import llama3_oracle as orc
import sampling_ref as ref
import synth

pytestmark = pytest.mark.gpu

# (T, top_k, top_p) of sampling_ref.CONFIGS, plus everything off
PARAMS = sorted({(T, k, p) for _, _, T, k, p in ref.CONFIGS} | {(1.0, 0, 1.0)})
U_LAST = 1.0 - 2.0 ** -24


@pytest.fixture(scope="module")
def ctx():
    return l3hip.op_context(0)


def _uniforms(rng, rows):
    return (rng.integers(0, 1 << 24, rows).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


# a row shorter than a wave, the tiny model's vocabulary, the register-resident path, n not a
# multiple of 4 and past 32768, the long-row path
@pytest.mark.parametrize("rows,n", [(64, 7), (64, 512), (64, 32000), (32, 40001), (16, 128256)])
def test_op_against_the_rule(ctx, rows, n):
    rng = np.random.default_rng(1000 + n)
    z = (rng.standard_normal((rows, n)) * 3).astype(np.float32)
    worst = 0.0
    for T, k, p in PARAMS:
        u = _uniforms(rng, rows)
        got = ctx.op_sample(z, T, k, p, u=u)
        assert got.shape == (rows,) and got.dtype == np.int32
        assert ((got >= 0) & (got < n)).all()
        d = [ref.distance(z[r], T, k, p, float(u[r]), int(got[r])) for r in range(rows)]
        worst = max(worst, max(d))
        bad = [(r, int(got[r]), float(u[r]), d[r]) for r in range(rows) if not d[r] <= ref.TOL]
        assert not bad, f"T={T} top_k={k} top_p={p}: (row, id, u, distance) {bad[:4]}"
    print(f"rows {rows} n {n}: worst CDF distance {worst:.3e}")


def test_top_k_is_exact(ctx):
    n, rows = 32000, 256
    rng = np.random.default_rng(5)
    z = (rng.standard_normal(n) * 3).astype(np.float32)
    zz = np.tile(z, (rows, 1))
    u = ((np.arange(rows) + 0.5) / rows).astype(np.float32)
    for k in (1, 2, 5, 64):
        got = ctx.op_sample(zz, 100.0, k, 1.0, u=u)
        kept, _ = ref.kept_set(z, 100.0, k, 1.0)
        assert kept.size == k
        assert set(got.tolist()) <= set(kept.tolist()), k
        if k <= 5:
            assert set(got.tolist()) == set(kept.tolist()), k
        if k == 1:
            assert (got == ctx.op_argmax(zz)).all()
    # four equal values straddling the boundary: the lower indices are kept
    top = float(z.max())
    for extra, k, want in ((None, 2, {5, 100}), (7777, 3, {7777, 5, 100}), (None, 3, {5, 100, 2000}),
                           (None, 4, {5, 100, 2000, 31000})):
        t = z.copy()
        t[[31000, 100, 2000, 5]] = top + 1
        if extra is not None:
            t[extra] = top + 2
        got = ctx.op_sample(np.tile(t, (rows, 1)), 100.0, k, 1.0, u=u)
        assert set(ref.kept_set(t, 100.0, k, 1.0)[0].tolist()) == want
        assert set(got.tolist()) == want, (k, sorted(set(got.tolist())))


def test_stratified_distribution(ctx):
    n, rows = 512, 4096
    z = (np.random.default_rng(6).standard_normal(n) * 3).astype(np.float32)
    u = ((np.arange(rows) + 0.5) / rows).astype(np.float32)
    got = ctx.op_sample(np.tile(z, (rows, 1)), 1.0, 0, 1.0, u=u)
    w = np.exp(z.astype(np.float64) - float(z.max()))
    mass = w / w.sum()
    count = np.bincount(got, minlength=n)
    err = np.abs(count - rows * mass)
    print(f"stratified: worst count error {err.max():.3f} of bound {rows * ref.TOL + 2:.3f}")
    assert (err <= rows * ref.TOL + 2).all(), (int(err.argmax()), float(err.max()))


def test_edge_rows(ctx):
    rng = np.random.default_rng(8)
    base = (rng.standard_normal((4, 1000)) * 3).astype(np.float32)
    nan_row = base.copy()
    nan_row[:, 700] = np.nan
    nan_row[:, 900] = np.nan
    inf_row = base.copy()
    inf_row[:, 123] = np.inf
    ninf = np.full((4, 1000), -np.inf, np.float32)
    one = base[:, :1].copy()
    u = np.array([0.0, 0.3, 0.7, U_LAST], np.float32)
    for T in (0.5, 1.0, 100.0):
        for x in (nan_row, inf_row, ninf, one):
            for k, p in ((0, 1.0), (5, 0.9)):
                assert (ctx.op_sample(x, T, k, p, u=u) == ctx.op_argmax(x)).all()
    assert (ctx.op_argmax(nan_row) == 700).all() and (ctx.op_argmax(inf_row) == 123).all()
    assert (ctx.op_argmax(ninf) == 0).all()
    # a temperature of 0 is the argmax; so is, on a row without ties, a very small one
    assert (ctx.op_sample(base, 0.0, 0, 1.0, u=u) == ctx.op_argmax(base)).all()
    assert (ctx.op_sample(base, 1e-3, 0, 1.0, u=u) == ctx.op_argmax(base)).all()
    # u = 0 and the largest u return the first and the last index of S
    t = np.array([0.1, 2.0, -1.0, 1.5, 0.3, 1.9, -0.5], np.float32)
    ends = np.array([0.0, U_LAST], np.float32)
    for k, p in ((0, 1.0), (3, 1.0), (0, 0.8), (3, 0.8), (1, 1.0)):
        idx, _ = ref.kept_set(t, 1.0, k, p)
        got = ctx.op_sample(np.tile(t, (2, 1)), 1.0, k, p, u=ends)
        assert got.tolist() == [int(idx[0]), int(idx[-1])], (k, p, got, idx)
    assert ref.kept_set(t, 1.0, 3, 1.0)[0].tolist() == [1, 3, 5]


def test_device_rng_is_host_rng(ctx):
    rng = np.random.default_rng(9)
    seed = (1 << 40) + 77
    for rows, n in ((64, 512), (16, 40001)):
        z = (rng.standard_normal((rows, n)) * 3).astype(np.float32)
        for row0 in (0, 5):
            for pos in (0, 17):
                u = np.array([l3hip.sample_uniform(seed, row0 + r, pos) for r in range(rows)], np.float32)
                a = ctx.op_sample(z, 0.8, 0, 0.9, u=None, seed=seed, row0=row0, pos=pos)
                b = ctx.op_sample(z, 0.8, 0, 0.9, u=u)
                assert (a == b).all(), (rows, n, row0, pos)
    # other counters give other draws
    a = ctx.op_sample(z, 0.8, 0, 0.9, seed=seed, row0=0, pos=0)
    assert (a != ctx.op_sample(z, 0.8, 0, 0.9, seed=seed, row0=0, pos=1)).any()
    assert (a != ctx.op_sample(z, 0.8, 0, 0.9, seed=seed + 1, row0=0, pos=0)).any()


def test_run_to_run_determinism(ctx):
    rng = np.random.default_rng(10)
    z = (rng.standard_normal((64, 32000)) * 3).astype(np.float32)
    u = _uniforms(rng, 64)
    for T, k, p in ((0.8, 0, 0.9), (0.7, 40, 0.95)):
        a = ctx.op_sample(z, T, k, p, u=u)
        assert (a == ctx.op_sample(z, T, k, p, u=u)).all()


# ---- the decode paths -------------------------------------------------------------------

L, NEW = 5, 24


@pytest.fixture(scope="module")
def tiny():
    args = synth.tiny(3)
    return args, synth.make_weights(args, synth.TINY_HIDDEN, seed=21, preset="default")


def _prompt(args, B, seed=3):
    return np.random.default_rng(seed).integers(0, args.vocab_size, (B, L))


def _eager_loop(model, prompt, total):
    """generate's schedule through greedy_step with want_logits (never a graph replay):
    ids [B, steps] and each step's logits rows."""
    ids, rows, nxt = [], [], None
    for i, pos in enumerate(range(prompt.shape[1], total)):
        nxt, lg = model.context.greedy_step(prompt if i == 0 else nxt.reshape(-1, 1), 0 if i == 0 else pos,
                                            want_logits=True)
        ids.append(nxt.copy())
        rows.append(np.array(lg))
    return np.stack(ids, axis=1), rows


@pytest.mark.parametrize("B", [1, 3])
def test_one_seed_one_sequence_on_every_path(tiny, B):
    args, w = tiny
    prompt = _prompt(args, B)
    total = L + NEW
    fresh = llama3.Llama(w, args, device=0)
    greedy = np.concatenate(list(fresh.generate(prompt, total)), axis=1)
    m = llama3.Llama(w, args, device=0)
    m.set_sampling(temperature=0.9, top_p=0.95, seed=1234)
    assert m.context.get_sampling() == {"temperature": np.float32(0.9), "top_k": 0, "top_p": np.float32(0.95),
                                        "seed": 1234}
    lazy = np.concatenate(list(m.generate(prompt, total)), axis=1)
    assert lazy.shape == (B, NEW)
    assert m.context.decode_stats()["graph_steps"] > 0  # the steps were graph replays
    assert not m.context.decode_persistent()
    assert not np.array_equal(lazy, greedy)
    assert np.array_equal(m.generate_all(prompt, total), lazy)
    assert not m.context.decode_persistent()
    eager, _ = _eager_loop(m, prompt, total)
    assert np.array_equal(eager, lazy)
    gen = m.generate(prompt, total)
    head = np.concatenate([next(gen) for _ in range(6)], axis=1)  # abandoned with steps run ahead
    del gen
    assert np.array_equal(head, lazy[:, :6])
    assert np.array_equal(np.concatenate(list(m.generate(prompt, total)), axis=1), lazy)
    m.set_sampling(temperature=0.9, top_p=0.95, seed=1235)
    assert not np.array_equal(np.concatenate(list(m.generate(prompt, total)), axis=1), lazy)
    m.set_sampling(0.0)
    assert np.array_equal(np.concatenate(list(m.generate(prompt, total)), axis=1), greedy)
    assert np.array_equal(m.generate_all(prompt, total), greedy)
    assert m.context.decode_persistent() == fresh.context.decode_persistent()


def _teacher_forced(args, w, prompt, new, T, k, p, seed):
    """The device's sampled ids fed to the oracle on the reference's schedule: every pick judged
    on the oracle's float64 logits with the step's own uniform."""
    B, L0 = prompt.shape
    m = llama3.Llama(w, args, device=0)
    m.set_sampling(T, k, p, seed)
    ids = m.generate_all(prompt, L0 + new)
    oracle = orc.OracleModel({name: np.asarray(v, np.float64) for name, v in w.items()}, args)
    tol = ref.TOL + 4e-4 / T
    worst = 0.0
    for i in range(new):
        logits = oracle(prompt if i == 0 else ids[:, i - 1:i], 0 if i == 0 else L0 + i)[:, -1, :]
        pos = L0 - 1 if i == 0 else L0 + i
        for b in range(B):
            u = l3hip.sample_uniform(seed, b, pos)
            d = ref.distance(logits[b], T, k, p, u, int(ids[b, i]))
            worst = max(worst, d)
            assert d <= tol, (i, b, int(ids[b, i]), u, d)
    return worst


def test_against_the_oracle_teacher_forced_tiny(tiny):
    args, w = tiny
    worst = _teacher_forced(args, w, _prompt(args, 3), NEW, 0.9, 0, 0.95, 99)
    print(f"tiny, teacher-forced: worst CDF distance {worst:.3e}")


def test_against_the_oracle_teacher_forced_stories15m_sharp():
    args = synth.stories15m(1)
    w = synth.make_weights(args, synth.STORIES15M_HIDDEN, seed=4, preset="sharp")
    prompt = np.random.default_rng(4).integers(0, args.vocab_size, (1, L))
    worst = _teacher_forced(args, w, prompt, 16, 0.9, 0, 0.95, 7)
    print(f"stories15M sharp, teacher-forced: worst CDF distance {worst:.3e}")


def test_generate_all_values_are_the_picked_logits(tiny):
    args, w = tiny
    prompt = _prompt(args, 3, seed=12)
    m = llama3.Llama(w, args, device=0)
    m.set_sampling(temperature=0.9, top_p=0.95, seed=31)
    ids, vals = m.context.greedy_generate(prompt, L + NEW, values=True)
    eager, rows = _eager_loop(m, prompt, L + NEW)
    assert np.array_equal(eager, ids)
    want = np.stack([r[np.arange(3), ids[:, i]] for i, r in enumerate(rows)], axis=1)
    assert np.abs(vals - want).max() <= 1e-5
    assert not np.array_equal(ids, np.stack([r.argmax(-1) for r in rows], axis=1))  # sampled, not the argmax


def test_set_sampling_is_refused_where_it_cannot_hold(tiny):
    args, w = tiny
    m = llama3.Llama(w, args, device=0)
    with pytest.raises(RuntimeError, match="top_p"):
        m.set_sampling(0.8, 0, 0.0)
    with pytest.raises(RuntimeError, match="temperature"):
        m.set_sampling(-1.0)
    assert m.context.get_sampling()["temperature"] == 0.0
