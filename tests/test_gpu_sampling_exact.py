"""The sample kernel's selects, tie cuts and index searches (sample.hip) pinned by equality.

test_gpu_sampling.py judges a pick by where u falls, within TOL = 1e-3: right for the exponential,
blind to a pick one index or one bucket off.  Here the rows are built so that every weight is an
exactly known integer (sampling_exact_ref), and the device must return the one index the integer
model and the float64 rule both name (test_sampling_exact_cpu.py shows they agree on every case of
these tables).  No tolerance is used anywhere in this module.
"""

import numpy as np
import pytest

import l3hip
import sampling_exact_ref as ex
import sampling_ref as ref

pytestmark = pytest.mark.gpu

# (T, top_k, top_p) of sampling_ref.CONFIGS, plus everything off
PARAMS = sorted({(T, k, p) for _, _, T, k, p in ref.CONFIGS} | {(1.0, 0, 1.0)})


@pytest.fixture(scope="module")
def ctx():
    return l3hip.op_context(0)


def _run(ctx, c):
    return ctx.op_sample(np.tile(c.z, (len(c.u), 1)), c.T, c.top_k, c.top_p, u=c.u).tolist()


@pytest.mark.parametrize("n", ex.REG_SIZES + ex.LONG_SIZES)
def test_plateau_picks_are_exact(ctx, n):
    """M elements at the maximum, everything else weightless: the pick is the model's index."""
    bad, cases = [], 0
    for c in ex.plateau_calls(n):
        got = _run(ctx, c)
        cases += len(got)
        bad += [(c.label, float(u), g, w) for u, g, w in zip(c.u, got, c.want) if g != w]
    print(f"n {n}: {cases} plateau cases")
    assert not bad, f"{len(bad)} of {cases} (label, u, got, want): {bad[:6]}"


@pytest.mark.parametrize("n", [32000, 65537])
def test_two_plateau_picks_are_exact(ctx, n):
    """The nucleus cut inside a second plateau of about half the weight: a threshold key below the
    maximum, a remainder carried through the three select levels, itau by weighted search."""
    bad, cases = [], 0
    for c, _ in ex.two_plateau_calls(n):
        if not len(c.u):
            continue
        got = _run(ctx, c)
        cases += len(got)
        bad += [(c.label, float(u), g, w) for u, g, w in zip(c.u, got, c.want) if g != w]
    print(f"n {n}: {cases} two-plateau cases")
    assert cases and not bad, f"{len(bad)} of {cases} (label, u, got, want): {bad[:6]}"


@pytest.mark.parametrize("n", [32000, 40001])
def test_top_k_sets_are_exact_on_adversarial_keys(ctx, n):
    """test_gpu_sampling.test_top_k_is_exact's way of reading the kept set, on rows of bit patterns.
    k <= 8 and T = 100: every kept member has at least a tenth of the mass, so 256 stratified
    uniforms reach each one and the set of picks is the kept set."""
    rows = 256
    u = ((np.arange(rows) + 0.5) / rows).astype(np.float32)
    for name, z, ks in ex.topk_rows(n):
        zz = np.tile(z, (rows, 1))
        for k in ks:
            assert k <= 8
            want = set(ref.kept_set(z, 100.0, k, 1.0)[0].tolist())
            assert len(want) == k
            got = set(ctx.op_sample(zz, 100.0, k, 1.0, u=u).tolist())
            assert got == want, (name, k, sorted(got), sorted(want))


def test_the_two_forms_agree_bit_for_bit(ctx):
    """Both forms add exact integers of the same per-element weights, and -inf weighs nothing, ranks
    last and is never drawn: a row and the same row padded into the long-row form give one id."""
    rng = np.random.default_rng(77)
    rows, n = 32, 32000
    z = (rng.standard_normal((rows, n)) * 3).astype(np.float32)
    padded = []
    for m in (40001, 131073):
        zp = np.full((rows, m), -np.inf, np.float32)
        zp[:, :n] = z
        padded.append(zp)
    for T, k, p in PARAMS:
        u = (rng.integers(0, 1 << 24, rows).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)
        base = ctx.op_sample(z, T, k, p, u=u)
        assert ((base >= 0) & (base < n)).all()
        for zp in padded:
            got = ctx.op_sample(zp, T, k, p, u=u)
            assert (got == base).all(), (T, k, p, zp.shape[1], np.flatnonzero(got != base).tolist(),
                                         got[got != base].tolist(), base[got != base].tolist())


def test_edge_rows_in_the_long_row_form(ctx):
    """NaN, +inf and all -inf rows return the argmax rule's answer with the special value at a wave's
    first index, a wave's last index and n - 1."""
    n = 40001
    _, ch, waves = ex.geometry(n)
    assert (ch, waves) == (2560, 16)
    rng = np.random.default_rng(78)
    base = (rng.standard_normal((4, n)) * 3).astype(np.float32)
    u = np.array([0.0, 0.3, 0.7, ex.U_LAST], np.float32)
    ninf = np.full((4, n), -np.inf, np.float32)
    assert (ctx.op_argmax(ninf) == 0).all()
    for at in (5 * ch, 9 * ch - 1, 15 * ch, n - 1):
        nan_row, inf_row = base.copy(), base.copy()
        nan_row[:, at] = np.nan
        nan_row[:, n - 1] = np.nan  # a later NaN loses to the first
        inf_row[:, at] = np.inf
        assert (ctx.op_argmax(nan_row) == at).all() and (ctx.op_argmax(inf_row) == at).all()
        for T, (k, p) in zip((0.5, 1.0, 100.0), ((0, 1.0), (5, 0.9), (0, 0.9))):
            for x, want in ((nan_row, at), (inf_row, at), (ninf, 0)):
                assert ctx.op_sample(x, T, k, p, u=u).tolist() == [want] * 4, (at, T, k, p)


@pytest.mark.parametrize("n", [32000, 40001])
def test_temperature_zero_on_a_plateau_is_its_first_member(ctx, n):
    u = np.array([0.0, 0.3, 0.7, ex.U_LAST], np.float32)
    for kind, members in ex.plateau_positions(n):
        for value in (3.5, "zeros"):
            z = ex.plateau_row(n, members, value)
            for k, p in ((0, 1.0), (3, 0.5)):
                got = ctx.op_sample(np.tile(z, (4, 1)), 0.0, k, p, u=u)
                assert got.tolist() == [members[0]] * 4, (kind, value, k, p, got)
