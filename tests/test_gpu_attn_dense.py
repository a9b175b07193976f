"""The dense attention kernels at kernel level (DESIGN.md "Dense attention at kernel level";
csrc/attn_kernel.h behind csrc/attention.hip, l3_op_attention_host): every instantiation the
dispatcher reaches — 42 attn_fwd_kernel (HD, QBW, G, KT) and 12 attn_decode_kernel (HD, FUSE_O) —
launched on its own on plain arrays, with the route it reports compared against the tables of
tests/attn_dense_ref.py, against the fp64 reference there, at every q-block, tile and cache edge.
tests/test_attn_dense_cpu.py shows the tables cover the full set."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import attn_dense_ref as ref
import l3hip

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHECK_LIB = os.path.join(os.path.dirname(HERE), "llama3.np_amd", "csrc", "libllama3hip_check.so")

# the project's kernel-against-reference bar for attention over N(0, 1) inputs
# (tests/test_gpu_ragged_extend.py, tests/test_gpu_ragged_split.py)
BOUND = 1e-5


@pytest.fixture(scope="module")
def ctx():
    return l3hip.op_context(0)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _launch(ctx, case, inp, **kw):
    """(out [B, L, width] without the guard row, route): the guard row checked here"""
    buf, route = ctx.op_attention(inp["q_s"], inp["cache_k"], inp["cache_v"], case.start_pos, inp["n_heads"],
                                  scaled=True, **kw)
    rows = case.B * case.L
    assert buf.shape[0] == rows + 1
    assert np.array_equal(_bits(buf[rows:]), _bits(l3hip.gemm_sentinel((1, buf.shape[1]), 7))), "guard row written"
    return buf[:rows].reshape(case.B, case.L, -1), route


def _against_fp64(ctx, case, inp=None):
    inp = ref.make_inputs(case) if inp is None else inp
    out, route = _launch(ctx, case, inp)
    assert route == case.route, (case, route)
    assert np.isfinite(out).all(), f"{case}: a poisoned slot was read"
    want = ref.reference(inp["q_s"], inp["cache_k"], inp["cache_v"], case.start_pos, inp["n_heads"])
    return float(np.abs(out.astype(np.float64) - want).max())


# ---- a. against fp64 on every route -------------------------------------------------------------

@pytest.mark.parametrize("hd,n_rep", ref.PARAMS)
def test_prefill_table_matches_fp64_on_its_route(ctx, hd, n_rep):
    """Every case of the prefill table: finite (no NaN slot read), the route the table expects, the
    guard row intact, max-abs against fp64 <= 1e-5.  Measured on an MI355X (worst case of the table,
    G = 1 / 2 / 4, the worse n_rep of each):
      HD 16   8.15e-07 / 8.59e-07 / 8.62e-07      HD 32   8.79e-07 / 8.66e-07 / 9.70e-07
      HD 48   1.07e-06 / 1.01e-06 / 1.13e-06      HD 64   1.06e-06 / 1.14e-06 / 1.35e-06
      HD 96   1.33e-06 / 1.53e-06 / 1.92e-06      HD 128  1.89e-06 / 1.89e-06 / 1.78e-06"""
    worst = 0.0
    for case in ref.prefill_cases(hd, n_rep):
        err = _against_fp64(ctx, case)
        assert err <= BOUND, (case, err)
        worst = max(worst, err)
    print(f"prefill HD {hd} n_rep {n_rep} G {ref.G_OF[n_rep]}: max-abs {worst:.3e}")


# ---- b. key census ------------------------------------------------------------------------------

def _census(ctx, case):
    inp = ref.census_inputs(case)
    out, route = _launch(ctx, case, inp)
    assert route == case.route, (case, route)
    H = inp["n_heads"]
    keys = (case.start_pos + np.arange(case.L) + 1).astype(np.float64)
    got = out.astype(np.float64).reshape(case.B, case.L, H, case.hd) * keys[None, :, None, None]
    want = ref.census(case)[None, :, None, :]
    bad = np.argwhere(~(np.rint(got) == want) | ~(np.abs(got - want) <= 1e-3))
    if bad.size:
        b, t, h, d = (int(x) for x in bad[0])
        raise AssertionError(f"{case}: sequence {b} query {t} (position {case.start_pos + t}) head {h}: "
                             f"{got[b, t, h, d]!r} keys of residue class {d} mod {case.hd}, "
                             f"{int(want[0, t, 0, d])} expected ({bad.shape[0]} elements differ)")


@pytest.mark.parametrize("hd,n_rep", ref.PARAMS)
def test_prefill_table_counts_every_key_once(ctx, hd, n_rep):
    """q = 0 and V one-hot by j % HD: out * keys is the exact number of keys of each residue class a
    query saw — a leaked or dropped key at any tile, group or block edge changes an integer"""
    for case in ref.prefill_cases(hd, n_rep):
        _census(ctx, case)


@pytest.mark.parametrize("hd,n_rep", ref.LONG_SHAPES)
def test_long_cache_single_row_launches(ctx, hd, n_rep):
    """L = 1 past 8192 slots (the prefill kernel) and at 8192 (the decode kernel), first and last
    position: the census, and fp64 at 1e-5.  Measured on an MI355X (prefill kernel at position
    8192 / decode kernel at 8191; one key at position 0 is exact on both): HD 16 4.22e-08 / 6.98e-09,
    HD 128 2.28e-07 / 4.08e-08."""
    for case in ref.long_cases(hd, n_rep):
        _census(ctx, case)
        err = _against_fp64(ctx, case)
        print(f"long HD {hd} Smax {case.smax} pos {case.start_pos} {case.route['kernel']}: max-abs {err:.3e}")
        assert err <= BOUND, (case, err)


# ---- c. softmax state under stress --------------------------------------------------------------

@pytest.mark.parametrize("hd,n_rep", ref.PARAMS)
def test_softmax_state_under_stress(ctx, hd, n_rep):
    """Exact scores (q~ = e_0; K[..., 0] a rising ramp, a falling ramp, a spike in an unmasked and in
    the diagonal tile), N(0, 1) values: only exp2 and the accumulation contribute, so 1e-5 holds.
    On the longest prefill length at start 0 and 17, and on the decode kernel at S = 257 and Smax.
    Measured on an MI355X (worst of the 36 parameters): rising 4.03e-07, falling 7.15e-07, spike in
    tile 0 2.38e-07, spike in the diagonal tile 2.38e-07."""
    longest = max(c.L for c in ref.prefill_cases(hd, n_rep))
    cases = [c for c in ref.prefill_cases(hd, n_rep) if c.L == longest and c.start_pos in (0, 17)]
    cases += [c for c in ref.decode_cases(hd, n_rep) if c.start_pos + 1 in (257, ref.SMAX_DECODE)]
    assert len(cases) == 4
    worst = dict.fromkeys(ref.STRESS, 0.0)
    for case in cases:
        for shape in ref.STRESS:
            err = _against_fp64(ctx, case, ref.stress_inputs(case, shape))
            assert err <= BOUND, (case, shape, err)
            worst[shape] = max(worst[shape], err)
    print(f"stress HD {hd} n_rep {n_rep}: " + "  ".join(f"{k} {v:.3e}" for k, v in worst.items()))


# ---- d. decode and fused O ----------------------------------------------------------------------

@pytest.mark.parametrize("hd,n_rep", ref.PARAMS)
def test_decode_table_matches_fp64_and_the_device_position(ctx, hd, n_rep):
    """The decode table against fp64 at 1e-5 on its route, and once more with the position read from
    a device word (the start_pos argument then holds another value): bit for bit the same.
    Measured on an MI355X (worst case of the table, G = 1 / 2 / 4, the worse n_rep of each):
      HD 16   3.43e-07 / 2.50e-07 / 2.66e-07      HD 32   2.29e-07 / 2.54e-07 / 3.15e-07
      HD 48   4.65e-07 / 2.92e-07 / 2.62e-07      HD 64   2.09e-07 / 5.13e-07 / 3.42e-07
      HD 96   3.35e-07 / 3.35e-07 / 4.52e-07      HD 128  5.90e-07 / 4.88e-07 / 4.99e-07"""
    worst = 0.0
    for case in ref.decode_cases(hd, n_rep):
        inp = ref.make_inputs(case)
        err = _against_fp64(ctx, case, inp)
        assert err <= BOUND, (case, err)
        worst = max(worst, err)
        out, _ = _launch(ctx, case, inp)
        dev, route = _launch(ctx, case, inp, pos_dev=True)
        assert route == case.route and np.array_equal(_bits(dev), _bits(out)), case
    print(f"decode HD {hd} n_rep {n_rep}: max-abs {worst:.3e}")


def test_prefill_kernel_reads_the_device_position(ctx):
    """start_of on the prefill kernel: a device position gives the argument form's bits"""
    for case in (ref.prefill_cases(16, 2)[-2], ref.prefill_cases(128, 3)[8], ref.long_cases(16, 1)[1]):
        assert case.route["kernel"] == "prefill" and case.start_pos > 0
        inp = ref.make_inputs(case)
        out, _ = _launch(ctx, case, inp)
        dev, route = _launch(ctx, case, inp, pos_dev=True)
        assert route == case.route and np.array_equal(_bits(dev), _bits(out)), case


@pytest.mark.parametrize("hd,n_rep", ref.PARAMS)
def test_fused_o_proj_matches_fp64(ctx, hd, n_rep):
    """parts[b, h] = Wo[:, h*HD:(h+1)*HD] @ out[b, h] of the fused decode launch, D in {4, 64, 68,
    192} (independent of H * HD here), B in {1, 2}.  Bound: 1e-5 * max(1, max |reference parts| of
    the case) — the bar of the plain launch as a per-element relative floor, the elements being
    sums of HD products of O(1) terms.  The plain decode launch's out times Wo in fp64 agrees with
    parts to the same bound.  Measured on an MI355X: worst max-abs 4.51e-06 (HD 128); worst
    error / bound per head size 16: 0.033, 32: 0.032, 48: 0.032, 64: 0.045, 96: 0.046, 128: 0.067 —
    the bound holds with a 15x margin (4x is the least this test accepts as meaningful)."""
    worst = worst_rel = 0.0
    for case in ref.fused_cases(hd, n_rep):
        inp = ref.make_inputs(case)
        H, D = inp["n_heads"], case.D
        parts, route = _launch(ctx, case, inp, wo=inp["wo"])          # [B, 1, H * D]; the guard row: [D, ...) untouched
        assert route == case.route, (case, route)
        parts = parts.reshape(case.B, H, D)
        assert np.isfinite(parts).all(), case
        want_out = ref.reference(inp["q_s"], inp["cache_k"], inp["cache_v"], case.start_pos, H)[:, 0]
        want = ref.reference_parts(want_out, inp["wo"], H)
        bound = BOUND * max(1.0, float(np.abs(want).max()))
        err = float(np.abs(parts.astype(np.float64) - want).max())
        assert err <= bound, (case, err, bound)
        plain_case = case._replace(route=dict(case.route, kernel="decode", grid=(H, case.B, 1)), D=0)
        plain, route = _launch(ctx, plain_case, inp)
        assert route == plain_case.route
        err2 = float(np.abs(parts.astype(np.float64) - ref.reference_parts(plain[:, 0], inp["wo"], H)).max())
        assert err2 <= bound, (case, err2, bound)
        worst, worst_rel = max(worst, err, err2), max(worst_rel, err / bound, err2 / bound)
    print(f"fused HD {hd} n_rep {n_rep}: max-abs {worst:.3e}, worst error / bound {worst_rel:.3f}")


# ---- e. last-rows launch ------------------------------------------------------------------------

@pytest.mark.parametrize("hd,n_rep", ref.PARAMS)
def test_last_rows_launch_is_the_full_launch_on_its_window(ctx, hd, n_rep):
    """launch_attention_last writes exactly rows [max(0, L - QW), L) of each sequence, bit for bit
    the full launch's (the claim in attention.hip), from one workgroup along x; every other row
    keeps its sentinel"""
    qw = 16 * (4 // ref.G_OF[n_rep])
    for case in ref.last_cases(hd, n_rep):
        inp = ref.make_inputs(case)
        full, _ = _launch(ctx, case, inp)
        last, route = _launch(ctx, case, inp, last=True)
        assert route == case.route and route["grid"][0] == 1, (case, route)
        lo = max(0, case.L - qw)
        assert np.isfinite(full).all() and np.array_equal(_bits(last[:, lo:]), _bits(full[:, lo:])), case
        sentinel = l3hip.gemm_sentinel((case.B * case.L, full.shape[2]), 6).reshape(full.shape)
        assert np.array_equal(_bits(last[:, :lo]), _bits(sentinel[:, :lo])), case


# ---- f. refusals --------------------------------------------------------------------------------

def test_what_the_dispatcher_refuses_is_an_error_by_name(ctx):
    rng = np.random.default_rng(0)

    def refuse(match, hd=16, H=2, kvh=2, B=1, L=1, start=0, smax=32, D=0, **kw):
        q = rng.standard_normal((B, L, H * hd)).astype(np.float32)
        ck = rng.standard_normal((B, kvh, smax, hd)).astype(np.float32)
        wo = rng.standard_normal((D, H * hd)).astype(np.float32) if D else None
        out = l3hip.gemm_sentinel((B * L + 1, H * D if D else H * hd), 3).copy()
        was = out.copy()
        with pytest.raises(RuntimeError, match=match):
            ctx.op_attention(q, ck, ck, start, H, wo=wo, out=out, **kw)
        assert np.array_equal(_bits(out), _bits(was))

    refuse(r"head size 80 has no attention instantiation", hd=80)
    refuse(r"head size 80 has no attention instantiation", hd=80, L=5)
    refuse(r"head size 80 has no attention instantiation", hd=80, L=5, last=True)
    refuse(r"n_heads % n_kv_heads != 0 \(H 3, KVH 2\)", H=3)
    refuse(r"n_heads % n_kv_heads != 0 \(H 3, KVH 2\)", H=3, L=4, last=True)
    refuse(r"fused O-proj is a decode launch: L == 1 and Smax <= 8192 \(L 2, Smax 32\)", L=2, D=8)
    refuse(r"fused O-proj is a decode launch: L == 1 and Smax <= 8192 \(L 1, Smax 8193\)", smax=8193, D=8)
    refuse(r"D 6 must be a multiple of 4", D=6)
    refuse(r"last-rows launch takes neither wo nor a device position", D=8, last=True)
    refuse(r"last-rows launch takes neither wo nor a device position", L=4, last=True, pos_dev=True)
    refuse(r"keys \[0, 33\) exceed Smax 32 \(start_pos 30 \+ L 3\)", L=3, start=30)
    refuse(r"keys \[0, 33\) exceed Smax 32 \(start_pos 32 \+ L 1\)", start=32)
    # and the same shapes one step inside are taken
    out, route = ctx.op_attention(rng.standard_normal((1, 3, 32)).astype(np.float32),
                                  np.ones((1, 2, 32, 16), np.float32), np.ones((1, 2, 32, 16), np.float32), 29, 2)
    assert route["kernel"] == "prefill" and np.allclose(out[:3], 1.0, atol=1e-6)


# ---- g. device checks ---------------------------------------------------------------------------

def test_check_build_records_no_violation():
    if not os.path.exists(CHECK_LIB):
        pytest.skip(f"{CHECK_LIB} missing: build it with `make -C llama3.np_amd/csrc check-lib` "
                    "(__graft_entry__.build() does)")
    env = dict(os.environ, L3_LIB_PATH=CHECK_LIB)
    r = subprocess.run([sys.executable, os.path.join(HERE, "attn_dense_checks_workload.py")], env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["enabled"] is True
    assert out["workload"] == {"kv_slot": 0, "attn_keys": 0, "token_id": 0}
    assert out["launches"] >= 6 * (6 + 1 + 1)
