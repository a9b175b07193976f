"""The reference and the case tables of tests/attn_dense_ref.py, checked without a GPU: the
reference against the reference model's own masked full-matrix formulation, the expected routes
against the full set of instantiations behind csrc/attention.hip (so the GPU tests cannot quietly
cover less), and every case's key range and poison layout."""

import numpy as np
import pytest

import attn_dense_ref as ref
import l3hip


def _all_cases():
    for hd, n_rep in ref.PARAMS:
        yield from ref.prefill_cases(hd, n_rep)
        yield from ref.decode_cases(hd, n_rep)
        yield from ref.fused_cases(hd, n_rep)
        yield from ref.last_cases(hd, n_rep)
    for hd, n_rep in ref.LONG_SHAPES:
        yield from ref.long_cases(hd, n_rep)


@pytest.mark.parametrize("hd,n_rep,kvh,B,L,start,smax", [
    (16, 1, 1, 1, 1, 0, 8), (16, 2, 2, 2, 5, 0, 8), (32, 3, 2, 2, 7, 9, 16), (48, 4, 1, 1, 17, 3, 40),
    (128, 8, 2, 1, 1, 19, 20),
])
def test_reference_equals_the_masked_full_matrix_formulation(hd, n_rep, kvh, B, L, start, smax):
    case = ref.Case(hd, n_rep, kvh, B, L, start, smax, {"kernel": "prefill"})
    inp = ref.make_inputs(case)
    a = ref.reference(inp["q_s"], inp["cache_k"], inp["cache_v"], start, inp["n_heads"])
    b = ref.reference_masked(inp["q_s"], inp["cache_k"], inp["cache_v"], start, inp["n_heads"])
    assert a.shape == (B, L, n_rep * kvh * hd) and np.isfinite(a).all()
    assert float(np.abs(a - b).max()) <= 1e-12


def test_parts_reference_sums_to_the_o_proj():
    case = ref.fused_cases(32, 3)[2]
    inp = ref.make_inputs(case)
    out = ref.reference(inp["q_s"], inp["cache_k"], inp["cache_v"], case.start_pos, inp["n_heads"])[:, 0]
    parts = ref.reference_parts(out, inp["wo"], inp["n_heads"])
    assert parts.shape == (case.B, inp["n_heads"], case.D)
    assert float(np.abs(parts.sum(axis=1) - out @ inp["wo"].astype(np.float64).T).max()) <= 1e-12


def test_expected_routes_cover_every_instantiation():
    """all 42 attn_fwd_kernel (HD, QBW, G, KT) and all 12 attn_decode_kernel (HD, FUSE_O)"""
    prefill = {(hd, qbw, g, ref.KT_OF[hd]) for hd in (16, 32, 48, 64) for qbw in (1, 2, 4) for g in (1, 2, 4)}
    prefill |= {(hd, 1, g, 32) for hd in (96, 128) for g in (1, 2, 4)}
    decode = {(hd, fused) for hd in ref.HDS for fused in (False, True)}
    assert len(prefill) == 42 and len(decode) == 12
    got_p, got_d = set(), set()
    for hd, n_rep in ref.PARAMS:  # the full launches only: the last-rows table adds nothing to the count
        for c in ref.prefill_cases(hd, n_rep) + ref.decode_cases(hd, n_rep) + ref.fused_cases(hd, n_rep):
            r = c.route
            if r["kernel"] == "prefill":
                got_p.add((r["hd"], r["qbw"], r["g"], r["kt"]))
            else:
                got_d.add((r["hd"], r["kernel"] == "decode_oproj"))
    assert got_p == prefill, prefill ^ got_p
    assert got_d == decode, decode ^ got_d
    # every n_rep of a group width at least once per head size, on the prefill and the decode kernel
    for hd in ref.HDS:
        for n_rep in ref.N_REPS:
            kinds = {c.route["kernel"] for c in ref.prefill_cases(hd, n_rep)}
            assert kinds == {"prefill", "decode"}, (hd, n_rep)
            assert all(c.route["g"] == ref.G_OF[n_rep] for c in ref.prefill_cases(hd, n_rep) if c.route["g"])
    # the long-cache table: L = 1 on both kernels, at the first and the last position
    for hd, n_rep in ref.LONG_SHAPES:
        cs = ref.long_cases(hd, n_rep)
        assert [(c.smax, c.start_pos, c.route["kernel"], c.route["qbw"]) for c in cs] == [
            (8193, 0, "prefill", 1), (8193, 8192, "prefill", 1), (8192, 0, "decode", 0), (8192, 8191, "decode", 0)]


def test_tables_hold_the_shapes_the_kernels_turn_on():
    for hd, n_rep in ref.PARAMS:
        w, kt = 4 // ref.G_OF[n_rep], ref.KT_OF[hd]
        cs = ref.prefill_cases(hd, n_rep)
        assert {c.L for c in cs} == {1, 16 * w, 16 * w + 1, 32 * w, 32 * w + 1, 64 * w + 17}
        for L in {c.L for c in cs}:
            starts = {c.start_pos for c in cs if c.L == L}
            want = {s for s in (0, 1, 17, kt - 2, kt - 1, kt, 300 - L) if s + L <= 300}
            assert starts == want and 300 - L in starts and 0 in starts, (hd, n_rep, L)
        assert all(c.kvh == 2 and c.B == 2 and c.smax == 300 and c.smax % 16 for c in cs)
        r = ref.ROWS_OF[hd]
        assert r == 256 // (hd // 4)
        ds = ref.decode_cases(hd, n_rep)
        assert {c.start_pos + 1 for c in ds} == {1, r, r + 1, 8 * r, 8 * r + 1, 256, 257, 700}
        assert all(c.L == 1 and c.smax == 700 and c.B == 2 for c in ds)
        fs = ref.fused_cases(hd, n_rep)
        assert {(c.D, c.B) for c in fs} == {(d, b) for d in (4, 64, 68, 192) for b in (1, 2)} and len(fs) == 8
        ls = ref.last_cases(hd, n_rep)
        assert {(c.L, c.start_pos) for c in ls} == {(L, s) for L in (16 * w - 1, 16 * w, 16 * w + 1, 64 * w + 17)
                                                    for s in (0, 17)}
        assert all(c.route["grid"][0] == 1 and c.route["qbw"] == 1 for c in ls)


def test_every_case_fits_its_cache_and_is_poisoned_as_stated():
    n = 0
    for c in _all_cases():
        n += 1
        assert c.start_pos >= 0 and c.L >= 1 and c.start_pos + c.L <= c.smax, c
        assert c.route["hd"] == c.hd and (c.n_rep * c.kvh) % c.kvh == 0
    assert n > 1500
    # the layout itself, on one case per kernel and edge (the arrays of the big cases are not built here)
    picks = [ref.prefill_cases(16, 2)[7], ref.prefill_cases(128, 3)[-1], ref.prefill_cases(48, 8)[-2],
             ref.decode_cases(96, 1)[3], ref.decode_cases(16, 4)[-1], ref.fused_cases(64, 6)[5],
             ref.last_cases(32, 2)[3], ref.long_cases(16, 1)[0], ref.long_cases(16, 1)[3]]
    for c in picks:
        for inp in (ref.make_inputs(c), ref.census_inputs(c)):
            end = c.start_pos + c.L
            for a in (inp["cache_k"], inp["cache_v"]):
                assert np.isfinite(a[:, :, :end]).all() and (np.abs(a[:, :, :end]) < 1e3).all()
                if c.route["kernel"] == "prefill":
                    up = min((end + 15) // 16 * 16, c.smax)
                    assert (a[:, :, end:up] == ref.FINITE_POISON).all()
                    assert np.isnan(a[:, :, up:]).all()
                else:
                    assert np.isnan(a[:, :, end:]).all()
    assert any(c.start_pos + c.L == c.smax for c in picks) and any((c.start_pos + c.L) % 16 for c in picks)


def test_census_counts_by_enumeration():
    c = ref.prefill_cases(16, 3)[9]
    want = np.array([[sum(1 for j in range(c.start_pos + t + 1) if j % c.hd == d) for d in range(c.hd)]
                     for t in range(c.L)])
    assert np.array_equal(ref.census(c), want)
    # and the reference on the census inputs gives census / keys
    inp = ref.census_inputs(c)
    out = ref.reference(inp["q_s"], inp["cache_k"], inp["cache_v"], c.start_pos, inp["n_heads"])
    keys = c.start_pos + np.arange(c.L)[:, None] + 1
    got = out.reshape(c.B, c.L, inp["n_heads"], c.hd) * keys[None, :, None, :]
    assert float(np.abs(got - want[None, :, None, :]).max()) <= 1e-9


def test_stress_scores_are_exact_in_fp32():
    c = ref.prefill_cases(64, 2)[-1]
    for shape in ref.STRESS:
        inp = ref.stress_inputs(c, shape)
        q = inp["q_s"].reshape(c.B, c.L, inp["n_heads"], c.hd)
        assert (q[..., 0] == 1).all() and not q[..., 1:].any()
        s = inp["cache_k"][0, 0, :c.start_pos + c.L, 0].astype(np.float64)
        assert np.array_equal(s * 2, np.round(s * 2)) and np.abs(s).max() <= 512  # halves: exact in fp32
        if shape.startswith("spike"):
            assert sorted(set(s)) == [0.0, 40.0] and (s == 40).sum() == 1


def test_entry_is_declared_bound_and_loud_without_a_context():
    assert "l3_op_attention_host" in l3hip.header_symbols()
    lib = l3hip.lib()
    assert lib.l3_op_attention_host(None, None, None, None, 1, 1, 0, 1, 1, 16, 1, 0, None, 0, None, 2, None) != 0
    assert b"null context" in lib.l3_last_error()
    q = l3hip.attn_scale_q(np.ones((1, 1, 16), np.float32), 16)
    assert q.dtype == np.float32 and q[0, 0, 0] == np.float32(1.4426950408889634 / 4.0)
