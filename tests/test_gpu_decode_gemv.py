"""The arguments a captured greedy decode step adds to its GEMV / lm_head launches, one launch at a
time (l3_op_decode_gemm_host, l3_op_argmax_parts_host, l3_op_kv_restore_host) against the NumPy
reference and the case tables of tests/decode_gemv_ref.py (DESIGN.md "Captured-decode GEMV arguments
at kernel level").

Every case asserts the route report first (family, rows per block, lanes per unit, written by
launch_gemm at the launch site), then values over the WHOLE buffers, guard space included: operands
are small integers, so every logit is exact in fp32 in any order and everything is compared bit for
bit (-0 taken as +0) — except EPI_SWIGLU's output, which goes through silu_f and is held to
gemm_epi_ref's bound.  The non-temporal forms (a 64 MB weight) are not run.
"""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import decode_gemv_ref as ref
import gemm_epi_ref as epi_ref
import l3hip
from gemm_epi_ref import QKV, RESID, STORE, SWIGLU

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHECK_LIB = os.path.join(os.path.dirname(HERE), "llama3.np_amd", "csrc", "libllama3hip_check.so")


@pytest.fixture(scope="module")
def ctx():
    return l3hip.op_context(0)


def _bits(a):
    return (np.ascontiguousarray(a, np.float32) + np.float32(0)).view(np.uint32)  # -0 -> +0


def _raw(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want, what):
    """Equal values bit for bit, -0 as +0 and any NaN as any NaN."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere((_bits(got) != _bits(want)) & ~(np.isnan(got) & np.isnan(want)))
    assert bad.size == 0, (what, len(bad), bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def _same_raw(got, want, what):
    bad = np.argwhere(_raw(got) != _raw(want))
    assert bad.size == 0, (what, len(bad), bad[:4].tolist())


def _route(out, want, what):
    got = {k: out["route"].get(k) for k in want}
    assert got == want, (what, out["route"], want)


def _parts_equal(got, want, what):
    assert np.array_equal(got["i"], want["i"]), (what, got["i"].tolist()[:12], want["i"].tolist()[:12])
    _same(got["v"], want["v"], what)


def _storage_kw(storage, norm, norm_w):
    kw = dict(storage=storage, norm=norm, eps=0.0)
    if norm_w is not None:
        kw["norm_w"] = norm_w
    return kw


# ---- A. amax_part (+ pos_adv) on the one-row EPI_STORE GEMV --------------------------------------

@pytest.mark.parametrize("case", ref.AMAX_CASES, ids=lambda c: c.id)
def test_amax_part(ctx, case):
    for k, scen in enumerate(ref.amax_scenarios(case)):
        what = (case.id, scen[0])
        x, w, norm_w, _, winner = ref.amax_inputs(case, scen)
        z, want = ref.amax_reference(case, x, w, norm_w)
        kw = _storage_kw(case.storage, case.norm, norm_w)
        plain = ctx.op_decode_gemm(STORE, x, w, **kw)
        _route(plain, case.route, what)
        adv = bool(k & 1)
        st = l3hip.DecState(7, hist_cap=0, hist=False, hist_val=False)
        out = ctx.op_decode_gemm(STORE, x, w, amax_part=True, state=st, pos_adv=adv, **kw)
        _route(out, case.route, what)
        assert out["amax_blocks"] == case.blocks, what
        _same_raw(out["c"], plain["c"], what)                      # C as without amax_part, guard row included
        _same_raw(out["c"][1:], l3hip.gemm_sentinel((1, case.N), 7), what)
        _same(out["c"][0], z, what)                                # ... and the exact logits
        got = out["amax_part"]
        _parts_equal(got[:case.blocks], want, what)
        _same_raw(got["v"][:case.blocks], out["c"][0][got["i"][:case.blocks]], what)  # the stored logit's bits
        guard = l3hip.argmax_parts_sentinel(case.N // 4 + 4, 1)
        assert np.array_equal(got[case.blocks:], guard[case.blocks:]), what
        assert st.pos == 7 + int(adv) and st.arrive == 0, (what, st.pos)
        # B on A's partials: the id is np.argmax of the logits
        ids = ctx.op_argmax_parts(got[:case.blocks][None])
        assert ids[0] == winner == ref.first_argmax(out["c"][0]), (what, ids)


# ---- B. argmax_parts_kernel -------------------------------------------------------------------------

def _check_state(st, rows, pos, hist_off, base, cap, ids, vals, what):
    slot = ref.hist_slot(pos, hist_off, base, cap)
    n = cap * rows + 1
    h, hv = l3hip.int_sentinel(n, 3), l3hip.gemm_sentinel(n, 11).copy()
    if slot is not None:
        h[slot * rows:(slot + 1) * rows] = ids
        hv[slot * rows:(slot + 1) * rows] = vals
    if st.hist is not None:
        assert np.array_equal(st.hist, h), (what, slot, st.hist.tolist(), h.tolist())
    if st.hist_val is not None:
        _same(st.hist_val, hv, what)
    assert st.pos == pos + (0 if hist_off else 1), (what, st.pos)
    assert st.arrive == 0, (what, st.arrive)


def test_argmax_parts_tables(ctx):
    tabs = ref.argmax_tables()
    k = 0
    for name, t, (v, i) in tabs:  # one row
        pos, base, cap, _ = ref.STATE_CASES[k % len(ref.STATE_CASES)]
        hist_off = (k // len(ref.STATE_CASES)) & 1
        st = l3hip.DecState(pos, base, cap, hist=k % 5 != 3, hist_val=k % 5 != 4)
        ids = ctx.op_argmax_parts(t[None], hist_off, st)
        assert ids[0] == i and ids[1] == l3hip.int_sentinel(2, 6)[1], (name, ids, i)
        _check_state(st, 1, pos, hist_off, base, cap, [i], [v], name)
        assert ctx.op_argmax_parts(t[None])[0] == i, name  # and without a state
        k += 1
    by_n = {}
    for name, t, win in tabs:
        by_n.setdefault(len(t), []).append((name, t, win))
    for n, group in by_n.items():  # three rows
        for g0 in range(0, len(group) - 2, 3):
            trio = group[g0:g0 + 3]
            table = np.stack([t for _, t, _ in trio])
            want_i = [w[1] for _, _, w in trio]
            want_v = [w[0] for _, _, w in trio]
            pos, base, cap, _ = ref.STATE_CASES[k % len(ref.STATE_CASES)]
            hist_off = (k // len(ref.STATE_CASES)) & 1
            st = l3hip.DecState(pos, base, cap, rows=3)
            ids = ctx.op_argmax_parts(table, hist_off, st)
            what = [nm for nm, _, _ in trio]
            assert ids[:3].tolist() == want_i and ids[3] == l3hip.int_sentinel(4, 6)[3], (what, ids)
            _check_state(st, 3, pos, hist_off, base, cap, want_i, want_v, what)
            k += 1
    assert k > 2 * len(ref.STATE_CASES)  # every state under both hist_off


# ---- C. amax_rows on the tiled EPI_STORE kernels ---------------------------------------------------

@pytest.mark.parametrize("case", ref.ROWS_CASES, ids=lambda c: c.id)
def test_amax_rows(ctx, case):
    x, w, _ = ref.rows_inputs(case)
    z, want = ref.rows_reference(case, x, w)
    M, N = case.M, case.N
    kw = dict(norm=case.norm, eps=0.0, force_tiled=case.force)
    plain = ctx.op_decode_gemm(STORE, x, w, **kw)
    _route(plain, case.route, case.id)
    _same(plain["c"][:M], z, case.id)
    c0 = l3hip.gemm_sentinel((M, N), 6)
    out = ctx.op_decode_gemm(STORE, x, w, amax_rows=True, **kw)
    _route(out, case.route, case.id)
    _same_raw(out["c"][:M], c0, case.id)                                     # C is left exactly as given
    _same_raw(out["c"][M:], l3hip.gemm_sentinel((1, N), 7), case.id)
    rec = out["amax_rows"]
    assert rec.shape == (M + 1, case.nct)
    guard = l3hip.argmax_parts_sentinel((M + 1, case.nct), 2)
    assert np.array_equal(rec[M:], guard[M:]), (case.id, rec[M:].tolist()[:1], guard[M:].tolist()[:1])
    _parts_equal(rec[:M], want, case.id)
    logits = plain["c"][:M]
    _same_raw(rec["v"][:M], np.take_along_axis(logits, rec["i"][:M].astype(np.int64), axis=1), case.id)
    ids = ctx.op_argmax_parts(rec[:M])
    assert ids[:M].tolist() == [ref.first_argmax(r) for r in logits], case.id


# ---- D. the O-proj partial rows ----------------------------------------------------------------------

def _run_parts(ctx, case, inp, **over):
    kw = _storage_kw(case.storage, case.norm, inp["norm_w"])
    if case.norm:
        kw["eps"] = 1e-5
    kw.update(over)
    if case.epi == SWIGLU:
        return ctx.op_decode_gemm(SWIGLU, inp["x"], gate_up=(inp["wg"], inp["wu"]), parts=inp["parts"], x_out=True, **kw)
    return ctx.op_decode_gemm(RESID, inp["x"], inp["w"], c=inp["c0"], parts=inp["parts"], **kw)


@pytest.mark.parametrize("case", ref.PARTS_CASES, ids=lambda c: c.id)
def test_parts(ctx, case):
    inp = ref.parts_inputs(case)
    xs, want, bound = ref.parts_reference(case, inp)
    out = _run_parts(ctx, case, inp)
    _route(out, case.route, case.id)
    M = case.M
    ldc = case.N // 2 if case.epi == SWIGLU else case.N
    _same_raw(out["c"][M:], l3hip.gemm_sentinel((1, ldc), 7), case.id)
    if case.epi == RESID:
        _same(out["c"][:M], want, case.id)
        return
    _same(out["x_out"][:M], xs, case.id)  # the summed row, in head order, the guard row never added
    _same_raw(out["x_out"][M:], l3hip.gemm_sentinel((M + 1, case.K), 13)[M:], case.id)
    err = np.abs(out["c"][:M].astype(np.float64) - want)
    over = np.argwhere(err > bound)
    assert over.size == 0, (case.id, len(over), over[:4].tolist(), err[tuple(over[0])], bound[tuple(over[0])])


def test_parts_x_out_is_the_same_under_every_storage(ctx):
    done = 0
    for base in [c for c in ref.PARTS_CASES if c.epi == SWIGLU and c.K == ref.PARTS_XOUT_K and c.storage == "fp32"]:
        outs = {}
        for st in ref.STORAGES:
            case = ref.PartsCase(base.epi, st, base.K, base.nparts, base.M, base.kind, base.norm)
            inp = ref.parts_inputs(case)
            outs[st] = _run_parts(ctx, case, inp)
            _route(outs[st], case.route, case.id)
        _same_raw(outs["bf16"]["x_out"], outs["fp32"]["x_out"], base.id)
        _same_raw(outs["fp8"]["x_out"], outs["fp32"]["x_out"], base.id)
        done += 1
    assert done >= 6


def test_parts_refusals(ctx):
    x = np.ones((1, 64), np.float32)
    w = np.ones((36, 64), np.float32)
    c = np.zeros((1, 36), np.float32)
    p = np.ones((1, 1, 36), np.float32)
    with pytest.raises(RuntimeError, match=r"nparts 0 outside \[1, 8\]"):
        ctx.op_decode_gemm(RESID, x, w, c=c, parts=p, nparts=0)
    with pytest.raises(RuntimeError, match=r"nparts 9 outside \[1, 8\]"):
        ctx.op_decode_gemm(RESID, x, w, c=c, parts=p, nparts=9)
    with pytest.raises(RuntimeError, match=r"parts go with epi 1 / 2, not epi 0"):
        ctx.op_decode_gemm(STORE, x, w, parts=np.ones((1, 1, 64), np.float32))
    g = ref.FOLD_GEO
    cos, sin = ref.synthetic_rope(4, g["HD"] // 2)
    q = dict(L=1, start_pos=1, Smax=4, q_scale=0.25, rope_cos=cos, rope_sin=sin, **g,
             cache_k=np.zeros((1, g["KVH"], 4, g["HD"]), np.float32), cache_v=np.zeros((1, g["KVH"], 4, g["HD"]), np.float32))
    with pytest.raises(RuntimeError, match=r"parts go with epi 1 / 2, not epi 3"):
        ctx.op_decode_gemm(QKV, x, np.ones((128, 64), np.float32), qkv=q, parts=np.ones((1, 1, 64), np.float32))
    x9 = np.ones((9, 64), np.float32)
    with pytest.raises(RuntimeError, match=r"parts take the one-row GEMV's range, not 9 x 64 x 36"):
        ctx.op_decode_gemm(RESID, x9, w, c=np.zeros((9, 36), np.float32), parts=np.ones((9, 1, 36), np.float32))
    # and one step inside is taken
    out = ctx.op_decode_gemm(RESID, x, w, c=c, parts=p)
    _same(out["c"][:1], np.full((1, 36), 65.0, np.float32), "inside")


# ---- E. the folded argmax --------------------------------------------------------------------------

def _fold_qkv(pos, B=1):
    g = ref.FOLD_GEO
    cos, sin = ref.synthetic_rope(ref.FOLD_SMAX, g["HD"] // 2)
    shape = (B, g["KVH"], ref.FOLD_SMAX, g["HD"])
    return dict(L=1, start_pos=pos, Smax=ref.FOLD_SMAX, q_scale=0.25, rope_cos=cos, rope_sin=sin,
                cache_k=l3hip.gemm_sentinel(shape, 3), cache_v=l3hip.gemm_sentinel(shape, 4), **g)


@pytest.mark.parametrize("case", ref.FOLD_CASES, ids=lambda c: c.id)
def test_fold(ctx, case):
    tab, w, norm_w = ref.fold_operands(case)
    kw = _storage_kw(case.storage, True, norm_w)
    unfolded = {}

    def plain(tok, pos, **more):
        key = (tok, pos, tuple(more))
        if key not in unfolded:
            unfolded[key] = ctx.op_decode_gemm(QKV, tab, w, a_rows=np.array([tok], np.int32), qkv=_fold_qkv(pos), **more, **kw)
            _route(unfolded[key], case.route, (case.id, tok))
        return unfolded[key]

    for k, (name, t, (v, tok)) in enumerate(ref.fold_tables()):
        what = (case.id, name)
        pos, base, cap = ref.FOLD_STATES[k % len(ref.FOLD_STATES)]
        st = l3hip.DecState(pos, base, cap, hist=k % 5 != 3, hist_val=k % 5 != 4)
        cache_pos = (3 * k + 1) % ref.FOLD_SMAX
        out = ctx.op_decode_gemm(QKV, tab, w, amax_in=t, state=st, qkv=_fold_qkv(cache_pos), **kw)
        _route(out, case.route, what)
        want = plain(tok, cache_pos)
        for name2 in ("q_out", "cache_k", "cache_v"):  # whole buffers: the guards are the un-folded launch's
            _same_raw(out[name2], want[name2], (what, name2))
        assert out["amax_ids"].tolist() == [tok, int(l3hip.int_sentinel(2, 5)[1])], (what, out["amax_ids"], tok)
        slot = ref.hist_slot(pos, 1, base, cap)
        n = cap + 1
        h, hv = l3hip.int_sentinel(n, 3), l3hip.gemm_sentinel(n, 11).copy()
        if slot is not None:
            h[slot], hv[slot] = tok, v
        if st.hist is not None:
            assert np.array_equal(st.hist, h), (what, slot, st.hist.tolist())
        if st.hist_val is not None:
            _same(st.hist_val, hv, what)
        assert st.pos == pos and st.arrive == 0, (what, st.pos)
    # a captured step sets the undo slots and the device position as well
    name, t, (v, tok) = next(x for x in ref.fold_tables() if x[0] == "n4096-win2048")
    st = l3hip.DecState(9, 0, 16)
    out = ctx.op_decode_gemm(QKV, tab, w, amax_in=t, state=st, qkv=_fold_qkv(9), kv_bak=True, pos_dev=True, **kw)
    _route(out, case.route, case.id)
    want = plain(tok, 9, kv_bak=True)
    for name2 in ("q_out", "cache_k", "cache_v", "kv_bak"):
        _same_raw(out[name2], want[name2], (case.id, "with kv_bak", name2))
    assert out["amax_ids"][0] == tok and st.hist[8] == tok and st.pos == 9


def test_fold_refusals(ctx):
    case = ref.FOLD_CASES[0]
    tab, w, _ = ref.fold_operands(case)
    t = ref.fold_tables()[1][1]
    st = lambda: l3hip.DecState(3, 0, 4)  # noqa: E731
    kw = dict(norm=True, eps=0.0)
    with pytest.raises(RuntimeError, match=r"amax_in takes M == 1 \(M 2\)"):
        ctx.op_decode_gemm(QKV, tab, w, amax_in=t, state=st(), a_rows=np.array([0, 1], np.int32), qkv=_fold_qkv(2, B=2), **kw)
    g = ref.FOLD_GEO
    with pytest.raises(RuntimeError, match=r"amax_in takes no col_base \(64\)"):
        ctx.op_decode_gemm(QKV, tab, w[g["H"] * g["HD"]:], amax_in=t, state=st(),
                           qkv=dict(_fold_qkv(2), col_base=g["H"] * g["HD"]), **kw)
    with pytest.raises(RuntimeError, match=r"amax_in takes no a_rows"):
        ctx.op_decode_gemm(QKV, tab, w, amax_in=t, state=st(), a_rows=np.array([0], np.int32), qkv=_fold_qkv(2), **kw)
    with pytest.raises(RuntimeError, match=r"amax_in_n 0"):
        ctx.op_decode_gemm(QKV, tab, w, amax_in=t, amax_in_n=0, state=st(), qkv=_fold_qkv(2), **kw)
    with pytest.raises(RuntimeError, match=r"amax_in takes amax_ids"):
        ctx.op_decode_gemm(QKV, tab, w, amax_in=t, amax_ids=False, state=st(), qkv=_fold_qkv(2), **kw)


# ---- F. the undo slots and their restore -------------------------------------------------------------

@pytest.mark.parametrize("case", ref.KV_CASES, ids=lambda c: c.id)
def test_kv_bak_and_restore(ctx, case):
    B, K, KVH, HD, Smax = case.B, case.K, case.KVH, case.HD, ref.KV_SMAX
    w = ref.kv_weight(case.N, K)
    x = np.random.default_rng(B * K).choice([-2.0, 2.0], (B, K)).astype(np.float32)
    cos, sin = ref.synthetic_rope(Smax, HD // 2)
    ck0, cv0 = l3hip.gemm_sentinel((B, KVH, Smax, HD), 3), l3hip.gemm_sentinel((B, KVH, Smax, HD), 4)
    bak0 = l3hip.gemm_sentinel((ref.KV_BAK_SLOTS + 1, 2, B, KVH, HD), 14)
    for pos, dev in ref.kv_positions(case):
        what = (case.id, pos, dev)
        q = dict(L=1, start_pos=pos, H=case.H, KVH=KVH, HD=HD, Smax=Smax, q_scale=0.25, rope_cos=cos, rope_sin=sin,
                 cache_k=ck0, cache_v=cv0)
        kw = dict(norm=True, eps=0.0, qkv=q)
        plain = ctx.op_decode_gemm(QKV, x, w, **kw)
        _route(plain, case.route, what)
        st = l3hip.DecState(pos, hist=False, hist_val=False) if dev else None
        out = ctx.op_decode_gemm(QKV, x, w, kv_bak=True, state=st, pos_dev=dev, **kw)
        _route(out, case.route, what)
        for name in ("q_out", "cache_k", "cache_v"):  # as without kv_bak, guards included
            _same_raw(out[name], plain[name], (what, name))
        assert not np.array_equal(_raw(out["cache_k"][:B, :, pos]), _raw(ck0[:, :, pos])), what  # the slot was written
        want = bak0.copy()
        slot = pos % ref.KV_BAK_SLOTS
        want[slot, 0] = ck0[:, :, pos]  # [k, v][row][head][hd]
        want[slot, 1] = cv0[:, :, pos]
        _same_raw(out["kv_bak"], want, (what, "kv_bak"))
        if st is not None:
            assert st.pos == pos
        # the restore puts the whole caches back
        for name, half, orig in (("cache_k", 0, ck0), ("cache_v", 1, cv0)):
            back = ctx.op_kv_restore(out[name], out["kv_bak"][slot, half], pos)
            _same_raw(back[:B], orig, (what, "restored", name))
            _same_raw(back[B:], plain[name][B:], (what, "restored guard", name))


# ---- G. device checks ----------------------------------------------------------------------------------

def test_check_build_records_no_violation():
    if not os.path.exists(CHECK_LIB):
        pytest.skip(f"{CHECK_LIB} missing: build it with `make -C llama3.np_amd/csrc check-lib` "
                    "(__graft_entry__.build() does)")
    env = dict(os.environ, L3_LIB_PATH=CHECK_LIB)
    r = subprocess.run([sys.executable, os.path.join(HERE, "decode_gemv_checks_workload.py")], env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["enabled"] is True
    assert out["workload"] == {"kv_slot": 0, "attn_keys": 0, "token_id": 0}
    assert out["groups"] == ["amax_part", "argmax_parts", "amax_rows", "parts", "fold", "kv_bak"]
