"""The persistent batch-1 decode step (decode_persist.hip) stage by stage, on every instance: one
step launched directly (l3_op_decode_persist_host), every stage's granules against the float64
reference of that stage fed the DEVICE's granules of the stage before (tests/decode_persist_ref.py),
and bit for bit: tags, the cache slot, the undo slot, position, epoch and history.

Bounds (DESIGN.md "Persistent step coverage").  The GEMV stages A, C, D, E and the lm_head: the
worst-case fp32 bound of tests/gemm_epi_ref.py, K 2^-24 (|x| . |w|) carried through the row factor,
RoPE, SwiGLU and the residual add; asserted as error / bound <= 1.  The attention stage B: ATTN_TOL
is 4x the worst |o - float64| / max(1, max |v|) measured on the MI355X over the case table below
(the kernel is deterministic; the factor covers other seeds), and may not exceed the ragged
attention module's 1e-5.  Each test prints its worst ratios (pytest -s).
"""

import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import decode_persist_ref as ref
import l3hip
import llama3

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHECK_LIB = os.path.join(os.path.dirname(HERE), "llama3.np_amd", "csrc", "libllama3hip_check.so")

ATTN_WORST = 3.67e-7  # measured: worst |o - float64| / max(1, max |v|) over CASES x positions (long_nrep8, pos 519)
ATTN_TOL = 4 * ATTN_WORST
ATTN_CAP = 1e-5
EMPTY_IDX = ref.EMPTY[1]


@pytest.fixture(scope="module")
def tmp():
    with tempfile.TemporaryDirectory() as d:
        yield d


_built = {}


def _setup(tmp, case, Smax=None):
    """(args, weights path, reference Model) of a case, made once."""
    key = (case.name, Smax or case.Smax)
    if key not in _built:
        args, w = ref.case_weights(case, Smax)
        path = os.path.join(tmp, f"{case.name}_{key[1]}.npz")
        np.savez(path, **w)
        _built[key] = (args, path, ref.Model(args, w, case.FD))
    return _built[key]


def _fresh(tmp, case, Smax=None):
    args, path, m = _setup(tmp, case, Smax)
    return llama3.Llama(path, args), m


def _caches(ctx, S):
    return [ctx.cache_read(l, 0, 0, S) for l in range(2)]


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, what
    assert (a.view(np.uint32) == b.view(np.uint32)).all(), what


def _ratio(dev, want, bound, what):
    err = np.abs(dev.astype(np.float64) - want)
    r = float((err / np.maximum(bound, 1e-300)).max())
    assert np.isfinite(dev).all() and r <= 1.0, f"{what}: error / bound {r:.3f} (worst error {err.max():.3e})"
    return r


def _step(model, case, ids, pos, *, steps=1, kv_bak=False, hist=None, token=None, prefilled=False):
    """Prefill ids[:, :pos] on the ordinary path (unless prefilled), then the persistent step at pos
    fed `token` (default ids[0, pos]).  hist: (base, cap), default a window that holds the step."""
    ctx = model.context
    S = model.args.max_seq_len
    if not prefilled:
        ctx.reset_cache()
        model(ids[:, :pos], 0)
    before = _caches(ctx, S)
    base, cap = hist if hist is not None else (pos - 2, 6)
    st = l3hip.DecState(pos, base, cap)
    tok = int(ids[0, pos]) if token is None else int(token)
    d = ctx.op_decode_persist(tok, st, steps=steps, kv_bak=kv_bak)
    return dict(d=d, st=st, before=before, after=_caches(ctx, S), tok=tok, pos=pos, base=base, cap=cap, steps=steps)


def _check_route(case, d):
    r = d["route"]
    assert r["instance"] == ref.instance_of(case.D, case.FD, case.D // case.H), r
    assert r["grid"] == ref.GRID and r["GL"] == ref.GL, r


def _check_stages(m, d, tok, pos, caches):
    """Every stage of the dump against its float64 reference, fed the device's own granules; the
    lm partials and the id.  caches: per layer (k, v) [KVH, S, HD] as they were before the launch.
    Returns the worst error / bound per stage ('B': error / max(1, max |v|))."""
    worst = dict.fromkeys("ABCDE", 0.0)
    worst["lm"] = 0.0
    for li in range(2):
        for s in ref.STAGES:
            assert (d["tags"][li][s] == d["tag"]).all(), (li, s, "tag")
    hin = m.emb[tok].astype(np.float32)
    for li in range(2):
        v = d["vals"][li]
        want, b = m.stage_a(li, hin, pos)
        worst["A"] = max(worst["A"], _ratio(v["qkv"], want, b, f"layer {li} stage A"))
        ck, cv = caches[li]
        want = m.stage_b(v["qkv"], ck, cv, pos)
        scale = max(1.0, float(np.abs(cv[:, :pos]).max()), float(np.abs(v["qkv"][m.qdim + m.kvdim:]).max()))
        err = float(np.abs(v["o"].astype(np.float64) - want).max()) / scale
        worst["B"] = max(worst["B"], err)
        assert np.isfinite(v["o"]).all() and err <= ATTN_TOL, f"layer {li} attention: {err:.3e} of max(1, max |v|)"
        want, b = m.stage_c(li, v["o"], hin)
        worst["C"] = max(worst["C"], _ratio(v["h1"], want, b, f"layer {li} stage C"))
        want, b = m.stage_d(li, v["h1"])
        worst["D"] = max(worst["D"], _ratio(v["hid"], want, b, f"layer {li} stage D"))
        want, b = m.stage_e(li, v["hid"], v["h1"])
        worst["E"] = max(worst["E"], _ratio(v["h2"], want, b, f"layer {li} stage E"))
        hin = v["h2"]
    z, zb = m.logits(hin)
    val, idx, margin, bnd = ref.lm_partials(z, zb)
    live = idx != EMPTY_IDX
    dv, di = d["lm_val"][:ref.NLM], d["lm_idx"][:ref.NLM]
    assert (d["lm_tag"][:ref.NLM] == d["tag"]).all()
    assert np.isneginf(dv[~live]).all() and (di[~live] == EMPTY_IDX).all(), "empty lm workgroups publish the sentinel"
    worst["lm"] = _ratio(dv[live], val[live], bnd[live], "lm partial value")
    clear = live & (margin > 2 * bnd)
    assert (di[clear] == idx[clear]).all(), np.flatnonzero(clear & (di != idx))
    assert (live & ~clear).sum() <= 0.02 * live.sum()
    for i in np.flatnonzero(live & ~clear):  # under the margin: still one of the range's near-maximal rows
        r0, r1 = ref.lm_ranges(m.VS)[i]
        assert r0 <= di[i] < r1 and z[di[i]] >= val[i] - 2 * bnd[i]
    want_id, want_val = ref.final_pick(dv, di)
    assert d["id"] == want_id
    return worst, (want_id, np.float32(want_val))


def _check_exact(m, r, first=None):
    """Bit for bit: the cache slot, every other slot, the undo slot, position, epoch, error word,
    history.  first: with two launches, the single-launch run of the first step (its id, value and
    cache rows)."""
    d, st, pos, steps = r["d"], r["st"], r["pos"], r["steps"]
    last = pos + steps - 1
    assert st.pos == pos + steps
    assert d["epoch"][0] == d["tag"] + 1 and d["epoch"][1] == 0 and d["err"] == 0
    for li in range(2):
        qkv = d["vals"][li]["qkv"]
        kn = qkv[m.qdim:m.qdim + m.kvdim].reshape(m.KVH, m.HD)
        vn = qkv[m.qdim + m.kvdim:].reshape(m.KVH, m.HD)
        for which, new in ((0, kn), (1, vn)):
            after, before = r["after"][li][which], r["before"][li][which]
            _same_bits(after[:, last], new, (li, which, "the step's slot"))
            keep = np.ones(after.shape[1], bool)
            keep[pos:last + 1] = False
            _same_bits(after[:, keep], before[:, keep], (li, which, "every other slot"))
            if first is not None:
                _same_bits(after[:, pos], first["after"][li][which][:, pos], (li, which, "the first launch's slot"))
    kb = d["kv_bak"]
    if kb is not None:
        want = l3hip.gemm_sentinel(kb.shape, 14).copy()
        for p in range(pos, last + 1):
            for li in range(2):
                want[li, 0, p % ref.KV_BAK_SLOTS, 0] = r["before"][li][0][:, p]
                want[li, 0, p % ref.KV_BAK_SLOTS, 1] = r["before"][li][1][:, p]
        _same_bits(kb, want, "kv_bak: the slots' previous contents, nothing else")
    # history: the last launch's id and value in slot last - base, the first launch's before it
    n = r["cap"] + 1
    hist, hval = l3hip.int_sentinel(n, 3), l3hip.gemm_sentinel(n, 11).copy()
    pv, pi = d["lm_val"][:ref.NLM], d["lm_idx"][:ref.NLM]
    fid, fval = ref.final_pick(pv, pi)
    entries = [(last - r["base"], fid, np.float32(fval))]
    if first is not None:
        entries.append((pos - r["base"], first["d"]["id"], first["st"].hist_val[pos - first["base"]]))
    for q, i, v in entries:
        if 0 <= q < r["cap"]:
            hist[q], hval[q] = i, v
    np.testing.assert_array_equal(st.hist, hist)
    _same_bits(st.hist_val, hval, "history values")


def _run_and_check(model, m, case, ids, pos, **kw):
    r = _step(model, case, ids, pos, **kw)
    _check_route(case, r["d"])
    worst, _ = _check_stages(m, r["d"], r["tok"], pos, r["before"])
    _check_exact(m, r)
    return r, worst


def _merge(a, b):
    return {k: max(a.get(k, 0.0), v) for k, v in b.items()}


@pytest.mark.parametrize("case", ref.CASES, ids=lambda c: c.name)
def test_case_table(tmp, case):
    model, m = _fresh(tmp, case)
    ids = ref.case_ids(case, case.Smax)
    worst = {}
    for pos in case.positions:
        _, w = _run_and_check(model, m, case, ids, pos)
        worst = _merge(worst, w)
    assert ATTN_TOL <= ATTN_CAP
    print(f"{case.name} {ref.facts(case)['instance']} positions {case.positions}: error / bound "
          + ", ".join(f"{k} {worst[k]:.3f}" for k in "ACDE") + f", lm {worst['lm']:.3f}; attention {worst['B']:.3e}")


@pytest.mark.parametrize("shape,msg", ref.REFUSED, ids=lambda x: str(x).replace(" ", ""))
def test_refused_shapes(tmp, shape, msg):
    D, H, KVH, FD = shape
    case = ref.Case("refused%d_%d" % (D, FD), D, H, KVH, FD, 512, 64, 120, (1,))
    model, _ = _fresh(tmp, case)
    ids = ref.case_ids(case, 16)
    model(ids[:, :5], 0)
    with pytest.raises(RuntimeError, match=msg):
        model.context.op_decode_persist(int(ids[0, 5]), l3hip.DecState(5, 0, 8))
    # the ordinary path: the graph of kernels, and the context still works
    out = model.generate_all(ids[:, :5], 12)
    assert out.shape == (1, 7) and not model.context.decode_persistent()


@pytest.mark.parametrize("case", ref.FORM_CASES, ids=lambda c: c.name)
def test_forms(tmp, case):
    """kv_bak present (the slot's previous contents non-zero: 40 tokens prefilled, the step at 20) and
    absent; two chained launches; a history window that excludes the slot."""
    model, m = _fresh(tmp, case)
    ids = ref.case_ids(case, 64)
    ctx = model.context
    # kv_bak, over a slot that holds something
    ctx.reset_cache()
    model(ids[:, :40], 0)
    r = _step(model, case, ids, 20, kv_bak=True, prefilled=True)
    assert all(np.abs(r["before"][li][w][:, 20]).min() > 0 for li in range(2) for w in range(2))
    _check_route(case, r["d"])
    _check_stages(m, r["d"], r["tok"], 20, r["before"])
    _check_exact(m, r)
    # a history window that excludes the slot: before it, and past its cap
    for hist in ((30, 4), (10, 10), (21, 4)):
        r = _step(model, case, ids, 20, hist=hist)
        assert not 0 <= 20 - hist[0] < hist[1]
        _check_exact(m, r)
    # no history arrays at all
    ctx.reset_cache()
    model(ids[:, :20], 0)
    st = l3hip.DecState(20, 0, 0, hist=False, hist_val=False)
    d0 = ctx.op_decode_persist(int(ids[0, 20]), st)
    assert st.pos == 21 and d0["err"] == 0
    # two chained launches against the two single launches they stand for
    one = _step(model, case, ids, 20, kv_bak=True, hist=(18, 6))
    _check_exact(m, one)
    two = _step(model, case, ids, 20, steps=2, kv_bak=True, hist=(18, 6))
    assert two["d"]["tag"] == one["d"]["tag"] + 2  # the dump is the second launch's
    mid = [(one["after"][li][0], one["after"][li][1]) for li in range(2)]
    _check_stages(m, two["d"], one["d"]["id"], 21, mid)
    _check_exact(m, two, first=one)


@pytest.mark.parametrize("case", ref.FORM_CASES, ids=lambda c: c.name)
def test_dirty_tail(tmp, case):
    """Cache rows past pos, though loaded (the clamped, unpredicated loads), never reach a result:
    the step at 20 over slots 20 .. 39 that hold another sequence's rows equals, bit for bit, the
    step on a context whose slots past 20 were never written.  Both contexts get rows [0, 20) from
    the same 20-token prefill; the dirty one then runs 20 more tokens at position 20."""
    ids = ref.case_ids(case, 64)
    clean, m = _fresh(tmp, case)
    logits = clean(ids[:, :20], 0)
    tok = int(np.argmax(logits[0, -1]))  # the id the 20-token prefix feeds
    dirty, _ = _fresh(tmp, case)
    dirty(ids[:, :20], 0)
    dirty(ids[:, 20:40], 20)
    rc = _step(clean, case, ids, 20, token=tok, kv_bak=True, prefilled=True)
    rd = _step(dirty, case, ids, 20, token=tok, kv_bak=True, prefilled=True)
    for li in range(2):
        for w in range(2):
            _same_bits(rc["before"][li][w][:, :20], rd["before"][li][w][:, :20], "the shared prefix")
            assert np.abs(rd["before"][li][w][:, 20:40]).min() > 0 and not rc["before"][li][w][:, 20:].any()
            _same_bits(rd["after"][li][w][:, 21:], rd["before"][li][w][:, 21:], "slots 21 .. stay")
    assert rc["d"]["tag"] == rd["d"]["tag"]
    for li in range(2):
        for s in ref.STAGES:
            _same_bits(rc["d"]["vals"][li][s], rd["d"]["vals"][li][s], (li, s))
    _same_bits(rc["d"]["lm_val"], rd["d"]["lm_val"], "lm values")
    np.testing.assert_array_equal(rc["d"]["lm_idx"], rd["d"]["lm_idx"])
    assert rc["d"]["id"] == rd["d"]["id"]
    _check_stages(m, rd["d"], tok, 20, rd["before"])
    _check_exact(m, rd)
    _check_exact(m, rc)


def test_repeat(tmp):
    """The same step on two fresh contexts gives identical dumps; a second step with another id on
    the same context leaves no owned granule with the old tag."""
    case = ref.CASES[5]
    ids = ref.case_ids(case, 64)
    runs = []
    for _ in range(2):
        model, m = _fresh(tmp, case)
        runs.append((model, _step(model, case, ids, 17)))
    a, b = runs[0][1]["d"], runs[1][1]["d"]
    assert a["tag"] == b["tag"] == 1 and a["id"] == b["id"] and a["epoch"] == b["epoch"]
    for li in range(2):
        for s in ref.STAGES:
            _same_bits(a["vals"][li][s], b["vals"][li][s], (li, s))
            np.testing.assert_array_equal(a["tags"][li][s], b["tags"][li][s])
    _same_bits(a["lm_val"], b["lm_val"], "lm values")
    np.testing.assert_array_equal(a["lm_idx"], b["lm_idx"])
    model = runs[0][0]
    other = (int(ids[0, 18]) + 7) % case.VS
    r = _step(model, case, ids, 18, token=other, prefilled=True)
    d = r["d"]
    assert d["tag"] == 2
    for li in range(2):
        for s in ref.STAGES:
            assert (d["tags"][li][s] == 2).all(), (li, s)
    assert (d["lm_tag"][:ref.NLM] == 2).all() and (d["lm_tag"][ref.NLM:] == 0).all()
    _check_stages(m, d, other, 18, r["before"])
    _check_exact(m, r)
    # and the ordinary path afterwards neither replays nor trusts the entry's state (the cache
    # cleared: the reference's loop never writes slot L, llama3.py:310-321, and reads what it holds)
    model.context.reset_cache()
    out = model.generate_all(ids[:, :5], 12)
    fresh, _ = _fresh(tmp, case)
    np.testing.assert_array_equal(out, fresh.generate_all(ids[:, :5], 12))


def test_check_build_records_no_violation():
    if not os.path.exists(CHECK_LIB):
        pytest.skip(f"{CHECK_LIB} missing: build it with `make -C llama3.np_amd/csrc check-lib` "
                    "(__graft_entry__.build() does)")
    env = dict(os.environ, L3_LIB_PATH=CHECK_LIB)
    r = subprocess.run([sys.executable, os.path.join(HERE, "decode_persist_checks_workload.py")], env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["enabled"] is True
    assert out["workload"] == {"kv_slot": 0, "attn_keys": 0, "token_id": 0}
    assert out["groups"] == ["first_slot", "last_slot", "two_launches", "streamed_lm"]
