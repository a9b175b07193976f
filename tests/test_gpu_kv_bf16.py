"""bf16 KV-cache storage (DESIGN.md "bf16 KV-cache storage"; ``Llama(..., kv_dtype="bf16")``,
l3_create_kv / l3_kv_info / l3_cache_read_host / l3_op_attn_*_ragged_kv_host).

The device rounds keys and values it computed in fp32, so no test compares it with an independently
rounded reference (tests/kv_bf16_ref.py explains why).  Each test asks one of two questions: (A) is
every stored value a correct rounding of the oracle's unrounded value, and (B) given the cache bits
the device itself stored, is the attention right — against a reference that attends over those
bits, at the project's existing bars (1e-5 op level, 1e-4 logits, ids exact)."""

import dataclasses
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import extend_attn_ref as ext
import kv_bf16_ref as kv
import l3hip
import llama3
import llama3_oracle as orc
import split_attn_ref as dec
import synth
from test_gpu_ragged import SHAPES
from test_gpu_ragged_extend import PLANS

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHECK_LIB = os.path.join(os.path.dirname(HERE), "llama3.np_amd", "csrc", "libllama3hip_check.so")

# (HD, n_rep) at KVH = 2, Smax = 256: the project's table (tests/test_gpu_ragged_split.py)
OP_SHAPES = [(16, 2), (48, 1), (64, 8), (96, 3), (128, 4)]
KVH, SMAX = 2, 256


@pytest.fixture(scope="module")
def ctx():
    return l3hip.op_context(0)


def _bf16_caches(inp):
    """the fp32 caches of an op's inputs as bf16 bits: NaN poison becomes 0x7fc0"""
    kb, vb = kv.to_bits(inp["cache_k"]), kv.to_bits(inp["cache_v"])
    assert ((kb == kv.NAN_BITS) == np.isnan(inp["cache_k"])).all()
    return kb, vb


def _new_slot_checks(ck, cv, kb, vb, want_k, v32, b, slots):
    """row b: K of the new slots passes check A at the fp32 op test's allowance, V is the RNE of
    the fp32 value, every other slot is bit for bit what went in."""
    for g in range(KVH):
        for p in slots:
            x = want_k[g][p] if want_k[g].ndim == 2 else want_k[g]
            eps = 1e-6 * float(np.abs(x).max())
            assert kv.check_a(kv.widen(ck[b, g, p]), x, eps).all(), (b, g, p)
    keep = np.ones(SMAX, bool)
    keep[list(slots)] = False
    assert np.array_equal(ck[b][:, keep], kb[b][:, keep]) and np.array_equal(cv[b][:, keep], vb[b][:, keep]), b
    assert np.array_equal(cv[b][:, ~keep], kv.to_bits(v32)), b


# ---- 1. extend op ------------------------------------------------------------------------------

@pytest.mark.parametrize("hd,n_rep", OP_SHAPES)
def test_extend_op(ctx, hd, n_rep):
    """Measured on an MI355X (max-abs error of out against the attend-over-returned-cache reference):
      (16, 2) 4.06e-07    (48, 1) 5.63e-07    (64, 8) 8.76e-07    (96, 3) 1.16e-06    (128, 4) 1.12e-06
    The bound, 1e-5, is the fp32 op test's (tests/test_gpu_ragged_extend.py)."""
    inp = ext.make_inputs(hd, n_rep)
    kb, vb = _bf16_caches(inp)
    _, want_k, _ = ext.reference(inp)  # the unrounded fp64 k of the new slots
    out, ck, cv = ctx.op_attn_extend_ragged(inp["qkv"], kb, vb, inp["rope_cos"], inp["rope_sin"], inp["starts"],
                                            inp["lens"], inp["n_heads"])
    assert ck.dtype == np.uint16 and cv.dtype == np.uint16 and out.dtype == np.float32
    assert np.isfinite(out).all()  # no poisoned slot was read
    want = kv.attend_extend(inp, kv.widen(ck), kv.widen(cv))
    err = float(np.abs(out.astype(np.float64) - want).max())
    print(f"HD {hd} n_rep {n_rep}: max-abs over the returned cache {err:.3e}")
    assert err <= 1e-5, err
    H = inp["n_heads"]
    for b, (st, n) in enumerate(ext.PAIRS):
        assert not out[b, n:].any(), b  # the pads
        v32 = inp["qkv"][b, :n, (H + KVH) * hd:].reshape(n, KVH, hd).transpose(1, 0, 2)
        _new_slot_checks(ck, cv, kb, vb, want_k[b], v32, b, range(st, st + n))


# ---- 2. decode op ------------------------------------------------------------------------------

@pytest.mark.parametrize("split", [0, 64])
@pytest.mark.parametrize("hd,n_rep", OP_SHAPES)
def test_decode_op(ctx, hd, n_rep, split):
    """Positions 0 and 1 are where an unrounded k / v in LDS would show: the new key is one of one
    or two, so its 2^-9 relative rounding is about 1e-3 of out against the 1e-5 bar.
    Measured on an MI355X, the same in both forms:
      (16, 2) 2.60e-07    (48, 1) 1.82e-07    (64, 8) 2.68e-07    (96, 3) 3.41e-07    (128, 4) 3.09e-07"""
    inp = dec.make_inputs(hd, n_rep, KVH, SMAX, dec.POSITIONS)
    kb, vb = _bf16_caches(inp)
    _, want_k, _ = dec.reference(inp)
    out, ck, cv = ctx.op_attn_decode_ragged(inp["qkv"], kb, vb, inp["rope_cos"], inp["rope_sin"], inp["pos"],
                                            inp["finished"], inp["n_heads"], SMAX, split)
    assert ck.dtype == np.uint16 and np.isfinite(out).all()
    want = kv.attend_decode(inp, kv.widen(ck), kv.widen(cv))
    err = float(np.abs(out.astype(np.float64) - want).max())
    print(f"HD {hd} n_rep {n_rep} split {split}: max-abs over the returned cache {err:.3e}")
    assert err <= 1e-5, err
    H = inp["n_heads"]
    for b, p in enumerate(inp["pos"]):
        if inp["finished"][b]:  # zeros out, its cache untouched
            assert not out[b].any()
            assert np.array_equal(ck[b], kb[b]) and np.array_equal(cv[b], vb[b])
            continue
        v32 = inp["qkv"][b, (H + KVH) * hd:].reshape(KVH, 1, hd)
        _new_slot_checks(ck, cv, kb, vb, want_k[b], v32, b, [int(p)])


# ---- 3. one-token extend against the decode kernel ---------------------------------------------

@pytest.mark.parametrize("hd,n_rep", OP_SHAPES)
def test_one_token_extend_agrees_with_the_decode_kernel(ctx, hd, n_rep):
    """Measured on an MI355X: out within 7.7e-07 at every shape, every new K bit pattern equal (the
    bound allows one ulp on up to 1 % of the elements: the kernels' RoPE may differ in the last fp32
    bit, which moves a key that sits on a tie; the expected share is about 1e-4)."""
    inp = ext.make_inputs(hd, n_rep, lq=1, pairs=tuple((p, 1) for p in dec.POSITIONS))
    kb, vb = _bf16_caches(inp)
    out, ck, cv = ctx.op_attn_extend_ragged(inp["qkv"], kb, vb, inp["rope_cos"], inp["rope_sin"], inp["starts"],
                                            inp["lens"], inp["n_heads"])
    d_out, dk, dv = ctx.op_attn_decode_ragged(inp["qkv"][:, 0], kb, vb, inp["rope_cos"], inp["rope_sin"],
                                              inp["starts"], np.zeros(len(dec.POSITIONS), np.int32), inp["n_heads"],
                                              SMAX, 0)
    err = float(np.abs(out[:, 0] - d_out).max())
    assert np.isfinite(out).all() and err <= 1e-5, err
    assert np.array_equal(cv, dv)
    # the two kernels' RoPE may differ in the last fp32 bit, which moves a key that sits on a tie
    new = np.stack([ck[b, :, p] for b, p in enumerate(dec.POSITIONS)]).astype(np.int32)
    new_d = np.stack([dk[b, :, p] for b, p in enumerate(dec.POSITIONS)]).astype(np.int32)
    same = float((new == new_d).mean())
    print(f"HD {hd} n_rep {n_rep}: out max-abs {err:.3e}, new K bits equal {same:.5f}")
    assert np.abs(new - new_d).max() <= 1 and same >= 0.99
    old = np.ones(ck.shape, bool)
    for b, p in enumerate(dec.POSITIONS):
        old[b, :, p] = False
    assert np.array_equal(ck[old], dk[old])


# ---- 4. model level ----------------------------------------------------------------------------

class Case:
    """A model of tests/test_gpu_ragged_extend.py's PLANS twice: kv_dtype="bf16" (under test) and
    None (its deviation from the oracle sizes check A's eps)."""

    def __init__(self, name):
        self.name = name
        self.args, hidden, _, _ = SHAPES[name]
        self.lens, self.cuts, _, self.max_new = PLANS[name]
        self.w = synth.make_weights(self.args, hidden, seed=31, preset="sharp")
        self.w64 = {k: np.asarray(v, np.float64) for k, v in self.w.items()}
        self.one = dataclasses.replace(self.args, max_batch_size=1)
        rng = np.random.default_rng(7)
        self.prompts = [rng.integers(0, self.args.vocab_size, n) for n in self.lens]
        self.first = [p[:c] for p, c in zip(self.prompts, self.cuts)]
        self.second = [p[c:] for p, c in zip(self.prompts, self.cuts)]
        self.bf = llama3.Llama(self.w, self.args, device=0, kv_dtype="bf16")
        self.f32 = llama3.Llama(self.w, self.args, device=0)

    # each scenario: (per-row calls [(ids, start), ...], per-row logits or None, per-row ids)
    def forward(self, m):
        lg = m.forward_ragged(self.prompts)
        return [[(p, 0)] for p in self.prompts], lg[:, 0], [[] for _ in self.prompts]

    def extend(self, m):
        m.forward_ragged(self.first)
        lg = m.extend_ragged(self.second, self.cuts)
        calls = [[(a, 0), (b, c)] for a, b, c in zip(self.first, self.second, self.cuts)]
        return calls, lg[:, 0], [[] for _ in self.prompts]

    def generate(self, m, split=0, **kw):
        m.context.set_ragged_attn_split(1 if split else 0, split)
        ids = m.generate_ragged(self.prompts, self.max_new, **kw)  # to the last cache slot
        m.context.set_ragged_attn_split(0)
        return [[(p, 0)] for p in self.prompts], None, ids

    def audit(self, m, scenario, **kw):
        """Run the scenario on a zeroed cache, read every layer's cache back and replay each row
        alone through the forced oracle.  Per row: the device's and the oracle's own k / v at every
        written slot, the returned and the replayed logits, the ids, the steps' logits and margins."""
        m.context.reset_cache()
        calls, logits, ids = getattr(self, scenario)(m, **kw)
        S, rows = self.args.max_seq_len, []
        for b in range(len(self.prompts)):
            caches = [m.context.cache_read(l, b, 0, S) for l in range(self.args.n_layers)]
            f = kv.ForcedOracle(self.w64, self.one, caches)
            last, steps, margins = kv.replay(f, calls[b], ids[b], self.max_new)
            T = sum(len(c) for c, _ in calls[b])
            if len(ids[b]):  # the hole the loop never writes reads as +0 (bit pattern 0 widens to +0.0)
                for k, v in caches:
                    assert not k[:, T].any() and not v[:, T].any() and not np.signbit(k[:, T]).any(), (b, T)
            rows.append(dict(audit=f.audit(), got=None if logits is None else logits[b], last=last,
                             ids=np.asarray(ids[b], np.int64), steps=steps, margins=margins))
        return rows


_cases = {}


@pytest.fixture
def case(request):
    if request.param not in _cases:
        _cases[request.param] = Case(request.param)
    return _cases[request.param]


SCENARIOS = {
    "forward_ragged": ("forward", {}),
    "extend_ragged": ("extend", {}),
    "generate_ragged": ("generate", {}),
    "generate_ragged_split64": ("generate", dict(split=64)),
    "generate_ragged_spec": ("generate", dict(speculate=dict(draft_len=4))),
}


@pytest.mark.parametrize("what", list(SCENARIOS))
@pytest.mark.parametrize("case", ["tiny", "gqa"], indirect=True)
def test_model(case, what):
    """Measured on an MI355X: see DESIGN.md "bf16 KV-cache storage" (e32 per case and the largest
    excess over ulp / 2 are printed below)."""
    scenario, kw = SCENARIOS[what]
    # eps: the parent kernels' own deviation from the oracle on the same calls (fp32 cache, read
    # back), times 4 — the forced flow perturbs later layers' inputs slightly
    e32 = max(float(np.abs(r["audit"][0] - r["audit"][1]).max()) for r in case.audit(case.f32, scenario, **kw))
    eps = 4 * e32
    rows = case.audit(case.bf, scenario, **kw)
    excess = 0.0
    for b, r in enumerate(rows):
        dk, xk, dv, xv = r["audit"]
        assert dk.shape[1] == (case.lens[b] if not len(r["ids"]) else case.max_new - 1), b  # every written slot
        excess = max(excess, kv.excess_a(dk, xk), kv.excess_a(dv, xv))
        assert kv.check_a(dk, xk, eps).all() and kv.check_a(dv, xv, eps).all(), (b, eps, excess)
        # the stored values are bf16: the low 16 bits of the widened floats are zero
        assert not (dk.astype(np.float32).view(np.uint32) & 0xFFFF).any()
        if r["got"] is not None:
            err = float(np.abs(r["got"].astype(np.float64) - r["last"]).max())
            assert err <= 1e-4, (b, err)
        n = len(r["ids"])
        if n:
            assert n == case.max_new - case.lens[b]
            close = r["margins"] < 1e-3  # a near-tie the fp32 logit error may flip: not compared
            assert int(close.sum()) <= math.ceil(n / 50), (b, int(close.sum()), n)
            want = r["steps"].argmax(-1)
            assert np.array_equal(r["ids"][~close], want[~close]), (b, r["ids"], want)
    print(f"{case.name} {what}: e32 {e32:.3e}, eps {eps:.3e}, largest excess over ulp/2 {excess:.3e}")


# ---- 5. fork -----------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["tiny", "gqa"], indirect=True)
def test_forked_row_equals_its_source(case):
    m, B = case.bf, len(case.lens)
    m.context.reset_cache()
    hist, chunk = case.prompts[-1][:-3], case.prompts[-1][-3:]
    m(hist[None], 0)  # row 0
    m.fork_cache(0, [B - 1], hist.size)
    for l in range(case.args.n_layers):
        k0, v0 = m.context.cache_read(l, 0, 0, hist.size)
        k1, v1 = m.context.cache_read(l, B - 1, 0, hist.size)
        assert k0.any() and np.array_equal(k0.view(np.uint32), k1.view(np.uint32))
        assert np.array_equal(v0.view(np.uint32), v1.view(np.uint32))
        k2, _ = m.context.cache_read(l, B - 1, hist.size, 1)
        assert not k2.any()  # nothing past the forked slots
    got = np.ascontiguousarray(m.extend_ragged([chunk] * B, [hist.size] * B))
    assert np.array_equal(got[0].view(np.uint32), got[B - 1].view(np.uint32))
    assert not np.array_equal(got[0].view(np.uint32), got[1].view(np.uint32))  # row 1 has no history


# ---- 6. plumbing -------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["tiny", "gqa"], indirect=True)
def test_plumbing(case):
    m, f, a = case.bf, case.f32, case.args
    S, B = a.max_seq_len, len(case.lens)
    info, info32 = m.context.kv_info(), f.context.kv_info()
    assert info["dtype"] == "bf16" and info32["dtype"] is None
    hd, kvh = a.dim // a.n_heads, a.n_kv_heads or a.n_heads
    assert info32["bytes"] == 2 * a.n_layers * a.max_batch_size * kvh * S * hd * 4
    assert info["bytes"] * 2 == info32["bytes"]
    # reset_cache zeroes
    m.context.reset_cache()
    ids = np.stack([p[:case.lens[0]] for p in case.prompts])
    lg = m(ids, 0)
    assert m.context.cache_read(0, 0, 0, 1)[0].any()
    m.context.reset_cache()
    for l in range(a.n_layers):
        for b in range(B):
            k, v = m.context.cache_read(l, b, 0, S)
            assert not k.any() and not v.any()
    # __call__ is the ragged forward of the rows, generate / generate_all are generate_ragged
    assert lg.shape == (B, 1, a.vocab_size)
    assert np.array_equal(np.ascontiguousarray(m.forward_ragged(list(ids))).view(np.uint32),
                          np.ascontiguousarray(lg).view(np.uint32))
    m.context.reset_cache()
    rag = np.stack(m.generate_ragged(list(ids), 24))
    m.context.reset_cache()
    assert np.array_equal(m.generate_all(ids, 24), rag)
    m.context.reset_cache()
    assert np.array_equal(np.concatenate(list(m.generate(ids, 24)), axis=1), rag)
    # every fp32-cache entry point refuses, names itself and kv_dtype, and leaves the context usable
    c = m.context
    x = np.zeros((1, 2, a.dim), np.float32)
    refused = {
        "l3_forward_host": lambda: c.forward(ids, 0),
        "l3_forward_dev": lambda: c.forward_dev(0, 1, 1, 0, 0),
        "l3_score_host": lambda: c.score(ids, ids, 0),
        "l3_greedy_step_host": lambda: c.greedy_step(ids, 0),
        "l3_greedy_generate_host": lambda: c.greedy_generate(ids, 24),
        "l3_greedy_generate_values_host": lambda: c.greedy_generate(ids, 24, values=True),
        "l3_layer_forward_host": lambda: c.layer_forward(0, x, 0),
        "l3_attention_forward_host": lambda: c.attention_forward(0, x, 0),
    }
    for name, call in refused.items():
        with pytest.raises(RuntimeError, match=f"{name}: this context stores its KV cache as bf16 \\(kv_dtype\\)"):
            call()
    with pytest.raises(NotImplementedError, match="kv_dtype"):
        m.score(ids)
    with pytest.raises(NotImplementedError, match="kv_dtype"):
        m.layers[0](x, 0, None, m.freqs_cos[:2], m.freqs_sin[:2])
    with pytest.raises(NotImplementedError, match="kv_dtype"):
        m.layers[0].attention(x, 0, None, m.freqs_cos[:2], m.freqs_sin[:2])
    lib = l3hip.lib()  # a storage code no kernel has: refused by the op before anything else is looked at
    assert lib.l3_op_attn_extend_ragged_kv_host(c.handle, None, None, None, 7, None, None, None, None, 1, 1, 2, 2, 16, 8,
                                                None) != 0
    assert b"kv_dtype 7" in lib.l3_last_error()
    m.context.reset_cache()
    again = m(ids, 0)
    assert np.array_equal(np.ascontiguousarray(again).view(np.uint32), np.ascontiguousarray(lg).view(np.uint32))
    # cache_read on the fp32 context: the stored floats — ranges agree with each other, the values
    # are the oracle's keys to fp32 accuracy and are not bf16 roundings
    f.context.reset_cache()
    lg32 = f(ids, 0)
    L = ids.shape[1]
    k_all, v_all = f.context.cache_read(0, B - 1, 0, S)
    k_sub, v_sub = f.context.cache_read(0, B - 1, 1, L - 1)
    assert np.array_equal(k_all[:, 1:L].view(np.uint32), k_sub.view(np.uint32))
    assert np.array_equal(v_all[:, 1:L].view(np.uint32), v_sub.view(np.uint32))
    assert not k_all[:, L:].any()
    o = kv.ForcedOracle(case.w64, case.one, [f.context.cache_read(l, B - 1, 0, S) for l in range(a.n_layers)])
    o(ids[B - 1:], 0)
    dk, xk, _, _ = o.audit()
    assert float(np.abs(dk - xk).max()) <= 1e-4 and (dk.astype(np.float32).view(np.uint32) & 0xFFFF).any()
    for bad in ((a.n_layers, 0, 0, 1), (0, a.max_batch_size, 0, 1), (0, 0, S, 1), (0, 0, -1, 1), (0, 0, 0, S + 1)):
        with pytest.raises(RuntimeError, match="l3_cache_read_host"):
            f.context.cache_read(*bad)
    # the storage is in effect: other logits than the fp32 model's, within the quantisation's reach
    assert not np.array_equal(np.ascontiguousarray(lg).view(np.uint32), np.ascontiguousarray(lg32).view(np.uint32))
    for b in range(B):
        plain = orc.OracleModel(case.w64, case.one)(ids[b:b + 1], 0)[0, -1]
        rounded = kv.RoundingOracle(case.w64, case.one, rel=0.0)(ids[b:b + 1], 0)[0, -1]
        e_q = float(np.abs(rounded - plain).max())
        err = float(np.abs(lg[b, 0].astype(np.float64) - plain).max())
        print(f"row {b}: E_q {e_q:.3e}, bf16 model against the plain oracle {err:.3e}")
        assert err <= 2 * e_q + 1e-4, (b, err, e_q)


# ---- 7. check library --------------------------------------------------------------------------

def test_check_build_records_no_violation():
    assert os.path.exists(CHECK_LIB), f"{CHECK_LIB} missing: __graft_entry__.build() makes it"
    env = dict(os.environ, L3_LIB_PATH=CHECK_LIB)
    r = subprocess.run([sys.executable, os.path.join(HERE, "kv_bf16_checks_workload.py")], env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["enabled"] is True
    assert out["workload"] == {"kv_slot": 0, "attn_keys": 0, "token_id": 0}
    assert out["kv_dtype"] == "bf16" and out["tokens"] > 0 and out["extends"] > 0
