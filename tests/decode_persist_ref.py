"""float64 reference of the persistent batch-1 decode step, one function per stage (test
infrastructure for tests/test_gpu_decode_persist.py and tests/test_decode_persist_cpu.py).

Written from the reference model's semantics (llama3.py:163-211 attention, :97-103 FFN, :111-114
RMSNorm, :304-320 final norm, lm_head and greedy argmax) through tests/gemm_epi_ref.py, not from the
kernel.  Each stage takes the stage before it as an argument: the GPU module passes the DEVICE's own
granules (as tests/test_gpu_scoring.py does for its reduction), so every bound is local to one
stage; `chain` passes each stage the reference's own output instead, which makes the whole a
restatement of the model that tests/test_decode_persist_cpu.py checks against oracle/llama3_oracle.py.

Stages (DESIGN.md "Persistent step coverage"): A rope(rmsnorm(hin) * w_norm @ Wqkv^T), q times
log2(e) / sqrt(HD); B base-2 softmax attention over cache rows [0, pos) and the new k, v; C hin + o @
Wo^T; D SwiGLU of the normed h1; E h1 + hid @ Wd^T; lm: per lm workgroup the argmax of rs * (h2_last
@ lm_head^T) over its row range, then the id by np.argmax's rule.

Bounds: the GEMV stages carry gemm_epi_ref's worst case K 2^-24 (|x| . |w|) through the row factor,
RoPE, SwiGLU and the residual add.  The library multiplies the norm weight into W in fp32 when the
model is finalised (one more rounding per weight: 2^-24 (|x| . |w|) on the dot product), which the
references below, taking the exact product, cover by the factor (K + 1) / K on a normed stage's bound.
"""

from collections import namedtuple

import numpy as np

import gemm_epi_ref as ger
import llama3_oracle as orc
import synth
from config import ModelArgs

U = ger.U
GL = 64            # layer workgroups
GRID = 256         # one workgroup per CU
NLM = GRID - GL    # lm workgroups
UPP = 16           # units (rows) per pass of a workgroup
KV_BAK_SLOTS = 32
EMPTY = (-np.inf, 0x7FFFFFFF)
STAGES = ("qkv", "o", "h1", "hid", "h2")

# the kernel's template instances (NCD, NCF, KPF, LMPF), in its table's order
INSTANCES = [(1, 3, 16, 8), (5, 12, 12, 11), (5, 12, 16, 8), (5, 16, 16, 4), (8, 16, 16, 2), (1, 12, 16, 8),
             (5, 3, 16, 8), (8, 12, 16, 2)]


def instance_of(D, FD, HD):
    """The instance rule restated: float4 chunks per lane of a row of D / FD floats rounded up to
    the next of (1, 5, 8) / (3, 12, 16), and the first table row with those whose KPF holds HD / 4."""
    nd, nf = (D + 63) // 64, (FD + 63) // 64
    ncd = 1 if nd <= 1 else 5 if nd <= 5 else 8 if nd <= 8 else 0
    ncf = 3 if nf <= 3 else 12 if nf <= 12 else 16 if nf <= 16 else 0
    for inst in INSTANCES:
        if inst[0] == ncd and inst[1] == ncf and HD // 4 <= inst[2]:
            return inst
    return None


def persist_ok(D, H, KVH, FD, VS, Smax=64, n_layers=2):
    """decode_persist_ok restated (the shape conditions of the persistent step)."""
    if H < 1 or D % H:
        return False
    HD = D // H
    qkvn = (H + 2 * KVH) * HD
    per = lambda n: (n + GL - 1) // GL  # noqa: E731
    return (D % 4 == 0 and FD % 4 == 0 and HD % 4 == 0 and 4 <= HD <= 64 and H <= GL and H % KVH == 0 and
            instance_of(D, FD, HD) is not None and qkvn % 2 == 0 and per(qkvn // 2) <= UPP and per(FD) <= UPP and
            per(D) <= UPP and D // 4 <= 256 and 1 <= Smax <= 8192 and VS >= 1 and n_layers >= 1)


Case = namedtuple("Case", "name D H KVH FD VS Smax seed positions")

_EDGE = (1, 15, 16, 17, 31, 63)
_LONG = (255, 256, 257, 511, 512, 519)

# DESIGN.md "Persistent step coverage": what each row reaches
CASES = [
    Case("baseline", 64, 4, 2, 192, 512, 64, 101, _EDGE),
    Case("idle_units", 32, 2, 1, 32, 4, 64, 102, (1, 63)),
    Case("one_head", 32, 1, 1, 32, 100, 64, 103, (1, 63)),
    Case("nrep4_stream", 64, 4, 1, 768, 24580, 64, 104, (1, 63)),
    Case("hd48_small", 96, 2, 2, 192, 512, 64, 105, (1, 63)),
    Case("kr_zeroed", 320, 20, 5, 768, 512, 64, 106, _EDGE),
    Case("full_fd_stream", 288, 6, 6, 1024, 12292, 64, 107, (1, 63)),
    Case("ncd8_bottom_stream", 352, 11, 11, 800, 6404, 64, 108, (1, 63)),
    Case("nrep5_partial", 480, 10, 2, 672, 512, 64, 109, _EDGE),
    Case("most_units", 512, 32, 32, 1024, 512, 64, 110, (1, 63)),
    Case("nrep8", 512, 8, 1, 1024, 512, 64, 111, (1, 63)),
    Case("hd64", 256, 4, 2, 512, 512, 64, 112, (1, 63)),
    # keys past the first 256 (max_seq_len 520, VS 512)
    Case("long_nrep4", 64, 4, 1, 768, 512, 520, 113, _LONG),
    Case("long_hd48", 96, 2, 2, 192, 512, 520, 114, _LONG),
    Case("long_nrep8", 512, 8, 1, 1024, 512, 520, 115, _LONG),
]
TABLE = CASES[:12]
FORM_CASES = [CASES[0], CASES[5], CASES[7]]  # the first, sixth and eighth rows

# (D, H, KVH, FD): refused, with the words the entry's error carries
REFUSED = [
    ((64, 4, 2, 1024), "no persistent instance for dim 64 with hidden_dim 1024"),
    ((352, 11, 11, 192), "no persistent instance for dim 352 with hidden_dim 192"),
    ((544, 17, 17, 192), "dim 544 has no persistent instance"),
    ((64, 4, 2, 1056), "hidden_dim 1056 has no persistent instance"),
    ((192, 2, 2, 192), "head_dim 96 exceeds"),
]


def case_args(case, Smax=None):
    return ModelArgs(dim=case.D, n_layers=2, n_heads=case.H, n_kv_heads=case.KVH, vocab_size=case.VS,
                     max_seq_len=Smax or case.Smax, max_batch_size=1)


def case_weights(case, Smax=None):
    """synth's sharp preset with all three kinds of norm weight redrawn in [0.5, 1.5] (synth's are
    ones, under which a wrong fold of the norm into the projection would not show)."""
    args = case_args(case, Smax)
    w = synth.make_weights(args, case.FD, seed=case.seed, preset="sharp")
    rng = np.random.default_rng(1000 + case.seed)
    for k in sorted(w):
        if k.endswith("layernorm.weight") or k == "model.norm.weight":
            w[k] = rng.uniform(0.5, 1.5, w[k].shape).astype(np.float32)
    return args, w


def case_ids(case, n):
    return np.random.default_rng(2000 + case.seed).integers(0, case.VS, (1, n))


def facts(case):
    """What the shape makes the kernel do (asserted by the CPU module, so the table keeps reaching it)."""
    HD = case.D // case.H
    inst = instance_of(case.D, case.FD, HD)
    per = (case.VS + NLM - 1) // NLM
    passes = (per + UPP - 1) // UPP
    qkvn = (case.H + 2 * case.KVH) * HD
    return dict(instance=inst, lm_rows=per, lm_passes=passes, streamed=max(0, passes - inst[3]),
                kr_zeroed=HD // 4 < inst[2], empty_lm=NLM - (case.VS + per - 1) // per,
                idle=[n for n in (qkvn // 2, case.D, case.FD) if n < GL], n_rep=case.H // case.KVH, HD=HD)


class Model:
    """The weights of one case in float64, the norm weights multiplied in exactly; RoPE tables as the
    library builds them (float64 cos / sin rounded to fp32) unless `exact_rope`."""

    def __init__(self, args, w, hidden, exact_rope=False):
        self.args = args
        self.D, self.H, self.KVH, self.FD, self.VS = args.dim, args.n_heads, args.kv_heads, hidden, args.vocab_size
        self.HD = self.D // self.H
        self.qdim, self.kvdim = self.H * self.HD, self.KVH * self.HD
        self.eps = args.norm_eps
        q = 1.4426950408889634 / np.sqrt(float(self.HD))
        self.q_scale = q if exact_rope else float(np.float32(q))
        cos, sin = orc.rope_tables(self.HD, args.max_seq_len)
        if not exact_rope:
            cos, sin = cos.astype(np.float32), sin.astype(np.float32)
        self.cos, self.sin = cos.astype(np.float64), sin.astype(np.float64)
        f = lambda k: np.asarray(w[k], np.float64)  # noqa: E731
        self.emb = f("model.embed_tokens.weight")
        self.layers = []
        for i in range(args.n_layers):
            p = f"model.layers.{i}."
            na, nf = f(p + "input_layernorm.weight"), f(p + "post_attention_layernorm.weight")
            qkv = np.concatenate([f(p + "self_attn.q_proj.weight"), f(p + "self_attn.k_proj.weight"),
                                  f(p + "self_attn.v_proj.weight")])
            self.layers.append(dict(wqkv=qkv * na, wo=f(p + "self_attn.o_proj.weight"),
                                    wg=f(p + "mlp.gate_proj.weight") * nf, wu=f(p + "mlp.up_proj.weight") * nf,
                                    wd=f(p + "mlp.down_proj.weight")))
        self.lm = f("lm_head.weight") * f("model.norm.weight")

    # ---- the stages: (value, bound), 1-D float64 ------------------------------------------------
    def stage_a(self, li, hin, pos):
        """[q | k | v] granules: q rotated and scaled, k rotated, v plain."""
        x = np.asarray(hin, np.float64)[None]
        r = ger.ref_qkv(x, self.layers[li]["wqkv"], self.cos, self.sin, L=1, start_pos=pos, H=self.H, KVH=self.KVH,
                        HD=self.HD, q_scale=self.q_scale, norm=True, eps=self.eps)
        val = np.concatenate([r["q"].ravel(), r["k"].ravel(), r["v"].ravel()])
        bound = np.concatenate([r["q_bound"].ravel(), r["k_bound"].ravel(), r["v_bound"].ravel()])
        return val, bound * (self.D + 1) / self.D

    def stage_b(self, qkv, cache_k, cache_v, pos):
        """Attention of every head: qkv the stage-A granules, cache_k / cache_v [KVH, >= pos, HD] the
        rows before the step.  Scores are already in base 2 (q carries log2(e) / sqrt(HD))."""
        qkv = np.asarray(qkv, np.float64)
        q = qkv[:self.qdim].reshape(self.H, self.HD)
        kn = qkv[self.qdim:self.qdim + self.kvdim].reshape(self.KVH, self.HD)
        vn = qkv[self.qdim + self.kvdim:].reshape(self.KVH, self.HD)
        out = np.empty((self.H, self.HD))
        n_rep = self.H // self.KVH
        for h in range(self.H):
            g = h // n_rep
            keys = np.concatenate([np.asarray(cache_k[g, :pos], np.float64), kn[g][None]])
            vals = np.concatenate([np.asarray(cache_v[g, :pos], np.float64), vn[g][None]])
            s = keys @ q[h]
            p = np.exp2(s - s.max())
            out[h] = (p @ vals) / p.sum()
        return out.ravel()

    def stage_c(self, li, o, hin):
        out, b = ger.ref_resid(np.asarray(o, np.float64)[None], self.layers[li]["wo"], np.asarray(hin, np.float64)[None])
        return out[0], b[0]

    def stage_d(self, li, h1):
        L = self.layers[li]
        out, b, _ = ger.ref_swiglu(np.asarray(h1, np.float64)[None], L["wg"], L["wu"], norm=True, eps=self.eps)
        return out[0], b[0] * (self.D + 1) / self.D

    def stage_e(self, li, hid, h1):
        out, b = ger.ref_resid(np.asarray(hid, np.float64)[None], self.layers[li]["wd"], np.asarray(h1, np.float64)[None])
        return out[0], b[0]

    def logits(self, h2):
        z, b = ger.ref_store(np.asarray(h2, np.float64)[None], self.lm, norm=True, eps=self.eps)
        return z[0], b[0] * (self.D + 1) / self.D

    def chain(self, token, pos, caches):
        """One whole step on the reference's own stage outputs: (logits, per layer new k, new v)."""
        h = self.emb[token]
        new = []
        for li in range(len(self.layers)):
            qkv, _ = self.stage_a(li, h, pos)
            o = self.stage_b(qkv, caches[li][0], caches[li][1], pos)
            h1, _ = self.stage_c(li, o, h)
            hid, _ = self.stage_d(li, h1)
            h, _ = self.stage_e(li, hid, h1)
            new.append((qkv[self.qdim:self.qdim + self.kvdim].reshape(self.KVH, self.HD),
                        qkv[self.qdim + self.kvdim:].reshape(self.KVH, self.HD)))
        return self.logits(h)[0], new


def lm_ranges(VS, nlm=NLM):
    """[r0, r1) of each lm workgroup: ceil(VS / nlm) rows each, the last ones short or empty."""
    per = (VS + nlm - 1) // nlm
    return [(min(VS, i * per), min(VS, (i + 1) * per)) for i in range(nlm)]


def lm_partials(logits, bound, nlm=NLM):
    """Per lm workgroup: (value, index) by np.argmax's rule over its rows — EMPTY without rows —
    the top-2 margin inside the range (inf with one row) and the largest logit bound in it."""
    val = np.full(nlm, -np.inf)
    idx = np.full(nlm, EMPTY[1], np.int64)
    margin = np.full(nlm, np.inf)
    bnd = np.zeros(nlm)
    for i, (r0, r1) in enumerate(lm_ranges(logits.size, nlm)):
        if r1 <= r0:
            continue
        seg = logits[r0:r1]
        a = int(np.argmax(seg))
        val[i], idx[i], bnd[i] = seg[a], r0 + a, bound[r0:r1].max()
        if seg.size > 1:
            margin[i] = seg[a] - np.partition(seg, -2)[-2]
    return val, idx, margin, bnd


def final_pick(vals, idxs):
    """The step's id and value from the partials, by np.argmax's rule (first index of the maximum;
    the partials are in index order, an empty one holds -inf)."""
    a = int(np.argmax(vals))
    return int(idxs[a]), vals[a]
