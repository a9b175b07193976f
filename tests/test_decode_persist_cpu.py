"""tests/decode_persist_ref.py without a device: the case table reaches what DESIGN.md "Persistent
step coverage" says it reaches, the refused shapes fail the restated eligibility, the stage
references chained together are the model (oracle/llama3_oracle.py), and the lm partial indices the
GPU module may excuse stay within its cap for the committed seeds."""

import ctypes
import os
import re

import numpy as np
import pytest

import decode_persist_ref as ref
import l3hip
import llama3_oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
KERNEL = os.path.join(os.path.dirname(HERE), "llama3.np_amd", "csrc", "decode_persist.hip")


def test_instance_table_is_the_kernels():
    """The restated instance table against the kernel source's L3_PERSIST_INSTANCES, row by row."""
    with open(KERNEL) as f:
        src = f.read()
    body = src.split("#define L3_PERSIST_INSTANCES(X)")[1].split("static int ncd_of")[0]
    rows = [tuple(int(x) for x in m) for m in re.findall(r"X\((\d+), (\d+), (\d+), (\d+)\)", body)]
    assert rows == ref.INSTANCES


def test_every_instance_is_reached():
    reached = {ref.facts(c)["instance"] for c in ref.TABLE}
    assert reached == set(ref.INSTANCES)
    for c in ref.CASES:
        assert ref.persist_ok(c.D, c.H, c.KVH, c.FD, c.VS, c.Smax), c.name


def test_table_reaches_what_it_claims():
    f = {c.name: ref.facts(c) for c in ref.CASES}
    want = {"baseline": (1, 3, 16, 8), "idle_units": (1, 3, 16, 8), "one_head": (1, 3, 16, 8),
            "nrep4_stream": (1, 12, 16, 8), "hd48_small": (5, 3, 16, 8), "kr_zeroed": (5, 12, 12, 11),
            "full_fd_stream": (5, 16, 16, 4), "ncd8_bottom_stream": (8, 16, 16, 2), "nrep5_partial": (8, 12, 16, 2),
            "most_units": (8, 16, 16, 2), "nrep8": (8, 16, 16, 2), "hd64": (5, 12, 16, 8)}
    for name, inst in want.items():
        assert f[name]["instance"] == inst, name
    # streamed lm passes: rows per lm workgroup, passes, passes past the ones held in registers
    assert (f["nrep4_stream"]["lm_rows"], f["nrep4_stream"]["lm_passes"], f["nrep4_stream"]["streamed"]) == (129, 9, 1)
    assert (f["full_fd_stream"]["lm_rows"], f["full_fd_stream"]["lm_passes"], f["full_fd_stream"]["streamed"]) == (65, 5, 1)
    assert (f["ncd8_bottom_stream"]["lm_rows"], f["ncd8_bottom_stream"]["lm_passes"],
            f["ncd8_bottom_stream"]["streamed"]) == (34, 3, 1)
    assert [n for n, v in f.items() if v["streamed"]] == ["nrep4_stream", "full_fd_stream", "ncd8_bottom_stream"]
    # the D4 < KPF branch: every head dim below 4 KPF
    assert f["kr_zeroed"]["kr_zeroed"] and f["kr_zeroed"]["HD"] == 16 and f["kr_zeroed"]["instance"][2] == 12
    assert not f["hd64"]["kr_zeroed"] and not f["nrep8"]["kr_zeroed"]
    # empty lm workgroups and idle layer workgroups
    assert f["idle_units"]["empty_lm"] == 188 and f["one_head"]["empty_lm"] == 92
    assert f["baseline"]["empty_lm"] == 21  # 512 rows: 3 each on 171 workgroups
    assert f["idle_units"]["idle"] == [32, 32, 32] and f["one_head"]["idle"] == [48, 32, 32]
    assert [v["n_rep"] for v in (f["nrep4_stream"], f["kr_zeroed"], f["nrep5_partial"], f["nrep8"])] == [4, 4, 5, 8]
    # the most units per stage: 12 / 8 / 16 / 8 per layer workgroup
    c = next(c for c in ref.CASES if c.name == "most_units")
    per = lambda n: (n + ref.GL - 1) // ref.GL  # noqa: E731
    assert (per(3 * c.D // 2), per(c.D), per(c.FD), per(c.D)) == (12, 8, 16, 8)
    # positions: every case the first and the last slot; the key groups' edges; keys past 256
    for c in ref.CASES:
        assert c.positions[0] in (1, 255) and c.positions[-1] == c.Smax - 1
    for i in (0, 5, 8):
        assert set(ref.CASES[i].positions) >= {15, 16, 17, 31}
    assert [ref.CASES[i].name for i in (0, 5, 7)] == [c.name for c in ref.FORM_CASES]


def test_refused_shapes_fail_the_eligibility():
    for (D, H, KVH, FD), _ in ref.REFUSED:
        assert not ref.persist_ok(D, H, KVH, FD, 512), (D, H, KVH, FD)
        assert D % H == 0 and (D // H) % 16 == 0 and D % 32 == 0 and FD % 32 == 0  # the context itself takes them


def test_binding_layout():
    assert ctypes.sizeof(l3hip.DecodePersistOp) == 4 * 4 + 6 * 8 + 6 * 4 + 8 * 4
    assert l3hip.DecodePersistOp.state.offset == 16 and l3hip.DecodePersistOp.route.offset == 88
    op = l3hip.DecodePersistOp()
    assert l3hip.lib().l3_op_decode_persist_host(None, ctypes.byref(op)) != 0


@pytest.mark.parametrize("case", [ref.CASES[0], ref.CASES[5], ref.CASES[4]], ids=lambda c: c.name)
def test_stage_chain_is_the_model(case):
    """Prefill of 9 tokens on the oracle in float64, then one step at position 9: the chained
    stage references give the oracle's logits to 1e-10 and its new cache rows."""
    args, w = ref.case_weights(case)
    w64 = {k: np.asarray(v, np.float64) for k, v in w.items()}
    o = orc.OracleModel(w64, args)
    ids = ref.case_ids(case, 10)
    o(ids[:, :9], 0)
    caches = [(L.cache_k[0].transpose(1, 0, 2).copy(), L.cache_v[0].transpose(1, 0, 2).copy()) for L in o.layers]
    want = o(ids[:, 9:10], 9)[0, 0]
    m = ref.Model(args, w, case.FD, exact_rope=True)
    got, new = m.chain(int(ids[0, 9]), 9, caches)
    assert np.abs(got - want).max() <= 1e-10 * max(1.0, np.abs(want).max())
    for li, L in enumerate(o.layers):
        assert np.abs(new[li][0] - L.cache_k[0, 9]).max() <= 1e-10
        assert np.abs(new[li][1] - L.cache_v[0, 9]).max() <= 1e-10


def test_lm_partials_rules():
    logits = np.array([1.0, 3.0, 3.0, 2.0, -1.0, 0.5, 0.25], np.float64)
    val, idx, margin, bnd = ref.lm_partials(logits, np.full(7, 0.5), nlm=5)  # 2 rows each: 4 ranges, 1 empty
    assert idx.tolist() == [1, 2, 5, 6, ref.EMPTY[1]] and val[:4].tolist() == [3.0, 3.0, 0.5, 0.25] and val[4] == -np.inf
    assert margin[:3].tolist() == [2.0, 1.0, 1.5] and margin[3] == np.inf
    assert ref.final_pick(val, idx) == (1, 3.0)


@pytest.mark.parametrize("case", ref.TABLE, ids=lambda c: c.name)
def test_under_margin_share_stays_within_the_cap(case):
    """The GPU module excuses an lm partial's index where the reference's top-2 margin inside the
    workgroup's range is within twice the logit bound, for at most 2 % of the partials: here, on
    the reference alone (a chained step at position 9), that share for every committed seed."""
    args, w = ref.case_weights(case)
    m = ref.Model(args, w, case.FD)
    ids = ref.case_ids(case, 10)
    zeros = np.zeros((case.KVH, 9, m.HD))
    h = m.emb[int(ids[0, 9])]
    for li in range(2):  # (an empty history changes the hidden state, not the logits' scale or bound)
        qkv, _ = m.stage_a(li, h, 9)
        h1, _ = m.stage_c(li, m.stage_b(qkv, zeros, zeros, 9), h)
        h, _ = m.stage_e(li, m.stage_d(li, h1)[0], h1)
    z, b = m.logits(h)
    _, idx, margin, bnd = ref.lm_partials(z, b)
    live = idx != ref.EMPTY[1]
    share = float((margin[live] <= 2 * bnd[live]).mean())
    print(f"{case.name}: under-margin lm partials {share:.4f}, worst logit bound {b.max():.2e}")
    assert share <= 0.02
