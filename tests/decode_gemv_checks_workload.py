"""Workload for tests/test_gpu_decode_gemv.py, run in its own process with L3_LIB_PATH set to the
device bounds-check build (libllama3hip_check.so): one case of each group of
tests/decode_gemv_ref.py — amax_part, argmax_parts, amax_rows, the O-proj partial rows, the folded
argmax and the undo slots at the last cache position — through l3_op_decode_gemm_host and its two
companions.  Prints one JSON line: whether the checks are compiled in, the counts after the
workload and the groups run."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "llama3.np_amd"))
import decode_gemv_ref as ref  # noqa: E402
import l3hip  # noqa: E402
from gemm_epi_ref import QKV, RESID, STORE, SWIGLU  # noqa: E402


def main():
    out = {"groups": []}
    op = l3hip.op_context(0)
    out["enabled"], _ = op.device_check_counts()

    case = ref.AMAX_CASES[2]
    x, w, norm_w, _, winner = ref.amax_inputs(case, ref.amax_scenarios(case)[3])
    r = op.op_decode_gemm(STORE, x, w, amax_part=True, state=l3hip.DecState(3), pos_adv=True)
    assert r["route"]["lanes_per_unit"] == case.lanes
    out["groups"].append("amax_part")

    ids = op.op_argmax_parts(r["amax_part"][:r["amax_blocks"]][None], 1, l3hip.DecState(4, 0, 8))
    assert ids[0] == winner
    name, t, (v, i) = ref.argmax_tables()[-1]
    assert op.op_argmax_parts(np.stack([t, t, t]), 0, l3hip.DecState(4, 0, 8, rows=3))[:3].tolist() == [i] * 3
    out["groups"].append("argmax_parts")

    case = next(c for c in ref.ROWS_CASES if c.M == 70 and c.N == 200 and c.force == 3)
    x, w, _ = ref.rows_inputs(case)
    r = op.op_decode_gemm(STORE, x, w, norm=case.norm, force_tiled=case.force, amax_rows=True)
    assert r["route"]["family"] == "tiled"
    out["groups"].append("amax_rows")

    for case in (c for c in ref.PARTS_CASES if c.K == 2048 and c.M == 3):
        inp = ref.parts_inputs(case)
        kw = dict(storage=case.storage, parts=inp["parts"])
        if case.epi == SWIGLU:
            r = op.op_decode_gemm(SWIGLU, inp["x"], gate_up=(inp["wg"], inp["wu"]), x_out=True, **kw)
        else:
            r = op.op_decode_gemm(RESID, inp["x"], inp["w"], c=inp["c0"], **kw)
        assert r["route"]["lanes_per_unit"] == case.lanes
    out["groups"].append("parts")

    g = ref.FOLD_GEO
    last = ref.FOLD_SMAX - 1
    cos, sin = ref.synthetic_rope(ref.FOLD_SMAX, g["HD"] // 2)
    shape = (1, g["KVH"], ref.FOLD_SMAX, g["HD"])
    for case in ref.FOLD_CASES:
        tab, w, norm_w = ref.fold_operands(case)
        name, t, (v, tok) = ref.fold_tables()[-1]
        q = dict(L=1, start_pos=last, Smax=ref.FOLD_SMAX, q_scale=0.25, rope_cos=cos, rope_sin=sin,
                 cache_k=np.zeros(shape, np.float32), cache_v=np.zeros(shape, np.float32), **g)
        kw = dict(norm=True, storage=case.storage)
        if norm_w is not None:
            kw["norm_w"] = norm_w
        r = op.op_decode_gemm(QKV, tab, w, amax_in=t, state=l3hip.DecState(last, 0, ref.FOLD_SMAX), qkv=q, kv_bak=True,
                              pos_dev=True, **kw)
        assert r["amax_ids"][0] == tok and r["route"]["lanes_per_unit"] == case.lanes
    out["groups"].append("fold")

    for case in ref.KV_CASES[:4]:
        w = ref.kv_weight(case.N, case.K)
        x = np.ones((case.B, case.K), np.float32)
        pos = ref.KV_SMAX - 1
        cos, sin = ref.synthetic_rope(ref.KV_SMAX, case.HD // 2)
        shape = (case.B, case.KVH, ref.KV_SMAX, case.HD)
        q = dict(L=1, start_pos=pos, H=case.H, KVH=case.KVH, HD=case.HD, Smax=ref.KV_SMAX, q_scale=0.25, rope_cos=cos,
                 rope_sin=sin, cache_k=np.zeros(shape, np.float32), cache_v=np.ones(shape, np.float32))
        r = op.op_decode_gemm(QKV, x, w, qkv=q, kv_bak=True, state=l3hip.DecState(pos), pos_dev=True)
        assert r["route"]["rows_per_block"] == case.rpb
        back = op.op_kv_restore(r["cache_v"], r["kv_bak"][pos % ref.KV_BAK_SLOTS, 1], pos)
        assert (back[:case.B] == 1).all()
    out["groups"].append("kv_bak")

    out["workload"] = op.device_check_counts()[1]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
