"""Workload for tests/test_gpu_ragged_attn.py, run in its own process with L3_LIB_PATH set to the
device bounds-check build (libllama3hip_check.so): of every head size, at an n_rep that rotates
through 1 .. 8, in both cache types, one random-kind batch of each form of tests/ragged_attn_ref.py
— the single-pass decode table, the three split settings, the extend table — all of which hold rows
that end in the last cache slot.  Prints one JSON line: whether the checks are compiled in, the
counts after the workload, the launches run and those the split form served."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "llama3.np_amd"))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
import l3hip  # noqa: E402
import ragged_attn_ref as ref  # noqa: E402


def main():
    out = {}
    op = l3hip.op_context(0)
    out["enabled"], _ = op.device_check_counts()
    launches = 0
    for i, hd in enumerate(ref.HDS):
        for j, kt in enumerate(ref.KTS):
            n_rep = (2 * i + 5 * j) % 8 + 1
            forms = [(ref.single_positions(hd), ref.SMAX, 0)] + [(ref.split_positions(c, s), s, c) for c, s in ref.SPLITS]
            for pos, s_cap, split in forms:
                inp = ref.decode_inputs(hd, n_rep, pos, s_cap)
                t = ref.to_bf16(inp) if kt == "bf16" else inp
                got, _, _ = op.op_attn_decode_ragged(t["qkv"], t["cache_k"], t["cache_v"], t["rope_cos"], t["rope_sin"],
                                                     t["pos"], t["finished"], t["n_heads"], s_cap, split)
                assert np.isfinite(got).all(), (hd, n_rep, kt, split)
                launches += 1
            inp = ref.extend_inputs(hd, n_rep, ref.extend_pairs(n_rep), ref.lq_of(n_rep))
            t = ref.to_bf16(inp) if kt == "bf16" else inp
            got, _, _ = op.op_attn_extend_ragged(t["qkv"], t["cache_k"], t["cache_v"], t["rope_cos"], t["rope_sin"],
                                                 t["starts"], t["lens"], t["n_heads"])
            assert np.isfinite(got).all(), (hd, n_rep, kt, "extend")
            launches += 1
    out["workload"] = op.device_check_counts()[1]
    out["launches"] = launches
    out["split_launches"] = int(op.ragged_attn_info()["split_launches"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
