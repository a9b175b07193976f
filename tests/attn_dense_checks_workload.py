"""Workload for tests/test_gpu_attn_dense.py, run in its own process with L3_LIB_PATH set to the
device bounds-check build (libllama3hip_check.so): the dense attention launches that end at the
last cache slot — of every (head size, n_rep) of tests/attn_dense_ref.py the prefill-table cases
with start_pos + L == Smax, the decode and fused-O cases with S == Smax, and the long-cache cases
at the last position — through l3_op_attention_host.  Prints one JSON line: whether the checks
are compiled in, the counts after the workload and the launches run."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "llama3.np_amd"))
import attn_dense_ref as ref  # noqa: E402
import l3hip  # noqa: E402


def main():
    out = {}
    op = l3hip.op_context(0)
    out["enabled"], _ = op.device_check_counts()
    cases = []
    for hd, n_rep in ref.PARAMS:
        cases += ref.prefill_cases(hd, n_rep) + ref.decode_cases(hd, n_rep) + ref.fused_cases(hd, n_rep)
    for hd, n_rep in ref.LONG_SHAPES:
        cases += ref.long_cases(hd, n_rep)
    launches = 0
    for case in cases:
        if case.start_pos + case.L != case.smax:
            continue
        inp = ref.make_inputs(case)
        got, route = op.op_attention(inp["q_s"], inp["cache_k"], inp["cache_v"], case.start_pos, inp["n_heads"],
                                     scaled=True, wo=inp.get("wo"))
        assert route == case.route, (case, route)
        assert np.isfinite(got[:-1]).all(), case
        launches += 1
    out["workload"] = op.device_check_counts()[1]
    out["launches"] = launches
    print(json.dumps(out))


if __name__ == "__main__":
    main()
