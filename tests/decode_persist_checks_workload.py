"""Workload for tests/test_gpu_decode_persist.py, run in its own process with L3_LIB_PATH set to the
device bounds-check build (libllama3hip_check.so): the persistent step through
l3_op_decode_persist_host at the first and the last cache slot, two chained launches (the second
reduces the first's partials to its token id, which the check build range-checks) and a vocabulary
whose lm workgroups stream a pass.  Prints one JSON line: whether the checks are compiled in, the
counts after the workload and the groups run."""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(ROOT, "llama3.np_amd"), os.path.join(ROOT, "oracle")]
import decode_persist_ref as ref  # noqa: E402
import l3hip  # noqa: E402
import llama3  # noqa: E402


def main():
    out = {"groups": []}
    with tempfile.TemporaryDirectory() as tmp:
        def model(case):
            args, w = ref.case_weights(case)
            path = os.path.join(tmp, case.name + ".npz")
            np.savez(path, **w)
            return llama3.Llama(path, args)

        case = ref.CASES[5]
        ids = ref.case_ids(case, case.Smax)
        m = model(case)
        ctx = m.context
        out["enabled"], _ = ctx.device_check_counts()
        for name, pos, steps in (("first_slot", 1, 1), ("last_slot", case.Smax - 1, 1), ("two_launches", case.Smax - 2, 2)):
            ctx.reset_cache()
            m(ids[:, :pos], 0)
            st = l3hip.DecState(pos, 0, case.Smax)
            d = ctx.op_decode_persist(int(ids[0, pos]), st, steps=steps, kv_bak=True)
            assert st.pos == pos + steps and d["err"] == 0 and 0 <= d["id"] < case.VS
            out["groups"].append(name)
        counts = ctx.device_check_counts()[1]

        case = ref.CASES[7]
        assert ref.facts(case)["streamed"] == 1
        ids = ref.case_ids(case, case.Smax)
        m2 = model(case)
        m2(ids[:, :9], 0)
        st = l3hip.DecState(9, 0, 16)
        d = m2.context.op_decode_persist(int(ids[0, 9]), st)
        assert st.pos == 10 and d["err"] == 0 and 0 <= d["id"] < case.VS
        out["groups"].append("streamed_lm")
        c2 = m2.context.device_check_counts()[1]
        out["workload"] = {k: counts[k] + c2[k] for k in counts}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
