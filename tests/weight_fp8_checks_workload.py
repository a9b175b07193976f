"""Workload for tests/test_gpu_weight_fp8.py::test_check_build_records_no_violation, run in its own
process with L3_LIB_PATH set to the device bounds-check build (libllama3hip_check.so) and
L3_DECODE_PERSIST=0: the tiny model under weight_dtype="fp8-e4m3-round" with
set_weight_bf16_rows(64, 0), batched and one-row generate_all and ragged generation to the last cache slot (the
fp8 forms' QKV epilogues at every position).  Prints one JSON line: the ids and the check build's
counts."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (HERE, os.path.join(REPO, "oracle"), os.path.join(REPO, "llama3.np_amd")):
    sys.path.insert(0, p)
import llama3  # noqa: E402
from test_gpu_weight_fp8 import Case  # noqa: E402


def main():
    c = Case("tiny", build=False)
    m = llama3.Llama(c.w, c.args, device=0, weight_dtype="fp8-e4m3-round")
    ctx = m.context
    ctx.set_weight_bf16_rows(64, 0)
    out = {"enabled": ctx.device_check_counts()[0]}
    out["generate_all"] = m.generate_all(c.pB, c.args.max_seq_len).tolist()
    ctx.reset_cache()
    out["generate_b1"] = m.generate_all(c.p5, c.args.max_seq_len).tolist()  # the GEMV's fp8 form, captured
    ctx.reset_cache()
    out["ragged"] = [r.tolist() for r in m.generate_ragged(c.rag, c.args.max_seq_len)]
    out["counts"] = ctx.device_check_counts()[1]
    info = ctx.weight_fp8_info()
    out["rows_launches"], out["gemv_launches"] = info["rows_launches"], info["gemv_launches"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
