"""Workload for tests/test_gpu_weight_bf16.py::test_check_build_records_no_violation, run in its
own process with L3_LIB_PATH set to the device bounds-check build (libllama3hip_check.so) and
L3_DECODE_PERSIST=0: the tiny model under weight_dtype="bf16-round", batch-1 generate and
generate_all to the last cache slot (the bf16-weight GEMV with every epilogue, the folded argmax,
kv_bak, the O-proj parts).  Prints one JSON line: the ids and the check build's counts."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (HERE, os.path.join(REPO, "oracle"), os.path.join(REPO, "llama3.np_amd")):
    sys.path.insert(0, p)
import llama3  # noqa: E402
from test_gpu_weight_bf16 import SHAPES, make_weights  # noqa: E402


def main():
    args, hidden = SHAPES["tiny"]
    m = llama3.Llama(make_weights(args, hidden), args, device=0, weight_dtype="bf16-round")
    ctx = m.context
    out = {"enabled": ctx.device_check_counts()[0]}
    prompt = np.random.default_rng(7).integers(0, args.vocab_size, (1, 5))
    out["generate"] = np.concatenate(list(m.generate(prompt, args.max_seq_len)), axis=1)[0].tolist()
    ctx.reset_cache()
    out["generate_all"] = m.generate_all(prompt, args.max_seq_len)[0].tolist()
    out["counts"] = ctx.device_check_counts()[1]
    out["persistent"] = ctx.decode_persistent()
    out["gemv_launches"] = ctx.weight_bf16_info()["gemv_launches"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
