"""Workload for tests/test_gpu_weight_bf16_rows.py::test_check_build_records_no_violation, run in
its own process with L3_LIB_PATH set to the device bounds-check build (libllama3hip_check.so) and
L3_DECODE_PERSIST=0: the tiny model under weight_dtype="bf16-round" with set_weight_bf16_rows(64, 0),
batched generate_all and ragged generation to the last cache slot (gemm_rows_bf16_kernel's QKV
epilogue at every position).  Prints one JSON line: the ids and the check build's counts."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (HERE, os.path.join(REPO, "oracle"), os.path.join(REPO, "llama3.np_amd")):
    sys.path.insert(0, p)
import llama3  # noqa: E402
from test_gpu_weight_bf16 import make_weights  # noqa: E402
from test_gpu_weight_bf16_rows import SHAPES  # noqa: E402


def main():
    args, hidden = SHAPES["tiny"]
    m = llama3.Llama(make_weights(args, hidden), args, device=0, weight_dtype="bf16-round")
    ctx = m.context
    ctx.set_weight_bf16_rows(64, 0)
    out = {"enabled": ctx.device_check_counts()[0]}
    prompt = np.random.default_rng(8).integers(0, args.vocab_size, (12, 5))  # Case.pB
    out["generate_all"] = m.generate_all(prompt, args.max_seq_len).tolist()
    ctx.reset_cache()
    lens = [1, 3, 7, 2, 5]
    rng = np.random.default_rng(3)
    rag = m.generate_ragged([rng.integers(0, args.vocab_size, n) for n in lens], args.max_seq_len)
    out["ragged"] = [r.tolist() for r in rag]
    out["ragged_lens"] = lens
    out["counts"] = ctx.device_check_counts()[1]
    out["launches"] = ctx.weight_bf16_rows_info()["launches"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
