"""Workload for tests/test_gpu_ragged.py, run in its own process with L3_LIB_PATH set to the
device bounds-check build (libllama3hip_check.so): ragged generates up to the last cache slot —
the tiny model (HD 16, two query heads per KV head) greedy, with a stop id, and sampled, and a
one-layer HD 128 model with four query heads per KV head.  Prints one JSON line: whether the
checks are compiled in, the counts after the workload and the tokens generated."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "llama3.np_amd"))
import llama3  # noqa: E402
import synth  # noqa: E402
from config import ModelArgs  # noqa: E402


def main():
    out = {}
    rng = np.random.default_rng(5)
    args = synth.tiny(4)
    m = llama3.Llama(synth.make_weights(args, synth.TINY_HIDDEN, seed=3, preset="sharp"), args)
    ctx = m.context
    out["enabled"], _ = ctx.device_check_counts()
    prompts = [rng.integers(0, args.vocab_size, n) for n in (1, 3, 7, 12)]
    rows = m.generate_ragged(prompts, args.max_seq_len)
    tokens = sum(r.size for r in rows)
    ctx.reset_cache()
    tokens += sum(r.size for r in m.generate_ragged(prompts, args.max_seq_len, stop_ids=[int(rows[1][20])]))
    ctx.reset_cache()
    m.set_sampling(0.8, 40, 0.95, 9)
    tokens += sum(r.size for r in m.generate_ragged(prompts, args.max_seq_len))
    m.forward_ragged(prompts)
    gqa = ModelArgs(dim=512, n_layers=1, n_heads=4, n_kv_heads=1, vocab_size=1024, max_seq_len=96, max_batch_size=3)
    g = llama3.Llama(synth.make_weights(gqa, 256, seed=3, preset="sharp"), gqa)
    tokens += sum(r.size for r in g.generate_ragged([rng.integers(0, 1024, n) for n in (3, 30, 64)], 96))
    # one device: the counters of both contexts' kernels are the library's
    out["workload"] = ctx.device_check_counts()[1]
    out["tokens"] = int(tokens)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
