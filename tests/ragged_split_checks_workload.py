"""Workload for tests/test_gpu_ragged_split.py, run in its own process with L3_LIB_PATH set to the
device bounds-check build (libllama3hip_check.so): the split-KV decode attention forced at 64-key
chunks — the tiny model (HD 16, two query heads per KV head, 200 cache slots) run to its last slot
greedy, with a stop id, and sampled; a one-layer HD 128 model with four query heads per KV head over
160 slots; and the op-level batch with rows at every chunk boundary.  Prints one JSON line: whether
the checks are compiled in, the counts after the workload, the tokens generated and the split
launches."""
import dataclasses
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "llama3.np_amd"))
import l3hip  # noqa: E402
import llama3  # noqa: E402
import split_attn_ref as ref  # noqa: E402
import synth  # noqa: E402
from config import ModelArgs  # noqa: E402

CH = 64


def main():
    out = {}
    rng = np.random.default_rng(5)
    args = dataclasses.replace(synth.tiny(4), max_seq_len=200)
    m = llama3.Llama(synth.make_weights(args, synth.TINY_HIDDEN, seed=3, preset="sharp"), args, ragged_split=CH)
    ctx = m.context
    out["enabled"], _ = ctx.device_check_counts()
    prompts = [rng.integers(0, args.vocab_size, n) for n in (1, 3, 7, 12)]
    rows = m.generate_ragged(prompts, args.max_seq_len)
    tokens = sum(r.size for r in rows)
    ctx.reset_cache()
    tokens += sum(r.size for r in m.generate_ragged(prompts, args.max_seq_len, stop_ids=[int(rows[1][90])]))
    ctx.reset_cache()
    m.set_sampling(0.8, 40, 0.95, 9)
    tokens += sum(r.size for r in m.generate_ragged(prompts, args.max_seq_len))
    launches = ctx.ragged_attn_info()["split_launches"]
    gqa = ModelArgs(dim=512, n_layers=1, n_heads=4, n_kv_heads=1, vocab_size=1024, max_seq_len=160, max_batch_size=3)
    g = llama3.Llama(synth.make_weights(gqa, 256, seed=3, preset="sharp"), gqa, ragged_split=CH)
    tokens += sum(r.size for r in g.generate_ragged([rng.integers(0, 1024, n) for n in (3, 30, 64)], 160))
    launches += g.context.ragged_attn_info()["split_launches"]
    op = l3hip.op_context(0)
    for hd, n_rep in ((16, 2), (128, 4)):
        inp = ref.make_inputs(hd, n_rep, 2, 256, ref.POSITIONS)
        got, _, _ = op.op_attn_decode_ragged(inp["qkv"], inp["cache_k"], inp["cache_v"], inp["rope_cos"],
                                             inp["rope_sin"], inp["pos"], inp["finished"], inp["n_heads"], 256, CH)
        assert np.isfinite(got).all()
    launches += op.ragged_attn_info()["split_launches"]
    # one device: the counters of every context's kernels are the library's
    out["workload"] = ctx.device_check_counts()[1]
    out["tokens"] = int(tokens)
    out["split_launches"] = int(launches)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
