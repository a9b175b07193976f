"""Workload for tests/test_gpu_kv_bf16.py, run in its own process with L3_LIB_PATH set to the
device bounds-check build (libllama3hip_check.so): the bf16 KV-cache paths run to the last cache
slot — the tiny model (HD 16, two query heads per KV head, 200 cache slots) with kv_dtype="bf16"
prefilled, extended in two steps up to slot 199, generated to the end with the single-pass and the
split-KV attention and speculatively, with a forked prefix; a one-layer HD 128 model with four
query heads per KV head over 160 slots; and the op-level batches on uint16 caches.  Prints one JSON
line: whether the checks are compiled in, the counts after the workload, the storage type, the
tokens generated and the extends run."""
import dataclasses
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "llama3.np_amd"))
import extend_attn_ref as ext  # noqa: E402
import l3hip  # noqa: E402
import llama3  # noqa: E402
import split_attn_ref as dec  # noqa: E402
import synth  # noqa: E402
from config import ModelArgs  # noqa: E402
from utils import bf16_bits  # noqa: E402


def main():
    out = {}
    rng = np.random.default_rng(5)
    args = dataclasses.replace(synth.tiny(4), max_seq_len=200)
    V, S = args.vocab_size, args.max_seq_len
    m = llama3.Llama(synth.make_weights(args, synth.TINY_HIDDEN, seed=3, preset="sharp"), args, kv_dtype="bf16")
    ctx = m.context
    out["enabled"], _ = ctx.device_check_counts()
    out["kv_dtype"] = ctx.kv_info()["dtype"]
    extends = tokens = 0
    first = (1, 3, 7, 12)
    m.forward_ragged([rng.integers(0, V, n) for n in first])
    m.extend_ragged([rng.integers(0, V, 70) for _ in first], first)
    m.extend_ragged([rng.integers(0, V, S - 70 - n) for n in first], [n + 70 for n in first])  # ends at slot 199
    extends += 3
    for split in (0, 1):
        ctx.set_ragged_attn_split(split, 64)
        ctx.reset_cache()
        tokens += sum(r.size for r in m.generate_ragged([rng.integers(0, V, n) for n in (40, 5, 1, 17)], S))
        ctx.reset_cache()
        m.forward_ragged([rng.integers(0, V, n) for n in first])
        rows = m.generate_ragged([rng.integers(0, V, n) for n in (40, 5, 1, 17)], S, start_pos=first)
        tokens += sum(r.size for r in rows)
        extends += 3
    ctx.set_ragged_attn_split(0)
    pre = rng.integers(0, V, 33)
    rest = [rng.integers(0, V, n) for n in (1, 2, 9, 30)]
    tokens += sum(r.size for r in m.generate_ragged(rest, S, prefix=pre))
    tokens += sum(r.size for r in m.generate_ragged(rest, S, prefix=pre, speculate=dict(draft_len=4)))
    tokens += int(m.generate_all(rng.integers(0, V, (4, 9)), S).size)
    extends += 5
    gqa = ModelArgs(dim=512, n_layers=1, n_heads=4, n_kv_heads=1, vocab_size=1024, max_seq_len=160, max_batch_size=3)
    g = llama3.Llama(synth.make_weights(gqa, 256, seed=3, preset="sharp"), gqa, kv_dtype="bf16")
    g.forward_ragged([rng.integers(0, 1024, n) for n in (3, 30, 64)])
    g.extend_ragged([rng.integers(0, 1024, n) for n in (157, 100, 17)], (3, 30, 64))  # rows 0 and 1 end at slot 159
    g.context.reset_cache()
    tokens += sum(r.size for r in g.generate_ragged([rng.integers(0, 1024, n) for n in (20, 1, 33)], 160))
    extends += 3
    op = l3hip.op_context(0)
    for hd, n_rep in ((16, 2), (96, 3), (128, 4)):
        inp = ext.make_inputs(hd, n_rep)
        got, _, _ = op.op_attn_extend_ragged(inp["qkv"], bf16_bits(inp["cache_k"]), bf16_bits(inp["cache_v"]),
                                             inp["rope_cos"], inp["rope_sin"], inp["starts"], inp["lens"],
                                             inp["n_heads"])
        assert np.isfinite(got).all()
        inp = dec.make_inputs(hd, n_rep, 2, 256, dec.POSITIONS)
        for split in (0, 64):
            got, _, _ = op.op_attn_decode_ragged(inp["qkv"], bf16_bits(inp["cache_k"]), bf16_bits(inp["cache_v"]),
                                                 inp["rope_cos"], inp["rope_sin"], inp["pos"], inp["finished"],
                                                 inp["n_heads"], 256, split)
            assert np.isfinite(got).all()
        extends += 1
    # one device: the counters of every context's kernels are the library's
    out["workload"] = ctx.device_check_counts()[1]
    out["tokens"] = int(tokens)
    out["extends"] = int(extends)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
