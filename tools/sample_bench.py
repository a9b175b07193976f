"""What sampling costs (DESIGN.md "Sampling"): the sample kernel against the argmax launch it
replaces, and the stories15M batch-1 decode step with sampling on against the two greedy paths.

Kernel times are HIP-event times of the L3_K_ARGMAX launch of eager decode steps
(l3_kernel_timing / l3_kernel_stats), on a one-layer model of the vocabulary under test so the
logits rows are real lm_head output: rows x n = 1 x 32000, 256 x 32000, 8 x 128256, sampling off
(the argmax launch of the greedy step: from the lm_head's partials at one row, argmax_kernel over
the rows otherwise; --full-row-argmax sets L3_LM_AMAX=0 so one row runs argmax_kernel too) and
on (T 0.8, top_p 0.9; and T 0.7, top_k 40, top_p 0.95).  Each figure is the median of 5 blocks
of 40 steps after 20 warm-up steps.

Decode: ms per step of Llama.generate_all (150 tokens, median of 7 runs after a warm-up run),
sampled / greedy with L3_DECODE_PERSIST=0 (the same graph of kernels, argmax in place of the
sample kernel) / greedy by default (the persistent step).

Prints one JSON line.
"""
import json
import os
import sys
import time

import numpy as np

if "--full-row-argmax" in sys.argv:
    os.environ["L3_LM_AMAX"] = "0"

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "llama3.np_amd"))
import l3hip  # noqa: E402
import llama3  # noqa: E402
import synth  # noqa: E402
from config import ModelArgs  # noqa: E402

SAMPLINGS = {"argmax": None, "sample_T0.8_p0.9": (0.8, 0, 0.9), "sample_T0.7_k40_p0.95": (0.7, 40, 0.95)}


def kernel_us(rows, n):
    args = ModelArgs(dim=64, n_layers=1, n_heads=4, n_kv_heads=2, vocab_size=n, max_seq_len=256,
                     max_batch_size=rows)
    w = synth.make_weights(args, 192, seed=1, preset="sharp")
    model = llama3.Llama(w, args, device=0, keep_host_weights=False)
    ctx = model.context
    ids = np.random.default_rng(rows).integers(0, n, (rows, 1))
    out = {}
    for name, prm in SAMPLINGS.items():
        ctx.set_sampling(*(prm or (0.0, 0, 1.0)), seed=11)
        pos = 0
        blocks = []
        for blk in range(6):  # block 0: warm-up
            ctx.kernel_timing(True, ["argmax"])
            for _ in range(20 if blk == 0 else 40):
                ctx.greedy_step(ids, pos)
                pos += 1
            ms, cnt = ctx.kernel_stats()["argmax"]
            if blk:
                blocks.append(1e3 * ms / cnt)
        ctx.kernel_timing(False)
        out[name] = {"us": round(float(np.median(blocks)), 2), "min": round(min(blocks), 2), "max": round(max(blocks), 2)}
    for name in list(SAMPLINGS)[1:]:
        out[name]["ratio_to_argmax"] = round(out[name]["us"] / out["argmax"]["us"], 2)
    return out


def decode_ms(state):
    os.environ["L3_DECODE_PERSIST"] = "0" if state == "greedy_graph" else "1"
    args = synth.stories15m(1)
    w = synth.make_weights(args, synth.STORIES15M_HIDDEN, seed=0, preset="default")
    model = llama3.Llama(w, args, device=0, keep_host_weights=False)
    if state == "sampled":
        model.set_sampling(temperature=0.8, top_p=0.9, seed=5)
    prompt = np.array([[1, 76, 505, 263, 12561]])
    model.generate_all(prompt, 150)
    runs = []
    for _ in range(7):
        t0 = time.perf_counter()
        ids = model.generate_all(prompt, 150)
        runs.append((time.perf_counter() - t0) / ids.shape[1] * 1e3)
    return {"ms_per_step": round(float(np.median(runs)), 4), "min": round(min(runs), 4), "max": round(max(runs), 4),
            "persistent": model.context.decode_persistent()}


def main():
    res = {"source_hash": l3hip.source_hash(), "lm_amax": os.environ.get("L3_LM_AMAX", "1"), "kernel_us": {}}
    for rows, n in ((1, 32000), (256, 32000), (8, 128256)):
        res["kernel_us"][f"{rows}x{n}"] = kernel_us(rows, n)
    if "--full-row-argmax" not in sys.argv:
        res["stories15M_b1_decode"] = {s: decode_ms(s) for s in ("sampled", "greedy_graph", "greedy_default")}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
