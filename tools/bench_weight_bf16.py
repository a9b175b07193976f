"""bf16 weight storage against fp32 on batch-1 (and batch-4) greedy decode at the Llama-3-8B shape
(DESIGN.md "bf16 weight storage").

One process, two contexts on the same synth.pool_weights mapping — fp32 (the parent's kernels,
unchanged) and weight_dtype="bf16-round" — decoding the same prompt, timed alternately:
each sample is `steps` device-loop decode steps (Llama.generate_all; the prefill and the graph
capture are paid by an untimed first call, and a sample is the time of a run of prompt + 1 + steps
tokens minus that of a run of prompt + 1 tokens, taken back to back).  Reports the median of the
samples as ms per token and the weight bytes one step streams (every projection and the lm_head
once) over that time in TB/s.

Prints one JSON line and, with --out, writes it to that file (keyed to l3_source_hash).

  python tools/bench_weight_bf16.py [--layers 32] [--steps 16] [--samples 5] [--batch 1,4] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "llama3.np_amd"))
import l3hip  # noqa: E402
import llama3  # noqa: E402
import synth  # noqa: E402

PEAK_HBM_TBS = 8.0  # HBM3E


def weight_elems(args, hidden):
    D, H, KVH = args.dim, args.n_heads, args.kv_heads
    HD = D // H
    return args.n_layers * ((H + 2 * KVH) * HD * D + D * H * HD + 3 * hidden * D) + args.vocab_size * D


def timed_run(model, prompt, total):
    model.context.reset_cache()
    t0 = time.perf_counter()
    ids = model.generate_all(prompt, total)
    return time.perf_counter() - t0, ids


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--batch", default="1")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    batches = [int(b) for b in a.batch.split(",")]
    L = 5
    args = synth.llama3_shape(n_layers=a.layers, max_batch_size=max(batches), max_seq_len=L + 2 + a.steps)
    w = synth.pool_weights(args, synth.LLAMA3_HIDDEN, seed=0)
    models = {"fp32": llama3.Llama(w, args, device=0),
              "bf16": llama3.Llama(w, args, device=0, weight_dtype="bf16-round")}
    elems = weight_elems(args, synth.LLAMA3_HIDDEN)
    info = models["bf16"].context.weight_bf16_info()
    out = {"workload": f"Llama-3-8B shape, {a.layers} layers, greedy decode, pool weights", "steps": a.steps,
           "samples": a.samples, "source_hash": l3hip.source_hash(), "bf16_copy_bytes": info["bytes"],
           "decode_persistent": {k: None for k in models}, "rows": []}
    for B in batches:
        prompt = np.random.default_rng(B).integers(0, args.vocab_size, (B, L))
        for m in models.values():  # warm-up: prefill kernels, graph capture, workspaces
            timed_run(m, prompt, L + 1 + a.steps)
        samples = {k: [] for k in models}
        for _ in range(a.samples):
            for k, m in models.items():  # alternately: drift hits both alike
                t_short, _ = timed_run(m, prompt, L + 1)
                t_long, _ = timed_run(m, prompt, L + 1 + a.steps)
                samples[k].append((t_long - t_short) / a.steps)
        row = {"B": B}
        for k, m in models.items():
            ms = float(np.median(samples[k])) * 1e3
            nbytes = elems * (2 if k == "bf16" else 4)
            row[k] = {"ms_per_token": round(ms, 4), "min_ms": round(min(samples[k]) * 1e3, 4),
                      "max_ms": round(max(samples[k]) * 1e3, 4),
                      "streamed_weight_TBs": round(nbytes / (ms * 1e-3) / 1e12, 3),
                      "hbm_frac": round(nbytes / (ms * 1e-3) / 1e12 / PEAK_HBM_TBS, 3)}
            out["decode_persistent"][k] = m.context.decode_persistent()
        row["speedup"] = round(row["fp32"]["ms_per_token"] / row["bf16"]["ms_per_token"], 3)
        out["rows"].append(row)
    out["bf16_gemv_launches"] = models["bf16"].context.weight_bf16_info()["gemv_launches"]
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
