#!/usr/bin/env python3
"""A/B of the ragged decode attention (DESIGN.md "Split-KV decode attention"): the single-pass
kernel (l3_set_ragged_attn_split mode 0, where it fits) against the split-KV form (mode 1) at
several chunk lengths, through Llama.generate_ragged at the Llama-3 head shape (HD 128, four query
heads per KV head, dim 4096) with a few layers and a small vocabulary so a run stays short.

Per (batch, configuration), alternating the configurations inside every repetition of one process:
  ms/step   host clock around generate_ragged (it ends in a device synchronise) for a call of
            `--steps` decode steps minus a call of none (the same prefill), over the steps;
  attn ms   HIP events around the L3_K_ATTN launches of the decode steps (the split form's two
            launches are one entry), taken in calls of their own with kernel timing on: the long
            call's total minus the prefill-only call's, over the difference of the counts.
Medians over the repetitions, with the min and max.  `--long` adds calls at a context the
single-pass kernel cannot take (split only).  Prints a table and one JSON line; --out writes both."""

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "llama3.np_amd"))
import l3hip  # noqa: E402
import llama3  # noqa: E402
import synth  # noqa: E402
from config import ModelArgs  # noqa: E402


def prompts_for(rng, vocab, B, context, steps):
    """B prompts of a ragged batch: row 0, the shortest, runs exactly `steps` decode steps up to
    `context`; row b is 2 * b tokens longer, so it finishes 2 * b steps earlier (a finished row's
    attention workgroups return at once)."""
    base = context - steps - 1
    assert 2 * (B - 1) < steps
    return [rng.integers(0, vocab, base + 2 * b) for b in range(B)]


def timed_call(model, prompts, max_new):
    model.context.reset_cache()
    model.context.synchronize()
    t0 = time.perf_counter()
    rows = model.generate_ragged(prompts, max_new)
    return (time.perf_counter() - t0) * 1e3, rows


def attn_stats(model, prompts, max_new):
    ctx = model.context
    ctx.kernel_timing(True, ["attn"])  # resets the counters
    ctx.reset_cache()
    model.generate_ragged(prompts, max_new)
    ms, cnt = ctx.kernel_stats()["attn"]
    ctx.kernel_timing(False)
    return ms, cnt


def med(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def measure(model, configs, prompts, context, steps, reps, warmup):
    """configs: [(label, mode, chunk)].  Returns label -> {"step_ms": ..., "attn_ms": ...}."""
    short = min(p.size for p in prompts) + 1  # the prefill's token only: no decode step
    step = {c[0]: [] for c in configs}
    attn = {c[0]: [] for c in configs}
    ids = {}
    for rep in range(warmup + reps):
        for label, mode, chunk in configs:  # alternate inside the repetition
            model.context.set_ragged_attn_split(mode, chunk)
            t_short, _ = timed_call(model, prompts, short)
            t_long, rows = timed_call(model, prompts, context)
            ms0, n0 = attn_stats(model, prompts, short)
            ms1, n1 = attn_stats(model, prompts, context)
            ids[label] = rows
            if rep >= warmup:
                step[label].append((t_long - t_short) / steps)
                attn[label].append((ms1 - ms0) / max(1, n1 - n0))
    out = {}
    first = ids[configs[0][0]]
    for label, _, _ in configs:
        same = all(np.array_equal(a, b) for a, b in zip(ids[label], first))
        out[label] = {"step_ms": med(step[label]), "attn_ms": med(attn[label]), "ids_equal_first": same}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--vocab", type=int, default=8192)
    ap.add_argument("--context", type=int, default=2048)
    ap.add_argument("--long", type=int, default=4096, help="a context past the single-pass limit (0: skip)")
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--chunks", default="128,256,512,1024")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    batches = [int(x) for x in a.batches.split(",")]
    chunks = [int(x) for x in a.chunks.split(",")]
    smax = max(a.context, a.long)
    args = ModelArgs(dim=4096, n_layers=a.layers, n_heads=32, n_kv_heads=8, vocab_size=a.vocab, max_seq_len=smax,
                     max_batch_size=max(batches))
    w = synth.pool_weights(args, synth.LLAMA3_HIDDEN, seed=1, pool_floats=1 << 26)
    model = llama3.Llama(w, args, device=a.device)
    rng = np.random.default_rng(2)
    result = {"source_hash": l3hip.lib().l3_source_hash().decode(), "layers": a.layers, "vocab": a.vocab,
              "hidden": synth.LLAMA3_HIDDEN, "steps": a.steps, "reps": a.reps, "runs": []}
    lines = [f"ragged decode attention A/B: dim 4096, HD 128, n_rep 4, {a.layers} layers, hidden "
             f"{synth.LLAMA3_HIDDEN}, vocab {a.vocab}; {a.steps} decode steps per call, medians of {a.reps} "
             f"[min .. max]; library {result['source_hash']}",
             f"{'context':>7} {'B':>2} {'kernel':<12} {'ms/step':>28} {'attn ms/launch':>30}  ids"]
    for context, configs in ((a.context, [("single-pass", 0, 0)] + [(f"split {c}", 1, c) for c in chunks]),
                             (a.long, [(f"split {c}", 0, c) for c in chunks])):
        if not context:
            continue
        for B in batches:
            prompts = prompts_for(rng, a.vocab, B, context, a.steps)
            r = measure(model, configs, prompts, context, a.steps, a.reps, a.warmup)
            for label, v in r.items():
                s, t = v["step_ms"], v["attn_ms"]
                lines.append(f"{context:>7} {B:>2} {label:<12} "
                             f"{s['median']:>9.4f} [{s['min']:.4f} .. {s['max']:.4f}] "
                             f"{t['median']:>11.4f} [{t['min']:.4f} .. {t['max']:.4f}]  "
                             f"{'same' if v['ids_equal_first'] else 'DIFFER'}")
                result["runs"].append({"context": context, "B": B, "kernel": label, **v})
            print("\n".join(lines[-len(r):]), flush=True)
    info = model.context.ragged_attn_info()
    result["split_launches"] = info["split_launches"]
    text = "\n".join(lines) + "\n" + json.dumps(result) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
