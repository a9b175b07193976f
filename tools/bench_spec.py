#!/usr/bin/env python3
"""A/B of lookup-drafted speculative decoding (DESIGN.md "Speculative decoding") on the model of
tools/bench_ragged_extend.py: the Llama-3 head shape (HD 128, four query heads per KV head, dim
4096) with a few layers and a small vocabulary, fp32 and bf16 weight storage, B = 1 and B = 8.

Per (storage, B, draft_len), `--tokens` tokens per row after a `--prompt`-token prompt:
  plain     Llama.generate_ragged: one decode step per token (the baseline, on this tree),
  accept    generate_ragged_spec with lookup = the row's true continuation: every draft is
            accepted, the ceiling of what a chunk can confirm,
  reject    generate_ragged_spec with a lookup in which every true token is followed by wrong ones:
            a full-length draft in every iteration and none of it accepted, the price of a wasted
            chunk.
ms per emitted token = the call's host time (prefill included, every call ends in a device
synchronise) / the tokens per row.  The routes alternate inside every repetition of one process;
medians over the repetitions with the min and max.  The counters (iterations, drafted, accepted,
summed over rows) say what each route really ran.  Prints a table and one JSON line; --out writes
both."""

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


def med(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def clock(model, fn):
    model.context.reset_cache()
    model.context.synchronize()
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def fmt(v):
    return f"{v['median']:>8.3f} [{v['min']:.3f} .. {v['max']:.3f}]"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--vocab", type=int, default=8192)
    ap.add_argument("--prompt", type=int, default=16)
    ap.add_argument("--tokens", type=int, default=128)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--draft-lens", default="3,7,15")
    ap.add_argument("--storages", default="fp32,bf16-round")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    batches = [int(x) for x in a.batches.split(",")]
    draft_lens = [int(x) for x in a.draft_lens.split(",")]
    max_new = a.prompt + a.tokens
    args = ModelArgs(dim=4096, n_layers=a.layers, n_heads=32, n_kv_heads=8, vocab_size=a.vocab, max_seq_len=max_new,
                     max_batch_size=max(batches))
    w = synth.pool_weights(args, synth.LLAMA3_HIDDEN, seed=1, pool_floats=1 << 26)
    rng = np.random.default_rng(2)
    result = {"source_hash": l3hip.lib().l3_source_hash().decode(), "layers": a.layers, "vocab": a.vocab,
              "hidden": synth.LLAMA3_HIDDEN, "prompt": a.prompt, "tokens": a.tokens, "reps": a.reps, "rows": []}
    lines = [f"speculative decoding A/B: dim 4096, HD 128, n_rep 4, {a.layers} layers, hidden {synth.LLAMA3_HIDDEN}, "
             f"vocab {a.vocab}; {a.tokens} tokens per row after a {a.prompt}-token prompt; ms per emitted token, "
             f"medians of {a.reps} [min .. max]; library {result['source_hash']}",
             f"{'storage':>10} {'B':>2} {'k':>2} {'plain':>28} {'accept':>28} {'reject':>28}  "
             f"iterations / drafted / accepted (accept; reject)  break-even"]
    for storage in a.storages.split(","):
        model = llama3.Llama(w, args, device=a.device, weight_dtype=None if storage == "fp32" else storage)
        for B in batches:
            prompts = [rng.integers(0, a.vocab, a.prompt) for _ in range(B)]
            truth = model.generate_ragged(prompts, max_new)
            for k in draft_lens:
                wrong = [np.concatenate([np.concatenate([[t], np.full(k, (t + 1) % a.vocab)]) for t in row])
                         for row in truth]
                routes = {
                    "plain": lambda: (model.generate_ragged(prompts, max_new), None),
                    "accept": lambda: model.generate_ragged_spec(prompts, max_new,
                                                                 speculate=dict(draft_len=k, lookup=truth)),
                    "reject": lambda: model.generate_ragged_spec(prompts, max_new,
                                                                 speculate=dict(draft_len=k, lookup=wrong)),
                }
                times = {r: [] for r in routes}
                last = {}
                for rep in range(a.warmup + a.reps):
                    for r, fn in routes.items():
                        ms, last[r] = clock(model, fn)
                        if rep >= a.warmup:
                            times[r].append(ms / a.tokens)
                stats = {r: med(times[r]) for r in routes}
                same = {r: all(np.array_equal(x, y) for x, y in zip(last[r][0], truth)) for r in routes}
                cnt = {r: [int(last[r][1][c].sum()) for c in ("row_steps", "drafted", "accepted")]
                       for r in ("accept", "reject")}
                # an iteration costs c_it whatever it accepts and emits 1 + (accepted per iteration):
                # speculation pays when that exceeds c_it / (a plain step), c_it taken from the reject route
                it_ms = stats["reject"]["median"] * a.tokens * B / max(1, cnt["reject"][0])
                plain_ms = stats["plain"]["median"]
                need = max(0.0, it_ms / plain_ms - 1.0)  # accepted draft tokens per iteration to break even
                lines.append(f"{storage:>10} {B:>2} {k:>2} {fmt(stats['plain']):>28} {fmt(stats['accept']):>28} "
                             f"{fmt(stats['reject']):>28}  {cnt['accept']}; {cnt['reject']}  "
                             f"{need:.2f} of {k} ({100 * need / k:.0f}%)"
                             + ("" if all(same.values()) else f"  ids DIFFER {same}"))
                print(lines[-1], flush=True)
                result["rows"].append({"storage": storage, "B": B, "draft_len": k, "ms_per_token": stats,
                                       "counters": cnt, "ids_equal": same, "iteration_ms": it_ms,
                                       "break_even_accepted_per_iteration": need})
        del model
    text = "\n".join(lines) + "\n" + json.dumps(result) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
