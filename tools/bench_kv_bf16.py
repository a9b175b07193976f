#!/usr/bin/env python3
"""A/B of the KV-cache storage (DESIGN.md "bf16 KV-cache storage"): an fp32 context against a
``kv_dtype="bf16"`` one, through Llama.generate_ragged at the Llama-3 head shape (HD 128, four
query heads per KV head, dim 4096) with a few layers and a small vocabulary so a run stays short
(tools/bench_ragged_split.py's model).

Per (context, batch) both models prefill the rows once, all but each row's last token; every
timed call then continues from there (``start_pos``), so no call repeats the prefill.  Row 0, the
shortest, runs exactly `--steps` decode steps that end at the context; row b is 2 * b tokens
longer.  Per (storage, kernel), the storages alternating inside every repetition of one process:
  ms/step   host clock around generate_ragged (it ends in a device synchronise) for a call of
            `--steps` decode steps minus a call of none (the same one-token extend), over the steps;
  attn ms   HIP events around the L3_K_ATTN launches of the decode steps (the split form's two
            launches are one entry), taken in calls of their own with kernel timing on: the long
            call's total minus the short call's, over the difference of the counts.
The kernels: split-KV forced at `--chunk`, and the single-pass kernel at contexts up to
`--single-max`.  Then one extend_ragged of a `--extend`-token chunk per row at the start that ends at
4096 (where the cache has 4096 slots): host ms per call and attn ms per entry.  Medians over the
repetitions with the min and max; kv_info bytes per context.  Prints a table and one JSON line;
--out writes both."""

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


def fmt(s):
    return f"{s['median']:>9.4f} [{s['min']:.4f} .. {s['max']:.4f}]"


def timed(fn, model):
    model.context.synchronize()
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def attn_stats(fn, model):
    ctx = model.context
    ctx.kernel_timing(True, ["attn"])  # resets the counters
    fn()
    ms, cnt = ctx.kernel_stats()["attn"]
    ctx.kernel_timing(False)
    return ms, cnt


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--vocab", type=int, default=8192)
    ap.add_argument("--contexts", default="2048,4096,8192")
    ap.add_argument("--single-max", type=int, default=2048, help="contexts up to this also run the single-pass kernel")
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--extend", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    batches = [int(x) for x in a.batches.split(",")]
    contexts = [int(x) for x in a.contexts.split(",")]
    args = ModelArgs(dim=4096, n_layers=a.layers, n_heads=32, n_kv_heads=8, vocab_size=a.vocab,
                     max_seq_len=max(contexts), max_batch_size=max(batches))
    w = synth.pool_weights(args, synth.LLAMA3_HIDDEN, seed=1, pool_floats=1 << 26)
    models = {"fp32": llama3.Llama(w, args, device=a.device),
              "bf16": llama3.Llama(w, args, device=a.device, kv_dtype="bf16")}
    rng = np.random.default_rng(2)
    result = {"source_hash": l3hip.lib().l3_source_hash().decode(), "layers": a.layers, "vocab": a.vocab,
              "hidden": synth.LLAMA3_HIDDEN, "steps": a.steps, "reps": a.reps, "max_seq_len": max(contexts),
              "max_batch_size": max(batches), "kv_bytes": {k: m.context.kv_info()["bytes"] for k, m in models.items()},
              "runs": [], "extends": []}
    lines = [f"KV-cache storage A/B: dim 4096, HD 128, n_rep 4, {a.layers} layers, hidden {synth.LLAMA3_HIDDEN}, "
             f"vocab {a.vocab}; caches of {max(batches)} rows x {max(contexts)} slots: "
             + ", ".join(f"{k} {v} bytes" for k, v in result["kv_bytes"].items())
             + f"; {a.steps} decode steps per call, medians of {a.reps} [min .. max]; library {result['source_hash']}",
             f"{'context':>7} {'B':>2} {'kernel':<12} {'kv':<5} {'ms/step':>28} {'attn ms/entry':>30}  ids"]
    for context in contexts:
        kernels = [(f"split {a.chunk}", 1)] + ([("single-pass", 0)] if context <= a.single_max else [])
        for B in batches:
            assert 2 * (B - 1) < a.steps
            base = context - a.steps - 1
            prompts = [rng.integers(0, a.vocab, base + 2 * b) for b in range(B)]
            starts = [p.size - 1 for p in prompts]
            last = [p[-1:] for p in prompts]
            short = min(p.size for p in prompts) + 1  # the extend's token only: no decode step
            for m in models.values():
                m.context.reset_cache()
                m.forward_ragged([p[:-1] for p in prompts])
            step = {(k, s): [] for k, _ in kernels for s in models}
            attn = {(k, s): [] for k, _ in kernels for s in models}
            ids = {}
            for rep in range(a.warmup + a.reps):
                for kname, mode in kernels:
                    for sname, m in models.items():  # alternate the storages inside the repetition
                        m.context.set_ragged_attn_split(mode, a.chunk)
                        t0, _ = timed(lambda: m.generate_ragged(last, short, start_pos=starts), m)
                        t1, rows = timed(lambda: m.generate_ragged(last, context, start_pos=starts), m)
                        ms0, n0 = attn_stats(lambda: m.generate_ragged(last, short, start_pos=starts), m)
                        ms1, n1 = attn_stats(lambda: m.generate_ragged(last, context, start_pos=starts), m)
                        ids[(kname, sname)] = rows
                        if rep >= a.warmup:
                            step[(kname, sname)].append((t1 - t0) / a.steps)
                            attn[(kname, sname)].append((ms1 - ms0) / max(1, n1 - n0))
            for kname, _ in kernels:
                for sname in models:
                    key = (kname, sname)
                    same = all(np.array_equal(x, y) for x, y in zip(ids[key], ids[(kernels[0][0], sname)]))
                    v = {"step_ms": med(step[key]), "attn_ms": med(attn[key]), "ids_equal_split": same}
                    lines.append(f"{context:>7} {B:>2} {kname:<12} {sname:<5} {fmt(v['step_ms'])} {fmt(v['attn_ms']):>30}  "
                                 f"{'same' if same else 'DIFFER'}")
                    print(lines[-1], flush=True)
                    result["runs"].append({"context": context, "B": B, "kernel": kname, "kv": sname, **v})
            if context == 4096 and a.extend:  # slots [0, 4032) hold the prefill; the chunk ends at slot 4095
                chunks = [rng.integers(0, a.vocab, a.extend) for _ in range(B)]
                at = [context - a.extend] * B
                host = {s: [] for s in models}
                ev = {s: [] for s in models}
                for rep in range(a.warmup + a.reps):
                    for sname, m in models.items():
                        t, _ = timed(lambda: m.extend_ragged(chunks, at), m)
                        ms, n = attn_stats(lambda: m.extend_ragged(chunks, at), m)
                        if rep >= a.warmup:
                            host[sname].append(t)
                            ev[sname].append(ms / max(1, n))
                for sname in models:
                    v = {"call_ms": med(host[sname]), "attn_ms": med(ev[sname])}
                    lines.append(f"{context:>7} {B:>2} {'extend ' + str(a.extend):<12} {sname:<5} {fmt(v['call_ms'])} "
                                 f"{fmt(v['attn_ms']):>30}  (ms/call)")
                    print(lines[-1], flush=True)
                    result["extends"].append({"start": at[0], "len": a.extend, "B": B, "kv": sname, **v})
    text = "\n".join(lines) + "\n" + json.dumps(result) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
