#!/usr/bin/env python3
"""A/B of ragged continuation (DESIGN.md "Ragged continuation") at the Llama-3 head shape (HD 128,
four query heads per KV head, dim 4096) with a few layers and a small vocabulary so a run stays
short.

Part 1, per (history, batch): a `--chunk`-token chunk per row appended to rows whose caches hold
histories of about `history` tokens (row b three tokens shorter than row b - 1),
  extend    Llama.extend_ragged(chunks, start_pos) on the caches a prefill left (the prefill is not
            timed; the extend rewrites the same slots every repetition),
  forward   Llama.forward_ragged(history + chunk): the whole history again, the only route without
            this feature.
Part 2, a `--prefix`-token prefix shared by the rows of a batch, short per-row suffixes, `--steps`
decode steps:
  prefix=   Llama.generate_ragged(suffixes, n, prefix=p): one prefill of the prefix, a fork, an extend,
  plain     Llama.generate_ragged(prefix + suffix, n): the prefix prefilled on every row.
Host clock around each call (every call ends in a device synchronise); the configurations alternate
inside every repetition of one process; medians over the repetitions with the min and max.  Prints
a table and one JSON line; --out writes both."""

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
    model.context.synchronize()
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def fmt(v):
    return f"{v['median']:>10.3f} [{v['min']:.3f} .. {v['max']:.3f}]"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--vocab", type=int, default=8192)
    ap.add_argument("--histories", default="1024,4096")
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--prefix", type=int, default=1024)
    ap.add_argument("--prefix-batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    histories = [int(x) for x in a.histories.split(",")]
    batches = [int(x) for x in a.batches.split(",")]
    smax = max(max(histories) + a.chunk, a.prefix + 64 + a.steps)
    args = ModelArgs(dim=4096, n_layers=a.layers, n_heads=32, n_kv_heads=8, vocab_size=a.vocab, max_seq_len=smax,
                     max_batch_size=max(max(batches), a.prefix_batch))
    w = synth.pool_weights(args, synth.LLAMA3_HIDDEN, seed=1, pool_floats=1 << 26)
    model = llama3.Llama(w, args, device=a.device)
    rng = np.random.default_rng(2)
    result = {"source_hash": l3hip.lib().l3_source_hash().decode(), "layers": a.layers, "vocab": a.vocab,
              "hidden": synth.LLAMA3_HIDDEN, "chunk": a.chunk, "reps": a.reps, "extend": [], "prefix": []}
    lines = [f"ragged continuation A/B: dim 4096, HD 128, n_rep 4, {a.layers} layers, hidden {synth.LLAMA3_HIDDEN}, "
             f"vocab {a.vocab}; ms per call, medians of {a.reps} [min .. max]; library {result['source_hash']}",
             f"{'history':>7} {'B':>2} {'extend ' + str(a.chunk) + ' tokens':>34} {'forward history + chunk':>34}  max |dlogit|"]
    for hist in histories:
        for B in batches:
            starts = [hist - 3 * b for b in range(B)]
            past = [rng.integers(0, a.vocab, n) for n in starts]
            chunks = [rng.integers(0, a.vocab, a.chunk) for _ in range(B)]
            whole = [np.concatenate([p, c]) for p, c in zip(past, chunks)]
            t_ext, t_fwd = [], []
            for rep in range(a.warmup + a.reps):
                model.context.reset_cache()
                model.forward_ragged(past)
                te, le = clock(model, lambda: np.array(model.extend_ragged(chunks, starts)))
                model.context.reset_cache()
                tf, lf = clock(model, lambda: np.array(model.forward_ragged(whole)))
                if rep >= a.warmup:
                    t_ext.append(te)
                    t_fwd.append(tf)
            diff = float(np.abs(le - lf).max())
            e, f = med(t_ext), med(t_fwd)
            lines.append(f"{hist:>7} {B:>2} {fmt(e):>34} {fmt(f):>34}  {diff:.2e}")
            print(lines[-1], flush=True)
            result["extend"].append({"history": hist, "B": B, "extend_ms": e, "forward_ms": f, "max_abs_logit_diff": diff})
    if a.prefix:
        B = a.prefix_batch
        pre = rng.integers(0, a.vocab, a.prefix)
        rest = [rng.integers(0, a.vocab, 16 + 3 * b) for b in range(B)]
        whole = [np.concatenate([pre, r]) for r in rest]
        max_new = a.prefix + min(r.size for r in rest) + a.steps
        t_pre, t_plain = [], []
        for rep in range(a.warmup + a.reps):
            model.context.reset_cache()
            tp, ip = clock(model, lambda: model.generate_ragged(rest, max_new, prefix=pre))
            model.context.reset_cache()
            tq, iq = clock(model, lambda: model.generate_ragged(whole, max_new))
            if rep >= a.warmup:
                t_pre.append(tp)
                t_plain.append(tq)
        same = all(np.array_equal(x, y) for x, y in zip(ip, iq))
        p, q = med(t_pre), med(t_plain)
        lines.append(f"shared prefix of {a.prefix} tokens, B {B}, suffixes of 16 .. {16 + 3 * (B - 1)} tokens, "
                     f"{a.steps} decode steps:")
        lines.append(f"  prefix= {fmt(p)}   plain {fmt(q)}   ids {'same' if same else 'DIFFER'}")
        print("\n".join(lines[-2:]), flush=True)
        result["prefix"].append({"prefix": a.prefix, "B": B, "steps": a.steps, "prefix_ms": p, "plain_ms": q,
                                 "ids_equal": same})
    text = "\n".join(lines) + "\n" + json.dumps(result) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
