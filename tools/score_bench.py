"""What scoring costs (DESIGN.md "Scoring"): Llama.score at the benchmark shape (stories15M,
B = 256, L = 256, VS = 32000) against the forward that runs every row through the last block
(__call__ after set_last_layer_rows(True)) and against the default forward, on one context.

Wall times are ms per call of the Python entry point (host ids in, host results out: 65 536
log-probabilities for score, 256 logits rows for the forwards), the median of --runs calls after
--warmup calls.  The scoring lm_head's own time is the HIP-event time of its L3_K_LMHEAD launches
(one per row chunk) in separate timed calls, reported as fp32 TF/s of 2 * B * L * D * VS; the
combine launches' time (L3_K_ARGMAX) beside it.

Prints one JSON line.
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


def wall_ms(fn, warmup, runs):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return {"ms": round(float(np.median(t)), 3), "min": round(min(t), 3), "max": round(max(t), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seq", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--workspace-mib", type=int, default=0, help="scoring workspace (0: the default)")
    a = ap.parse_args()
    args = synth.stories15m(a.batch)
    B, L = a.batch, min(a.seq, args.max_seq_len)
    w = synth.make_weights(args, synth.STORIES15M_HIDDEN, seed=0, preset="default")
    model = llama3.Llama(w, args, device=0, keep_host_weights=False)
    ctx = model.context
    ctx.set_score_workspace(a.workspace_mib << 20)
    ids = np.random.default_rng(0).integers(0, args.vocab_size, (B, L))
    res = {"source_hash": l3hip.source_hash(), "B": B, "L": L, "workspace_mib": a.workspace_mib or 64}
    res["forward_default"] = wall_ms(lambda: model(ids, 0), a.warmup, a.runs)
    ctx.set_last_layer_rows(True)
    res["forward_all_rows"] = wall_ms(lambda: model(ids, 0), a.warmup, a.runs)
    ctx.set_last_layer_rows(False)
    res["score"] = wall_ms(lambda: model.score(ids), a.warmup, a.runs)
    res["score_to_forward_all_rows"] = round(res["score"]["ms"] / res["forward_all_rows"]["ms"], 3)
    ctx.kernel_timing(True, ["lmhead", "argmax"])
    for _ in range(a.runs):
        model.score(ids)
    st = ctx.kernel_stats()
    ctx.kernel_timing(False)
    lm_ms = st["lmhead"][0] / a.runs
    flop = 2.0 * B * L * args.dim * args.vocab_size
    res["score_lm_head"] = {"ms": round(lm_ms, 3), "launches": st["lmhead"][1] // a.runs,
                            "tflops": round(flop / (lm_ms * 1e-3) / 1e12, 1)}
    res["score_combine"] = {"ms": round(st["argmax"][0] / a.runs, 3), "launches": st["argmax"][1] // a.runs}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
