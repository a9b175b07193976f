"""The bf16 rows kernel (DESIGN.md "bf16 weight storage for 2-64 rows") against another build of the
library — the parent commit's — on batched greedy decode at the Llama-3-8B shape.

A library is chosen per process (L3_LIB_PATH), so the driver starts two worker processes of this
file, one per library, each with the same synth.pool_weights model under weight_dtype="bf16-round"
(this tree's worker with set_weight_bf16_rows(--rows, --min-bytes); the other library as it is),
and alternates them sample by sample over pipes: both stay alive for the whole session, one runs
while the other waits.  A sample is `steps` device-loop decode steps (Llama.generate_all): the time
of a run of prompt + 1 + steps tokens minus that of a run of prompt + 1 tokens, taken back to back,
after an untimed first call per batch size that pays the prefill kernels and the graph capture.
Reports, per batch size, the median of the samples as ms per step with the min and max, the ratio
of the medians, and whether the two libraries emitted the same ids.

Prints a table and one JSON line and, with --out, writes the JSON line to that file.

  python tools/bench_weight_bf16_rows.py --other-lib /path/to/parent/libllama3hip.so
      [--layers 32] [--steps 16] [--samples 5] [--batch 1,2,4,8,16,32,64] [--rows 64] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = 5  # prompt tokens


def worker(a):
    sys.path.insert(0, os.path.join(REPO, "llama3.np_amd"))
    import l3hip
    import llama3
    import synth

    batches = [int(b) for b in a.batch.split(",")]
    args = synth.llama3_shape(n_layers=a.layers, max_batch_size=max(batches), max_seq_len=L + 2 + a.steps)
    w = synth.pool_weights(args, synth.LLAMA3_HIDDEN, seed=0)
    model = llama3.Llama(w, args, device=0, weight_dtype="bf16-round")
    ctx = model.context
    has_rows = hasattr(ctx, "set_weight_bf16_rows") and hasattr(l3hip.lib(), "l3_set_weight_bf16_rows")
    if a.set_rows and not has_rows:
        raise SystemExit("this library has no l3_set_weight_bf16_rows")
    if a.set_rows:
        ctx.set_weight_bf16_rows(a.rows, a.min_bytes)

    def run(prompt, total):
        ctx.reset_cache()
        t0 = time.perf_counter()
        ids = model.generate_all(prompt, total)
        return time.perf_counter() - t0, ids

    print(json.dumps({"ready": True, "source_hash": l3hip.source_hash(),
                      "rows_info": ctx.weight_bf16_rows_info() if has_rows else None}), flush=True)
    for line in sys.stdin:
        cmd = json.loads(line)
        if cmd.get("quit"):
            break
        B = cmd["B"]
        prompt = np.random.default_rng(B).integers(0, args.vocab_size, (B, L))
        if cmd.get("warm"):
            _, ids = run(prompt, L + 1 + a.steps)
            print(json.dumps({"ids": np.asarray(ids).tolist()}), flush=True)
            continue
        t_short, _ = run(prompt, L + 1)
        t_long, _ = run(prompt, L + 1 + a.steps)
        print(json.dumps({"ms": (t_long - t_short) / a.steps * 1e3,
                          "launches": ctx.weight_bf16_rows_info()["launches"] if has_rows else 0,
                          "gemv_launches": ctx.weight_bf16_info()["gemv_launches"]}), flush=True)


class Worker:
    def __init__(self, a, lib, set_rows):
        env = dict(os.environ)
        for k in ("L3_WEIGHT_BF16", "L3_WEIGHT_BF16_ROWS", "L3_WEIGHT_BF16_MIN_BYTES"):
            env.pop(k, None)
        if lib:
            env["L3_LIB_PATH"] = os.path.abspath(lib)
        else:
            env.pop("L3_LIB_PATH", None)
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--layers", str(a.layers), "--steps", str(a.steps),
               "--batch", a.batch, "--rows", str(a.rows), "--min-bytes", str(a.min_bytes)]
        if set_rows:
            cmd.append("--set-rows")
        self.p = subprocess.Popen(cmd, env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)

    def read(self):
        line = self.p.stdout.readline()
        if not line:
            raise SystemExit(f"a worker ended early (exit status {self.p.wait()})")
        return json.loads(line)

    def ask(self, **cmd):
        self.p.stdin.write(json.dumps(cmd) + "\n")
        self.p.stdin.flush()
        return self.read()

    def close(self):
        try:
            self.p.stdin.write(json.dumps({"quit": True}) + "\n")
            self.p.stdin.flush()
        except OSError:
            pass
        self.p.wait()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--other-lib", default=None, help="the library to compare against (the parent commit's build)")
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--batch", default="1,2,4,8,16,32,64")
    ap.add_argument("--rows", type=int, default=64, help="max_rows of this tree's worker")
    ap.add_argument("--min-bytes", type=int, default=32 << 20)
    ap.add_argument("--other-set-rows", action="store_true",
                    help="the other library has the setting too and takes --rows / --min-bytes (A/B of two builds of the kernel)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--set-rows", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    if not a.other_lib or not os.path.exists(a.other_lib):
        raise SystemExit("--other-lib: the library to compare against is required")
    workers = {"other": Worker(a, a.other_lib, a.other_set_rows), "this": Worker(a, None, True)}
    try:
        ready = {k: w.read() for k, w in workers.items()}
        out = {"workload": f"Llama-3-8B shape, {a.layers} layers, bf16-round storage, greedy device-loop decode, "
                           "pool weights", "steps": a.steps, "samples": a.samples,
               "source_hash": {k: r["source_hash"] for k, r in ready.items()},
               "rows_setting": ready["this"]["rows_info"], "rows": []}
        print(f"{'B':>3} {'other ms/step':>30} {'this ms/step':>30} {'other/this':>10}  ids", flush=True)
        for B in [int(b) for b in a.batch.split(",")]:
            ids = {k: w.ask(B=B, warm=True)["ids"] for k, w in workers.items()}
            samples = {k: [] for k in workers}
            last = {}
            for _ in range(a.samples):
                for k, w in workers.items():  # alternately: drift hits both alike
                    last[k] = w.ask(B=B)
                    samples[k].append(last[k]["ms"])
            row = {"B": B, "ids_equal": ids["other"] == ids["this"]}
            for k in workers:
                row[k] = {"ms_per_step": round(float(np.median(samples[k])), 4), "min_ms": round(min(samples[k]), 4),
                          "max_ms": round(max(samples[k]), 4)}
            row["rows_launches_total"] = last["this"]["launches"]
            row["speedup"] = round(row["other"]["ms_per_step"] / row["this"]["ms_per_step"], 3)
            out["rows"].append(row)

            def fmt(r):
                return f"{r['ms_per_step']:>9.3f} [{r['min_ms']:.3f} .. {r['max_ms']:.3f}]"
            print(f"{B:>3} {fmt(row['other']):>30} {fmt(row['this']):>30} {row['speedup']:>10.3f}  "
                  f"{'equal' if row['ids_equal'] else 'DIFFER'}", flush=True)
    finally:
        for w in workers.values():
            w.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
