"""fp8 weight storage (DESIGN.md "fp8 weight storage") against the bf16 storage of the same tree, on
batched greedy decode at the Llama-3-8B shape.

The driver starts one worker process of this file per variant, each with the same synth.pool_weights
model, and alternates them sample by sample over pipes: all stay alive for the whole session, one
runs while the others wait.  Variants:

  fp8       weight_dtype="fp8-e4m3-round", set_weight_bf16_rows(--rows, --min-bytes)
  bf16      weight_dtype="bf16-round", the same rows setting
  fp8_nt32  fp8 with L3_FP8_NT_MB=32: non-temporal loads from 32 MiB of stored codes on (the A/B of
            the threshold; the default is 64)
  fp8_off   fp8 with the rows kernel off (max_rows 0): 2+ rows on the fp32 routes of this tree, on the
            same model W_q — the ids the fp8 variant must reproduce, and the evidence for max_rows
  fp8_lpu64 fp8 with L3_GEMV_LPU=64: the GEMV at 64 lanes per unit whatever K (the A/B of the lane count)

A sample is `steps` device-loop decode steps (Llama.generate_all): the time of a run of
prompt + 1 + steps tokens minus that of a run of prompt + 1 tokens, taken back to back, after an
untimed first call per batch size that pays the prefill kernels and the graph capture.  Reports, per
batch size and variant, the median of the samples as ms per step with the min and max; bf16 / fp8
with the share of the 2x byte ceiling reached ((ratio - 1) / (2 - 1) of the step, all of whose other
work is unchanged); TB/s of stored weight bytes per step; and whether fp8 and fp8_off emitted the
same ids.

Prints a table and one JSON line and, with --out, writes the JSON line to that file.

  python tools/bench_weight_fp8.py [--variants fp8,bf16,fp8_nt32,fp8_off] [--layers 32] [--steps 16]
      [--samples 5] [--batch 1,2,4,8,16,32,64] [--rows 64] [--out FILE]
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
VARIANTS = {  # name -> (weight_dtype, rows kernel on, environment)
    "fp8": ("fp8-e4m3-round", True, {}),
    "bf16": ("bf16-round", True, {}),
    "fp8_nt32": ("fp8-e4m3-round", True, {"L3_FP8_NT_MB": "32"}),
    "fp8_off": ("fp8-e4m3-round", False, {}),
    "fp8_lpu64": ("fp8-e4m3-round", True, {"L3_GEMV_LPU": "64"}),
}


def worker(a):
    sys.path.insert(0, os.path.join(REPO, "llama3.np_amd"))
    import l3hip
    import llama3
    import synth

    dtype, rows_on, _ = VARIANTS[a.worker]
    batches = [int(b) for b in a.batch.split(",")]
    args = synth.llama3_shape(n_layers=a.layers, max_batch_size=max(batches), max_seq_len=L + 2 + a.steps)
    w = synth.pool_weights(args, synth.LLAMA3_HIDDEN, seed=0)
    model = llama3.Llama(w, args, device=0, weight_dtype=dtype)
    ctx = model.context
    ctx.set_weight_bf16_rows(a.rows if rows_on else 0, a.min_bytes)
    info = ctx.weight_fp8_info() if dtype.startswith("fp8") else ctx.weight_bf16_info()

    def run(prompt, total):
        ctx.reset_cache()
        t0 = time.perf_counter()
        ids = model.generate_all(prompt, total)
        return time.perf_counter() - t0, ids

    print(json.dumps({"ready": True, "source_hash": l3hip.source_hash(), "stored_bytes": info["bytes"],
                      "rows_info": ctx.weight_bf16_rows_info()}), flush=True)
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
        print(json.dumps({"ms": (t_long - t_short) / a.steps * 1e3}), flush=True)


class Worker:
    def __init__(self, a, name):
        env = dict(os.environ)
        for k in ("L3_WEIGHT_BF16", "L3_WEIGHT_FP8", "L3_WEIGHT_BF16_ROWS", "L3_WEIGHT_BF16_MIN_BYTES", "L3_FP8_NT_MB"):
            env.pop(k, None)
        env.update(VARIANTS[name][2])
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", name, "--layers", str(a.layers), "--steps",
               str(a.steps), "--batch", a.batch, "--rows", str(a.rows), "--min-bytes", str(a.min_bytes)]
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
    ap.add_argument("--variants", default="fp8,bf16,fp8_nt32,fp8_off")
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--batch", default="1,2,4,8,16,32,64")
    ap.add_argument("--rows", type=int, default=64, help="max_rows of the variants with the rows kernel on")
    ap.add_argument("--min-bytes", type=int, default=32 << 20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    names = a.variants.split(",")
    if any(n not in VARIANTS for n in names) or "fp8" not in names:
        raise SystemExit(f"--variants: a list of {sorted(VARIANTS)} with fp8 among them")
    workers = {n: Worker(a, n) for n in names}  # they load side by side
    try:
        ready = {k: w.read() for k, w in workers.items()}
        out = {"workload": f"Llama-3-8B shape, {a.layers} layers, greedy device-loop decode, pool weights",
               "steps": a.steps, "samples": a.samples, "source_hash": ready["fp8"]["source_hash"],
               "stored_bytes": {k: r["stored_bytes"] for k, r in ready.items()},
               "rows_setting": {k: r["rows_info"] for k, r in ready.items()}, "rows": []}
        print(f"{'B':>3} " + " ".join(f"{n + ' ms/step':>30}" for n in names) + "  bf16/fp8  ceiling  fp8 TB/s  ids", flush=True)
        for B in [int(b) for b in a.batch.split(",")]:
            ids = {k: w.ask(B=B, warm=True)["ids"] for k, w in workers.items()}
            samples = {k: [] for k in workers}
            for _ in range(a.samples):
                for k, w in workers.items():  # alternately: drift hits all alike
                    samples[k].append(w.ask(B=B)["ms"])
            row = {"B": B}
            for k in workers:
                row[k] = {"ms_per_step": round(float(np.median(samples[k])), 4), "min_ms": round(min(samples[k]), 4),
                          "max_ms": round(max(samples[k]), 4)}
            f8 = row["fp8"]["ms_per_step"]
            row["fp8_tb_per_s"] = round(out["stored_bytes"]["fp8"] / (f8 * 1e-3) / 1e12, 3)
            if "bf16" in row:
                row["bf16_over_fp8"] = round(row["bf16"]["ms_per_step"] / f8, 3)
                row["share_of_2x_ceiling"] = round(row["bf16_over_fp8"] - 1, 3)
            if "fp8_off" in row:
                row["ids_equal_fp32_routes"] = ids["fp8"] == ids["fp8_off"]
                row["fp32_routes_over_fp8"] = round(row["fp8_off"]["ms_per_step"] / f8, 3)
            out["rows"].append(row)

            def fmt(r):
                return f"{r['ms_per_step']:>9.3f} [{r['min_ms']:.3f} .. {r['max_ms']:.3f}]"
            eq = row.get("ids_equal_fp32_routes")
            print(f"{B:>3} " + " ".join(f"{fmt(row[n]):>30}" for n in names) +
                  f"  {row.get('bf16_over_fp8', 0):>8.3f} {row.get('share_of_2x_ceiling', 0):>8.3f} {row['fp8_tb_per_s']:>9.3f}"
                  f"  {'-' if eq is None else 'equal' if eq else 'DIFFER'}", flush=True)
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
