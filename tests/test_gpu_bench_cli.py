"""bench.py's command line on the GPU: a plain run prints the headline line only and
``--dump-outputs`` writes what the timed path computed (the last step's logits).

The benchmark is the subject here, so each test starts it once (2 timed steps, about a second).
The dumped rows are checked against the oracle on the benchmark's own seeded inputs at the
project's parity bar (1e-4 max-abs on the logits, as smoke() and tests/test_gpu_parity.py).
"""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import llama3_oracle as orc
import synth

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ["ms_per_step_median", "ms_per_step_serialized", "ms_per_step_all_rows_last_layer",
             "ms_per_step_with_logits_d2h", "roofline", "whole_step", "gemm_x6", "cpu_baseline",
             "kernel_ms"]


def _bench(*argv):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", *argv],
                       env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [x for x in p.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_plain_run_line_and_dumped_logits(tmp_path):
    d = tmp_path / "dump"
    line = _bench("--steps", "2", "--warmup", "1", "--dump-outputs", str(d))
    assert line["steps"] == 2 and line["warmup"] == 1 and line["full"] is False
    assert line["unit"] == "tokens/s" and line["higher_is_better"] is True and line["dtype"] == "fp32"
    assert line["ms_per_step"] > 0
    # value is the tokens of the timed steps over their wall time
    assert line["value"] == pytest.approx(256 * 256 / (line["ms_per_step"] * 1e-3), rel=1e-3)
    assert not [k for k in FULL_ONLY if k in line]
    assert sorted(os.listdir(d)) == ["logits.npy"]
    got = np.load(d / "logits.npy")
    assert got.dtype == np.float32 and got.shape == (256, 32000) and np.isfinite(got).all()
    # the benchmark's inputs: weights seed 0, rank 0's ids default_rng(100); rows are independent
    args = synth.stories15m(256)
    w = synth.make_weights(args, synth.STORIES15M_HIDDEN, seed=0)
    ids = np.random.default_rng(100).integers(0, args.vocab_size, (256, 256)).astype(np.int32)
    rows = [0, 255]
    want = orc.OracleModel(w, synth.stories15m(len(rows)))(ids[rows].astype(np.int64), 0)
    err = float(np.max(np.abs(got[rows].astype(np.float64) - want.reshape(len(rows), -1))))
    print(f"dumped logits vs oracle, rows {rows}: max-abs {err:.3e}")
    assert err <= 1e-4
