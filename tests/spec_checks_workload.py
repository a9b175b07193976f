"""Workload for tests/test_gpu_spec.py, run in its own process with L3_LIB_PATH set to the device
bounds-check build (libllama3hip_check.so): speculative generation to the last cache slot — the
tiny model (HD 16, two query heads per KV head, 200 cache slots) from position 0 and continued
from per-row offsets, with no lookup, with a lookup that is right (every chunk as long as it may
be, up to the last slot) and with one that is wrong in places, at draft lengths 1, 7 and 15, with
a stop id and sampled; a one-layer HD 128 model with four query heads per KV head over 160 slots;
verify calls that end at the last slot; and the draft op at its stride edges.  Prints one JSON
line: whether the checks are compiled in, the counts after the workload, the tokens generated and
the draft tokens run and accepted."""
import dataclasses
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "llama3.np_amd"))
import l3hip  # noqa: E402
import llama3  # noqa: E402
import synth  # noqa: E402
from config import ModelArgs  # noqa: E402


def main():
    out = {}
    rng = np.random.default_rng(5)
    args = dataclasses.replace(synth.tiny(4), max_seq_len=200)
    V, S = args.vocab_size, args.max_seq_len
    m = llama3.Llama(synth.make_weights(args, synth.TINY_HIDDEN, seed=3, preset="sharp"), args)
    ctx = m.context
    out["enabled"], _ = ctx.device_check_counts()
    tokens = drafted = accepted = 0

    def run(model, prompts, max_new, **kw):
        nonlocal tokens, drafted, accepted
        spec = kw.pop("speculate")
        rows, st = model.generate_ragged_spec(prompts, max_new, speculate=spec, **kw)
        tokens += sum(r.size for r in rows)
        drafted += int(st["drafted"].sum())
        accepted += int(st["accepted"].sum())
        return rows

    prompts = [rng.integers(0, V, n) for n in (1, 3, 7, 12)]
    truth = m.generate_ragged(prompts, S)
    wrong = [np.where(np.arange(t.size) % 5 == 3, (t + 1) % V, t) for t in truth]
    for draft_len in (1, 7, 15):
        for lookup in (None, truth, wrong):
            ctx.reset_cache()
            rows = run(m, prompts, S, speculate=dict(draft_len=draft_len, ngram_max=8, lookup=lookup))
            assert all(np.array_equal(r, t) for r, t in zip(rows, truth))
    # continued from per-row offsets, with a stop id, and sampled
    first = (1, 3, 7, 12)
    ctx.reset_cache()
    m.forward_ragged([p[:n] for p, n in zip([rng.integers(0, V, 40) for _ in first], first)])
    rest = [rng.integers(0, V, n) for n in (40, 5, 1, 17)]
    rows = run(m, rest, S, start_pos=first, speculate=dict(draft_len=7))
    run(m, rest, S, start_pos=first, stop_ids=[int(rows[1][90])], speculate=dict(draft_len=7, lookup=rows))
    m.set_sampling(0.8, 40, 0.95, 9)
    run(m, rest, S, prefix=rng.integers(0, V, 33), speculate=dict(draft_len=15, lookup=rows))
    m.set_sampling(0.0)
    # verify calls whose chunks end at the last slot
    ctx.reset_cache()
    m.forward_ragged(prompts)
    m.verify_ragged([t[:S - p.size - 1] for t, p in zip(truth, prompts)], [p.size + 1 for p in prompts])
    gqa = ModelArgs(dim=512, n_layers=1, n_heads=4, n_kv_heads=1, vocab_size=1024, max_seq_len=160, max_batch_size=3)
    g = llama3.Llama(synth.make_weights(gqa, 256, seed=3, preset="sharp"), gqa)
    gp = [rng.integers(0, 1024, n) for n in (3, 30, 64)]
    gt = g.generate_ragged(gp, 160)
    for draft_len, lookup in ((4, None), (15, gt), (7, [np.where(np.arange(t.size) % 4 == 1, 0, t) for t in gt])):
        g.context.reset_cache()
        rows = run(g, gp, 160, speculate=dict(draft_len=draft_len, lookup=lookup))
        assert all(np.array_equal(r, t) for r, t in zip(rows, gt))
    op = l3hip.op_context(0)
    seqs = [rng.integers(0, 2, n) for n in (1, 2, 255, 256, 257, 1025, 4097)]
    seq = np.zeros((len(seqs), 4097), np.int32)
    for b, r in enumerate(seqs):
        seq[b, :r.size] = r
    op.op_spec_draft(seq, [r.size for r in seqs], [15] * len(seqs), 15, 8, 1)
    # one device: the counters of every context's kernels are the library's
    out["workload"] = ctx.device_check_counts()[1]
    out["tokens"] = int(tokens)
    out["drafted"] = int(drafted)
    out["accepted"] = int(accepted)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
