"""The references of tests/kv_bf16_ref.py against a simulated device (no GPU): a rounding oracle
whose k / v carry an fp32-sized perturbation before they are rounded to bf16.  Check A must accept
it and reject wrong roundings; the forced replay must reproduce its logits; and on the plans the GPU
test generates on, every step's top-2 margin must leave room for the 1e-4 logit bar."""

import dataclasses

import numpy as np
import pytest

import kv_bf16_ref as kv
import llama3
import synth
from utils import round_bf16
from test_gpu_ragged import SHAPES
from test_gpu_ragged_extend import PLANS


class Sim:
    """One model of the GPU test's plans, each row alone on the simulated device: prefill at 0, then
    greedy to max_new_tokens with the reference's schedule."""

    def __init__(self, name):
        self.args, hidden, _, _ = SHAPES[name]
        self.lens, _, _, self.max_new = PLANS[name]
        w = synth.make_weights(self.args, hidden, seed=31, preset="sharp")
        self.w64 = {k: np.asarray(v, np.float64) for k, v in w.items()}
        self.one = dataclasses.replace(self.args, max_batch_size=1)
        rng = np.random.default_rng(7)
        self.prompts = [rng.integers(0, self.args.vocab_size, n) for n in self.lens]
        self.rows = []
        for b, p in enumerate(self.prompts):
            dev = kv.RoundingOracle(self.w64, self.one, rel=2e-6, seed=b)
            logits = [dev(p[None], 0)[0, -1]]
            ids = [int(logits[0].argmax())]
            for i, pos in enumerate(range(p.size + 1, self.max_new)):
                logits.append(dev(np.array([[ids[-1]]]), pos)[0, -1])
                ids.append(int(logits[-1].argmax()))
            self.rows.append((p, np.array(ids), np.array(logits), dev.caches()))


_sims = {}


@pytest.fixture(params=["tiny", "gqa"])
def sim(request):
    if request.param not in _sims:
        _sims[request.param] = Sim(request.param)
    return _sims[request.param]


def _forced(sim, row):
    p, ids, logits, caches = sim.rows[row]
    f = kv.ForcedOracle(sim.w64, sim.one, caches)
    last, steps, margins = kv.replay(f, [(p, 0)], ids, sim.max_new)
    return f, steps, margins


def test_helpers():
    bits = np.array([0x3F80, 0x3F81, 0xBF80, 0x0000, 0x4000], np.uint16)
    assert kv.widen(bits).tolist() == [1.0, 1.0078125, -1.0, 0.0, 2.0]
    assert kv.ulp_bf16(np.array([1.0, 1.99, 2.0, -0.75, 3e-3])).tolist() == \
        [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 2.0 ** -16]
    x = np.random.default_rng(0).standard_normal(4096).astype(np.float32)
    assert np.array_equal(kv.widen(kv.to_bits(x)).astype(np.float32), round_bf16(x))
    assert kv.check_a(kv.widen(kv.to_bits(x)), x, 0.0).all()  # RNE of the value itself: eps 0


def test_check_a_accepts_the_simulated_device(sim):
    for row in range(len(sim.rows)):
        f, _, _ = _forced(sim, row)
        dk, xk, dv, xv = f.audit()
        assert dk.shape[1] == sim.max_new - 1  # every slot but the hole
        for d, x in ((dk, xk), (dv, xv)):
            eps = 4e-6 * np.abs(x).max(axis=-1, keepdims=True)
            assert kv.check_a(d, x, eps).all(), row


def test_check_a_rejects_wrong_roundings(sim):
    f, _, _ = _forced(sim, len(sim.rows) - 1)
    dk, xk, _, _ = f.audit()
    eps = 4e-6 * np.abs(xk).max(axis=-1, keepdims=True)
    x32 = xk.astype(np.float32)
    trunc = kv.widen((x32.view(np.uint32) >> 16).astype(np.uint16))  # toward zero
    assert not kv.check_a(trunc, xk, eps).all()
    assert kv.check_a(trunc, xk, eps).mean() < 0.6  # about half the elements round up
    one_off = dk + kv.ulp_bf16(dk)
    # survivors: values that sat on a tie, and elements so small beside their row's largest that a
    # whole ulp is within eps (|x| < 2^8 eps, about 1e-3 of the largest: a few per cent of N(0, 1))
    assert kv.check_a(one_off, xk, eps).mean() < 0.05
    shifted = np.roll(dk, 1, axis=1)  # every slot holds its neighbour's key
    assert kv.check_a(shifted, xk, eps).mean() < 0.1


def test_forced_replay_reproduces_the_device_and_margins_leave_room(sim):
    for row, (p, ids, logits, _) in enumerate(sim.rows):
        _, steps, margins = _forced(sim, row)
        assert steps.shape == logits.shape
        err = float(np.abs(steps - logits).max())
        assert err <= 1e-9, (row, err)
        assert np.array_equal(steps.argmax(-1), ids)
        print(f"row {row}: smallest top-2 margin {margins.min():.3e}")
        assert margins.min() >= 1e-3, (row, float(margins.min()))


def test_unknown_kv_dtype_is_refused_before_any_device_is_touched():
    args = synth.tiny(1)
    w = synth.make_weights(args, synth.TINY_HIDDEN, seed=1, preset="sharp")
    with pytest.raises(ValueError, match="kv_dtype 'int3'"):
        llama3.Llama(w, args, kv_dtype="int3")
    with pytest.raises(NotImplementedError, match="kv_dtype"):
        llama3.Llama(w, args, devices=[0, 1], kv_dtype="bf16")
