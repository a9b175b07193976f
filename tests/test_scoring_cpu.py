"""Scoring, CPU side: the reference helpers of scoring_ref.py against the oracle and against
hand-made rows, and the C ABI's three scoring entry points (header and ctypes bindings).  No
device is used.
"""

import math
import re

import numpy as np
import pytest

import l3hip
import llama3_oracle as orc
import scoring_ref as ref
import synth


@pytest.mark.parametrize("shape", ["tiny", "stories15m"])
def test_all_logits_last_position_is_the_oracle_call(shape):
    if shape == "tiny":
        args, hidden, B, L = synth.tiny(2), synth.TINY_HIDDEN, 2, 9
    else:
        args, hidden, B, L = synth.stories15m(1), synth.STORIES15M_HIDDEN, 1, 6
    w = synth.make_weights(args, hidden, seed=3, preset="sharp")
    ids = np.random.default_rng(1).integers(0, args.vocab_size, (B, L))
    z = ref.all_logits(orc.OracleModel(w, args), ids, 0)
    want = orc.OracleModel(w, args)(ids, 0)
    assert z.shape == (B, L, args.vocab_size) and z.dtype == np.float64
    assert np.max(np.abs(z[:, -1] - want[:, 0])) <= 1e-12
    # a second piece at start_pos = L on the caches the first wrote
    m1, m2 = orc.OracleModel(w, args), orc.OracleModel(w, args)
    nxt = ids[:, :3]
    ref.all_logits(m1, ids, 0)
    m2(ids, 0)
    assert np.max(np.abs(ref.all_logits(m1, nxt, L)[:, -1] - m2(nxt, L)[:, 0])) <= 1e-12


def test_rule_on_hand_made_rows():
    inf = math.inf
    z = np.array([
        [2.0, 2.0, 2.0, 2.0],        # all equal
        [0.0, -inf, 0.0, 0.0],       # one -inf
        [-inf, -inf, -inf, -inf],    # all -inf
        [1.0, math.nan, 3.0, math.nan],  # NaN: the first one wins the argmax
        [1.0, 5.0, 5.0, 0.0],        # target -1; first maximum
        [0.0, inf, 0.0, 0.0],        # +inf maximum
    ])
    t = np.array([3, 1, 0, 2, -1, 1])
    lp, lse, am, margin = ref.logprobs64(z, t)
    assert lp[0] == pytest.approx(-math.log(4.0), abs=1e-15) and lse[0] == pytest.approx(2.0 + math.log(4.0))
    assert am[0] == 0 and margin[0] == 0.0
    assert lp[1] == -inf and lse[1] == pytest.approx(math.log(3.0)) and am[1] == 0
    assert ref.logprobs64(z[1:2], np.array([2]))[0][0] == pytest.approx(-math.log(3.0))
    assert math.isnan(lp[2]) and am[2] == 0
    assert math.isnan(lp[3]) and am[3] == 1
    assert lp[4] == 0.0 and am[4] == 1
    assert lse[4] == pytest.approx(5.0 + math.log(2.0 + math.exp(-4.0) + math.exp(-5.0)))
    assert math.isnan(lp[5]) and am[5] == 1
    # no target scores 0.0 on the rows that score NaN otherwise too
    assert (ref.logprobs64(z, np.full(6, -1))[0] == 0.0).all()
    # large logits: the maximum is subtracted
    big = np.array([[1000.0, 999.0, -1000.0]])
    assert ref.logprobs64(big, np.array([0]))[0][0] == pytest.approx(-math.log1p(math.exp(-1.0)))
    with pytest.raises(ValueError):
        ref.logprobs64(z, np.array([4, 0, 0, 0, 0, 0]))


SCORING_ABI = {"l3_score_host": 8, "l3_op_linear_logprob_host": 10, "l3_set_score_workspace": 2}


def test_header_declares_and_l3hip_binds_the_scoring_entry_points():
    with open(l3hip.HEADER) as f:
        text = f.read()
    for name, nargs in SCORING_ABI.items():
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\)\s*;", text, re.M)
        assert m, f"{name} is not declared in include/llama3hip.h"
        assert len(m.group(1).split(",")) == nargs, name
        assert name in l3hip._SIGNATURES, f"{name} has no ctypes binding"
        assert len(l3hip._SIGNATURES[name][1]) == nargs, name
        assert hasattr(l3hip.lib(), name), f"{name} is not exported"
    for meth in ("score", "op_linear_logprob", "set_score_workspace"):
        assert callable(getattr(l3hip.Context, meth, None)), meth
    # each new entry point cites the reference lines it extends, as the others do
    for name in SCORING_ABI:
        head = text[:text.index("int " + name)]
        assert "llama3.py:285-308" in head[head.rindex("/*"):], name
