"""Ragged batches (DESIGN.md "Ragged batches"; l3_ragged_forward_host / l3_ragged_generate_host,
csrc/ragged.hip): prompts of different lengths in one batch.  The reference for row b is the
oracle run on that row alone (max_batch_size 1, a zeroed cache): its prefill logits within the
project's 1e-4 bar, its greedy ids exactly ("sharp" weights: top-1 margins far above the fp32
error).  Each model's oracle rows are computed once and shared by the tests below."""

import dataclasses
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import llama3
import llama3_oracle as orc
import synth
from config import ModelArgs

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHECK_LIB = os.path.join(os.path.dirname(HERE), "llama3.np_amd", "csrc", "libllama3hip_check.so")

# name -> (args, hidden, prompt lengths, max_new_tokens of the long run)
#   tiny:    HD 16, n_rep 2, Smax 64; the long run ends at the last cache slot
#   stories: the stories15M shape, HD 48, n_rep 1, more than one 16-row tile of prefill rows
#   gqa:     one layer, HD 128, n_rep 4; Lmax + steps reaches max_seq_len
SHAPES = {
    "tiny": (synth.tiny(4), synth.TINY_HIDDEN, (1, 3, 7, 12), 64),
    "stories": (synth.stories15m(5), synth.STORIES15M_HIDDEN, (2, 9, 9, 17, 33), 41),
    "gqa": (ModelArgs(dim=512, n_layers=1, n_heads=4, n_kv_heads=1, vocab_size=1024, max_seq_len=96,
                      max_batch_size=3), 256, (3, 30, 64), 96),
}


class Case:
    def __init__(self, name):
        self.args, hidden, self.lens, self.max_new = SHAPES[name]
        self.w = synth.make_weights(self.args, hidden, seed=31, preset="sharp")
        self.w64 = {k: np.asarray(v, np.float64) for k, v in self.w.items()}
        rng = np.random.default_rng(7)
        self.prompts = [rng.integers(0, self.args.vocab_size, n) for n in self.lens]
        self.model = llama3.Llama(self.w, self.args, device=0)
        one = dataclasses.replace(self.args, max_batch_size=1)
        self.logits, self.ids = [], []
        for p in self.prompts:  # the reference: each row alone on a zeroed cache
            self.logits.append(orc.OracleModel(self.w64, one)(p[None], 0)[0, -1])
            self.ids.append(orc.greedy_ids(orc.OracleModel(self.w64, one), p[None], self.max_new)[0])

    def padded(self, fill=0):
        ids = np.full((len(self.lens), max(self.lens)), fill, np.int64)
        for b, p in enumerate(self.prompts):
            ids[b, :p.size] = p
        return ids, np.array(self.lens, np.int32)

    def want(self, max_new):
        """row b's first max(0, max_new - len_b) greedy ids (a greedy prefix does not depend on
        where the loop ends)"""
        return [ids[:max(0, max_new - n)] for ids, n in zip(self.ids, self.lens)]


_cases = {}


@pytest.fixture
def case(request):
    name = request.param
    if name not in _cases:
        _cases[name] = Case(name)
    _cases[name].model.context.reset_cache()
    _cases[name].model.set_sampling(0.0)
    return _cases[name]


def _same_rows(got, want):
    assert len(got) == len(want)
    for b, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.int64 and np.array_equal(g, w), (b, g, w)


# ---- logits ----------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["tiny", "stories"], indirect=True)
def test_prefill_logits_match_each_row_alone(case):
    got = case.model.forward_ragged(case.prompts)
    assert got.shape == (len(case.lens), 1, case.args.vocab_size) and got.dtype == np.float32
    for b, want in enumerate(case.logits):
        err = float(np.abs(got[b, 0].astype(np.float64) - want).max())
        print(f"row {b} (len {case.lens[b]}): max-abs {err:.3e}")
        assert err <= 1e-4, (b, err)
    # the pad entries are never looked at: garbage and out-of-range values change nothing
    ids, lens = case.padded()
    base = np.array(case.model.context.ragged_forward(ids, lens))
    assert np.array_equal(base, got[:, 0])
    for fill in (case.args.vocab_size - 1, 10 ** 12, -5 * case.args.vocab_size):
        case.model.context.reset_cache()
        junk, _ = case.padded(fill)
        assert np.array_equal(np.array(case.model.context.ragged_forward(junk, lens)), base), fill


@pytest.mark.parametrize("case", ["tiny", "stories"], indirect=True)
def test_pad_slots_read_as_zero_in_a_following_decode(case):
    """A full-length forward first fills slots [0, Lmax) of every row; the ragged prefill must
    leave [len_b, Lmax) zero again, or row b's decode steps (which attend slot len_b, the one the
    reference never writes) give other ids."""
    rng = np.random.default_rng(11)
    case.model(rng.integers(0, case.args.vocab_size, (len(case.lens), max(case.lens))), 0)
    steps = 12
    max_new = min(case.lens) + steps
    _same_rows(case.model.generate_ragged(case.prompts, max_new), case.want(max_new))


# ---- greedy ids ------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["tiny", "stories", "gqa"], indirect=True)
def test_greedy_ids_match_each_row_alone(case):
    got = case.model.generate_ragged(case.prompts, case.max_new)
    _same_rows(got, case.want(case.max_new))
    assert [g.size for g in got] == [case.max_new - n for n in case.lens]
    # a row as long as max_new_tokens yields nothing; the others their prefix
    case.model.context.reset_cache()
    short = max(case.lens)
    got = case.model.generate_ragged(case.prompts, short)
    _same_rows(got, case.want(short))
    assert got[-1].size == 0 and got[0].size == short - case.lens[0]
    # through the context: [B, cap] with -1 past each row's tokens
    case.model.context.reset_cache()
    ids, lens = case.padded()
    out, n = case.model.context.ragged_generate(ids, lens, short)
    assert out.shape == (len(lens), short - min(case.lens)) and n.dtype == np.int32
    assert n.tolist() == [short - x for x in case.lens]
    for b in range(len(lens)):
        assert (out[b, n[b]:] == -1).all() and np.array_equal(out[b, :n[b]], got[b])


# ---- equal lengths ---------------------------------------------------------------------------

SAMPLING = (0.8, 40, 0.95, 4321)


@pytest.mark.parametrize("case", ["tiny"], indirect=True)
def test_equal_lengths_reproduce_generate_all(case):
    m, V = case.model, case.args.vocab_size
    rng = np.random.default_rng(13)
    prompt = rng.integers(0, V, (3, 5))
    total = 29
    for sampling in (None, SAMPLING):
        if sampling:
            m.set_sampling(*sampling)
        m.context.reset_cache()
        want = m.generate_all(prompt, total)
        m.context.reset_cache()
        got = m.generate_ragged(list(prompt), total)
        assert np.array_equal(np.stack(got), want), sampling
    # sampling is still on: row 0 draws (seed, 0, position) whatever the other rows' lengths
    m.context.reset_cache()
    ragged = m.generate_ragged([prompt[0], prompt[1][:3], rng.integers(0, V, 8)], total)
    assert np.array_equal(ragged[0], want[0])
    assert ragged[1].size == total - 3 and ragged[2].size == total - 8
    m.set_sampling(0.0)
    m.context.reset_cache()
    assert not np.array_equal(np.stack(m.generate_ragged(list(prompt), total)), want)  # it was sampled


# ---- stop ids --------------------------------------------------------------------------------

def _truncate(rows, stops):
    out = []
    for r in rows:
        hit = np.flatnonzero(np.isin(r, stops))
        out.append(r[:hit[0] + 1] if hit.size else r)
    return out


@pytest.mark.parametrize("case", ["tiny"], indirect=True)
def test_stop_ids_end_a_row(case):
    m, max_new = case.model, 40
    base = m.generate_ragged(case.prompts, max_new)
    _same_rows(base, case.want(max_new))
    stop = int(base[1][len(base[1]) // 2])  # a token row 1 emits mid-way
    want = _truncate(base, [stop])
    assert want[1].size < base[1].size
    m.context.reset_cache()
    _same_rows(m.generate_ragged(case.prompts, max_new, stop_ids=[stop]), want)
    m.context.reset_cache()
    ids, lens = case.padded()
    out, n = m.context.ragged_generate(ids, lens, max_new, stop_ids=[stop, 10 ** 9])
    assert n.tolist() == [w.size for w in want]
    for b, w in enumerate(want):
        assert np.array_equal(out[b, :n[b]], w) and (out[b, n[b]:] == -1).all()


@pytest.mark.parametrize("case", ["tiny"], indirect=True)
def test_all_rows_stopping_early_returns_and_leaves_the_context_usable(case):
    m = case.model
    base = case.want(case.max_new)
    stops = sorted({int(r[min(1, r.size - 1)]) for r in base})  # every row stops within two tokens
    want = _truncate(base, stops)
    assert max(w.size for w in want) <= 2
    _same_rows(m.generate_ragged(case.prompts, case.max_new, stop_ids=stops), want)
    # the same context then runs an ordinary batch correctly
    m.context.reset_cache()
    prompt = np.random.default_rng(17).integers(0, case.args.vocab_size, (4, 5))
    assert np.array_equal(m.generate_all(prompt, 20), orc.greedy_ids(orc.OracleModel(case.w64, case.args), prompt, 20))


# ---- errors ----------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["tiny"], indirect=True)
def test_errors_are_reported_before_anything_runs(case):
    m, ctx, V = case.model, case.model.context, case.args.vocab_size
    ids, lens = case.padded()
    probe = np.random.default_rng(19).integers(0, V, (2, 6))
    before = np.array(m(probe, 0))
    ctx.reset_cache()

    def bad(match, ids, lens, max_new=20):
        with pytest.raises(RuntimeError, match=match):
            ctx.ragged_forward(ids, lens)
        with pytest.raises(RuntimeError, match=match):
            ctx.ragged_generate(ids, lens, max_new)

    zero = lens.copy()
    zero[1] = 0
    bad(r"lens\[1\] = 0 outside \[1, 12\]", ids, zero)
    long = lens.copy()
    long[0] = 13
    bad(r"lens\[0\] = 13 outside \[1, 12\]", ids, long)
    bad("batch 5 exceeds max_batch_size 4", np.zeros((5, 3), np.int64), np.full(5, 3, np.int32))
    with pytest.raises(RuntimeError, match="last decode position 64 exceeds max_seq_len 64"):
        ctx.ragged_generate(ids, lens, 65)
    oob = ids.copy()
    oob[2, 6] = V  # the last real position of row 2 (len 7)
    bad(f"token id {V} out of range for vocab_size {V}", oob, lens)
    with pytest.raises(RuntimeError, match="lens"):
        m.forward_ragged([[1, 2], []])
    with pytest.raises(ValueError):
        ctx.ragged_forward(ids, lens[:2])
    # nothing was launched: the cache is still zero and a normal forward gives what it gave
    assert np.array_equal(np.array(m(probe, 0)), before)


# ---- check library ---------------------------------------------------------------------------

def test_check_build_records_no_violation():
    assert os.path.exists(CHECK_LIB), f"{CHECK_LIB} missing: __graft_entry__.build() makes it"
    env = dict(os.environ, L3_LIB_PATH=CHECK_LIB)
    r = subprocess.run([sys.executable, os.path.join(HERE, "ragged_checks_workload.py")], env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["enabled"] is True
    assert out["workload"] == {"kv_slot": 0, "attn_keys": 0, "token_id": 0}
    assert out["tokens"] > 0
