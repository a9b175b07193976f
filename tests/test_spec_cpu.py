"""Speculative decoding with lookup drafts (DESIGN.md "Speculative decoding"), the part that needs
no GPU: the properties of the Python specification (tests/spec_ref.py) that the GPU tests compare
against, the header's declarations and the bindings' argument types, the library's exports, and
the argument errors that are reported before a context is looked at."""

import ctypes
import re
import subprocess

import numpy as np
import pytest

import l3hip
import spec_ref

ENTRY_POINTS = ("l3_ragged_generate_spec_host", "l3_ragged_verify_host", "l3_op_spec_draft_host")
CTYPE = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}


# ---- the reference itself --------------------------------------------------------------------

@pytest.mark.parametrize("alphabet", [2, 5, 1000])
@pytest.mark.parametrize("draft_len", [0, 1, 4, 15])
def test_simulate_returns_the_true_ids_for_any_lookup(alphabet, draft_len):
    rng = np.random.default_rng(alphabet * 100 + draft_len)
    for trial in range(20):
        prompt = rng.integers(0, alphabet, rng.integers(1, 12))
        true = rng.integers(0, alphabet, rng.integers(0, 60))
        for lookup in ([], true, rng.integers(0, alphabet, 30), true[::-1]):
            n_max = int(rng.integers(1, 9))
            n_min = int(rng.integers(1, n_max + 1))
            ids, steps, drafted, accepted = spec_ref.simulate(lookup, prompt, true, draft_len, n_max, n_min)
            assert ids == true.tolist()
            assert 0 <= accepted <= drafted <= steps * draft_len
            # every token but the prefill's comes from an iteration: one per step, plus the accepted
            assert len(ids) == (1 + steps + accepted if len(ids) else 0)
            if draft_len == 0:
                assert steps == max(0, true.size - 1) and drafted == 0


def test_draft_rule_by_hand():
    d = spec_ref.draft
    assert d([], 4, 3, 1) == [] and d([5], 4, 3, 1) == []         # an empty history, one token: nothing to match
    assert d([5, 5], 4, 3, 1) == [5]                               # n_max longer than the history: n = E - 1 = 1
    assert d([1, 2, 3, 9, 1, 2, 3], 4, 8, 1) == [9, 1, 2, 3]       # n_max 8 > E - 1: the longest suffix that fits
    assert d([1, 2, 3, 9, 1, 2, 3], 2, 3, 1) == [9, 1]             # k cuts the draft
    assert d([1, 2, 3, 9, 1, 2, 3], 0, 3, 1) == []                 # k = 0
    assert d([7, 8, 7, 8, 7], 4, 2, 1) == [8, 7]                   # the largest j (2), its continuation clipped at E
    assert d([7, 8, 7, 8, 7], 4, 1, 1) == [8, 7]                   # n = 1: j = 2 again
    assert d([4, 4], 3, 1, 1) == [4]                               # j = E - n - 1 = 0: one token before E
    assert d([1, 2, 3, 4, 5, 3], 3, 3, 2) == []                    # only a 1-gram matches, n_min 2 forbids it
    assert d([1, 2, 3, 4, 5, 3], 3, 3, 1) == [4, 5, 3]
    assert d([6, 1, 2, 6, 1, 3, 6, 1], 2, 3, 1) == [3, 6]          # n = 2 ([6, 1]): the later match wins


def test_counters_by_hand():
    sim = spec_ref.simulate
    # no repeats anywhere: nothing is ever drafted, one token per step
    assert sim([], [9], [1, 2, 3, 4], 4, 3, 1) == ([1, 2, 3, 4], 3, 0, 0)
    # a period-2 row: after "1 2 1" every draft is right; k = min(4, R - m - 1) shortens the last ones
    true = [1, 2] * 5
    ids, steps, drafted, accepted = sim([], [2], true, 4, 3, 1)
    assert ids == true and drafted == accepted and steps + accepted == len(true) - 1
    # the lookup is the answer: the prompt's last token is matched across the seam lookup | prompt
    assert sim([5, 6, 7, 8, 9], [5], [6, 7, 8, 9], 4, 3, 1) == ([6, 7, 8, 9], 1, 2, 2)
    # ... a match that straddles the seam (the lookup ends with 3, the prompt starts with 4)
    assert spec_ref.draft([1, 2, 3] + [4, 8, 3, 4], 2, 2, 2) == [8, 3]
    # a wrong draft token costs nothing but its slot: accepted stops before it
    assert sim([5, 6, 0, 8], [5], [6, 7, 8, 9], 4, 3, 1) == ([6, 7, 8, 9], 3, 2, 0)
    # a stop id inside an accepted run: counted as accepted, cut after the stop id
    ids, steps, drafted, accepted = sim([5, 6, 7, 8, 9, 10, 11], [5], [6, 7, 8, 9, 10, 11], 4, 3, 1, stop_ids=[8])
    assert ids == [6, 7, 8] and (steps, drafted, accepted) == (1, 4, 4) and len(ids) < 1 + steps + accepted
    # a stop id as the first token, and a row with no budget
    assert sim([], [5], [6, 7], 4, 3, 1, stop_ids=[6]) == ([6], 0, 0, 0)
    assert sim([1, 2], [5], [], 4, 3, 1) == ([], 0, 0, 0)


# ---- the ABI ---------------------------------------------------------------------------------

def _declaration(name):
    with open(l3hip.HEADER) as f:
        text = f.read()
    m = re.search(r"^int\s+" + name + r"\s*\(([^)]*)\)\s*;", text, re.M | re.S)
    assert m, f"{name} is not declared in include/llama3hip.h"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_header_declares_the_entry_points():
    declared = l3hip.header_symbols()
    for name in ENTRY_POINTS:
        assert name in declared
    assert _declaration("l3_ragged_generate_spec_host") == [
        "l3_ctx* ctx", "const int64_t* ids_host", "const int32_t* lens", "const int32_t* starts", "int32_t B",
        "int32_t Lmax", "int32_t max_new_tokens", "const int64_t* stop_ids", "int32_t n_stop",
        "const int64_t* lookup_host", "const int32_t* lookup_lens", "int32_t Lk", "int32_t draft_len",
        "int32_t ngram_max", "int32_t ngram_min", "int64_t* out_ids_host", "int32_t* out_lens", "int32_t* row_steps",
        "int32_t* drafted", "int32_t* accepted"]
    assert _declaration("l3_ragged_verify_host") == [
        "l3_ctx* ctx", "const int64_t* ids_host", "const int32_t* lens", "const int32_t* starts", "int32_t B",
        "int32_t Lmax", "int64_t* chosen_host", "int32_t* n_accept"]
    assert _declaration("l3_op_spec_draft_host") == [
        "l3_ctx* ctx", "const int32_t* seq", "const int32_t* seq_lens", "const int32_t* k", "int32_t B",
        "int32_t Smax", "int32_t draft_len", "int32_t ngram_max", "int32_t ngram_min", "int32_t* out",
        "int32_t* out_n"]
    assert l3hip.version() == "0.19"


def test_binding_argument_types_match_the_header():
    for name in ENTRY_POINTS:
        res, args = l3hip._SIGNATURES[name]
        assert res is ctypes.c_int
        params = _declaration(name)
        assert len(args) == len(params), name
        for a, p in zip(args, params):
            ctype = p.rsplit(" ", 1)[0]
            want = ctypes.c_void_p if ctype.endswith("*") else CTYPE[ctype]
            assert a is want, (name, p, a)
        fn = getattr(l3hip.lib(), name)
        assert list(fn.argtypes) == args and fn.restype is ctypes.c_int
    for method in ("ragged_generate_spec", "ragged_verify", "op_spec_draft"):
        assert callable(getattr(l3hip.Context, method))


def test_library_exports_the_entry_points():
    lib = l3hip.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", l3hip.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in ENTRY_POINTS:
        assert hasattr(lib, name)
        assert name in exported, name  # unmangled: extern "C"


def _spec(lib, draft_len=4, ngram_max=3, ngram_min=1, lk=0):
    return lib.l3_ragged_generate_spec_host(None, None, None, None, 1, 1, 4, None, 0, None, None, lk, draft_len,
                                            ngram_max, ngram_min, None, None, None, None, None)


def test_argument_errors_are_reported_without_a_device():
    lib = l3hip.lib()
    for kw, msg in ((dict(draft_len=16), b"l3_ragged_generate_spec_host: draft_len 16 outside [0, 15]"),
                    (dict(draft_len=-1), b"draft_len -1 outside [0, 15]"),
                    (dict(ngram_max=9), b"ngram_min 1, ngram_max 9 (1 <= ngram_min <= ngram_max <= 8)"),
                    (dict(ngram_min=0), b"ngram_min 0, ngram_max 3"),
                    (dict(ngram_min=3, ngram_max=2), b"ngram_min 3, ngram_max 2"),
                    (dict(lk=-1), b"Lk -1 is negative"),
                    (dict(), b"null context")):
        assert _spec(lib, **kw) != 0
        assert msg in lib.l3_last_error(), lib.l3_last_error()
    assert lib.l3_ragged_verify_host(None, None, None, None, 1, 1, None, None) != 0
    assert b"null context" in lib.l3_last_error()
    seq, lens, k = np.zeros((2, 8), np.int32), np.array([8, 3], np.int32), np.array([1, 4], np.int32)
    out, n = np.zeros((2, 4), np.int32), np.zeros(2, np.int32)

    def op(seq=seq, lens=lens, k=k, B=2, smax=8, draft_len=4, ngram_max=3, ngram_min=1, out=out, n=n):
        p = [None if a is None else l3hip.ptr(a) for a in (seq, lens, k)]
        return lib.l3_op_spec_draft_host(None, *p, B, smax, draft_len, ngram_max, ngram_min,
                                         None if out is None else l3hip.ptr(out), None if n is None else l3hip.ptr(n))

    for kw, msg in ((dict(draft_len=16), b"l3_op_spec_draft_host: draft_len 16 outside [0, 15]"),
                    (dict(ngram_max=9), b"ngram_max 9"), (dict(ngram_min=0), b"ngram_min 0"),
                    (dict(B=0), b"bad shape B=0 Smax=8"), (dict(smax=0), b"bad shape B=2 Smax=0"),
                    (dict(seq=None), b"l3_op_spec_draft_host: null argument"), (dict(k=None), b"null argument"),
                    (dict(out=None), b"null argument"), (dict(n=None), b"null argument"),
                    (dict(lens=np.array([8, 9], np.int32)), b"seq_lens[1] = 9 outside [0, 8]"),
                    (dict(lens=np.array([-1, 3], np.int32)), b"seq_lens[0] = -1 outside [0, 8]"),
                    (dict(k=np.array([1, 5], np.int32)), b"k[1] = 5 outside [0, 4]"),
                    (dict(k=np.array([-1, 0], np.int32)), b"k[0] = -1 outside [0, 4]"),
                    (dict(), b"null context")):
        assert op(**kw) != 0
        assert msg in lib.l3_last_error(), (kw, lib.l3_last_error())
