"""No device: the tables, inputs and fp64 reference of tests/ragged_attn_ref.py (DESIGN.md "Ragged
attention at kernel level") — that the tables reach all 54 instantiations of csrc/ragged.hip and
csrc/ragged_extend.hip and every edge they are meant to, each by name; that the Python copy of the
LDS footprint agrees with the refusals the existing tests pin; that the reference equals the
project's other formulations; that the census inputs count what the census says; and that every
stress row that can has a spread no fp32 exp2 survives without the max subtraction."""

import numpy as np
import pytest

import extend_attn_ref as ext
import ragged_attn_ref as ref
import split_attn_ref as dec

# a rotation through the n_rep of each head size, for the checks that cost a Python loop per head
ROTATION = [(hd, (i + j * 3) % 8 + 1) for i, hd in enumerate(ref.HDS) for j in range(2)]


def test_parameters_reach_all_54_instantiations():
    """single-pass, split, append, extend <HD, KT>: 4 x 12, and combine <HD>: 6 — every test of the
    GPU module runs every (HD, n_rep) in both cache types through each of the five kernels"""
    assert ref.HDS == (16, 32, 48, 64, 96, 128) and ref.N_REPS == tuple(range(1, 9))
    assert len(ref.PARAMS) == 48 and set(ref.PARAMS) == {(hd, r) for hd in ref.HDS for r in ref.N_REPS}
    assert ref.KTS == ("f32", "bf16")
    inst = {(k, hd, kt) for k in ("single", "split", "append", "extend") for hd, _ in ref.PARAMS for kt in ref.KTS}
    inst |= {("combine", hd, None) for hd, _ in ref.PARAMS}
    assert len(inst) == 54
    for n_rep in ref.N_REPS:
        kvh = ref.kvh_of(n_rep)
        assert kvh == (3 if n_rep <= 4 else 1) and n_rep * kvh <= 12
    assert {ref.kvh_of(r) for r in ref.N_REPS} == {1, 3}  # KVH = 1, and one that is no power of two


@pytest.mark.parametrize("hd", ref.HDS)
def test_single_pass_positions_reach_every_edge(hd):
    pos, r = ref.single_positions(hd), 256 // (hd // 4)
    assert {0, 1} <= set(pos), "one key, two keys"
    assert {63, 64, 65} <= set(pos), "the softmax lane stride"
    assert {r - 1, r, r + 1} <= set(pos), "the P.V key groups"
    assert {2 * r - 1, 2 * r, 2 * r + 1} <= set(pos), "the bf16 P.V's doubled groups"
    assert {255, 256, 257} <= set(pos), "the score loop's second trip"
    assert ref.SMAX - 1 in pos and max(pos) == ref.SMAX - 1, "the last slot"
    assert all(0 <= p < ref.SMAX for p in pos)
    for n_rep in ref.N_REPS:  # the guard row is last and finished
        inp = ref.decode_inputs(hd, n_rep, pos[:3], ref.SMAX)
        assert inp["finished"].tolist() == [0, 0, 0, 1] and inp["n_heads"] == n_rep * ref.kvh_of(n_rep)


def test_split_settings_reach_every_edge():
    assert ref.SPLITS == ((64, 320), (320, 384), (128, 320))
    for chunk, s_cap in ref.SPLITS:
        pos = ref.split_positions(chunk, s_cap)
        n_split = -(-s_cap // chunk)
        assert chunk % 64 == 0 and s_cap % 4 == 0 and max(pos) == s_cap - 1, "the last slot"
        for c in range(n_split):
            here = {p - c * chunk for p in pos if p // chunk == c}
            assert {0, 1} <= here, "an owner chunk with only the new key, and with one cached key"
            assert chunk - 1 in here or (c + 1) * chunk > s_cap, "the new key in the chunk's last slot"
        assert max(p // chunk for p in pos) == n_split - 1
    # chunk 320: longer than the 256-thread score pass (the split kernel's own second trip), two chunks in the grid
    assert ref.SPLITS[1][0] > 256 and -(-ref.SPLITS[1][1] // ref.SPLITS[1][0]) == 2
    assert max(p // 64 for p in ref.split_positions(64, 320)) + 1 >= 5  # five chunks for the combine


def test_lds_copy_fits_every_launch_and_agrees_with_the_pinned_refusals():
    worst = max((ref.decode_lds_bytes(r, hd, ref.SMAX), hd, r) for hd, r in ref.PARAMS)
    assert worst == (12040 * 4, 128, 8)
    for hd, r in ref.PARAMS:
        assert ref.decode_lds_bytes(r, hd, ref.SMAX) <= ref.RAGGED_LDS_BYTES
        for chunk, s_cap in ref.SPLITS:  # the split form, and its single-pass twin at the same s_cap
            assert ref.decode_lds_bytes(r, hd, chunk) <= ref.RAGGED_LDS_BYTES
            assert ref.decode_lds_bytes(r, hd, s_cap) <= ref.RAGGED_LDS_BYTES
    # tests/test_gpu_ragged_split.py test_op_refuses_what_no_kernel_takes
    assert ref.decode_lds_bytes(8, 128, 1024) == 70688 > ref.RAGGED_LDS_BYTES
    assert ref.decode_lds_bytes(8, 128, 896) == 66592 > ref.RAGGED_LDS_BYTES
    assert ref.decode_lds_bytes(8, 128, 832) <= ref.RAGGED_LDS_BYTES
    for hd in ref.HDS:  # the host's q_scale: double arithmetic, one rounding
        assert ref.q_scale(hd).dtype == np.float32 and abs(float(ref.q_scale(hd)) * np.sqrt(hd) / dec.LOG2E - 1) < 6e-8


@pytest.mark.parametrize("n_rep", ref.N_REPS)
def test_extend_rows_reach_every_edge(n_rep):
    tq, lq, pairs = ref.tq_of(n_rep), ref.lq_of(n_rep), ref.extend_pairs(n_rep)
    assert tq == 64 // n_rep and lq == 2 * tq + 17 and lq <= ref.SMAX
    assert {5: 60, 6: 60, 7: 63}.get(n_rep, 64 - 64 % n_rep) == tq * n_rep  # live query rows of 64
    lens, starts = {n for _, n in pairs}, {s for s, _ in pairs}
    assert lens == {0, 1, tq - 1, tq, tq + 1, 2 * tq + 1, lq}
    assert {0, 1, 17, ref.EXT_KT - 2, ref.EXT_KT - 1, ref.EXT_KT} <= starts
    for n in lens - {0}:
        assert (ref.SMAX - n, n) in pairs, "a chunk that ends in the last slot"
    assert all(s + n <= ref.SMAX and 0 <= s < ref.SMAX for s, n in pairs) and len(set(pairs)) == len(pairs)
    assert pairs[-1][1] == 0, "the guard row"
    assert any(n == 0 for _, n in pairs[:-1]), "an all-pad row inside the batch"
    assert -(-lq // tq) >= 3 and lq % tq and any(n == lq for _, n in pairs), "three or more query tiles, the last partial"
    # the append's 16-token tiles: a partial first tile, a full one, and a partial tile after full ones
    assert any(n < ref.EXT_TA for n in lens - {0}) and any(n > ref.EXT_TA and n % ref.EXT_TA for n in lens)
    # the per-wave masked decision (masked = k0 + EXT_KT - 1 > w_lo), both sides, for every live wave
    # of the first and the second query tile, with an unmasked key tile in front
    for t0 in (0, tq):
        for wid in range(4):
            if wid * 16 >= tq * n_rep:
                continue
            sides = set()
            for s, n in pairs:
                n_live = min(tq, n - t0)
                if n_live < tq:
                    continue
                w_lo = ref.wave_lo(s, t0, wid, n_live, n_rep)
                if w_lo >= 2 * ref.EXT_KT - 2:
                    sides.add(w_lo % ref.EXT_KT)
            assert {ref.EXT_KT - 1, ref.EXT_KT - 2} <= sides, (t0, wid, sorted(sides))
    assert all(s + lq <= ref.SMAX for s in ref.masked_edge_starts(n_rep))


def test_long_extend_table_has_three_full_query_tiles():
    assert ref.LQ_LONG == 130 and -(-ref.LQ_LONG // ref.tq_of(1)) == 3
    assert any(n == ref.LQ_LONG for _, n in ref.LONG_PAIRS) and ref.LONG_PAIRS[-1][1] == 0
    assert any(s + n == ref.SMAX for s, n in ref.LONG_PAIRS)
    assert all(s + n <= ref.SMAX and n <= ref.LQ_LONG for s, n in ref.LONG_PAIRS)


# ---- the reference against the project's other formulations --------------------------------------

@pytest.mark.parametrize("hd,n_rep", ROTATION)
def test_decode_reference_equals_the_chunked_formulation(hd, n_rep):
    for chunk, s_cap in ref.SPLITS[:2]:
        inp = ref.decode_inputs(hd, n_rep, ref.split_positions(chunk, s_cap), s_cap)
        want, new_k, new_v, _ = ref.decode_reference(inp)
        assert float(np.abs(dec.chunked(inp, chunk) - want).max()) <= 1e-12
        old, ok, ov = dec.reference(inp)
        assert float(np.abs(old - want).max()) <= 1e-12
        assert np.array_equal(np.nan_to_num(ok), np.nan_to_num(new_k)) and np.array_equal(np.isnan(ov), np.isnan(new_v))
        assert not want[-1].any() and np.abs(want[:-1]).max() > 0


@pytest.mark.parametrize("hd,n_rep", ROTATION)
def test_extend_reference_equals_the_masked_full_matrix(hd, n_rep):
    pairs, lq = ref.extend_pairs(n_rep), ref.lq_of(n_rep)
    inp = ref.extend_inputs(hd, n_rep, pairs, lq)
    want, new_k, new_v, _ = ref.extend_reference(inp)
    assert float(np.abs(ref.masked_full(inp) - want).max()) <= 1e-12
    for b, (_, n) in enumerate(pairs):
        assert not want[b, n:].any() and (n == 0 or np.abs(want[b, :n]).min() > 0)
    if (hd, n_rep) == ROTATION[0]:  # and the loop-per-token reference of tests/extend_attn_ref.py
        old, ok, ov = ext.reference(inp)
        assert float(np.abs(old - want).max()) <= 1e-12
        for b, (st, n) in enumerate(pairs):
            assert np.array_equal(ok[b, :, st:st + n], new_k[b]) and np.array_equal(ov[b, :, st:st + n], new_v[b])


# ---- census ---------------------------------------------------------------------------------------

def _brute(n_keys, hd):
    return np.bincount(np.arange(n_keys) % hd, minlength=hd)


@pytest.mark.parametrize("hd,n_rep", ROTATION)
def test_census_equals_a_brute_force_count_and_the_inputs_count_it(hd, n_rep):
    inp = ref.decode_inputs(hd, n_rep, ref.single_positions(hd), ref.SMAX, "census")
    want = ref.decode_census(inp)
    out = ref.decode_reference(inp, "census")[0].reshape(len(inp["pos"]), -1, hd)
    for b, p in enumerate(inp["pos"][:-1]):
        assert np.array_equal(want[b], _brute(p + 1, hd))
        assert float(np.abs(out[b] * (p + 1) - want[b][None]).max()) <= 1e-9
    pairs, lq = ref.extend_pairs(n_rep), ref.lq_of(n_rep)
    inp = ref.extend_inputs(hd, n_rep, pairs, lq, "census")
    want = ref.extend_census(inp)
    out = ref.extend_reference(inp, "census")[0].reshape(len(pairs), lq, -1, hd)
    for b, (s, n) in enumerate(pairs):
        for t in (0, n // 2, n - 1) if n else ():
            assert np.array_equal(want[b, t], _brute(s + t + 1, hd))
        keys = s + np.arange(n) + 1
        assert n == 0 or float(np.abs(out[b, :n] * keys[:, None, None] - want[b, :n, None]).max()) <= 1e-9
    # exact in bf16 as well
    v = ref.to_bf16(inp)["cache_v"]
    for b, (s, n) in enumerate(pairs):  # the history; [s, s + n) holds what the append replaces, NaN follows
        assert set(np.unique(v[b, :, :s]).tolist()) <= {0, 0x3F80} and (v[b, :, s + n:] == 0x7FC0).all()


# ---- stress ---------------------------------------------------------------------------------------

def _spread_ok(spread, visible, what):
    """every row with two or more visible keys: a spread of at least 150, which 2^x of fp32 cannot
    hold (a variant without the max subtraction overflows); one-key rows have no spread to give"""
    for b, (sp, n) in enumerate(zip(spread, visible)):
        if n >= 2:
            assert sp >= ref.SPREAD_MIN and sp > 128  # 2^128 is past fp32, (what, b, sp, n)


@pytest.mark.parametrize("kt", ref.KTS)
@pytest.mark.parametrize("hd,n_rep", ref.PARAMS)
def test_stress_rows_meet_the_spread_cap(hd, n_rep, kt):
    """In the fp64 reference alone.  For a bf16 cache the scores are those of the rounded keys
    (the new key rounded as the kernels' kv_bf16_rne does: to nearest even)"""
    import kv_bf16_ref as kv
    tables = [(ref.single_positions(hd), ref.SMAX)] + [(ref.split_positions(c, s), s) for c, s in ref.SPLITS]
    pairs, lq = ref.extend_pairs(n_rep), ref.lq_of(n_rep)
    for shape in ref.STRESS:
        for pos, smax in tables:
            inp = ref.decode_inputs(hd, n_rep, pos, smax, "stress", shape)
            if kt == "bf16":
                nk = ref.decode_reference(inp, scores_only=True)[1]
                ck = kv.widen(kv.to_bits(inp["cache_k"][..., :1]))  # q = e_0: component 0 is the score
                for b, p in enumerate(pos):
                    ck[b, :, p] = kv.widen(kv.to_bits(nk[b][:, :1]))
                spread = ref.decode_reference(inp, "stress", (ck, ck), scores_only=True)[3]
            else:
                spread = ref.decode_reference(inp, "stress", scores_only=True)[3]
            _spread_ok(spread[:-1], [p + 1 for p in pos], (shape, smax))
            if shape == "rising" and smax == ref.SMAX:
                assert max(spread) > 254  # over 320 keys
        inp = ref.extend_inputs(hd, n_rep, pairs, lq, "stress", shape)
        if kt == "bf16":
            _, nk, _, _ = ref.extend_reference(inp, scores_only=True)
            ck = kv.widen(kv.to_bits(inp["cache_k"][..., :1]))
            for b, (s, n) in enumerate(pairs):
                ck[b, :, s:s + n] = kv.widen(kv.to_bits(nk[b][..., :1]))
            spread = ref.extend_reference(inp, "stress", (ck, ck), scores_only=True)[3]
        else:
            spread = ref.extend_reference(inp, "stress", scores_only=True)[3]
        _spread_ok(spread, [s + n if n else 0 for s, n in pairs], (shape, "extend"))


def test_stress_shapes_place_their_keys():
    for n in (1, 2, 7, 64, 161, 320):
        up, down = ref.stress_scores("rising", n), ref.stress_scores("falling", n)
        assert up[-1] == 0 and down[0] == 0 and (n == 1 or (np.diff(up) >= 1).all() and (np.diff(down) <= -1).all())
        low, high, new = (ref.stress_scores("spike_low", n), ref.stress_scores("spike_high", n),
                          ref.stress_scores("spike_high", n, at_new=True))
        assert low.argmax() == min(5, n - 1) and high.argmax() == max(n - 2, 0) and new.argmax() == n - 1
        assert low.max() == high.max() == new.max() == ref.SPIKE and np.count_nonzero(low) == 1
    # spike_high lands on the new key itself in some live decode row of every table
    for pos in [ref.single_positions(16)] + [ref.split_positions(c, s) for c, s in ref.SPLITS]:
        assert any(b % 3 == 0 and p >= 1 for b, p in enumerate(pos))
