"""The case tables and inputs of tests/decode_gemv_ref.py, checked without a device: they reach every
instantiation the GPU tests claim, and every tie / NaN / order-sensitive case has exactly one right
answer under the float64 / np.argmax rule (a condition on the inputs, not on any kernel)."""

import ctypes

import numpy as np
import pytest

import decode_gemv_ref as ref
import gemm_epi_ref as epi_ref
import l3hip


def better(v, i, bv, bi):
    """The strict total order of the argmax rule, one pair at a time."""
    vn, bn = v != v, bv != bv
    if vn or bn:
        return vn and (not bn or i < bi)
    return v > bv or (v == bv and i < bi)


def scan(table):
    bv, bi = -np.inf, ref.EMPTY_I
    for v, i in zip(table["v"].tolist(), table["i"].tolist()):
        if better(v, i, bv, bi):
            bv, bi = v, i
    return bv, bi


# ---- the tables reach what they claim -----------------------------------------------------------

def test_lane_rule_and_reachable_lane_counts():
    assert [ref.lanes_for("store", "fp32", K) for K in ref.KS] == [16, 16, 32, 64]
    assert [ref.lanes_for("store", "bf16", K) for K in ref.KS] == [16, 16, 16, 32]
    assert [ref.lanes_for("store", "fp8", K) for K in ref.KS] == [16, 16, 16, 16]
    assert [ref.lanes_for("parts_swiglu", "fp32", K) for K in ref.KS] == [32, 32, 64, 64]
    assert [ref.lanes_for("parts_swiglu", "bf16", K) for K in ref.KS] == [32, 32, 32, 64]
    # the compact storages' partial-rows forms past what K <= 2048 reaches
    assert [ref.lanes_for("parts_swiglu", "fp8", K) for K in (2048, 4096)] == [32, 64]
    assert [ref.lanes_for("parts_resid", "bf16", K) for K in (1024, 2048, 4096)] == [16, 32, 64]
    assert [ref.lanes_for("parts_resid", "fp8", K) for K in (2048, 4096, 8192)] == [16, 32, 64]
    assert [ref.units_per_block(l) for l in (16, 32, 64)] == [16, 8, 4]
    assert [ref.gemv_rows(K) for K in (2048, 4096, 8192)] == [3, 3, 2]


def test_every_case_uses_a_listed_k():
    for c in ref.AMAX_CASES + ref.FOLD_CASES:
        assert c.K in ref.KS, c.id
    for c in ref.PARTS_CASES:
        assert c.K in ref.KS or (c.storage != "fp32" and c.K in ref.PARTS_KS_COMPACT), c.id
        if c.K not in ref.KS:  # a larger K only where no listed K reaches the form
            form = "parts_swiglu" if c.epi == epi_ref.SWIGLU else "parts_resid"
            assert c.lanes not in {ref.lanes_for(form, c.storage, K) for K in ref.KS}, c.id
        mr = 1 if c.M <= 1 else 2 if c.M <= 2 else 4
        assert mr * c.K <= ref.GEMV_LDS_K and c.N * c.K <= ref.SMALL_W, c.id  # the direct GEMV's range


@pytest.mark.parametrize("cases,form", [(ref.AMAX_CASES, "store"), (ref.FOLD_CASES, "fold")])
def test_amax_part_and_fold_reach_every_fp32_lane_count_and_one_per_compact_storage(cases, form):
    by = {}
    for c in cases:
        assert c.lanes == ref.lanes_for(form, c.storage, c.K)
        assert c.route["family"] == ref.FAMILY[c.storage] and c.route["lanes_per_unit"] == c.lanes
        by.setdefault(c.storage, set()).add(c.lanes)
    assert by["fp32"] == {16, 32, 64}
    assert len(by["bf16"]) == 1 and len(by["fp8"]) == 1


def test_amax_part_runs_with_and_without_the_norm_at_every_lane_count():
    seen = {(c.storage, c.lanes, c.norm) for c in ref.AMAX_CASES}
    for st, lanes in {(c.storage, c.lanes) for c in ref.AMAX_CASES}:
        assert (st, lanes, True) in seen and (st, lanes, False) in seen


def test_parts_reach_every_lane_count_of_every_form_and_storage():
    by = {}
    for c in ref.PARTS_CASES:
        form = "parts_swiglu" if c.epi == epi_ref.SWIGLU else "parts_resid"
        by.setdefault((form, c.storage), set()).add(c.lanes)
    for form in ("parts_swiglu", "parts_resid"):
        for st in ref.STORAGES:
            assert sorted(by[(form, st)]) == ref.PARTS_LANES[form], (form, st)  # the dispatcher's set, in every storage
    assert ref.PARTS_LANES == {"parts_swiglu": [32, 64], "parts_resid": [16, 32, 64]}
    for form, st in by:
        for lanes in by[(form, st)]:
            mine = [c for c in ref.PARTS_CASES if c.lanes == lanes and c.storage == st and
                    ("parts_swiglu" if c.epi == epi_ref.SWIGLU else "parts_resid") == form]
            got = {(c.nparts, c.M, c.kind) for c in mine}
            # three rows, but two where four staged rows of K are past the GEMV range (fp8 EPI_RESID at 64 lanes)
            rows = 2 if (form, st, lanes) == ("parts_resid", "fp8", 64) else 3
            assert {(1, 1, "int"), (3, 1, "int"), (8, 1, "int"), (3, 1, "order"), (8, 1, "order"), (3, rows, "int"),
                    (3, rows, "order")} <= got, (form, st, lanes)


def test_both_fold_passes_and_the_reducers_second_pass_are_reached():
    fold = ref.fold_tables()
    assert any(len(t) > ref.FOLD_PASS and int(np.flatnonzero(t["v"] == 1000.0)[0]) >= ref.FOLD_PASS
               for n, t, _ in fold if "win" in n)
    assert any(len(t) <= ref.FOLD_PASS for _, t, _ in fold)
    tabs = ref.argmax_tables()
    assert any(len(t) > ref.PARTS_PASS and int(np.flatnonzero(t["v"] == 1000.0)[0]) >= ref.PARTS_PASS
               for n, t, _ in tabs if "win" in n)
    assert any(len(t) > 2 * ref.PARTS_PASS for _, t, _ in tabs)  # a third pass too


def test_every_planted_winner_position_is_in_the_tables():
    names = {n for n, _, _ in ref.argmax_tables()}
    for n in ref.PARTS_N:
        for p in ref.PARTS_WINNERS:
            p = n - 1 if p < 0 else p
            if p < n:
                assert f"n{n}-win{p}" in names
    names = {n for n, _, _ in ref.fold_tables()}
    for n in ref.FOLD_N:
        for p in ref.FOLD_WINNERS:
            p = n - 1 if p < 0 else p
            if p < n:
                assert f"n{n}-win{p}" in names
    for case in ref.AMAX_CASES:
        sc = {n: c for n, c, _ in ref.amax_scenarios(case)}
        assert sc["col0"] == [0] and sc["last_of_block0"] == [case.upb - 1] and sc["first_of_block1"] == [case.upb]
        assert sc["last_valid"] == [case.N - 1]
        waves = [sc[f"wave{k}_of_block2"][0] for k in range(4)]
        assert [(c // case.upb, (c % case.upb) // case.upw) for c in waves] == [(2, k) for k in range(4)]
        a, b = sc["tie_across_waves"]
        assert a // case.upb == b // case.upb and (a % case.upb) // case.upw != (b % case.upb) // case.upw
        a, b = sc["tie_across_blocks"]
        assert a // case.upb != b // case.upb
        if case.upw >= 2:
            a, b = sc["tie_in_unit_group"]
            assert a // case.upw == b // case.upw
        assert case.N % 4 == 0 and case.blocks == -(-case.N // case.upb) > 1
        if case.lanes < 64:  # (four units per block and N % 4 == 0 leave no short block at 64 lanes)
            assert case.N % case.upb == 4


# ---- exactly one right answer --------------------------------------------------------------------

@pytest.mark.parametrize("case", ref.AMAX_CASES, ids=lambda c: c.id)
def test_amax_scenarios_have_one_right_answer(case):
    kinds = set()
    for scen in ref.amax_scenarios(case):
        name, cols, kind = scen
        kinds.add(kind)
        x, w, norm_w, eps, winner = ref.amax_inputs(case, scen)
        if np.isfinite(w).all():
            assert np.array_equal(ref.dequant(w, case.storage), w), "the storage form holds the same model"
        z, parts = ref.amax_reference(case, x, w, norm_w)  # (asserts the logits are order-independent)
        assert ref.first_argmax(z) == winner, (case.id, name)
        assert ref.reduce_parts(parts)[1] == winner
        assert len(parts) == case.blocks and all(0 <= p["i"] < case.N for p in parts)
        if kind == "win":
            assert np.flatnonzero(z == z.max()).tolist() == sorted(cols), (case.id, name)
        elif kind == "zeros":
            assert z.max() == 0 and (z == 0).sum() == 3 and (z < 0).sum() == case.N - 3
        elif kind == "nan_inf":
            assert np.isnan(z).sum() == 1 and np.isposinf(z).sum() == 1
        else:
            b = cols[0] // case.upb
            assert np.isneginf(z[b * case.upb:(b + 1) * case.upb]).all() and parts[b]["i"] == b * case.upb
    assert kinds == ({"win"} if case.storage == "fp8" or case.norm else {"win", "zeros", "nan_inf", "neginf"})


def test_argmax_and_fold_tables_have_one_right_answer():
    for name, t, (v, i) in ref.argmax_tables() + ref.fold_tables():
        sv, si = scan(t)
        assert si == i and (sv == v or (sv != sv and v != v)), name
        # the same table in any order gives the same winner: the order is total
        perm = np.random.default_rng(len(t)).permutation(len(t))
        assert scan(t[perm])[1] == i, name
    for name, t, (v, i) in ref.argmax_tables():
        if "lower-index-later" in name or "empties" in name:
            continue
        row = np.full(int(t["i"].max()) + 1, -np.inf, np.float32)  # indices rise with the position: a logits row
        row[t["i"]] = t["v"]
        if not np.isneginf(t["v"]).all():
            assert ref.first_argmax(row) == i, name
    for name, t, _ in ref.fold_tables():
        assert t["i"].min() >= 0 and t["i"].max() < ref.FOLD_VOCAB, name
    for c in ref.FOLD_CASES:
        tab, w, norm_w = ref.fold_operands(c)
        assert len({r.tobytes() for r in tab}) == len(tab)
        assert np.array_equal(ref.dequant(w, c.storage), w)


@pytest.mark.parametrize("case", ref.ROWS_CASES, ids=lambda c: c.id)
def test_rows_inputs_have_one_right_answer(case):
    x, w, plan = ref.rows_inputs(case)
    z, rec = ref.rows_reference(case, x, w)
    assert rec.shape == (case.M, case.nct)
    cols = [c for p in plan for c in p]
    assert len(cols) == len(set(cols)) and plan[0] == [case.N - 1]
    if case.N % ref.TILE:
        assert plan[0][0] // ref.TILE == case.nct - 1  # the partial last tile
    for r in range(case.M):
        assert ref.reduce_parts(rec[r])[1] == ref.first_argmax(z[r])
        if plan[r] and not case.edge:
            assert np.flatnonzero(z[r] == z[r].max()).tolist() == sorted(plan[r]), (case.id, r)
    if case.edge:
        assert np.isnan(rec["v"][:, :2]).all() and np.isneginf(rec["v"][:, 2]).all() and np.isposinf(rec["v"][:, 3]).all()
        assert (rec["i"][:, 2] == 2 * ref.TILE).all()
    if case.force == 0:
        assert case.N * case.K > ref.SMALL_W and (case.N - 1) * case.K // 4 * 4 <= ref.SMALL_W + 4 * case.K


def test_rows_cases_cover_the_issue_matrix():
    forced = {(c.force, c.M, c.N) for c in ref.ROWS_CASES if c.force and not c.edge}
    assert forced == {(f, M, N) for f in (1, 2, 3) for M in (1, 17, 33, 70) for N in (192, 200)}
    assert sorted((c.M, c.route["bm"]) for c in ref.ROWS_CASES if not c.force) == [(9, 32), (40, 64), (70, 128)]
    placed = {c % ref.TILE for case in ref.ROWS_CASES if case.M == 70 for p in ref.rows_plan(case) for c in p}
    assert {0, 63} <= placed and {o // 16 for o in placed} == {0, 1, 2, 3} and {(o % 16) // 4 for o in placed} == {0, 1, 2, 3}


@pytest.mark.parametrize("case", ref.PARTS_CASES, ids=lambda c: c.id)
def test_parts_inputs(case):
    inp = ref.parts_inputs(case)
    xs, out, bound = ref.parts_reference(case, inp)
    base = inp["x"] if case.epi == epi_ref.SWIGLU else inp["c0"]
    seq = ref.sum_parts_f32(base, inp["parts"])
    assert np.abs(seq).max() <= 16  # small integers: the dot products stay exact
    for name in ("w", "wg", "wu"):
        if name in inp:
            assert np.array_equal(ref.dequant(inp[name], case.storage), inp[name])
    if case.kind == "order":
        p = inp["parts"].astype(np.float32)
        rev = base.copy()
        for h in reversed(range(case.nparts)):
            rev = rev + p[:, h]
        tree = base + p.sum(axis=1, dtype=np.float32)
        exact = base.astype(np.float64) + p.astype(np.float64).sum(axis=1)
        assert (rev != seq).any() and (tree != seq).any() and (exact != seq).any(), case.id
    # the guard row that follows the parts is non-zero everywhere
    assert (l3hip.gemm_sentinel((1, base.shape[1]), 12) != 0).all()


def test_parts_inputs_do_not_depend_on_the_storage():
    for epi in (epi_ref.SWIGLU,):
        cases = [c for c in ref.PARTS_CASES if c.epi == epi and c.K == ref.PARTS_XOUT_K]
        assert {c.storage for c in cases} == set(ref.STORAGES)
        for c in cases:
            a, b = ref.parts_inputs(c, "fp32"), ref.parts_inputs(c, "fp8")
            assert np.array_equal(a["x"], b["x"]) and np.array_equal(a["parts"], b["parts"])


def test_state_and_kv_tables():
    assert {ref.hist_slot(p, 0, b, c) for p, b, c, _ in ref.STATE_CASES} >= {None, 0, 7}
    for p, b, c, slot in ref.STATE_CASES:
        assert ref.hist_slot(p, 0, b, c) == slot
    slots = [ref.hist_slot(p, 1, b, c) for p, b, c in ref.FOLD_STATES]
    assert None in slots and 0 in slots and 7 in slots and slots.count(None) >= 2
    assert {p % ref.KV_BAK_SLOTS for p in ref.KV_POS} == {0, 31, 1, 7} and ref.KV_SMAX - 1 in ref.KV_POS
    assert sorted(c.rpb for c in ref.KV_CASES) == [1, 1, 1, 2, 4, 8]
    assert sorted(c.B for c in ref.KV_CASES if not c.big) == [1, 3, 8] and sorted(c.B for c in ref.KV_CASES if c.big) == [2, 4, 8]
    for c in ref.KV_CASES:
        assert c.KVH in (1, 2) and c.HD in (32, 64) and c.rpb * c.K <= 16384
        assert c.big == (c.rpb > 1)
        assert {d for _, d in ref.kv_positions(c)} == {False, True}
        assert [p for p, _ in ref.kv_positions(c)][::2 if not c.big else 1] == list(ref.KV_POS)


# ---- the entry points ----------------------------------------------------------------------------

def test_entry_points_are_exported_and_loud_without_a_device():
    lib = l3hip.lib()
    for name in ("l3_op_decode_gemm_host", "l3_op_argmax_parts_host", "l3_op_kv_restore_host"):
        assert name in l3hip.header_symbols()
    op = l3hip.DecodeGemmOp()
    assert lib.l3_op_decode_gemm_host(None, ctypes.byref(op)) != 0
    assert b"null context" in lib.l3_last_error()
    assert lib.l3_op_argmax_parts_host(None, None, 1, 1, 0, None, None) != 0
    assert lib.l3_op_kv_restore_host(None, None, 2, None, 1, 1, 1, 4, 0) != 0
    assert l3hip.ARGMAX_PART.itemsize == 8 and ref.PART == l3hip.ARGMAX_PART
    assert ref.KV_BAK_SLOTS == l3hip.KV_BAK_SLOTS
