"""The exact-pick tables of test_gpu_sampling_exact.py without a device: the integer model of
sampling_exact_ref agrees with sampling_ref's float64 rule on every case, and the tables reach
what they are meant to reach (bucket widths, waves, cuts inside the second plateau, key levels)."""

import numpy as np
import pytest

import sampling_exact_ref as ex
import sampling_ref as ref


def test_kernel_geometry_restated():
    """n against ch and s (DESIGN.md "Exact picks")."""
    assert [ex.geometry(n) for n in ex.REG_SIZES] == [(True, 2048, 1), (True, 2048, 1), (True, 2048, 2),
                                                      (True, 2048, 16), (True, 2048, 16)]
    assert [ex.geometry(n) for n in ex.LONG_SIZES] == [(False, 2112, 16), (False, 2560, 16), (False, 4160, 16),
                                                       (False, 8256, 16), (False, 16448, 16)]
    assert [ex.search_shift(n) for n in ex.LONG_SIZES] == [0, 0, 1, 2, 3]
    assert 65537 - 15 * 4160 == 3137 and ex.bucket_shift(3137) == 0
    assert {ex.search_shift(n) for n in ex.REG_SIZES} == {0}
    assert sum(ex.geometry(n)[2] > 1 for n in ex.REG_SIZES) >= 3


def test_integer_products():
    rng = np.random.default_rng(1)
    for _ in range(2000):
        a, f = int(rng.integers(0, 1 << 62)), int(rng.integers(0, 1 << 32))
        assert ex.mul_frac_floor(a, f) == a * f >> 32
        assert ex.mul_frac_ceil(a, f) == -(-a * f >> 32)
    assert ex.frac_of(0.0) == 0 and ex.frac_of(ex.U_LAST) == ex.W and ex.frac_of(0.5) == 1 << 31
    assert int(float(np.float32(0.9)) * 2.0 ** 32) == 0xE6666600


@pytest.mark.parametrize("n", ex.REG_SIZES + ex.LONG_SIZES)
def test_plateau_model_is_the_float64_rule(n):
    _, ch, waves = ex.geometry(n)
    cases, kinds, waves_hit, seen, values = 0, set(), set(), set(), set()
    exact_cut = inexact_cut = crossing = 0
    for c in ex.plateau_calls(n):
        idx, w = ref.kept_set(c.z, c.T, c.top_k, float(np.float32(c.top_p)))
        assert np.array_equal(idx, c.meta["kept"]), c.label
        assert len(c.u) >= 2 and c.u[0] == 0.0 and c.u[-1] == np.float32(ex.U_LAST)
        got = [ref.draw(idx, w, float(u)) for u in c.u]
        assert got == c.want, (c.label, c.u.tolist(), got, c.want)
        members = idx[w > 0]
        assert c.want[0] == members[0] and c.want[-1] == members[-1]
        assert (w[w > 0] == 1.0).all()
        cases += len(c.u)
        kinds.add(c.meta["kind"])
        if c.meta["M"] > 1:
            values.add(c.meta["value"])
        waves_hit |= set((np.asarray(c.want) // ch).tolist())
        seen.add((c.top_p, min(c.top_k, c.meta["M"] + 2)))
        if c.top_p in (0.5, 0.75) and c.meta["M"] > 1:
            whole = c.meta["M"] * c.top_p == int(c.meta["M"] * c.top_p)
            exact_cut += whole
            inexact_cut += not whole
        crossing += len(set((members // ch).tolist())) > 1
    print(f"n {n}: {cases} cases, kinds {sorted(kinds)}, waves picked from {sorted(waves_hit)}")
    assert {"ends", "single", "scattered"} <= kinds
    # the mixed zeros tie on a plateau of several members at every size
    assert "zeros" in values and len(values) >= 3 and (n <= 2048 or values == set(ex.PLATEAU_VALUES))
    assert all(any(p == q for q, _ in seen) for p in ex.TOP_PS)
    if n > 7:
        assert "buckets" in kinds and exact_cut and inexact_cut
    if waves > 1:
        assert "waves" in kinds and crossing and {0, waves - 1} <= waves_hit and len(waves_hit) >= min(waves, 3)
    if n in (2049, 65537):
        assert "dense" in kinds


def test_two_plateau_cases_survive_and_cover():
    for n in (32000, 65537):
        kept = candidates = 0
        thirds, crosses = set(), 0
        for c, cand in ex.two_plateau_calls(n):
            candidates += cand
            kept += len(c.u)
            if not len(c.u):
                continue
            thirds.add(c.meta["third"])
            crosses += c.meta["crosses"]
            # the float64 rule's weight of the second plateau lies inside the +-1e-4 band too
            idx, w = ref.kept_set(c.z, c.T, c.top_k, float(np.float32(c.top_p)))
            assert np.array_equal(idx, c.meta["kept"]), c.label
            assert abs(w.min() - 0.5) < 1e-6 and w.max() == 1.0
            assert [ref.draw(idx, w, float(u)) for u in c.u] == c.want, c.label
        print(f"n {n}: {kept} of {candidates} two-plateau cases kept, {crosses} calls cross a wave boundary")
        assert 2 * kept >= candidates
        assert thirds == {0, 1, 2} and crosses


@pytest.mark.parametrize("n", [32000, 40001])
def test_top_k_rows_are_what_they_claim(n):
    _, ch, _ = ex.geometry(n)
    rows = dict((name, (z, ks)) for name, z, ks in ex.topk_rows(n))
    assert set(rows) == {"share12", "share22", "negative", "zeros", "denormal", "tie6"}
    for name, (z, ks) in rows.items():
        assert z.shape == (n,) and z.dtype == np.float32 and max(ks) <= 8
        order = np.argsort(-z.astype(np.float64), kind="stable")
        top = z[order[:8]].astype(np.float64)
        assert np.isfinite(top).all() and top[0] - top[-1] <= 2.0
        key = ex.order_key(z)
        assert (np.diff(key[order].astype(np.int64)) <= 0).all()  # the keys' order is the values'
    key = ex.order_key(rows["share12"][0])
    assert len(set(key >> 20)) == 1 and len(set(key)) == n
    srt = np.sort(key)[::-1]
    assert len(set(srt[:4] >> 10)) == 4 and len(set(srt[4:9] >> 10)) == 1  # level 1, then level 2, decides
    key = np.sort(ex.order_key(rows["share22"][0]))[::-1]
    assert len(set(key >> 20)) == 1 and len(set(key[:12] >> 10)) == 1 and len(set(key[:12])) == 12
    z = rows["negative"][0]
    key = np.sort(ex.order_key(z))[::-1]
    assert (z < 0).all() and len(set(key >> 20)) == 1
    assert len(set(key[:4] >> 10)) == 4 and len(set(key[4:10] >> 10)) == 1 and len(set(key[4:10])) == 6
    z = rows["zeros"][0]
    zero = np.flatnonzero(z == 0)
    assert np.signbit(z[zero]).tolist() == [True, False, True, False, True] and (z > 0).sum() == 2
    assert len(set(ex.order_key(z)[zero])) == 1
    z = rows["denormal"][0]
    assert (np.abs(z) < np.finfo(np.float32).tiny).all() and (z != 0).all() and (z < 0).any() and (z > 0).any()
    z, ks = rows["tie6"]
    tie = np.flatnonzero(z == np.sort(z)[-3])
    assert tie.size == 6 and (tie // ch).tolist() == [6, 6, 6, 7, 7, 7] and ks == (3, 5, 7)
    for k, members in zip(ks, (1, 3, 5)):
        assert set(tie[:members]) <= set(ref.kept_set(z, 100.0, k, 1.0)[0].tolist())
        assert tie[members] not in ref.kept_set(z, 100.0, k, 1.0)[0]
