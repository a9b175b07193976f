"""Sampling without a device: the generator's known answers, the host binding of the generator
against its NumPy restatement, the acceptance rule's power (it accepts a float32 restatement of
the rule and rejects near misses), and the argument checks of the C entry points."""

import numpy as np
import pytest

import l3hip
import sampling_ref as ref


def test_philox_known_answers():
    """Random123's Philox4x32-10 vectors."""
    f = 0xFFFFFFFF
    kat = [
        ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
        ((f, f, f, f), (f, f), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
        ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
         (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
    ]
    for ctr, key, want in kat:
        assert ref.philox4x32_10(ctr, key) == want


def test_host_uniform_matches_numpy_bit_for_bit():
    rng = np.random.default_rng(7)
    triples = [(0, 0, 0), (1 << 32, 0, 0), ((1 << 64) - 1, 0, 0), (5, 0, 17), (5, 3, 0),
               ((1 << 40) + 12345, 255, 2047)]
    while len(triples) < 1000:
        seed = int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2))
        if len(triples) % 3 == 0:
            seed &= 0xFFFFFFFF
        triples.append((seed, int(rng.integers(0, 256)), int(rng.integers(0, 1 << 20))))
    assert sum(s >= 1 << 32 for s, _, _ in triples) > 300
    for seed, row, pos in triples:
        u = l3hip.sample_uniform(seed, row, pos)
        assert 0.0 <= u < 1.0
        assert u == ref.uniform(seed, row, pos), (seed, row, pos)


@pytest.mark.parametrize("cfg", [ref.CONFIGS[0], ref.CONFIGS[2]])
def test_acceptance_rule_accepts_float32_and_rejects_mutants(cfg):
    n, scale, T, k, p = cfg
    rng = np.random.default_rng(n)
    draws = 200
    rejected = {"top_p ignored": 0, "T off by 5 %": 0, "u shifted by 0.01": 0}
    worst = 0.0
    for _ in range(draws):
        z = (rng.standard_normal(n) * scale).astype(np.float32)
        u = float(np.float32(rng.integers(0, 1 << 24)) * np.float32(2.0 ** -24))
        d = ref.distance(z, T, k, p, u, ref.sample(z, T, k, p, u, np.float32))
        worst = max(worst, d)
        assert d <= ref.TOL, d
        rejected["top_p ignored"] += not ref.accept(z, T, k, p, u, ref.sample(z, T, k, 1.0, u, np.float32))
        rejected["T off by 5 %"] += not ref.accept(z, T, k, p, u, ref.sample(z, T * 1.05, k, p, u, np.float32))
        rejected["u shifted by 0.01"] += not ref.accept(z, T, k, p, u,
                                                       ref.sample(z, T, k, p, min(u + 0.01, 1 - 2.0 ** -24), np.float32))
    print(f"float32 restatement worst distance {worst:.3e}; mutants rejected {rejected} of {draws}")
    for name, cnt in rejected.items():
        assert cnt >= 0.2 * draws, (name, cnt)


def test_reference_rule_small_cases():
    """The restatement itself on rows worked by hand."""
    z = np.array([0.0, 2.0, 1.0, 2.0, -np.inf], np.float32)
    idx, _ = ref.kept_set(z, 1.0, 2, 1.0)
    assert idx.tolist() == [1, 3]
    idx, _ = ref.kept_set(z, 1.0, 3, 1.0)
    assert idx.tolist() == [1, 2, 3]
    idx, _ = ref.kept_set(z, 1.0, 0, 0.3)  # masses 1, 1, 1/e, 1/e^2, 0 in rank order: total 2.503
    assert idx.tolist() == [1]
    idx, _ = ref.kept_set(z, 1.0, 0, 0.6)
    assert idx.tolist() == [1, 3]
    assert ref.sample(z, 1.0, 0, 1.0, 0.0) == 0
    assert ref.sample(z, 1.0, 0, 1.0, 1 - 2.0 ** -24) == 3
    assert ref.kept_set(np.array([1.0, np.nan]), 1.0, 0, 1.0) is None
    assert ref.sample(np.array([1.0, np.nan, np.nan]), 1.0, 0, 1.0, 0.3) == 1
    assert ref.sample(np.array([1.0, np.inf]), 1.0, 0, 1.0, 0.3) == 1
    assert ref.sample(np.array([-np.inf, -np.inf]), 1.0, 0, 1.0, 0.9) == 0


def test_set_sampling_without_context_is_loud():
    lib = l3hip.lib()
    assert lib.l3_set_sampling(None, 0.8, 0, 0.9, 0) != 0
    assert b"null context" in lib.l3_last_error()
    assert lib.l3_get_sampling(None, None, None, None, None) != 0
    assert b"null context" in lib.l3_last_error()
    x, out = np.zeros(4, np.float32), np.zeros(1, np.int32)
    with pytest.raises(RuntimeError, match="null context"):
        l3hip.check(lib.l3_op_sample_host(None, l3hip.ptr(x), 1, 4, 0.8, 0, 0.9, None, 0, 0, 0, l3hip.ptr(out)))
    assert lib.l3_sample_uniform(0, 0, 0, None) != 0
    assert b"null argument" in lib.l3_last_error()


@pytest.mark.parametrize("T,k,p,msg", [
    (float("nan"), 0, 1.0, "temperature"), (-0.5, 0, 1.0, "temperature"), (float("inf"), 0, 1.0, "temperature"),
    (0.8, -1, 1.0, "top_k -1 must be >= 0"),
    (0.8, 0, 0.0, "top_p"), (0.8, 0, 1.5, "top_p"), (0.8, 0, float("nan"), "top_p"), (0.8, 0, -0.1, "must be in (0, 1]"),
])
def test_out_of_range_sampling_arguments_are_rejected_with_a_message(T, k, p, msg):
    """Checked before the context, so no device is needed to tell."""
    lib = l3hip.lib()
    assert lib.l3_set_sampling(None, T, k, p, 0) != 0
    err = lib.l3_last_error().decode()
    assert msg in err and "l3_set_sampling" in err, err
    assert lib.l3_op_sample_host(None, None, 1, 4, T, k, p, None, 0, 0, 0, None) != 0
    err = lib.l3_last_error().decode()
    assert msg in err and "l3_op_sample_host" in err, err


def test_op_sample_rejects_bad_shapes_and_uniforms_without_a_device():
    lib = l3hip.lib()
    x = np.zeros(4, np.float32)
    out = np.zeros(1, np.int32)
    assert lib.l3_op_sample_host(None, l3hip.ptr(x), 0, 4, 0.8, 0, 0.9, None, 0, 0, 0, l3hip.ptr(out)) != 0
    assert b"bad shape" in lib.l3_last_error()
    for bad in (1.0, -0.25, float("nan")):
        u = np.array([bad], np.float32)
        assert lib.l3_op_sample_host(None, l3hip.ptr(x), 1, 4, 0.8, 0, 0.9, l3hip.ptr(u), 0, 0, 0, l3hip.ptr(out)) != 0
        assert b"outside [0, 1)" in lib.l3_last_error()
