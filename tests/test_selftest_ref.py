"""Host reference of the GPU self-test (native/selftest_ref.h), reached through
the C ABI of libegpu_kernels.so, which needs no GPU for these calls.

The oracle below is written independently in numpy from the description of
the checks (uint32 arithmetic for the integer chain; an integer matmul, the
C/D lane map and the hash for the MFMA signature; float64 for the FMA chain,
see _fma_chain). The literals pin the values, so that reference and kernel
cannot drift together.
"""
import numpy as np
import pytest

from elastic_gpu_agent_amd.isolation import probes

U = np.uint32
LANES = np.arange(64, dtype=np.uint32)


@pytest.fixture(autouse=True)
def _wrapping_uint32():
    with np.errstate(over="ignore"):
        yield


def _mix32(x):
    x = x.astype(U) if isinstance(x, np.ndarray) else U(x)
    x = x ^ (x >> U(16))
    x = x * U(0x7FEB352D)
    x = x ^ (x >> U(15))
    x = x * U(0x846CA68B)
    return x ^ (x >> U(16))


def _rotl(x, k):
    return (x << U(k)) | (x >> U(32 - k))


def _lane_seeds(seed, pattern, stream):
    s = _mix32(U(seed) + U(pattern) * U(0x9E3779B9))
    return _mix32(s + LANES * U(0x85EBCA6B) + U(stream) * U(0xC2B2AE35))


def _weights():
    return (U(2) * LANES + U(1)) * U(0x01000193)


def _reduce(values):
    return int((values.astype(U) * _weights()).sum(dtype=np.uint64) & 0xFFFFFFFF)


def _popcount(x):
    return np.array([bin(int(v)).count("1") for v in x], dtype=U)


def _int_sig(seed, pattern, rounds):
    x = _lane_seeds(seed, pattern, 0)
    h = np.zeros(64, dtype=U)
    for _ in range(rounds):
        x = x * U(1664525) + U(1013904223)
        x = x ^ (x << U(13))
        x = x ^ (x >> U(17))
        x = x ^ (x << U(5))
        hi = ((x.astype(np.uint64) * np.uint64(0x9E3779B9)) >> np.uint64(32)).astype(U)
        h = _rotl(h, 5) ^ hi
        h = h + _popcount(x)
    return _reduce(h ^ x)


def _unit(bits):
    return ((bits & U(0x007FFFFF)) | U(0x3F800000)).view(np.float32)


def _fma_chain(s, rounds):
    """x, a, b in [1,2) are 24-bit values: x*a has at most 48 significant
    bits and x*a+b at most 49 (it is below 6, with 46 fraction bits), so the
    float64 expression is exact and the one conversion to float32 rounds once,
    to nearest even: the definition of fmaf."""
    x = _unit(s)
    a = _unit(_mix32(s + U(1)))
    b = _unit(_mix32(s + U(2)))
    h = np.zeros_like(s)
    for _ in range(rounds):
        y = (x.astype(np.float64) * a.astype(np.float64) + b.astype(np.float64))
        u = y.astype(np.float32).view(U)
        x = _unit(u)
        h = _rotl(h, 7) + (u & U(0x007FFFFF))
    return h


def _fma_sig(seed, pattern, rounds):
    return _reduce(_fma_chain(_lane_seeds(seed, pattern, 1), rounds))


def _operands(seed, pattern, rnd):
    """A (32x16) and B (16x32) of one round from the A/B lane maps."""
    s = _lane_seeds(seed, pattern, 2)
    wa = _mix32(s + U(2 * rnd))
    wb = _mix32(s + U(2 * rnd + 1))
    a = np.zeros((32, 16), dtype=np.int64)
    b = np.zeros((16, 32), dtype=np.int64)
    for lane in range(64):
        for j in range(8):
            k = 8 * (lane >> 5) + j
            a[lane & 31, k] = ((int(wa[lane]) >> (3 * j)) & 7) % 7 - 3
            b[k, lane & 31] = ((int(wb[lane]) >> (3 * j)) & 7) % 7 - 3
    return a, b


def tile_signature(d):
    """Signature of a 32x32 integer tile: per lane, hash the 16 accumulators
    found through the C/D lane map, then the weighted lane sum. (Also used by
    the GPU tests.)"""
    hashes = np.zeros(64, dtype=U)
    for lane in range(64):
        h = 0
        for reg in range(16):
            row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
            h = (h * 0x01000193 + int(d[row][lane & 31])) & 0xFFFFFFFF
        hashes[lane] = h
    return _reduce(hashes)


def _mfma_sig(seed, pattern, rounds):
    d = np.zeros((32, 32), dtype=np.int64)
    for r in range(rounds):
        a, b = _operands(seed, pattern, r)
        assert np.abs(a).max() <= 3 and np.abs(b).max() <= 3
        d += a @ b
    return tile_signature(d)


@pytest.mark.parametrize("seed", [0, 0x1234ABCD])
@pytest.mark.parametrize("rounds", [1, 2, 5])
def test_reference_matches_numpy_oracle(seed, rounds):
    got = probes.selftest_expected(seed, rounds)
    assert len(got) == 64
    for pattern in range(64):
        want = (_int_sig(seed, pattern, rounds), _fma_sig(seed, pattern, rounds),
                _mfma_sig(seed, pattern, rounds))
        assert got[pattern] == want, f"pattern {pattern}"


def test_literal_signatures():
    """Values fixed when the checks were written; the FMA ones are what
    std::fmaf gives (native/selftest_ref_selftest.cpp checks the same
    literals in a plain C++ build)."""
    e = probes.selftest_expected(0, 4)
    assert e[0] == (0x3EA752FF, 0x29C8A963, 0x63D636BE)
    assert e[1] == (0x5D888A1C, 0x59A04B97, 0x58FAF12B)
    f = probes.selftest_expected(0x1234ABCD, 5)
    assert f[63] == (0xBB87C225, 0x2DAC9D18, 0x89BB1E15)


def test_patterns_are_distinct():
    e = probes.selftest_expected(3, 2)
    for field in range(3):
        assert len({rec[field] for rec in e}) == 64


def test_expected_is_deterministic_and_seeded():
    assert probes.selftest_expected(9, 3) == probes.selftest_expected(9, 3)
    assert probes.selftest_expected(9, 3) != probes.selftest_expected(10, 3)


@pytest.mark.parametrize("rounds", [0, -1, probes.SELFTEST_MAX_ROUNDS + 1])
def test_expected_rejects_rounds(rounds):
    with pytest.raises(probes.ProbeError, match="rounds"):
        probes.selftest_expected(0, rounds)


def test_rounds_bound_keeps_accumulator_exact():
    # |acc| <= rounds * 16 products of at most 3*3
    assert probes.SELFTEST_MAX_ROUNDS * 16 * 9 < 2 ** 24


@pytest.mark.parametrize(
    "kwargs, needle",
    [
        (dict(hbm_bytes=(1 << 20) + 8), "hbm_bytes"),
        (dict(rounds=0), "rounds"),
        (dict(rounds=probes.SELFTEST_MAX_ROUNDS + 1), "rounds"),
        (dict(blocks=0), "blocks"),
        (dict(blocks=-3), "blocks"),
        (dict(lds_bytes=probes.SELFTEST_MAX_LDS + 4), "lds_bytes"),
        (dict(lds_bytes=32770), "lds_bytes"),
        (dict(_inject=("mfma", 17), blocks=17), "inject_arg"),
        (dict(_inject=("hbm", 4098)), "inject_arg"),
    ],
)
def test_bad_arguments_fail_before_any_gpu_call(kwargs, needle):
    """Validation comes before the first HIP call: the same error code with
    or without a GPU, and nothing is launched."""
    with pytest.raises(probes.ProbeError, match=needle) as ei:
        probes.selftest(0, **kwargs)
    assert "rc=-1" in str(ei.value)


def test_mfma_tile_rejects_bad_pattern_and_rounds():
    with pytest.raises(probes.ProbeError, match="pattern"):
        probes.selftest_mfma_tile(0, 64, 0, 1)
    with pytest.raises(probes.ProbeError, match="rounds"):
        probes.selftest_mfma_tile(0, 0, 0, 0)
