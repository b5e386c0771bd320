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


def hbm_words(first, n, seed):
    """Memory-path pattern, from its definition: element i (16 bytes) holds
    words k = 0..3, word = mix32(low32(4*i + k) + mix32(seed + (i >> 30))).
    The 34-bit word index of the 64 GiB maximum is split: its low 32 bits are
    mixed directly, its top bits (i >> 30) choose the base. Returns the 4*n
    words of elements first .. first+n in memory order. (Also used by the GPU
    tests, as is lds_words.)"""
    i = np.arange(first, first + n, dtype=np.uint64)
    base = _mix32(U(seed) + (i >> np.uint64(30)).astype(U))
    index = i[:, None] * np.uint64(4) + np.arange(4, dtype=np.uint64)[None, :]
    low = (index & np.uint64(0xFFFFFFFF)).astype(U)
    return _mix32(low + base[:, None]).reshape(-1)


def lds_words(first, n, seed):
    """LDS march pattern: word w holds mix32(w * 0x9E3779B9 + seed)."""
    w = np.arange(first, first + n, dtype=np.uint64).astype(U)
    return _mix32(w * U(0x9E3779B9) + U(seed))


PATTERN_SEEDS = [0, 0x5EED1234, 0xFFFFFFFF]
# (first element, count): the start of a buffer; the elements around 2^30,
# where the word index passes 2^32; the last elements of the 64 GiB maximum
HBM_RANGES = [(0, 4096), ((1 << 30) - 2, 4), ((1 << 32) - 4, 4)]
TEST_BUFFER_WORDS = ((1 << 20) + 16) // 4  # the scratch buffer of the GPU tests
FULL_LDS_WORDS = probes.SELFTEST_MAX_LDS // 4


@pytest.mark.parametrize("seed", PATTERN_SEEDS)
@pytest.mark.parametrize("first, n", HBM_RANGES)
def test_hbm_pattern_matches_numpy_oracle(seed, first, n):
    got = np.array(probes.selftest_hbm_words(first, n, seed), dtype=U)
    assert got.shape == (4 * n,)
    assert np.array_equal(got, hbm_words(first, n, seed))


@pytest.mark.parametrize("seed", PATTERN_SEEDS)
def test_lds_pattern_matches_numpy_oracle(seed):
    got = np.array(probes.selftest_lds_words(0, FULL_LDS_WORDS, seed), dtype=U)
    assert np.array_equal(got, lds_words(0, FULL_LDS_WORDS, seed))
    # a range that does not start at word 0
    got = probes.selftest_lds_words(FULL_LDS_WORDS - 3, 3, seed)
    assert got == lds_words(FULL_LDS_WORDS - 3, 3, seed).tolist()


HBM_LITERAL_5 = [0xB0F32E7B, 0x4ED33942, 0x7C2F3B42, 0xB550FDFC]
HBM_LITERAL_2_30 = [0x256ED7E7, 0x9C5BFF77, 0x3EA41702, 0xCD705CB3,
                    0x1053218A, 0x2C99BDF2, 0x0BC690C9, 0xCC3419C6]
HBM_LITERAL_LAST = [0x0EDCFFDA, 0x1F22948E, 0x005CD305, 0x123A4A88]
LDS_LITERAL_255 = [0xA9C4CDC2, 0x9BAD4BAF, 0x5A47CEC1]
LDS_LITERAL_LAST = [0xC272BD73]


def test_pattern_literals():
    """Values taken from the oracle above when it was written;
    native/selftest_ref_selftest.cpp checks the same literals against the
    header in a plain C++ build."""
    for words in (probes.selftest_hbm_words, lambda *a: hbm_words(*a).tolist()):
        assert words(0, 1, 0) == [0x00000000, 0x688990C0, 0xD1132181, 0x53F1E9DD]
        assert words(5, 1, 0x5EED1234) == HBM_LITERAL_5
        assert words((1 << 30) - 1, 2, 0x5EED1234) == HBM_LITERAL_2_30
        assert words((1 << 32) - 1, 1, 0xFFFFFFFF) == HBM_LITERAL_LAST
    for words in (probes.selftest_lds_words, lambda *a: lds_words(*a).tolist()):
        assert words(0, 2, 0) == [0x00000000, 0x01FCE552]
        assert words(255, 3, 0x5EED1234) == LDS_LITERAL_255
        assert words(40959, 1, 0xFFFFFFFF) == LDS_LITERAL_LAST


@pytest.mark.parametrize("seed", PATTERN_SEEDS)
def test_pattern_words_are_distinct(seed):
    """mix32 is a bijection of the 32-bit words and so is adding a constant
    or multiplying by an odd one, hence two addresses of one buffer never hold
    the same word: a write that lands on the wrong address line, at any
    distance, is a miscompare."""
    hbm = np.array(probes.selftest_hbm_words(0, TEST_BUFFER_WORDS // 4, seed), dtype=U)
    assert hbm.size == TEST_BUFFER_WORDS and np.unique(hbm).size == hbm.size
    distance = 1
    while distance < hbm.size:  # follows from the line above; kept explicit
        assert not (hbm[distance:] == hbm[:-distance]).any(), distance
        distance *= 2
    lds = np.array(probes.selftest_lds_words(0, FULL_LDS_WORDS, seed), dtype=U)
    assert lds.size == 40960 and np.unique(lds).size == lds.size
    # beyond 2^30 elements the low index repeats and only the base differs
    far = probes.selftest_hbm_words(1 << 30, 1, seed)
    assert all(a != b for a, b in zip(far, hbm[:4].tolist()))


@pytest.mark.parametrize(
    "call, needle",
    [
        (lambda: probes.selftest_hbm_words((1 << 32) - 1, 2), "elements"),
        (lambda: probes.selftest_hbm_words((1 << 32) + 1, 0), "elements"),
        (lambda: probes.selftest_lds_words(40959, 2), "words"),
        (lambda: probes.selftest_lds_words(40961, 0), "words"),
    ],
)
def test_pattern_exports_reject_ranges_past_the_maximum(call, needle):
    with pytest.raises(probes.ProbeError, match=needle) as ei:
        call()
    assert "rc=-1" in str(ei.value)


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
        # the placed LDS injection: a word outside lds_bytes, a pass that is
        # neither the pattern nor the complement
        (dict(_inject=("lds", 0, 256, 0), lds_bytes=1024), "inject_sub word"),
        (dict(_inject=("lds", 0, 257, 1), lds_bytes=1028), "inject_sub word"),
        (dict(_inject=("lds", 0, 8192, 0), lds_bytes=32768), "inject_sub word"),
        (dict(_inject=("lds", 0, 40960, 1), lds_bytes=163840), "inject_sub word"),
        (dict(_inject=("lds", 0, 0, 2)), "inject_sub .* pass"),
        (dict(_inject=("lds", 0, 0, 127)), "inject_sub .* pass"),
        (dict(_inject=("lds", 3, 0, 0), blocks=3), "inject_arg"),
    ],
)
def test_bad_arguments_fail_before_any_gpu_call(kwargs, needle):
    """Validation comes before the first HIP call: the same error code with
    or without a GPU, and nothing is launched."""
    with pytest.raises(probes.ProbeError, match=needle) as ei:
        probes.selftest(0, **kwargs)
    assert "rc=-1" in str(ei.value)


def test_records_validate_the_placed_injection_too():
    with pytest.raises(probes.ProbeError, match="inject_sub word") as ei:
        probes.selftest_records(0, blocks=3, lds_bytes=1024, _inject=("lds", 1, 256, 1))
    assert "rc=-1" in str(ei.value)


@pytest.mark.parametrize("inject", [("mfma", 0, 0, 0), ("lds", 0, 1 << 24, 0),
                                    ("lds", 0, 0, 128), ("lds", 0, -1, 0), ("lds", 0, 5)])
def test_placed_injection_without_an_encoding_is_a_value_error(inject):
    with pytest.raises(ValueError):
        probes.selftest(0, _inject=inject)


BUF = (1 << 20) + 16


@pytest.mark.parametrize(
    "kwargs, needle",
    [
        (dict(corrupt=range(0, 4 * 65, 4)), "65 corrupt offsets"),
        (dict(corrupt=[4098]), "offset 4098"),
        (dict(corrupt=[BUF]), f"offset {BUF}"),
        (dict(corrupt=[8, 4096, 8]), "offset 8 is given twice"),
        (dict(corrupt=[0], corrupt_pass=2), "corrupt_pass"),
        (dict(corrupt=[0], corrupt_pass=-1), "corrupt_pass"),
        (dict(hbm_bytes=BUF + 8), "hbm_bytes"),
        (dict(hbm_bytes=0, corrupt=[0]), "offset 0"),
    ],
)
def test_memory_check_entry_rejects_bad_arguments_before_any_gpu_call(kwargs, needle):
    kwargs = {"hbm_bytes": BUF, **kwargs}
    kwargs["corrupt"] = list(kwargs.get("corrupt", ()))
    with pytest.raises(probes.ProbeError, match=needle) as ei:
        probes.selftest_hbm(0, seed=1, **kwargs)
    assert "rc=-1" in str(ei.value)


@pytest.mark.parametrize(
    "hbm_bytes, march_pass, needle",
    [
        (probes.SELFTEST_MAX_IMAGE + 16, 0, "hbm_bytes"),
        (0, 0, "hbm_bytes"),
        (24, 1, "hbm_bytes"),
        (16, 2, "pass"),
        (16, -1, "pass"),
    ],
)
def test_memory_image_rejects_bad_arguments_before_any_gpu_call(hbm_bytes, march_pass, needle):
    assert probes.SELFTEST_MAX_IMAGE == (16 << 20) + 16
    with pytest.raises(probes.ProbeError, match=needle) as ei:
        probes.selftest_hbm_image(0, hbm_bytes, 1, march_pass)
    assert "rc=-1" in str(ei.value)


def test_mfma_tile_rejects_bad_pattern_and_rounds():
    with pytest.raises(probes.ProbeError, match="pattern"):
        probes.selftest_mfma_tile(0, 64, 0, 1)
    with pytest.raises(probes.ProbeError, match="rounds"):
        probes.selftest_mfma_tile(0, 0, 0, 0)
