"""Host reference of the matrix sweep (native/selftest_mx_ref.h), reached
through the C ABI of libegpu_kernels.so, which needs no GPU for these calls.

The oracle below is independent of the header's reference: it takes the
ENCODED lane registers the generator emits (mx_selftest_lane_regs), unpacks
them with Python integers, decodes them with literal tables written here (FP4,
FP6), torch's float8 views (e4m3fn, e5m2), numpy views (f16, bf16, int8) and
2.0**(e-127) for E8M0, places them through lane maps written here, multiplies
in float64, reads the tile back through the C/D map and hashes. A second
oracle regenerates the 3-bit codes from the seed alone and checks that the
decoded bits are the table entries the codes name. The literals pin the values.
"""
import ctypes

import numpy as np
import pytest
import torch

from elastic_gpu_agent_amd.isolation import probes

from test_selftest_ref import U, _lane_seeds, _mix32, _reduce

KINDS = list(probes.MX_KINDS)
TABLE = [0.0, 0.5, -1.0, 1.5, 2.0, -3.0, 4.0, -6.0]

# OCP MX element formats, every code
FP4 = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0,
       -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0]
_FP6_POS = [0.0, 0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875,
            1.0, 1.125, 1.25, 1.375, 1.5, 1.625, 1.75, 1.875,
            2.0, 2.25, 2.5, 2.75, 3.0, 3.25, 3.5, 3.75,
            4.0, 4.5, 5.0, 5.5, 6.0, 6.5, 7.0, 7.5]
FP6 = _FP6_POS + [-v for v in _FP6_POS]

# kind -> (M, K, bits and decoder name of A, of B, scaled)
FORMATS = {
    "f16": (32, 16, (16, "f16"), (16, "f16"), False),
    "i8": (32, 32, (8, "i8"), (8, "i8"), False),
    "fp8": (32, 16, (8, "e4m3"), (8, "e4m3"), False),
    "bf8": (32, 16, (8, "e5m2"), (8, "e5m2"), False),
    "bf16s": (16, 32, (16, "bf16"), (16, "bf16"), False),
    "mxfp8": (32, 64, (8, "e4m3"), (8, "e4m3"), True),
    "mxfp6": (32, 64, (6, "e2m3"), (6, "e2m3"), True),
    "mxfp4": (32, 64, (4, "e2m1"), (4, "e2m1"), True),
    "mxmix": (16, 128, (8, "e4m3"), (4, "e2m1"), True),
}


@pytest.fixture(autouse=True)
def _wrapping_uint32():
    with np.errstate(over="ignore"):
        yield


def _decode(name, codes):
    codes = np.asarray(codes, dtype=np.uint32)
    if name == "e2m1":
        return np.array([FP4[c] for c in codes])
    if name == "e2m3":
        return np.array([FP6[c] for c in codes])
    if name == "e4m3":
        return torch.tensor(codes.astype(np.uint8)).view(torch.float8_e4m3fn).double().numpy()
    if name == "e5m2":
        return torch.tensor(codes.astype(np.uint8)).view(torch.float8_e5m2).double().numpy()
    if name == "f16":
        return codes.astype(np.uint16).view(np.float16).astype(np.float64)
    if name == "bf16":
        return (codes << U(16)).view(np.float32).astype(np.float64)
    assert name == "i8"
    return codes.astype(np.uint8).view(np.int8).astype(np.float64)


def _unpack(regs, count, bits):
    """element j of a lane's registers: little-endian, contiguous"""
    big = sum(int(w) << (32 * i) for i, w in enumerate(regs))
    assert big >> (count * bits) == 0, "bits above the last element"
    return [(big >> (j * bits)) & ((1 << bits) - 1) for j in range(count)]


def _k_of(m, k, bits, scaled, lane, j):
    """The A/B lane map: contiguous, but an 8-bit operand of a scaled
    instruction is two runs of 16, the second K/2 further on."""
    e = k * m // 64
    if scaled and bits == 8:
        return 16 * (lane // m) + j % 16 + (k // 2) * (j // 16)
    return e * (lane // m) + j


def _cd_row(m, lane, reg):
    if m == 32:
        return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
    return 4 * (lane >> 4) + reg


def round_operands(kind, pattern, seed, rnd):
    """(A, B, EA, EB): decoded M x K and K x M operands and the scale exponents
    per (row, k-block) and (k-block, column), from the encoded registers."""
    m, k, (abits, aname), (bbits, bname), scaled = FORMATS[kind]
    e = k * m // 64
    ra, rb, sa, sb = probes.mx_selftest_lane_regs(kind, pattern, seed, rnd)
    a = np.zeros((m, k))
    b = np.zeros((k, m))
    nkb = k // 32 if scaled else 1
    ea = np.zeros((m, nkb))
    eb = np.zeros((nkb, m))
    for lane in range(64):
        va = _decode(aname, _unpack(ra[lane], e, abits))
        vb = _decode(bname, _unpack(rb[lane], e, bbits))
        for j in range(e):
            a[lane % m, _k_of(m, k, abits, scaled, lane, j)] = va[j]
            b[_k_of(m, k, bbits, scaled, lane, j), lane % m] = vb[j]
        if scaled:
            # A's live byte is byte 0, B's is byte 2; a lane's scale belongs
            # to k-block lane // m of its row (column)
            ea[lane % m, lane // m] = (sa[lane] & 0xFF) - 127
            eb[lane // m, lane % m] = ((sb[lane] >> 16) & 0xFF) - 127
        else:
            assert sa[lane] == 0 and sb[lane] == 0
    return a, b, ea, eb


def tile(kind, pattern, seed, rounds):
    m, k, _, _, scaled = FORMATS[kind]
    d = np.zeros((m, m))
    kb_len = 32 if scaled else k
    for r in range(rounds):
        a, b, ea, eb = round_operands(kind, pattern, seed, r)
        for kb in range(k // kb_len):
            part = a[:, kb * kb_len:(kb + 1) * kb_len] @ b[kb * kb_len:(kb + 1) * kb_len, :]
            d += part * 2.0 ** (ea[:, kb][:, None] + eb[kb, :][None, :])
    return d


def mx_tile_signature(kind, units):
    """Signature of a tile given in hash units (acc*4; i8: acc): per lane,
    hash its accumulators through the C/D lane map, then the weighted lane sum.
    (Also used by the GPU tests.)"""
    m = FORMATS[kind][0]
    hashes = np.zeros(64, dtype=U)
    for lane in range(64):
        h = 0
        for reg in range(m * m // 64):
            v = int(units[_cd_row(m, lane, reg)][lane % m])
            h = (h * 0x01000193 + v) & 0xFFFFFFFF
        hashes[lane] = h
    return _reduce(hashes)


def _units(kind, d):
    scaled = d if kind == "i8" else d * 4
    assert np.array_equal(scaled, np.round(scaled)), "not a whole number of hash units"
    return scaled.astype(np.int64)


@pytest.fixture(scope="module")
def expected():
    return {(seed, rounds): probes.mx_selftest_expected(seed, rounds)
            for seed in (0, 0x5EED1234) for rounds in (1, 5)}


@pytest.mark.parametrize("seed", [0, 0x5EED1234])
@pytest.mark.parametrize("rounds", [1, 5])
def test_reference_matches_numpy_oracle(expected, seed, rounds):
    got = expected[(seed, rounds)]
    assert len(got) == 16
    for pattern in (0, 1, 7, 15):
        for kind in KINDS:
            want = mx_tile_signature(kind, _units(kind, tile(kind, pattern, seed, rounds)))
            assert got[pattern][kind] == want, f"{kind}, pattern {pattern}"


def test_literal_signatures():
    """Values fixed when the sweep was written (native/selftest_mx_ref_selftest.cpp
    checks the same literals in a plain C++ build)."""
    e = probes.mx_selftest_expected(0, 4)
    assert e[0] == LITERAL_SEED0_ROUNDS4_PATTERN0
    f = probes.mx_selftest_expected(0x1234ABCD, 5)
    assert f[15] == LITERAL_SEED1234ABCD_ROUNDS5_PATTERN15


LITERAL_SEED0_ROUNDS4_PATTERN0 = {
    "f16": 0xD31CA4DC, "i8": 0xD2B496C9, "fp8": 0xEF4FDAFC, "bf8": 0x914FF51C,
    "bf16s": 0x086CA5E4, "mxfp8": 0x50E52C95, "mxfp6": 0xAC3FC9F3, "mxfp4": 0xDAC9186E,
    "mxmix": 0x814D2EB4,
}
LITERAL_SEED1234ABCD_ROUNDS5_PATTERN15 = {
    "f16": 0x0C45D149, "i8": 0x3D85514F, "fp8": 0xFB3FEE4F, "bf8": 0xD5463610,
    "bf16s": 0xC05DC16C, "mxfp8": 0xA0653B19, "mxfp6": 0x2E8E4650, "mxfp4": 0xA7AF8CA7,
    "mxmix": 0xA4A98714,
}


def _codes(kind, pattern, seed, rnd, which):
    """The generator's 3-bit codes and scale bits, from the seed alone."""
    m, k = FORMATS[kind][:2]
    e = k * m // 64
    s = _lane_seeds(seed, pattern, 3 + KINDS.index(kind))
    w = [_mix32(s + U(16 * rnd + 8 * which + i)) for i in range(5)]
    codes = np.array([[(int(w[j // 10][lane]) >> (3 * (j % 10))) & 7 for j in range(e)]
                      for lane in range(64)])
    return codes, np.array([int(x) & 1 for x in w[4]])


def _round_scale(kind, pattern, seed, rnd):
    base = _mix32(U(seed) + U(pattern) * U(0x9E3779B9))
    s64 = _mix32(base + U(64) * U(0x85EBCA6B) + U(3 + KINDS.index(kind)) * U(0xC2B2AE35))
    return int(_mix32(s64 + U(rnd))) % 81 - 40


def test_generator_guarantees():
    """Over all 16 patterns x 64 lanes x rounds {0, 1, 2, 255}: every decoded
    element is the table entry its 3-bit code names (so no NaN, no infinity),
    no scale byte is 0xFF, the filler bytes differ from the live one, every
    table entry occurs, both da / db values occur, S_r takes both signs."""
    seed = 0x5EED1234
    for kind in KINDS:
        m, k, (abits, aname), (bbits, bname), scaled = FORMATS[kind]
        e = k * m // 64
        factor = 2.0 if kind == "i8" else 1.0
        seen = set()
        bits_seen = {0: set(), 1: set()}
        signs = set()
        for pattern in range(16):
            for rnd in (0, 1, 2, 255):
                ra, rb, sa, sb = probes.mx_selftest_lane_regs(kind, pattern, seed, rnd)
                sr = _round_scale(kind, pattern, seed, rnd)
                signs.add(np.sign(sr))
                for which, regs, bits, name, words in ((0, ra, abits, aname, sa),
                                                       (1, rb, bbits, bname, sb)):
                    codes, lane_bits = _codes(kind, pattern, seed, rnd, which)
                    raw = np.array([_unpack(regs[lane], e, bits) for lane in range(64)])
                    vals = _decode(name, raw.reshape(-1)).reshape(64, e)
                    assert np.isfinite(vals).all()
                    want = np.array(TABLE)[codes] * factor
                    assert np.array_equal(vals, want), (kind, pattern, rnd, which)
                    seen.update(np.unique(vals / factor).tolist())
                    if not scaled:
                        continue
                    live_byte = 0 if which == 0 else 2
                    for lane in range(64):
                        by = [(words[lane] >> (8 * i)) & 0xFF for i in range(4)]
                        assert 0xFF not in by and len(set(by)) == 4
                        bit = int(lane_bits[lane])
                        if kind == "mxmix" and ((lane // m) & 1) != which:
                            bit = 0  # the k-block's other operand carries the bit
                        assert by[live_byte] - 127 == (sr if which == 0 else -sr) + bit
                        bits_seen[which].add(bit)
        assert seen == set(TABLE), kind
        if scaled:
            assert bits_seen == {0: {0, 1}, 1: {0, 1}}, kind
            assert signs >= {-1, 1}, kind


def test_product_scale_keeps_mxmix_within_the_bound():
    """mxmix has K = 128: its product scale must stay at 2^0..2^1."""
    for pattern in range(16):
        _, _, ea, eb = round_operands("mxmix", pattern, 7, 3)
        for kb in range(4):  # only the exponents of one k-block meet
            total = ea[:, kb][:, None] + eb[kb, :][None, :]
            assert total.min() >= 0 and total.max() <= 1


def test_rounds_bound_keeps_every_accumulator_exact():
    """Worst case per round in hash units (acc*4; i8: acc): K products of at
    most 6*6 (i8: 12*12), times the largest product scale, times 4."""
    assert probes.MX_MAX_ROUNDS == 256
    for kind in KINDS:
        m, k, _, _, scaled = FORMATS[kind]
        if kind == "i8":
            worst = k * 144
        else:
            worst = k * 36 * 4 * ((2 if kind == "mxmix" else 4) if scaled else 1)
        assert worst * probes.MX_MAX_ROUNDS < 2 ** 24, kind


def test_patterns_and_kinds_are_distinct():
    e = probes.mx_selftest_expected(3, 2)
    for kind in KINDS:
        assert len({rec[kind] for rec in e}) == 16
    assert len(set(e[0].values())) == len(KINDS)


def test_expected_is_deterministic_and_seeded():
    assert probes.mx_selftest_expected(9, 3) == probes.mx_selftest_expected(9, 3)
    assert probes.mx_selftest_expected(9, 3) != probes.mx_selftest_expected(10, 3)


@pytest.mark.parametrize(
    "kwargs, needle",
    [
        (dict(blocks=0), "blocks"),
        (dict(blocks=65537), "blocks"),
        (dict(rounds=0), "rounds"),
        (dict(rounds=257), "rounds"),
        (dict(_inject=("mxfp4", 5), blocks=5), "inject_block"),
    ],
)
def test_bad_arguments_fail_before_any_gpu_call(kwargs, needle):
    """Validation comes before the first HIP call: the same error code with
    or without a GPU, and nothing is launched."""
    with pytest.raises(probes.ProbeError, match=needle) as ei:
        probes.mx_selftest(0, **kwargs)
    assert "rc=-1" in str(ei.value)


def test_unknown_kind_and_pattern_are_rejected():
    with pytest.raises(probes.ProbeError, match="unknown kind"):
        probes.mx_selftest_tile(0, "fp64", 0, 0, 1)
    with pytest.raises(probes.ProbeError, match="pattern"):
        probes.mx_selftest_tile(0, "f16", 16, 0, 1)
    with pytest.raises(probes.ProbeError, match="rounds"):
        probes.mx_selftest_tile(0, "f16", 0, 0, 0)
    with pytest.raises(ValueError, match="unknown matrix kind"):
        probes.mx_selftest(0, _inject=("mfma", 0))
    for rounds in (0, 257):
        with pytest.raises(probes.ProbeError, match="rounds"):
            probes.mx_selftest_expected(0, rounds)


def test_null_outputs_are_rejected():
    lib = probes._lib()
    buf = (ctypes.c_int32 * 2048)()
    params = probes._MxParams(1, 1, 0, -1, -1)
    assert lib.egpu_mxtest_expected(0, 1, None) == -1
    assert b"null" in lib.egpu_last_error()
    assert lib.egpu_mxtest(0, ctypes.byref(params), None) == -1
    assert lib.egpu_mxtest(0, None, ctypes.byref(probes._MxReport())) == -1
    assert lib.egpu_mxtest_records(0, ctypes.byref(params), None, 4) == -1
    assert lib.egpu_mxtest_tile(0, 0, 0, 0, 1, buf, buf, buf, buf, None) == -1
    assert lib.egpu_mxtest_tile(0, 0, 0, 0, 1, None, buf, buf, buf, buf) == -1
