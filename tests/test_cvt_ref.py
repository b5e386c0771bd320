"""Host side of the conversion sweep (native/selftest_cvt_ref.h through
libegpu_kernels.so): generator, generic encoder, expected signatures and
argument checks. None of it uses a GPU.

`reference` below is the numpy float64 oracle (OCP grids from (exponent bits,
mantissa bits, bias), nearest grid point with ties to the even code, packing
with np.packbits); it shares nothing with the header. The GPU test compares the
instructions with it, this file compares the header's encoder with it and with
the generator's closed form.
"""
import numpy as np
import pytest

from elastic_gpu_agent_amd.isolation import probes
from elastic_gpu_agent_amd.isolation.probes import ProbeError

KINDS = list(probes.CVT_KINDS)
SEED = 0x5EED1234
# (exponent bits, mantissa bits, bias, largest finite magnitude code)
NARROW = {"e4m3": (4, 3, 7, 0x7E), "e5m2": (5, 2, 15, 0x7B), "e2m3": (2, 3, 1, 0x1F),
          "e3m2": (3, 2, 3, 0x1F), "e2m1": (2, 1, 1, 0x07)}
WIDE_BITS = {"f32": 32, "f16": 16, "bf16": 16}
# bits one code occupies: "word" two bytes in a 16-bit half, "nib" two nibbles in
# a byte, "pk6" 32 codes in 24 bytes, "byte" one byte
CODE_BITS = {"word": 8, "byte": 8, "nib": 4, "pk6": 6}
# kind -> groups of (direction, narrow, wide, packing, elements per lane), in the
# order their registers follow each other
GROUPS = {
    "enc_fp8": [("enc", "e4m3", "f32", "word", 32)], "enc_bf8": [("enc", "e5m2", "f32", "word", 32)],
    "enc_fp6": [("enc", "e2m3", "f32", "pk6", 32)], "enc_bf6": [("enc", "e3m2", "f32", "pk6", 32)],
    "enc_fp4": [("enc", "e2m1", "f32", "nib", 32)],
    "dec_fp8": [("dec", "e4m3", "f32", "word", 32)], "dec_bf8": [("dec", "e5m2", "f32", "word", 32)],
    "dec_fp6": [("dec", "e2m3", "f32", "pk6", 32)], "dec_bf6": [("dec", "e3m2", "f32", "pk6", 32)],
    "dec_fp4": [("dec", "e2m1", "f32", "nib", 32)],
    "x16": [("enc", "e4m3", "f16", "word", 16), ("enc", "e2m1", "bf16", "nib", 16),
            ("dec", "e4m3", "f16", "word", 16), ("dec", "e2m1", "bf16", "nib", 16)],
    "plain": [("enc", "e4m3", "f32", "word", 8), ("enc", "e5m2", "f32", "word", 8),
              ("dec", "e4m3", "f32", "word", 8), ("dec", "e4m3", "f32", "byte", 8),
              ("dec", "e5m2", "f32", "byte", 8)],
}
# v_cvt_scalef32_2xpk16_*: the source element found at each packed position
PK6_SOURCE = [j // 2 + 16 * (j % 2) for j in range(32)]


def grid(fmt):
    """Magnitude of every finite code, in code order."""
    e, m, bias, top = NARROW[fmt]
    c = np.arange(top + 1)
    ex, fr = c >> m, c & ((1 << m) - 1)
    return np.where(ex == 0, fr, (1 << m) + fr) * 2.0 ** (np.maximum(ex, 1) - bias - m)


def unpack(regs, bits, n):
    """The first n little-endian `bits`-wide fields of each lane's registers."""
    b = np.unpackbits(np.ascontiguousarray(regs, np.uint32).view(np.uint8), axis=1, bitorder="little")
    return b[:, :n * bits].reshape(len(regs), n, bits).astype(np.int64) @ (1 << np.arange(bits))


def pack(values, bits):
    b = ((values[:, :, None] >> np.arange(bits)) & 1).astype(np.uint8).reshape(len(values), -1)
    return np.packbits(b, axis=1, bitorder="little").view(np.uint32).astype(np.int64)


def wide_value(bits, wide):
    if wide == "f16":
        return bits.astype(np.uint16).view(np.float16).astype(np.float64)
    return (bits << (16 if wide == "bf16" else 0)).astype(np.uint32).view(np.float32).astype(np.float64)


def wide_code(value, wide):  # every value the sweep decodes to is exact in its format
    if wide == "f16":
        return value.astype(np.float16).view(np.uint16).astype(np.int64)
    return value.astype(np.float32).view(np.uint32).astype(np.int64) >> (16 if wide == "bf16" else 0)


def nearest_code(x, fmt):
    """Nearest grid point, ties to the even code, sign kept (also of zero)."""
    e, m, _, _ = NARROW[fmt]
    g, a = grid(fmt), np.abs(x)
    hi = np.minimum(np.searchsorted(g, a), len(g) - 1)
    lo = np.maximum(hi - 1, 0)
    up = (g[hi] - a < a - g[lo]) | ((g[hi] - a == a - g[lo]) & (hi % 2 == 0))
    return np.where(up, hi, lo) | (np.signbit(x).astype(np.int64) << (e + m))


def groups_of(kind, src, old):
    """(group, its source registers, its old words) in register order."""
    s0 = o0 = 0
    for grp in GROUPS[kind]:
        direction, _, wide, packing, n = grp
        ns = n * (WIDE_BITS[wide] if direction == "enc" else CODE_BITS[packing]) // 32
        no = n // 2 if direction == "enc" and packing != "pk6" else 0
        yield grp, src[:, s0:s0 + ns], old[:, o0:o0 + no]
        s0, o0 = s0 + ns, o0 + no


def reference(kind, src, old, scale):
    """The 64 x 32 result registers: encode divides by 2^S, decode multiplies."""
    src, old = np.array(src, np.int64), np.array(old, np.int64)
    S = (((np.array(scale, np.int64) >> 23) & 0xFF) - 127 if kind != "plain" else np.zeros(64))[:, None]
    out = []
    for (direction, fmt, wide, packing, n), s, o in groups_of(kind, src, old):
        e, m, _, _ = NARROW[fmt]
        cb = CODE_BITS[packing]
        if direction == "enc":
            code = nearest_code(wide_value(unpack(s, WIDE_BITS[wide], n), wide) / 2.0 ** S, fmt)
            if packing == "pk6":  # the two 16-element source vectors come out interleaved
                out.append(pack(code[:, PK6_SOURCE], 6))
                continue
            shift = 2 * cb * (np.arange(n // 2) % (16 // cb))  # half i & 1, or byte i & 3
            pair = code[:, 0::2] | (code[:, 1::2] << cb)
            out.append((o & ~(((1 << 2 * cb) - 1) << shift) | (pair << shift)) & 0xFFFFFFFF)
        else:
            code = unpack(s, cb, n)
            value = np.where(code >> (e + m) & 1, -1.0, 1.0) * grid(fmt)[code & ((1 << (e + m)) - 1)]
            out.append(pack(wide_code(value * 2.0 ** S, wide), WIDE_BITS[wide]))
    out = np.concatenate(out, axis=1)
    return np.pad(out, ((0, 0), (0, 32 - out.shape[1]))).astype(np.uint32)


def encode_elements(kind, src, old, scale, res):
    """For a single-group encode kind: per element the magnitude code c, the
    quarter q, the sign, and the code found in `res`."""
    ((_, fmt, wide, packing, n), s, _), = groups_of(kind, np.array(src, np.int64), np.array(old, np.int64))
    e, m, _, _ = NARROW[fmt]
    S = (((np.array(scale, np.int64) >> 23) & 0xFF) - 127)[:, None]
    x = wide_value(unpack(s, WIDE_BITS[wide], n), wide) / 2.0 ** S
    g = np.append(grid(fmt), 2 * grid(fmt)[-1] - grid(fmt)[-2])
    c = np.searchsorted(g, np.abs(x), side="right") - 1
    q = (np.abs(x) - g[c]) * 4 / (g[c + 1] - g[c])
    res = np.array(res, np.uint32)
    if packing == "pk6":
        got = unpack(res[:, :6], 6, n)[:, np.argsort(PK6_SOURCE)]
    else:  # the written half or byte of register i holds elements 2i, 2i+1
        cb = CODE_BITS[packing]
        field = res[:, :n // 2].astype(np.int64) >> (2 * cb * (np.arange(n // 2) % (16 // cb)))
        got = np.stack([field & ((1 << cb) - 1), field >> cb & ((1 << cb) - 1)], axis=2).reshape(64, n)
    return c, q, np.signbit(x), got, (e + m)


def test_kind_names_and_bits():
    assert KINDS == ["enc_fp8", "enc_bf8", "enc_fp6", "enc_bf6", "enc_fp4", "dec_fp8", "dec_bf8",
                     "dec_fp6", "dec_bf6", "dec_fp4", "x16", "plain"] == list(GROUPS)
    assert [probes.CVT_KINDS[k] for k in KINDS] == [1 << i for i in range(len(KINDS))]
    assert not set(KINDS) & (set(probes.MX_KINDS) | set(probes.MOVE_KINDS) | set(probes._INJECT_KINDS))


@pytest.mark.parametrize("round", [0, 1])
@pytest.mark.parametrize("pattern", [0, 15])
@pytest.mark.parametrize("kind", KINDS[:5])
def test_generic_encoder_equals_closed_form_and_wave_covers_every_pair(kind, pattern, round):
    src, old, scale, res = probes.cvt_selftest_lane_regs(kind, pattern, SEED, round)
    c, q, neg, got, sign_bit = encode_elements(kind, src, old, scale, res)
    top = NARROW[GROUPS[kind][0][1]][3]
    assert np.isin(q, [0, 1, 2, 3]).all() and (c <= top).all()
    assert not ((c == top) & (q >= 2)).any()  # nothing rounds above the largest finite code
    closed = c + ((q > 2) | ((q == 2) & (c % 2 == 1))) | (neg.astype(np.int64) << sign_bit)
    bad = np.argwhere(got != closed)
    assert bad.size == 0, f"first wrong (lane, element): {bad[:8].tolist()}"
    pairs = {(int(a), int(b), bool(s)) for a, b, s in zip(c.ravel(), q.ravel(), neg.ravel())}
    assert len(pairs) == 2 * (4 * (top + 1) - 2)  # every (c, q, sign) but the two over the top


@pytest.mark.parametrize("round", [0, 1])
@pytest.mark.parametrize("pattern", [0, 15])
@pytest.mark.parametrize("kind", KINDS)
def test_host_reference_equals_numpy_and_sources_are_finite_normals(kind, pattern, round):
    src, old, scale, res = probes.cvt_selftest_lane_regs(kind, pattern, SEED, round)
    bad = np.argwhere(np.array(res, np.uint32) != reference(kind, src, old, scale))
    assert bad.size == 0, f"first wrong (lane, register): {bad[:8].tolist()}"
    assert all(s & 0x807FFFFF == 0 and 0 < s >> 23 < 255 for s in scale)  # 2^S, not NaN
    for (direction, fmt, wide, packing, n), s, _ in groups_of(kind, np.array(src, np.int64),
                                                              np.array(old, np.int64)):
        if direction == "enc":  # zero, or a normal number: biased exponent neither 0 nor all ones
            bits = unpack(s, WIDE_BITS[wide], n)
            mant = {"f32": 23, "f16": 10, "bf16": 7}[wide]
            all_ones = (1 << (WIDE_BITS[wide] - 1 - mant)) - 1
            ex = bits >> mant & all_ones
            assert ((ex != 0) | (bits & ((1 << mant) - 1) == 0)).all() and (ex != all_ones).all()
        else:
            e, m, _, top = NARROW[fmt]
            mags = unpack(s, CODE_BITS[packing], n) & ((1 << (e + m)) - 1)
            assert (mags <= top).all()
            if n >= 16:  # one wave, one round: every finite code, both signs
                assert len(np.unique(unpack(s, CODE_BITS[packing], n))) == 2 * (top + 1)


def test_expected_is_stable_and_depends_on_pattern_seed_and_rounds():
    a, again = probes.cvt_selftest_expected(7, 2), probes.cvt_selftest_expected(7, 2)
    other_seed, three = probes.cvt_selftest_expected(8, 2), probes.cvt_selftest_expected(7, 3)
    assert a == again and len(a) == probes.CVT_PATTERNS
    for kind in KINDS:
        assert len({a[p][kind] for p in range(probes.CVT_PATTERNS)}) == probes.CVT_PATTERNS
        assert all(a[p][kind] not in (other_seed[p][kind], three[p][kind]) for p in range(16))


@pytest.mark.parametrize("call", [
    lambda: probes.cvt_selftest(0, blocks=0),
    lambda: probes.cvt_selftest(0, blocks=65537),
    lambda: probes.cvt_selftest(0, rounds=0),
    lambda: probes.cvt_selftest(0, rounds=probes.CVT_MAX_ROUNDS + 1),
    lambda: probes.cvt_selftest(0, blocks=2, _inject=("enc_fp4", 2)),
    lambda: probes.cvt_selftest_records(0, blocks=0),
    lambda: probes.cvt_selftest_expected(0, 0),
    lambda: probes.cvt_selftest_expected(0, probes.CVT_MAX_ROUNDS + 1),
    lambda: probes.cvt_selftest_tile(0, "nope"),
    lambda: probes.cvt_selftest_tile(0, "x16", pattern=16),
    lambda: probes.cvt_selftest_tile(0, "x16", round=probes.CVT_MAX_ROUNDS),
    lambda: probes.cvt_selftest_lane_regs("nope"),
    lambda: probes.cvt_selftest_lane_regs("plain", pattern=-1),
])
def test_bad_arguments_raise_before_any_hip_call(call):
    with pytest.raises(ProbeError, match="rc=-1"):
        call()
