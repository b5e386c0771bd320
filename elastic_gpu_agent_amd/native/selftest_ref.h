// selftest_ref.h — host reference of the GPU self-test (egpu_selftest.hip).
//
// Host-only: plain C++17, no HIP call, no GPU type. It computes the 64
// expected (int_sig, fma_sig, mfma_sig) records by emulating the 64 lanes of
// a wave one after another, a plain integer 32x32x16 matmul, and the C/D lane
// map of the 32x32x16 MFMA. The per-lane step functions are the single
// definition of the input generators; egpu_selftest.hip re-defines
// EGPU_ST_FN so the kernel runs the same steps per lane (what the kernel adds
// is everything a GPU can get wrong: the cross-lane reduction, the MFMA and
// its lane maps, LDS and memory traffic). tests/test_selftest_ref.py holds an
// independent numpy oracle and literal values, so header and kernel cannot
// drift together unnoticed.
//
// Inputs are a pure function of (pattern, seed, rounds), pattern in [0, 64).
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#ifndef EGPU_ST_FN
#define EGPU_ST_FN inline
#endif

// |acc| <= rounds * 16 * 3 * 3 = 144 * rounds must stay below 2^24 for the
// f32 accumulator to be exact (that alone allows 116,508). The bound is far
// lower because the host reference costs 64 * rounds * 16,384 multiply-adds
// and a probe has to answer in seconds: 4096 * 144 = 589,824 < 2^24.
#define EGPU_SELFTEST_MAX_ROUNDS 4096
#define EGPU_SELFTEST_PATTERNS 64
#define EGPU_SELFTEST_MAX_LDS 163840

namespace egpu_st {

EGPU_ST_FN uint32_t mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

EGPU_ST_FN uint32_t rotl32(uint32_t x, int k) { return (x << k) | (x >> (32 - k)); }

// Portable popcount / high multiply: the kernel overrides neither, the
// compiler turns both into one instruction (v_bcnt_u32_b32, v_mul_hi_u32).
EGPU_ST_FN uint32_t popc32(uint32_t x) {
  x = x - ((x >> 1) & 0x55555555u);
  x = (x & 0x33333333u) + ((x >> 2) & 0x33333333u);
  x = (x + (x >> 4)) & 0x0f0f0f0fu;
  return (x * 0x01010101u) >> 24;
}

EGPU_ST_FN uint32_t mulhi32(uint32_t a, uint32_t b) {
  return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32);
}

// stream: 0 = integer chain, 1 = FMA chain, 2 = MFMA operands
EGPU_ST_FN uint32_t lane_seed(uint32_t seed, int pattern, int lane, int stream) {
  uint32_t s = mix32(seed + (uint32_t)pattern * 0x9e3779b9u);
  return mix32(s + (uint32_t)lane * 0x85ebca6bu + (uint32_t)stream * 0xc2b2ae35u);
}

// Weight of lane l in the cross-lane reduction sum(v_l * w_l) mod 2^32. The
// weights are odd and distinct, so two lanes swapping their values changes
// the sum (unless the values differ by a multiple of 2^31 / (la - lb)).
EGPU_ST_FN uint32_t lane_weight(int lane) { return (2u * (uint32_t)lane + 1u) * 0x01000193u; }

// ---- integer chain: LCG + xorshift, high multiply, rotate, popcount
EGPU_ST_FN uint32_t int_chain(uint32_t x, int rounds) {
  uint32_t h = 0;
  for (int r = 0; r < rounds; ++r) {
    x = x * 1664525u + 1013904223u;
    x ^= x << 13;
    x ^= x >> 17;
    x ^= x << 5;
    h = rotl32(h, 5) ^ mulhi32(x, 0x9e3779b9u);
    h += popc32(x);
  }
  return h ^ x;
}

// ---- FP32 FMA chain. x, a, b are all in [1,2): x*a+b is in [2,6), then the
// exponent is forced back to 0 by keeping the 23 mantissa bits. No denormal,
// infinity or NaN can occur, so the one correctly rounded fmaf() per step is
// the whole specification (fmaf is called by name: nothing depends on the
// compiler contracting a multiply and an add).
EGPU_ST_FN float bits_to_unit(uint32_t bits) {
  uint32_t u = (bits & 0x007fffffu) | 0x3f800000u;
  float f;
  memcpy(&f, &u, 4);
  return f;
}

EGPU_ST_FN uint32_t fma_chain(uint32_t s, int rounds) {
  float x = bits_to_unit(s);
  const float a = bits_to_unit(mix32(s + 1u));
  const float b = bits_to_unit(mix32(s + 2u));
  uint32_t h = 0;
  for (int r = 0; r < rounds; ++r) {
    x = fmaf(x, a, b);
    uint32_t u;
    memcpy(&u, &x, 4);
    x = bits_to_unit(u);
    h = rotl32(h, 7) + (u & 0x007fffffu);
  }
  return h;
}

// ---- MFMA operands: element j (0..7) of a lane's A (which = 0) or B
// (which = 1) fragment in round r, a whole number in [-3, 3].
EGPU_ST_FN uint32_t mfma_word(uint32_t s, int round, int which) {
  return mix32(s + 2u * (uint32_t)round + (uint32_t)which);
}

EGPU_ST_FN int mfma_elem(uint32_t word, int j) { return (int)((word >> (3 * j)) & 7u) % 7 - 3; }

// hash of a lane's 16 accumulators, taken as integers, in register order
EGPU_ST_FN uint32_t acc_hash_step(uint32_t h, int v) { return h * 0x01000193u + (uint32_t)v; }

// ---- memory-path pattern: word k (0..3) of 16-byte element i
EGPU_ST_FN uint32_t hbm_word(uint64_t i, int k, uint32_t seed) {
  uint32_t base = mix32(seed + (uint32_t)(i >> 30));
  return mix32((uint32_t)(i * 4u + (uint64_t)k) + base);
}

// ---- LDS march pattern of word index `word`
EGPU_ST_FN uint32_t lds_word(uint32_t word, uint32_t seed) {
  return mix32(word * 0x9e3779b9u + seed);
}

// Fills A (32x16) and B (16x32), row-major, of one round from the lane maps
// A[l&31][8*(l>>5)+j] and B[8*(l>>5)+j][l&31].
inline void mfma_operands(uint32_t seed, int pattern, int round, int8_t a[512], int8_t b[512]) {
  for (int l = 0; l < 64; ++l) {
    const uint32_t s = lane_seed(seed, pattern, l, 2);
    const uint32_t wa = mfma_word(s, round, 0), wb = mfma_word(s, round, 1);
    for (int j = 0; j < 8; ++j) {
      const int k = 8 * (l >> 5) + j;
      a[(l & 31) * 16 + k] = (int8_t)mfma_elem(wa, j);
      b[k * 32 + (l & 31)] = (int8_t)mfma_elem(wb, j);
    }
  }
}

// D (32x32 row-major) += sum over rounds of A_r * B_r
inline void mfma_tile(uint32_t seed, int pattern, int rounds, int32_t d[1024]) {
  int8_t a[512], b[512];
  for (int i = 0; i < 1024; ++i) d[i] = 0;
  for (int r = 0; r < rounds; ++r) {
    mfma_operands(seed, pattern, r, a, b);
    for (int i = 0; i < 32; ++i)
      for (int k = 0; k < 16; ++k) {
        const int av = a[i * 16 + k];
        for (int j = 0; j < 32; ++j) d[i * 32 + j] += av * b[k * 32 + j];
      }
  }
}

// signature of a D tile: every lane hashes its 16 accumulators (C/D lane map
// col = l&31, row = (reg&3) + 8*(reg>>2) + 4*(l>>5)), then the lane reduction
inline uint32_t mfma_sig_of_tile(const int32_t d[1024]) {
  uint32_t sig = 0;
  for (int l = 0; l < 64; ++l) {
    uint32_t h = 0;
    for (int reg = 0; reg < 16; ++reg) {
      const int row = (reg & 3) + 8 * (reg >> 2) + 4 * (l >> 5);
      h = acc_hash_step(h, d[row * 32 + (l & 31)]);
    }
    sig += h * lane_weight(l);
  }
  return sig;
}

struct expected_record {
  uint32_t int_sig, fma_sig, mfma_sig;
};

inline bool rounds_ok(int rounds) { return rounds >= 1 && rounds <= EGPU_SELFTEST_MAX_ROUNDS; }

inline expected_record expected_for(uint32_t seed, int pattern, int rounds) {
  expected_record e{0, 0, 0};
  for (int l = 0; l < 64; ++l) {
    e.int_sig += int_chain(lane_seed(seed, pattern, l, 0), rounds) * lane_weight(l);
    e.fma_sig += fma_chain(lane_seed(seed, pattern, l, 1), rounds) * lane_weight(l);
  }
  int32_t d[1024];
  mfma_tile(seed, pattern, rounds, d);
  e.mfma_sig = mfma_sig_of_tile(d);
  return e;
}

// out[3*p .. 3*p+2] = (int_sig, fma_sig, mfma_sig) of pattern p.
// Returns 0, or -1 when rounds is outside [1, EGPU_SELFTEST_MAX_ROUNDS].
inline int expected_all(uint32_t seed, int rounds, uint32_t out[EGPU_SELFTEST_PATTERNS * 3]) {
  if (!rounds_ok(rounds)) return -1;
  for (int p = 0; p < EGPU_SELFTEST_PATTERNS; ++p) {
    const expected_record e = expected_for(seed, p, rounds);
    out[3 * p] = e.int_sig;
    out[3 * p + 1] = e.fma_sig;
    out[3 * p + 2] = e.mfma_sig;
  }
  return 0;
}

}  // namespace egpu_st
