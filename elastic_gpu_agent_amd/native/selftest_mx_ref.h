// selftest_mx_ref.h — host reference of the matrix sweep (egpu_selftest_mx.hip).
//
// Host-only: plain C++17, no HIP call, no GPU type. The sweep runs nine MFMA
// kinds (f16, i8, OCP fp8/bf8, the 16x16 bf16 shape, and the block-scaled
// f8f6f4 instructions with fp8, fp6, fp4 and mixed operands) on every wave and
// hashes each accumulator tile into one signature per kind. This header
// computes the 16 x 9 expected signatures.
//
// As in selftest_ref.h the per-lane step functions (EGPU_ST_FN) are the single
// definition of the operand generators: lane_operands<KIND>() returns the
// ENCODED A and B fragments and scale words of one lane, and the kernel feeds
// exactly those registers to the instruction. What the reference adds is its
// own side of the contract: it unpacks the fragments again, DECODES every
// element and scale with decoders written from the OCP definitions (all codes,
// not just the eight the generator uses), places them through the A/B lane
// maps, multiplies in double, and reads the result back through the C/D map.
// tests/test_mx_ref.py holds an independent numpy oracle and literal values.
//
// Inputs are a pure function of (kind, pattern, seed, rounds), pattern in
// [0, 16).
#pragma once

#include <cmath>
#include <cstdint>
#include <limits>

#include "selftest_ref.h"

// Every operand element is one of {0, 0.5, -1, 1.5, 2, -3, 4, -6} (i8: twice
// that), so a product is a multiple of 0.25 of magnitude at most 36 (i8: a
// whole number, at most 144), and the signature hashes (int)(acc * 4) (i8:
// acc). Worst case per round, in hash units:
//   f16, fp8, bf8   K = 16:  16 * 36 * 4      =  2,304
//   bf16s           K = 32:  32 * 36 * 4      =  4,608
//   i8              K = 32:  32 * 144         =  4,608  (i32 accumulator)
//   mxfp8/6/4       K = 64:  64 * 36 * 4 * 4  = 36,864  (product scale <= 2^2)
//   mxmix           K = 128: 128 * 36 * 4 * 4 = 73,728
// The f32 accumulator is exact while |acc * 4| < 2^24 (every partial sum is a
// multiple of 0.25). 36,864 * 256 = 9,437,184 < 2^24, but 73,728 * 256 is not,
// so mxmix keeps its product scale at 2^0..2^1: a lane of an even k-block may
// set da and never db, a lane of an odd k-block db and never da (scale_bit).
// Both bits still take both values in every tile, and the kind's worst case
// becomes 128 * 36 * 2 * 4 = 36,864 like the others.
#define EGPU_MX_MAX_ROUNDS 256
#define EGPU_MX_PATTERNS 16
#define EGPU_MX_NKINDS 9

namespace egpu_mx {

using egpu_st::acc_hash_step;
using egpu_st::lane_seed;
using egpu_st::lane_weight;
using egpu_st::mix32;

enum { K_F16 = 0, K_I8, K_FP8, K_BF8, K_BF16S, K_MXFP8, K_MXFP6, K_MXFP4, K_MXMIX };
enum { F_F16 = 0, F_BF16, F_I8, F_E4M3, F_E5M2, F_E2M3, F_E2M1 };

// Tile M = N, depth K, element formats of A and B, and whether the instruction
// takes E8M0 block scales. A lane supplies E = K * M / 64 elements of each
// operand and holds NREG = M * M / 64 accumulators.
template <int KIND> struct traits;
#define EGPU_MX_TRAITS(kind, m, k, fa, fb, scaled)               \
  template <> struct traits<kind> {                              \
    static constexpr int M = m, K = k, FA = fa, FB = fb;         \
    static constexpr int E = k * m / 64, NREG = m * m / 64;      \
    static constexpr bool SCALED = scaled;                       \
  }
EGPU_MX_TRAITS(K_F16, 32, 16, F_F16, F_F16, false);
EGPU_MX_TRAITS(K_I8, 32, 32, F_I8, F_I8, false);
EGPU_MX_TRAITS(K_FP8, 32, 16, F_E4M3, F_E4M3, false);
EGPU_MX_TRAITS(K_BF8, 32, 16, F_E5M2, F_E5M2, false);
EGPU_MX_TRAITS(K_BF16S, 16, 32, F_BF16, F_BF16, false);
EGPU_MX_TRAITS(K_MXFP8, 32, 64, F_E4M3, F_E4M3, true);
EGPU_MX_TRAITS(K_MXFP6, 32, 64, F_E2M3, F_E2M3, true);
EGPU_MX_TRAITS(K_MXFP4, 32, 64, F_E2M1, F_E2M1, true);
EGPU_MX_TRAITS(K_MXMIX, 16, 128, F_E4M3, F_E2M1, true);
#undef EGPU_MX_TRAITS

EGPU_ST_FN constexpr int fmt_bits(int fmt) {
  return fmt == F_F16 || fmt == F_BF16 ? 16 : fmt == F_E2M3 ? 6 : fmt == F_E2M1 ? 4 : 8;
}

// ---- lane maps (the one place they are written down)
// A: lane l supplies row l % M and E elements j = 0..E-1; B mirrors it (column
// l % M, the same k). For every unscaled kind, and for FP6 and FP4 operands of
// the scaled instructions, the elements are contiguous: k = E * (l / M) + j.
// An 8-bit operand of a scaled instruction (E = 32, eight registers) is two
// runs of 16: registers 0-3 hold k = 16 * (l / M) + j, registers 4-7 hold
// K / 2 + 16 * (l / M) + (j - 16).
// Scales: the scale register of lane l applies to row (column) l % M and the
// 32-element k-block l / M, whatever the element format. For FP6 and FP4 that
// block is the lane's own data; for an 8-bit operand it is not.
EGPU_ST_FN constexpr int ab_index(int m, int lane) { return lane % m; }
EGPU_ST_FN constexpr int ab_k(int m, int e, int bits, int lane, int j) {
  return e == 32 && bits == 8 ? 16 * (lane / m) + (j & 15) + (16 * 64 / m) * (j >> 4)
                              : e * (lane / m) + j;
}
// C/D: column l % M; 32x32: row = (reg&3) + 8*(reg>>2) + 4*(l>>5), 16
// registers; 16x16: row = 4*(l>>4) + reg, 4 registers.
EGPU_ST_FN constexpr int cd_row(int m, int lane, int reg) {
  return m == 32 ? (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5) : 4 * (lane >> 4) + reg;
}

// ---- generator: 3 bits choose an element of {0, 0.5, -1, 1.5, 2, -3, 4, -6}
// Word i (0..3) of a lane's operand carries ten 3-bit codes; word 4 carries the
// lane's scale bit.
EGPU_ST_FN uint32_t gen_word(uint32_t s, int round, int which, int i) {
  return mix32(s + (uint32_t)(16 * round + 8 * which + i));
}

EGPU_ST_FN uint32_t elem_code(const uint32_t w[5], int j) {
  return (w[j / 10] >> (3 * (j % 10))) & 7u;
}

// The encoding of table entry c in each format, eight entries packed into
// constants so the lookup is a shift on the host and on the GPU alike.
//   f16   0000 3800 BC00 3E00 4000 C200 4400 C600
//   bf16  0000 3F00 BF80 3FC0 4000 C040 4080 C0C0
//   i8    twice the table: 0 1 -2 3 4 -6 8 -12
//   e4m3  00 30 B8 3C 40 C4 48 CC      e5m2  00 38 BC 3E 40 C2 44 C6
//   e2m3  00 04 28 0C 10 34 18 3C      e2m1  0 1 A 3 4 D 6 F
EGPU_ST_FN uint32_t encode(int fmt, uint32_t c) {
  switch (fmt) {
    case F_F16:
      return (uint32_t)((c < 4 ? 0x3E00BC0038000000ull >> (16 * c)
                               : 0xC6004400C2004000ull >> (16 * (c - 4))) & 0xffffu);
    case F_BF16:
      return (uint32_t)((c < 4 ? 0x3FC0BF803F000000ull >> (16 * c)
                               : 0xC0C04080C0404000ull >> (16 * (c - 4))) & 0xffffu);
    case F_I8:
      return (uint32_t)((0xF408FA0403FE0100ull >> (8 * c)) & 0xffu);
    case F_E4M3:
      return (uint32_t)((0xCC48C4403CB83000ull >> (8 * c)) & 0xffu);
    case F_E5M2:
      return (uint32_t)((0xC644C2403EBC3800ull >> (8 * c)) & 0xffu);
    case F_E2M3:
      return (uint32_t)((0x3C1834100C280400ull >> (8 * c)) & 0x3fu);
    default:  // F_E2M1
      return (0xF6D43A10u >> (4 * c)) & 0xfu;
  }
}

// Four times the value of table entry c (i8: of twice the entry): what the
// tile entry point reports as the operand a lane meant to supply.
EGPU_ST_FN int elem_x4(int fmt, uint32_t c) {
  const int v = (int)(int8_t)((0xE810F40806FC0200ull >> (8 * c)) & 0xffu);
  return fmt == F_I8 ? 2 * v : v;
}

// Packs E elements of FMT contiguously, little-endian, element 0 in the low
// bits of out[0]: 16- and 8-bit elements fall on their natural boundaries, FP4
// is two per byte with the low nibble first, FP6 is 32 elements in 24 bytes.
template <int FMT, int E>
EGPU_ST_FN void build_frag(const uint32_t w[5], uint32_t out[8]) {
  constexpr int B = fmt_bits(FMT);
  static_assert(E * B <= 256, "an operand is at most 8 registers");
#pragma unroll
  for (int i = 0; i < 8; ++i) out[i] = 0;
#pragma unroll
  for (int j = 0; j < E; ++j) {
    const uint32_t bits = encode(FMT, elem_code(w, j));
    const int off = j * B;
    out[off >> 5] |= bits << (off & 31);
    if ((off & 31) + B > 32) out[(off >> 5) + 1] |= bits >> (32 - (off & 31));
  }
}

// ---- scales. S_r is the same for every lane of a round; the lane adds one
// bit. A's exponent is S_r + da, B's is -S_r + db, so the scale of a product is
// 2^0..2^2 while each operand's exponent byte moves through [87, 168].
EGPU_ST_FN int round_scale(uint32_t seed, int pattern, int kind, int round) {
  return (int)(mix32(lane_seed(seed, pattern, 64, 3 + kind) + (uint32_t)round) % 81u) - 40;
}

// The lane's bit: da (which = 0) or db (which = 1). For mxmix only one of the
// two may be set in a k-block (see EGPU_MX_MAX_ROUNDS).
EGPU_ST_FN int scale_bit(int kind, int m, int lane, int which, const uint32_t w[5]) {
  if (kind == K_MXMIX && ((lane / m) & 1) != which) return 0;
  return (int)(w[4] & 1u);
}

// The scale register of a lane: the live E8M0 byte at `live_byte`, and three
// different valid exponents in the other bytes, so that an instruction that
// selects the wrong byte is off by 2^3, 2^5, 2^7 or 2^9.
EGPU_ST_FN uint32_t scale_word(int exponent, int live_byte) {
  const uint32_t live = (uint32_t)(127 + exponent);
  uint32_t word = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    word |= (i == live_byte ? live : live + 3u + 2u * (uint32_t)i) << (8 * i);
  return word;
}

enum { SCALE_BYTE_A = 0, SCALE_BYTE_B = 2 };  // = the opsel the kernel passes

// Everything one lane hands to the instruction in one round.
struct lane_regs {
  uint32_t a[8], b[8];    // encoded fragments
  uint32_t sa, sb;        // scale registers (0 for unscaled kinds)
  uint32_t wa[5], wb[5];  // the generator words behind them
};

template <int KIND>
EGPU_ST_FN void lane_operands(uint32_t seed, int pattern, int lane, int round, lane_regs* r) {
  using T = traits<KIND>;
  const uint32_t s = lane_seed(seed, pattern, lane, 3 + KIND);
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    r->wa[i] = gen_word(s, round, 0, i);
    r->wb[i] = gen_word(s, round, 1, i);
  }
  build_frag<T::FA, T::E>(r->wa, r->a);
  build_frag<T::FB, T::E>(r->wb, r->b);
  r->sa = r->sb = 0;
  if (T::SCALED) {
    const int sr = round_scale(seed, pattern, KIND, round);
    r->sa = scale_word(sr + scale_bit(KIND, T::M, lane, 0, r->wa), SCALE_BYTE_A);
    r->sb = scale_word(-sr + scale_bit(KIND, T::M, lane, 1, r->wb), SCALE_BYTE_B);
  }
}

// ---------------------------------------------------------------- host only
// Decoders, from the OCP 8-bit floating point and microscaling definitions and
// IEEE 754. They cover every code of every format; the generator's eight
// entries are a small subset.

inline double decode_ieee(uint32_t bits, int ebits, int mbits, bool ieee_specials) {
  const int bias = (1 << (ebits - 1)) - 1;
  const uint32_t sign = (bits >> (ebits + mbits)) & 1u;
  const int e = (int)((bits >> mbits) & ((1u << ebits) - 1u));
  const uint32_t m = bits & ((1u << mbits) - 1u);
  double v;
  if (ieee_specials && e == (1 << ebits) - 1)
    v = m ? std::numeric_limits<double>::quiet_NaN() : std::numeric_limits<double>::infinity();
  else if (e == 0)
    v = std::ldexp((double)m, 1 - bias - mbits);
  else
    v = std::ldexp((double)((1u << mbits) | m), e - bias - mbits);
  return sign ? -v : v;
}

inline double decode_f16(uint32_t b) { return decode_ieee(b & 0xffffu, 5, 10, true); }
inline double decode_bf16(uint32_t b) { return decode_ieee(b & 0xffffu, 8, 7, true); }
inline double decode_e5m2(uint32_t b) { return decode_ieee(b & 0xffu, 5, 2, true); }
// e4m3fn: no infinity; S.1111.111 is NaN and the other 1111 codes are numbers
inline double decode_e4m3fn(uint32_t b) {
  if ((b & 0x7fu) == 0x7fu) return std::numeric_limits<double>::quiet_NaN();
  return decode_ieee(b & 0xffu, 4, 3, false);
}
// the MX element formats have neither infinity nor NaN
inline double decode_e2m3(uint32_t b) { return decode_ieee(b & 0x3fu, 2, 3, false); }
inline double decode_e2m1(uint32_t b) { return decode_ieee(b & 0xfu, 2, 1, false); }
// E8M0: 2^(e - 127); 0xFF is NaN
inline double decode_e8m0(uint32_t b) {
  b &= 0xffu;
  return b == 0xffu ? std::numeric_limits<double>::quiet_NaN() : std::ldexp(1.0, (int)b - 127);
}

inline double decode(int fmt, uint32_t bits) {
  switch (fmt) {
    case F_F16: return decode_f16(bits);
    case F_BF16: return decode_bf16(bits);
    case F_I8: return (double)(int8_t)(bits & 0xffu);
    case F_E4M3: return decode_e4m3fn(bits);
    case F_E5M2: return decode_e5m2(bits);
    case F_E2M3: return decode_e2m3(bits);
    default: return decode_e2m1(bits);
  }
}

// element j of a packed fragment (the inverse of build_frag's packing)
inline uint32_t extract(const uint32_t frag[8], int j, int bits) {
  const int off = j * bits;
  uint64_t v = frag[off >> 5];
  if ((off >> 5) + 1 < 8) v |= (uint64_t)frag[(off >> 5) + 1] << 32;
  return (uint32_t)(v >> (off & 31)) & ((1u << bits) - 1u);
}

// Decoded operands of one round: A (M x K) and B (K x M) row-major, and the
// scale exponents (e - 127) per (row, k-block) and (k-block, column); the
// scale arrays are zero for unscaled kinds.
struct round_operands {
  double a[2048], b[2048];
  int sa[64], sb[64];
};

template <int KIND>
inline void decode_round(uint32_t seed, int pattern, int round, round_operands* o) {
  using T = traits<KIND>;
  for (int i = 0; i < 64; ++i) o->sa[i] = o->sb[i] = 0;
  for (int l = 0; l < 64; ++l) {
    lane_regs r;
    lane_operands<KIND>(seed, pattern, l, round, &r);
    const int idx = ab_index(T::M, l);
    for (int j = 0; j < T::E; ++j) {
      const int ka = ab_k(T::M, T::E, fmt_bits(T::FA), l, j);
      const int kb = ab_k(T::M, T::E, fmt_bits(T::FB), l, j);
      o->a[idx * T::K + ka] = decode(T::FA, extract(r.a, j, fmt_bits(T::FA)));
      o->b[kb * T::M + idx] = decode(T::FB, extract(r.b, j, fmt_bits(T::FB)));
    }
    if (T::SCALED) {
      const int kb = l / T::M, nkb = T::K / 32;
      o->sa[idx * nkb + kb] = (int)std::ilogb(decode_e8m0(r.sa >> (8 * SCALE_BYTE_A)));
      o->sb[kb * T::M + idx] = (int)std::ilogb(decode_e8m0(r.sb >> (8 * SCALE_BYTE_B)));
    }
  }
}

// D (M x M row-major) = sum over rounds of A_r * B_r, every 32-element k-block
// scaled by 2^(sa + sb). `last`, when given, receives the last round's operands.
template <int KIND>
inline void tile(uint32_t seed, int pattern, int rounds, double d[1024], round_operands* last) {
  using T = traits<KIND>;
  constexpr int KB = T::SCALED ? 32 : T::K;  // one block = the whole K when unscaled
  round_operands local;
  round_operands* o = last ? last : &local;
  for (int i = 0; i < T::M * T::M; ++i) d[i] = 0.0;
  for (int r = 0; r < rounds; ++r) {
    decode_round<KIND>(seed, pattern, r, o);
    for (int i = 0; i < T::M; ++i)
      for (int kb = 0; kb < T::K / KB; ++kb) {
        double part[32] = {0};
        for (int k = kb * KB; k < (kb + 1) * KB; ++k) {
          const double av = o->a[i * T::K + k];
          if (av == 0.0) continue;
          for (int n = 0; n < T::M; ++n) part[n] += av * o->b[k * T::M + n];
        }
        for (int n = 0; n < T::M; ++n) {
          const int e = T::SCALED ? o->sa[i * (T::K / 32) + kb] + o->sb[kb * T::M + n] : 0;
          d[i * T::M + n] += std::ldexp(part[n], e);
        }
      }
  }
}

// what a lane hashes for one accumulator: acc * 4 as an integer (i8: acc)
template <int KIND> inline int hash_unit(double acc) {
  return (int)(KIND == K_I8 ? acc : acc * 4.0);
}

// signature of a D tile: every lane hashes its accumulators in register order
// through the C/D map, then the weighted lane sum
template <int KIND> inline uint32_t sig_of_tile(const double d[1024]) {
  using T = traits<KIND>;
  uint32_t sig = 0;
  for (int l = 0; l < 64; ++l) {
    uint32_t h = 0;
    for (int reg = 0; reg < T::NREG; ++reg)
      h = acc_hash_step(h, hash_unit<KIND>(d[cd_row(T::M, l, reg) * T::M + l % T::M]));
    sig += h * lane_weight(l);
  }
  return sig;
}

template <int KIND> inline uint32_t expected_sig(uint32_t seed, int pattern, int rounds) {
  double d[1024];
  tile<KIND>(seed, pattern, rounds, d, nullptr);
  return sig_of_tile<KIND>(d);
}

// calls f.template operator()<KIND>() for the runtime kind; false if unknown
template <typename F> inline bool for_kind(int kind, F&& f) {
  switch (kind) {
    case K_F16: f.template operator()<K_F16>(); return true;
    case K_I8: f.template operator()<K_I8>(); return true;
    case K_FP8: f.template operator()<K_FP8>(); return true;
    case K_BF8: f.template operator()<K_BF8>(); return true;
    case K_BF16S: f.template operator()<K_BF16S>(); return true;
    case K_MXFP8: f.template operator()<K_MXFP8>(); return true;
    case K_MXFP6: f.template operator()<K_MXFP6>(); return true;
    case K_MXFP4: f.template operator()<K_MXFP4>(); return true;
    case K_MXMIX: f.template operator()<K_MXMIX>(); return true;
  }
  return false;
}

inline bool rounds_ok(int rounds) { return rounds >= 1 && rounds <= EGPU_MX_MAX_ROUNDS; }

struct expected_fn {
  uint32_t seed;
  int pattern, rounds;
  uint32_t* out;
  template <int KIND> void operator()() { *out = expected_sig<KIND>(seed, pattern, rounds); }
};

// out[NKINDS * p + kind] = signature of `kind` for pattern p.
// Returns 0, or -1 when rounds is outside [1, EGPU_MX_MAX_ROUNDS].
inline int expected_all(uint32_t seed, int rounds,
                        uint32_t out[EGPU_MX_PATTERNS * EGPU_MX_NKINDS]) {
  if (!rounds_ok(rounds)) return -1;
  for (int p = 0; p < EGPU_MX_PATTERNS; ++p)
    for (int kind = 0; kind < EGPU_MX_NKINDS; ++kind) {
      expected_fn f{seed, p, rounds, &out[EGPU_MX_NKINDS * p + kind]};
      for_kind(kind, f);
    }
  return 0;
}

}  // namespace egpu_mx
