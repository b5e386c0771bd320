// selftest_cvt_ref.h — host reference of the conversion sweep
// (egpu_selftest_cvt.hip).
//
// Host-only: plain C++17, no HIP call, no GPU type. The sweep runs the gfx950
// conversion instructions that quantise to and dequantise from the OCP FP8,
// FP6 and FP4 formats (the v_cvt_scalef32_* family and the unscaled FP8
// converts) and folds the raw result registers into one signature per kind.
//
// Shared with the kernel (EGPU_ST_FN): the GENERATOR (lane_sources), the group
// table that says which registers a kind reads and writes, and the fold. The
// generator emits bit patterns with integer arithmetic only, so neither side
// rounds anything but the instruction under test. Host only: decoders and a
// generic round-to-nearest-even encoder written from the OCP and IEEE
// definitions in double precision, and the LAYOUTS (convert_lane): which
// element lands in which bits of which result register.
//
// Encode elements are built as (|c| + q * gap / 4) * 2^S from a finite target
// code c, a quarter-gap offset q (q = 2 is an exact tie) and the lane's scale
// exponent S, so the correct result is known in closed form (closed_form);
// the reference does NOT use it, tests compare the two.
//
// Never generated: NaN or infinity codes and inputs, the scale byte 0xFF,
// anything that rounds above the largest finite magnitude (the largest code
// gets q = 0, 1 only), a subnormal of the SOURCE format, a scale with a
// non-zero mantissa.
//
// Ranges of S. Every source must be zero or an exact normal number of its
// format, every decode result zero or an exact normal number of its format:
//   f32 side   smallest non-zero source is e5m2's quarter gap 2^-18 * 2^S and
//              the largest 57344 * 2^S < 2^(16+S): any S in [-108, 111] would
//              do; the sweep uses [-40, 40] like the matrix sweep's scales.
//   x16        e4m3 from f16: quarter-gap sources reach 2^(-11+S) and f16's
//              smallest normal is 2^-14, so S >= -3; 448 * 2^S <= 65504 gives
//              S <= 7. e4m3 to f16: 2^(-9+S) >= 2^-14 gives S >= -5, and again
//              S <= 7. The kind uses one scale per lane, so [-3, 7]; the bf16
//              groups (e2m1, at most 4 significant bits of bf16's 8) share it.
//   plain      unscaled, S = 0.
// A source has at most 6 significant bits (4 * 15 + 3), within f16's 11 and
// bf16's 8.
#pragma once

#include <cmath>
#include <cstdint>

#include "selftest_mx_ref.h"

// The host reference rounds 16 patterns x 12 kinds x 2048 elements per round in
// double precision (about 20 ms); the bound keeps a probe's reference at about
// a second.
#define EGPU_CVT_MAX_ROUNDS 64
#define EGPU_CVT_PATTERNS 16
#define EGPU_CVT_NKINDS 12
#define EGPU_CVT_NSRC 32  // source registers of a lane, at most
#define EGPU_CVT_NOLD 16  // words whose untouched bits must survive
#define EGPU_CVT_NRES 32  // result registers of a lane, at most

namespace egpu_cv {

using egpu_st::acc_hash_step;
using egpu_st::lane_seed;
using egpu_st::mix32;

enum {
  K_ENC_FP8 = 0, K_ENC_BF8, K_ENC_FP6, K_ENC_BF6, K_ENC_FP4,
  K_DEC_FP8, K_DEC_BF8, K_DEC_FP6, K_DEC_BF6, K_DEC_FP4, K_X16, K_PLAIN
};
enum { N_E4M3 = 0, N_E5M2, N_E2M3, N_E3M2, N_E2M1 };  // narrow formats
enum { W_F32 = 0, W_F16, W_BF16 };                     // wide formats
enum { ENC = 0, DEC };
// How the narrow side is packed:
//   P_WORD  two 8-bit codes in the 16-bit half `sel` of a register
//   P_NIB   two 4-bit codes in byte `sel` of a register, low nibble first
//   P_PK6   32 6-bit codes little-endian in 6 registers
//   P_BYTE  one 8-bit code in byte `sel` of a register (decode only)
enum { P_WORD = 0, P_NIB, P_PK6, P_BYTE };

struct format {
  int ebits, mbits, bias, max_mag;  // max_mag: the largest finite magnitude code
};
EGPU_ST_FN constexpr format narrow(int f) {
  return f == N_E4M3 ? format{4, 3, 7, 0x7E}
       : f == N_E5M2 ? format{5, 2, 15, 0x7B}
       : f == N_E2M3 ? format{2, 3, 1, 0x1F}
       : f == N_E3M2 ? format{3, 2, 3, 0x1F}
                     : format{2, 1, 1, 0x07};
}
EGPU_ST_FN constexpr format wide(int f) {
  return f == W_F32 ? format{8, 23, 127, 0x7F7FFFFF}
       : f == W_F16 ? format{5, 10, 15, 0x7BFF}
                    : format{8, 7, 127, 0x7F7F};
}
EGPU_ST_FN constexpr int bits_of(format f) { return 1 + f.ebits + f.mbits; }

// A kind is one to five groups of conversions; a group is `elems` elements
// per lane and round through one instruction.
struct group {
  int dir, nfmt, wfmt, pack, elems;
};
EGPU_ST_FN constexpr int n_groups(int kind) { return kind == K_X16 ? 4 : kind == K_PLAIN ? 5 : 1; }
EGPU_ST_FN constexpr group group_of(int kind, int g) {
  switch (kind) {
    case K_ENC_FP8: return {ENC, N_E4M3, W_F32, P_WORD, 32};
    case K_ENC_BF8: return {ENC, N_E5M2, W_F32, P_WORD, 32};
    case K_ENC_FP6: return {ENC, N_E2M3, W_F32, P_PK6, 32};
    case K_ENC_BF6: return {ENC, N_E3M2, W_F32, P_PK6, 32};
    case K_ENC_FP4: return {ENC, N_E2M1, W_F32, P_NIB, 32};
    case K_DEC_FP8: return {DEC, N_E4M3, W_F32, P_WORD, 32};
    case K_DEC_BF8: return {DEC, N_E5M2, W_F32, P_WORD, 32};
    case K_DEC_FP6: return {DEC, N_E2M3, W_F32, P_PK6, 32};
    case K_DEC_BF6: return {DEC, N_E3M2, W_F32, P_PK6, 32};
    case K_DEC_FP4: return {DEC, N_E2M1, W_F32, P_NIB, 32};
    case K_X16:
      return g == 0 ? group{ENC, N_E4M3, W_F16, P_WORD, 16}    // ..._pk_fp8_f16
           : g == 1 ? group{ENC, N_E2M1, W_BF16, P_NIB, 16}    // ..._pk_fp4_bf16
           : g == 2 ? group{DEC, N_E4M3, W_F16, P_WORD, 16}    // ..._pk_f16_fp8
                    : group{DEC, N_E2M1, W_BF16, P_NIB, 16};   // ..._pk_bf16_fp4
    default:  // K_PLAIN
      return g == 0 ? group{ENC, N_E4M3, W_F32, P_WORD, 8}     // v_cvt_pk_fp8_f32
           : g == 1 ? group{ENC, N_E5M2, W_F32, P_WORD, 8}     // v_cvt_pk_bf8_f32
           : g == 2 ? group{DEC, N_E4M3, W_F32, P_WORD, 8}     // v_cvt_pk_f32_fp8
           : g == 3 ? group{DEC, N_E4M3, W_F32, P_BYTE, 8}     // v_cvt_f32_fp8
                    : group{DEC, N_E5M2, W_F32, P_BYTE, 8};    // v_cvt_f32_bf8
  }
}
EGPU_ST_FN constexpr bool scaled(int kind) { return kind != K_PLAIN; }
EGPU_ST_FN constexpr int scale_lo(int kind) { return kind == K_PLAIN ? 0 : kind == K_X16 ? -3 : -40; }
EGPU_ST_FN constexpr int scale_hi(int kind) { return kind == K_PLAIN ? 0 : kind == K_X16 ? 7 : 40; }

// Registers a group reads (src), preserves bits of (old) and writes (res).
EGPU_ST_FN constexpr int n_src(group g) {
  return g.dir == ENC ? g.elems * bits_of(wide(g.wfmt)) / 32
       : g.pack == P_PK6 ? 6 : g.pack == P_NIB ? g.elems / 8 : g.elems / 4;
}
EGPU_ST_FN constexpr int n_old(group g) {
  return g.dir == ENC && g.pack != P_PK6 ? g.elems / 2 : 0;
}
EGPU_ST_FN constexpr int n_res(group g) {
  return g.dir == DEC ? g.elems * bits_of(wide(g.wfmt)) / 32 : g.pack == P_PK6 ? 6 : g.elems / 2;
}
// First register of group g in the lane's src / old / res arrays (g = n_groups:
// the kind's totals).
EGPU_ST_FN constexpr int src_base(int kind, int g) {
  int n = 0;
  for (int i = 0; i < g; ++i) n += n_src(group_of(kind, i));
  return n;
}
EGPU_ST_FN constexpr int old_base(int kind, int g) {
  int n = 0;
  for (int i = 0; i < g; ++i) n += n_old(group_of(kind, i));
  return n;
}
EGPU_ST_FN constexpr int res_base(int kind, int g) {
  int n = 0;
  for (int i = 0; i < g; ++i) n += n_res(group_of(kind, i));
  return n;
}

// ---- generator
// One element: sign, magnitude code (0..max_mag) and quarter-gap offset q.
struct element {
  uint32_t sign, mag, q;
};

EGPU_ST_FN uint32_t group_seed(uint32_t seed, int pattern, int kind, int g, int round) {
  return mix32(lane_seed(seed, pattern, 64, 32 + kind) + (uint32_t)(8 * round + g));
}

// Element j of lane `lane`. The wave's 64 * elems elements of a round are
// consecutive values of t; t * odd + c is a bijection of [0, 2048) and, for 1024
// consecutive t, of its low ten bits: k = {mag:7, sign:1, q:2}. So a wave with
// 16 or 32 elements per lane meets every (mag, sign, q) of a format of at most
// 8 bits in every round; the 8-element groups of `plain` take two rounds.
EGPU_ST_FN element gen_element(uint32_t gseed, format nf, int elems, int round, int lane, int j) {
  const uint32_t t = (uint32_t)(lane * elems + j) + (uint32_t)(64 * elems) * (uint32_t)round;
  const uint32_t k = (t * 1237u + gseed) & 1023u;
  element e{(k >> 2) & 1u, (k >> 3) % (uint32_t)(nf.max_mag + 1), k & 3u};
  if (e.mag == (uint32_t)nf.max_mag) e.q &= 1u;  // never above the largest finite magnitude
  return e;
}

// The bits, in wide format wf, of (-1)^sign * (|c| + q * gap / 4) * 2^S, c the
// narrow code of magnitude e.mag. The gap to the next code is one unit of c's
// significand, so the value is n = 4 * sig + q units of 2^(exp - 2 + S).
EGPU_ST_FN uint32_t wide_bits(format wf, format nf, element e, int S) {
  const uint32_t ex = e.mag >> nf.mbits, frac = e.mag & ((1u << nf.mbits) - 1u);
  const uint32_t sig = ex ? ((1u << nf.mbits) | frac) : frac;
  const int exp = (ex ? (int)ex : 1) - nf.bias - nf.mbits;
  const uint32_t n = 4u * sig + e.q;  // at most 63
  const uint32_t sign = e.sign << (wf.ebits + wf.mbits);
  if (n == 0) return sign;
  int p = 0;
  while ((n >> (p + 1)) != 0) ++p;  // p = floor(log2 n) <= 5
  const uint32_t biased = (uint32_t)(p + exp - 2 + S + wf.bias);
  return sign | (biased << wf.mbits) | ((n << (wf.mbits - p)) & ((1u << wf.mbits) - 1u));
}

EGPU_ST_FN uint32_t narrow_code(format nf, element e) {
  return (e.sign << (nf.ebits + nf.mbits)) | e.mag;
}

// What the generator knows the rounded code to be: below the tie c, above it
// the next code, on it whichever of the two is even.
EGPU_ST_FN uint32_t closed_form(format nf, element e) {
  const uint32_t up = e.q > 2u || (e.q == 2u && (e.mag & 1u)) ? 1u : 0u;
  return (e.sign << (nf.ebits + nf.mbits)) | (e.mag + up);
}

// The f32 scale operand of a lane: 2^S, mantissa zero.
EGPU_ST_FN int lane_scale(uint32_t seed, int pattern, int kind, int round, int lane) {
  const uint32_t span = (uint32_t)(scale_hi(kind) - scale_lo(kind) + 1);
  return scale_lo(kind) + (int)(mix32(group_seed(seed, pattern, kind, 7, round) + (uint32_t)lane) % span);
}
EGPU_ST_FN uint32_t scale_bits(int S) { return (uint32_t)(127 + S) << 23; }

// A word whose bits the instruction must leave alone where it does not write.
// Rounds 2k and 2k+1 are complements, so every preserved bit is seen both ways.
EGPU_ST_FN uint32_t old_word(uint32_t seed, int pattern, int kind, int round, int lane, int i) {
  const uint32_t w = mix32(group_seed(seed, pattern, kind, 6, round >> 1) + (uint32_t)(16 * lane + i));
  return (round & 1) ? ~w : w;
}

// Everything one lane hands to the instructions of a kind in one round.
struct lane_io {
  uint32_t src[EGPU_CVT_NSRC];
  uint32_t old[EGPU_CVT_NOLD];
  uint32_t scale;  // f32 bits
};

EGPU_ST_FN void put_bits(uint32_t* regs, int off, int bits, uint32_t v) {
  regs[off >> 5] |= v << (off & 31);
  if ((off & 31) + bits > 32) regs[(off >> 5) + 1] |= v >> (32 - (off & 31));
}

// Sources are packed little-endian, element j at bit j * width of the group's
// registers (see the P_* packings for the narrow side).
template <int KIND>
EGPU_ST_FN void lane_sources(uint32_t seed, int pattern, int lane, int round, lane_io* io) {
#pragma unroll
  for (int i = 0; i < EGPU_CVT_NSRC; ++i) io->src[i] = 0;
#pragma unroll
  for (int i = 0; i < EGPU_CVT_NOLD; ++i)
    io->old[i] = i < old_base(KIND, n_groups(KIND)) ? old_word(seed, pattern, KIND, round, lane, i) : 0;
  const int S = lane_scale(seed, pattern, KIND, round, lane);
  io->scale = scale_bits(S);
#pragma unroll
  for (int g = 0; g < n_groups(KIND); ++g) {
    constexpr int kind = KIND;
    const group gr = group_of(kind, g);
    const format nf = narrow(gr.nfmt), wf = wide(gr.wfmt);
    const uint32_t gs = group_seed(seed, pattern, KIND, g, round);
    uint32_t* dst = io->src + src_base(kind, g);
#pragma unroll
    for (int j = 0; j < gr.elems; ++j) {
      const element e = gen_element(gs, nf, gr.elems, round, lane, j);
      if (gr.dir == ENC)
        put_bits(dst, j * bits_of(wf), bits_of(wf), wide_bits(wf, nf, e, S));
      else
        put_bits(dst, j * (gr.pack == P_PK6 ? 6 : gr.pack == P_NIB ? 4 : 8), bits_of(nf),
                 narrow_code(nf, e));
    }
  }
}

// ---- fold: odd weights distinct per (lane, register), summed over the wave,
// then chained over the rounds. A decoded f32 has at most 12 significant bits
// at its top, and a sum of such words times anything has as many zeros at its
// bottom, so every word goes through mix32 (a bijection) first: one changed
// bit anywhere changes the term in all 32.
EGPU_ST_FN uint32_t reg_weight(int lane, int reg) {
  return (2u * (uint32_t)(lane * EGPU_CVT_NRES + reg) + 1u) * 0x01000193u;
}
EGPU_ST_FN uint32_t fold_term(uint32_t word, int lane, int reg) {
  return mix32(word) * reg_weight(lane, reg);
}
EGPU_ST_FN uint32_t round_step(uint32_t sig, uint32_t round_sum) {
  return acc_hash_step(sig, (int)round_sum);
}

// ---------------------------------------------------------------- host only

// the one decoder the matrix sweep's header lacks: e3m2 (bias 3, no inf, no NaN)
inline double decode_e3m2(uint32_t b) { return egpu_mx::decode_ieee(b & 0x3fu, 3, 2, false); }

inline double decode_narrow(int nfmt, uint32_t code) {
  switch (nfmt) {
    case N_E4M3: return egpu_mx::decode_e4m3fn(code);
    case N_E5M2: return egpu_mx::decode_e5m2(code);
    case N_E2M3: return egpu_mx::decode_e2m3(code);
    case N_E3M2: return decode_e3m2(code);
    default: return egpu_mx::decode_e2m1(code);
  }
}
inline double decode_wide(int wfmt, uint32_t bits) {
  return wfmt == W_F32 ? egpu_mx::decode_ieee(bits, 8, 23, true)
       : wfmt == W_F16 ? egpu_mx::decode_f16(bits)
                       : egpu_mx::decode_bf16(bits);
}

// Round-to-nearest-even of a finite value into a format, from the definition:
// pick the binade (clamped to the subnormal one), scale so that one unit is one
// significand step, round the integer to nearest with ties to even, and let a
// carry run into the exponent. Saturates at max_mag (the sweep never gets there).
inline uint32_t encode_rne(format f, double v) {
  const uint32_t sign = std::signbit(v) ? 1u << (f.ebits + f.mbits) : 0u;
  const double a = std::fabs(v);
  if (a == 0.0) return sign;
  int e = std::ilogb(a);
  if (e < 1 - f.bias) e = 1 - f.bias;
  const double units = std::ldexp(a, f.mbits - e);  // exact: a power of two
  double r = std::floor(units);
  const double rest = units - r;
  if (rest > 0.5 || (rest == 0.5 && std::fmod(r, 2.0) == 1.0)) r += 1.0;
  const uint64_t mag = ((uint64_t)(e + f.bias - 1) << f.mbits) + (uint64_t)r;
  return sign | (mag > (uint64_t)f.max_mag ? (uint32_t)f.max_mag : (uint32_t)mag);
}

inline uint32_t get_bits(const uint32_t* regs, int nregs, int off, int bits) {
  uint64_t v = regs[off >> 5];
  if ((off >> 5) + 1 < nregs) v |= (uint64_t)regs[(off >> 5) + 1] << 32;
  return (uint32_t)(v >> (off & 31)) & (bits == 32 ? 0xffffffffu : (1u << bits) - 1u);
}

// Where v_cvt_scalef32_2xpk16_* puts source element j (0..15 the first vector,
// 16..31 the second) among the 32 packed results.
inline int pk6_slot(int j) { return j < 16 ? 2 * j : 2 * (j - 16) + 1; }

inline int scale_exponent(uint32_t scale) { return (int)((scale >> 23) & 0xffu) - 127; }

// LAYOUTS. What the instructions of `kind` must leave in the lane's result
// registers. Encode divides by 2^S, decode multiplies by it, S the exponent of
// the lane's scale operand.
//   encode P_WORD  conversion i takes elements 2i, 2i+1 and writes res[i]: the
//                  16-bit half i & 1 becomes code(2i) | code(2i+1) << 8, the
//                  other half keeps old[i]
//   encode P_NIB   conversion i writes byte i & 3 of res[i]:
//                  code(2i) | code(2i+1) << 4; the other bytes keep old[i]
//   encode P_PK6   the two 16-element source vectors are interleaved: element
//                  k of the first (source register k) lands at bit 6 * 2k of the
//                  6 result registers, element k of the second (source
//                  register 16 + k) at bit 6 * (2k + 1). An MI355X showed this;
//                  the first vector does not fill positions 0..15.
//   decode P_WORD  conversion i reads half i & 1 of src[i >> 1] and gives
//                  elements 2i (low byte), 2i+1
//   decode P_NIB   conversion i reads byte i & 3 of src[i >> 2]: elements 2i
//                  (low nibble), 2i+1
//   decode P_BYTE  conversion i reads byte i & 3 of src[i >> 2]: element i
//   decode P_PK6   element j from bit 6 * j
// Decoded elements are stored in element order, f32 one per register, 16-bit
// results two per register with the even element in the low half.
inline void convert_lane(int kind, const lane_io& io, uint32_t res[EGPU_CVT_NRES]) {
  for (int i = 0; i < EGPU_CVT_NRES; ++i) res[i] = 0;
  const int S = scaled(kind) ? scale_exponent(io.scale) : 0;
  for (int g = 0; g < n_groups(kind); ++g) {
    const group gr = group_of(kind, g);
    const format nf = narrow(gr.nfmt), wf = wide(gr.wfmt);
    const uint32_t* src = io.src + src_base(kind, g);
    const uint32_t* old = io.old + old_base(kind, g);
    uint32_t* out = res + res_base(kind, g);
    const int wb = bits_of(wf);
    if (gr.dir == ENC) {
      uint32_t code[32];
      for (int j = 0; j < gr.elems; ++j)
        code[j] = encode_rne(nf, std::ldexp(decode_wide(gr.wfmt, get_bits(src, n_src(gr), j * wb, wb)), -S));
      if (gr.pack == P_PK6) {
        for (int j = 0; j < gr.elems; ++j) put_bits(out, 6 * pk6_slot(j), 6, code[j]);
      } else {
        for (int i = 0; i < gr.elems / 2; ++i) {
          const bool word = gr.pack == P_WORD;
          const int shift = word ? 16 * (i & 1) : 8 * (i & 3);
          const uint32_t mask = (word ? 0xffffu : 0xffu) << shift;
          const uint32_t pair = code[2 * i] | (code[2 * i + 1] << (word ? 8 : 4));
          out[i] = (old[i] & ~mask) | (pair << shift);
        }
      }
    } else {
      for (int j = 0; j < gr.elems; ++j) {
        const int cb = gr.pack == P_PK6 ? 6 : gr.pack == P_NIB ? 4 : 8;
        const uint32_t code = get_bits(src, n_src(gr), j * cb, bits_of(nf));
        put_bits(out, j * wb, wb, encode_rne(wf, std::ldexp(decode_narrow(gr.nfmt, code), S)));
      }
    }
  }
}

// calls f.template operator()<KIND>() for the runtime kind; false if unknown
template <typename F> inline bool for_kind(int kind, F&& f) {
  switch (kind) {
    case K_ENC_FP8: f.template operator()<K_ENC_FP8>(); return true;
    case K_ENC_BF8: f.template operator()<K_ENC_BF8>(); return true;
    case K_ENC_FP6: f.template operator()<K_ENC_FP6>(); return true;
    case K_ENC_BF6: f.template operator()<K_ENC_BF6>(); return true;
    case K_ENC_FP4: f.template operator()<K_ENC_FP4>(); return true;
    case K_DEC_FP8: f.template operator()<K_DEC_FP8>(); return true;
    case K_DEC_BF8: f.template operator()<K_DEC_BF8>(); return true;
    case K_DEC_FP6: f.template operator()<K_DEC_FP6>(); return true;
    case K_DEC_BF6: f.template operator()<K_DEC_BF6>(); return true;
    case K_DEC_FP4: f.template operator()<K_DEC_FP4>(); return true;
    case K_X16: f.template operator()<K_X16>(); return true;
    case K_PLAIN: f.template operator()<K_PLAIN>(); return true;
  }
  return false;
}

struct sources_fn {
  uint32_t seed;
  int pattern, lane, round;
  lane_io* io;
  template <int KIND> void operator()() { lane_sources<KIND>(seed, pattern, lane, round, io); }
};

// Sources and reference results of one lane. Returns false for an unknown kind.
inline bool lane_reference(int kind, uint32_t seed, int pattern, int lane, int round, lane_io* io,
                           uint32_t res[EGPU_CVT_NRES]) {
  if (!for_kind(kind, sources_fn{seed, pattern, lane, round, io})) return false;
  convert_lane(kind, *io, res);
  return true;
}

inline uint32_t expected_sig(uint32_t seed, int pattern, int kind, int rounds) {
  uint32_t sig = 0;
  for (int r = 0; r < rounds; ++r) {
    uint32_t sum = 0;
    for (int lane = 0; lane < 64; ++lane) {
      lane_io io;
      uint32_t res[EGPU_CVT_NRES];
      lane_reference(kind, seed, pattern, lane, r, &io, res);
      for (int reg = 0; reg < EGPU_CVT_NRES; ++reg) sum += fold_term(res[reg], lane, reg);
    }
    sig = round_step(sig, sum);
  }
  return sig;
}

inline bool rounds_ok(int rounds) { return rounds >= 1 && rounds <= EGPU_CVT_MAX_ROUNDS; }
inline bool kind_ok(int kind) { return kind >= 0 && kind < EGPU_CVT_NKINDS; }

// out[p][kind] = signature of `kind` for pattern p.
// Returns 0, or -1 when rounds is outside [1, EGPU_CVT_MAX_ROUNDS].
inline int expected_all(uint32_t seed, int rounds, uint32_t out[EGPU_CVT_PATTERNS][EGPU_CVT_NKINDS]) {
  if (!rounds_ok(rounds)) return -1;
  for (int p = 0; p < EGPU_CVT_PATTERNS; ++p)
    for (int kind = 0; kind < EGPU_CVT_NKINDS; ++kind) out[p][kind] = expected_sig(seed, p, kind, rounds);
  return 0;
}

}  // namespace egpu_cv
