// selftest_atomic_ref.h — host reference of the atomic sweep
// (egpu_selftest_atomic.hip).
//
// Host-only apart from the EGPU_ST_FN part: plain C++17, no HIP call. The sweep
// executes read-modify-write atomics in the LDS and behind the vector memory
// path and checks what they leave in memory and what they return.
//
// Shared with the kernel (EGPU_ST_FN): the op table (which opcode a kind issues
// in which slot), the GENERATOR (gen_op: cell and operands of one lane in one
// slot; init_word: what a cell holds before the atomics) and the fold. Host
// only: the REFERENCE (apply: what one atomic does to its cell and returns),
// the replay of a workgroup's 256 lanes, and the closed form of the grid cells.
//
// Layout. An arena is 1024 words (4 KiB): 8 slots of 128 words. Slot s of a
// kind issues one opcode (slot_of) into its own 128 words, so no cell ever
// meets two opcodes. A 64-bit cell is two words, low word first. Every address
// is 128 * s + a generator function of (lane, slot, group, round >> 1, seed).
//
// Cell map of a slot: the wave's 64 lanes are permuted (p = lane * odd + c mod
// 64) and lanes p >> fl share a cell, a same-address fan-in of 2^fl = 1, 2, 4,
// 16 or 64 lanes of one wave; 2^sl = 1, 2 or 4 waves then share the cells. A
// lane whose cell would fall outside the slot's words sits the slot out
// (active = false), which depends on the generator alone. Returning contended
// ops and the claim use wave-private cells (sl = 0).
//
// ORDER INDEPENDENCE. Every contended op commutes and associates on the values
// generated, so the reference applies the 256 lanes in lane order and any other
// order gives the same cells:
//   add u32/u64, and, or, xor, min, max   commutative and associative as such;
//   FP add                  operands and initial cells are whole numbers in
//       [-3, 3] (never -0), so a cell that n lanes add to holds partial sums
//       of magnitude at most 3 * (n + 1) in any order. All whole numbers up
//       to 2^(p) are exact in a format with p significand bits: 2^8 for bf16,
//       2^11 for f16, 2^24 for f32, 2^53 for f64. The largest fan-in is 64
//       lanes x 4 waves = 256, 3 * 257 = 771 < 2^11, so only bf16 needs a
//       bound: shape_of halves the wave sharing until 3 * (fan-in + 1) <= 256,
//       that is fan-in <= 64. With +0 and no -0 among the values and round to
//       nearest, no sum is -0. No NaN, infinity or subnormal is generated.
//   f64 min/max             non-zero whole numbers, |v| <= 2^20
//   add-return, inc, dec    every lane of a cell passes the same operand (an
//       odd constant, one wrap limit), so the cell walks one fixed sequence
//       and the returned values are a known set, whoever gets which;
//   swap                    returned values plus the final value are the
//       initial value plus every operand, as a multiset. Which of them stays
//       in the cell is not determined, so a swap cell's final word is not
//       folded with the arena: the cell's first lane (`lead`, chosen by the
//       generator) folds it next to its own returned word, same weight.
// The fold of returned words is therefore symmetric per cell: mix32(word) times
// the weight of the CELL (cell_weight), the same weight its final word gets.
// With one lane per cell that is a weight per lane and slot.
//   claim                   all lanes of a cell compare-and-swap EMPTY for
//       their id, once. Who wins is not determined, so neither the returned
//       nor the final words are folded; each lane folds its own consistency
//       flag (returned == EMPTY ? final == id : final == returned) times its
//       lane weight, plus one if it won. The sum is known: every active lane
//       consistent, one winner per cell.
// Integer rounds 2k and 2k+1 use complementary initial cells and operands
// (and/or keep one-hot masks so that a fan-in of 256 does not saturate; inc,
// dec, add-return and claim keep their structured operands).
//
// Grid cells (g_grid). Every lane of every workgroup adds into one 4 KiB slice
// that is zero before the launch and is never re-initialised: there is no
// barrier across the grid. Its f64 operands are whole numbers in [-3, 3] times
// 2^24, so that sums reach the upper significand. A cell takes at most 256
// lanes per workgroup and round: the sum of magnitudes is at most
// 3 * 2^24 * 256 * blocks * rounds, exact while that is <= 2^53, so
// blocks * rounds <= 2^21 / 3 = 699,050 (EGPU_AT_GRID_MAX_WORK). The integer
// cells are exact modulo 2^32 and 2^64 for any grid.
#pragma once

#include <cstdint>
#include <cstring>

#include "selftest_cvt_ref.h"

// The host replay costs 4 groups x 11 kinds x 256 lanes x 8 slots per round
// (under a millisecond); the bound is the siblings'.
#define EGPU_AT_MAX_ROUNDS 64
#define EGPU_AT_GROUPS 4
#define EGPU_AT_PATTERNS 16  // 4 groups x 4 waves
#define EGPU_AT_NKINDS 11
#define EGPU_AT_WORDS 1024
#define EGPU_AT_NSLOT 8
#define EGPU_AT_SLOT_WORDS 128
#define EGPU_AT_LANES 256
#define EGPU_AT_OP_WORDS 6  // {op or 0, first word of the cell, a lo, a hi, b lo, b hi}
#define EGPU_AT_GRID_MAX_WORK 699050
#define EGPU_AT_EMPTY 0xFFFFFFFFu

namespace egpu_at {

using egpu_st::acc_hash_step;
using egpu_st::lane_seed;
using egpu_st::lane_weight;
using egpu_st::mix32;

enum {
  K_L_ADD = 0, K_L_LOGIC, K_L_RTN, K_L_CAS, K_L_FADD,
  K_G_ADD, K_G_LOGIC, K_G_RTN, K_G_CAS, K_G_FADD, K_G_GRID
};
enum {
  OP_NONE = 0,
  // non-returning, workgroup-shared cells
  OP_ADD32, OP_ADD64, OP_AND, OP_OR, OP_XOR, OP_MINI, OP_MAXI, OP_MINU, OP_MAXU,
  OP_FADD32, OP_FADD64, OP_PKF16, OP_PKBF16, OP_FMIN64, OP_FMAX64,
  // returning, wave-private cells
  OP_ADDR32, OP_ADDR64, OP_INC, OP_DEC, OP_SWAP, OP_CAS32, OP_CAS64, OP_CLAIM
};
// which fan-ins a slot rotates through
enum { FM_ANY = 0, FM_PRIV, FM_ONE, FM_GRID };

EGPU_ST_FN constexpr bool is_lds(int kind) { return kind < K_G_ADD; }
EGPU_ST_FN constexpr bool is64(int op) {
  return op == OP_ADD64 || op == OP_FADD64 || op == OP_FMIN64 || op == OP_FMAX64 ||
         op == OP_ADDR64 || op == OP_CAS64;
}
EGPU_ST_FN constexpr bool returns(int op) { return op >= OP_ADDR32; }
EGPU_ST_FN constexpr bool is_fp_add(int op) { return op >= OP_FADD32 && op <= OP_PKBF16; }
// the largest whole number below which every whole number is exact
EGPU_ST_FN constexpr int exact_limit(int op) {
  return op == OP_PKBF16 ? 1 << 8 : op == OP_PKF16 ? 1 << 11 : 1 << 24;
}

struct slot {
  int op, fm;
};
EGPU_ST_FN constexpr slot slot_of(int kind, int s) {
  if (kind == K_G_GRID)
    return s == 0 ? slot{OP_ADD32, FM_GRID} : s == 1 ? slot{OP_ADD64, FM_GRID}
         : s == 2 ? slot{OP_XOR, FM_GRID} : s == 3 ? slot{OP_MAXU, FM_GRID}
         : s == 4 ? slot{OP_FADD64, FM_GRID} : slot{OP_NONE, FM_ONE};
  switch (kind % 5) {
    case K_L_ADD: return s < 6 ? slot{(s & 1) ? OP_ADD64 : OP_ADD32, FM_ANY} : slot{OP_NONE, FM_ONE};
    case K_L_LOGIC: return s < 7 ? slot{OP_AND + s, FM_ANY} : slot{OP_NONE, FM_ONE};
    case K_L_RTN:
      return s < 4 ? slot{s == 0 ? OP_ADDR32 : s == 1 ? OP_INC : s == 2 ? OP_DEC : OP_SWAP, FM_PRIV}
           : s == 4 ? slot{OP_ADDR32, FM_ONE} : s == 5 ? slot{OP_ADDR64, FM_ONE}
           : s == 6 ? slot{OP_SWAP, FM_ONE} : slot{OP_NONE, FM_ONE};
    case K_L_CAS:
      return s == 0 ? slot{OP_CAS32, FM_ONE} : s == 1 ? slot{OP_CAS64, FM_ONE}
           : s < 4 ? slot{OP_CLAIM, FM_PRIV} : slot{OP_NONE, FM_ONE};
    default:  // K_L_FADD; f64 min/max exist behind the memory path only
      return s < 4 ? slot{OP_FADD32 + s, FM_ANY}
           : (s < 6 && !is_lds(kind)) ? slot{OP_FMIN64 + (s - 4), FM_ANY} : slot{OP_NONE, FM_ONE};
  }
}

// fl: log2 of the lanes of one wave per cell; sl: log2 of the waves per cell;
// cw: cells of one wave (or of the waves that share them)
struct shape {
  int fl, sl, cw;
};
EGPU_ST_FN constexpr int fan_log(int i) { return i == 0 ? 0 : i == 1 ? 1 : i == 2 ? 2 : i == 3 ? 4 : 6; }
EGPU_ST_FN constexpr shape shape_of(int kind, int s, int group, int round) {
  const slot st = slot_of(kind, s);
  const int q = s + group + 3 * (round >> 1);
  int fl = 0, sl = 0;
  if (st.fm == FM_PRIV) {
    fl = fan_log(1 + (q & 3));
  } else if (st.fm != FM_ONE) {
    fl = fan_log(q % 5);
    sl = st.fm == FM_GRID ? 2 : (s + (group >> 1) + (round >> 1)) % 3;
  }
  if (is_fp_add(st.op))
    while (sl > 0 && 3 * ((1 << (fl + sl)) + 1) > exact_limit(st.op)) --sl;
  const int cap = (EGPU_AT_SLOT_WORDS / (is64(st.op) ? 2 : 1)) >> (2 - sl);
  return shape{fl, sl, (64 >> fl) < cap ? (64 >> fl) : cap};
}

// ---- generator

EGPU_ST_FN uint32_t slot_seed(uint32_t seed, int kind, int s, int group, int round) {
  return mix32(lane_seed(seed, group, 64, 64 + kind) + (uint32_t)(16 * (round >> 1) + s));
}
EGPU_ST_FN uint32_t cell_hash(uint32_t hs, int cellword) {
  return mix32(hs + 0x51ed27u * (uint32_t)(cellword + 1));
}
EGPU_ST_FN uint64_t u64_of(uint32_t lo, uint32_t hi) { return ((uint64_t)hi << 32) | lo; }
// two hashed words, complemented in odd rounds
EGPU_ST_FN uint64_t int_pair(uint32_t h, int round) {
  const uint64_t v = u64_of(mix32(h), mix32(h + 1u));
  return (round & 1) ? ~v : v;
}
// a whole number in [-3, 3]; the round counts, there is no FP complement
EGPU_ST_FN int whole7(uint32_t h, int round) {
  return (int)(mix32(h + 0x9e3779b9u * (uint32_t)(round & 1)) % 7u) - 3;
}
EGPU_ST_FN int nonzero_whole(uint32_t h, int round) {
  const uint32_t m = mix32(h + 0x9e3779b9u * (uint32_t)(round & 1));
  const int v = 1 + (int)(m & 0xfffffu);
  return (m >> 31) ? -v : v;
}
// encodings of n in [-3, 3], +0 for 0
EGPU_ST_FN uint32_t bf16_of(int n) {
  const int m = n < 0 ? -n : n;
  return (m == 0 ? 0u : m == 1 ? 0x3F80u : m == 2 ? 0x4000u : 0x4040u) | (n < 0 ? 0x8000u : 0u);
}
EGPU_ST_FN uint32_t f16_of(int n) {
  const int m = n < 0 ? -n : n;
  return (m == 0 ? 0u : m == 1 ? 0x3C00u : m == 2 ? 0x4000u : 0x4200u) | (n < 0 ? 0x8000u : 0u);
}
EGPU_ST_FN uint32_t f32_of(int n) { return bf16_of(n) << 16; }
EGPU_ST_FN uint64_t f64_of(double v) {  // v a whole number: the conversion that made it is exact
  uint64_t b;
  memcpy(&b, &v, 8);
  return b;
}
// an FP value of the op's format from one hash
EGPU_ST_FN uint64_t fp_value(int op, uint32_t h, int round, bool grid) {
  switch (op) {
    case OP_FADD32: return f32_of(whole7(h, round));
    case OP_PKF16: return f16_of(whole7(h, round)) | (f16_of(whole7(h + 77u, round)) << 16);
    case OP_PKBF16: return bf16_of(whole7(h, round)) | (bf16_of(whole7(h + 77u, round)) << 16);
    case OP_FADD64: return f64_of((double)whole7(h, round) * (grid ? 16777216.0 : 1.0));
    default: return f64_of((double)nonzero_whole(h, round));  // f64 min/max
  }
}
EGPU_ST_FN uint32_t wrap_limit(uint32_t ch) { return 3u + (ch & 63u); }

// What the 32- or 64-bit cell at `cellword` holds before the atomics.
EGPU_ST_FN uint64_t init_cell(int kind, int op, uint32_t hs, int round, int cellword) {
  const uint32_t ch = cell_hash(hs, cellword);
  if (kind == K_G_GRID || op == OP_NONE) return 0;
  if (op >= OP_FADD32 && op <= OP_FMAX64) return fp_value(op, ch, round, false);
  if (op == OP_INC || op == OP_DEC) return mix32(ch) % (wrap_limit(ch) + 1u);
  if (op == OP_CLAIM) return EGPU_AT_EMPTY;
  const uint64_t v = int_pair(ch, round);
  return is64(op) ? v : (uint32_t)v;
}
EGPU_ST_FN uint32_t init_word(int kind, uint32_t seed, int group, int round, int word) {
  const int s = word / EGPU_AT_SLOT_WORDS, op = slot_of(kind, s).op;
  const uint32_t hs = slot_seed(seed, kind, s, group, round);
  if (!is64(op)) return (uint32_t)init_cell(kind, op, hs, round, word);
  return (uint32_t)(init_cell(kind, op, hs, round, word & ~1) >> (32 * (word & 1)));
}

struct op_t {
  int op;  // OP_NONE: the lane sits this slot out
  int cell;  // first word of the cell in the arena
  uint64_t a, b;  // operand; compare value (cas, claim)
  bool lead;  // the first of the wave's lanes on this cell
};

EGPU_ST_FN op_t gen_op(int kind, int s, uint32_t seed, int group, int round, int tid) {
  const slot st = slot_of(kind, s);
  const shape sp = shape_of(kind, s, group, round);
  const uint32_t hs = slot_seed(seed, kind, s, group, round);
  const int wave = tid >> 6, lane = tid & 63;
  const int p = (int)(((uint32_t)lane * (2u * (hs & 31u) + 1u) + (hs >> 5)) & 63u);
  const int c = p >> sp.fl;
  op_t o{OP_NONE, EGPU_AT_SLOT_WORDS * s, 0, 0, false};
  if (st.op == OP_NONE || c >= sp.cw) return o;
  o.op = st.op;
  o.lead = (p & ((1 << sp.fl) - 1)) == 0;
  o.cell = EGPU_AT_SLOT_WORDS * s + ((wave >> sp.sl) * sp.cw + c) * (is64(st.op) ? 2 : 1);
  const uint32_t ch = cell_hash(hs, o.cell);
  const uint32_t lh = mix32(hs + 0x9e3779b9u * (uint32_t)(tid + 1));
  const uint64_t mask = is64(st.op) ? ~0ull : 0xffffffffull;
  switch (st.op) {
    case OP_AND: o.a = (uint32_t)~(1u << ((ch + 5u * (uint32_t)(p & 7)) & 31u)); break;
    case OP_OR: o.a = 1u << ((ch + 5u * (uint32_t)(p & 7)) & 31u); break;
    case OP_ADDR32: case OP_ADDR64: o.a = u64_of(mix32(ch + 2u) | 1u, mix32(ch + 3u)) & mask; break;
    case OP_INC: case OP_DEC: o.a = wrap_limit(ch); break;
    case OP_CAS32: case OP_CAS64:
      o.a = int_pair(lh, round) & mask;
      o.b = init_cell(kind, st.op, hs, round, o.cell) ^
            ((lh & 1u) ? 0ull : 1ull << ((lh >> 1) & (is64(st.op) ? 63u : 31u)));
      break;
    case OP_CLAIM: o.a = (uint32_t)(tid + 1); o.b = EGPU_AT_EMPTY; break;
    case OP_FADD32: case OP_FADD64: case OP_PKF16: case OP_PKBF16: case OP_FMIN64: case OP_FMAX64:
      o.a = fp_value(st.op, lh, round, kind == K_G_GRID);
      break;
    default: o.a = int_pair(lh, round) & mask; break;  // add, xor, min, max, swap
  }
  return o;
}

// ---- fold
// cell_weight: odd and distinct per word of the arena. Final words and returned
// words of a cell share it (see the top). A round's sum goes through
// round_step; a wave's signature of a kind chains its rounds.
EGPU_ST_FN uint32_t cell_weight(int word) { return (2u * (uint32_t)word + 1u) * 0x01000193u; }
EGPU_ST_FN uint32_t final_term(int kind, int word, uint32_t value) {
  const int op = slot_of(kind, word / EGPU_AT_SLOT_WORDS).op;
  return op == OP_CLAIM || op == OP_SWAP ? 0u : mix32(value) * cell_weight(word);
}
// what a lane adds for one slot: ret is what its atomic returned, fin the low
// word of its cell after the barrier (claim and swap only)
EGPU_ST_FN uint32_t lane_term(const op_t& o, int tid, uint64_t ret, uint32_t fin) {
  if (!returns(o.op)) return 0u;
  if (o.op == OP_CLAIM) {
    const uint32_t r = (uint32_t)ret, id = (uint32_t)o.a;
    const bool ok = r == EGPU_AT_EMPTY ? fin == id : fin == r;
    return (ok ? lane_weight(tid) : 0u) + (r == EGPU_AT_EMPTY ? 1u : 0u);
  }
  uint32_t t = mix32((uint32_t)ret) * cell_weight(o.cell);
  if (o.op == OP_SWAP && o.lead) t += mix32(fin) * cell_weight(o.cell);
  if (is64(o.op)) t += mix32((uint32_t)(ret >> 32)) * cell_weight(o.cell + 1);
  return t;
}
EGPU_ST_FN uint32_t round_step(uint32_t sig, uint32_t round_sum) {
  return acc_hash_step(sig, (int)round_sum);
}

// ---------------------------------------------------------------- host only

inline uint64_t load_cell(const uint32_t* cells, int w, bool wide) {
  return wide ? u64_of(cells[w], cells[w + 1]) : cells[w];
}
inline void store_cell(uint32_t* cells, int w, bool wide, uint64_t v) {
  cells[w] = (uint32_t)v;
  if (wide) cells[w + 1] = (uint32_t)(v >> 32);
}
inline double f64_from(uint64_t b) {
  double v;
  memcpy(&v, &b, 8);
  return v;
}
// a + b in a 16- or 32-bit format, through double and the conversion sweep's
// round-to-nearest-even encoder (exact here, see the top)
inline uint32_t fp_add(int wfmt, uint32_t a, uint32_t b) {
  return egpu_cv::encode_rne(egpu_cv::wide(wfmt), egpu_cv::decode_wide(wfmt, a) + egpu_cv::decode_wide(wfmt, b));
}
inline uint32_t pk_add(int wfmt, uint32_t a, uint32_t b) {
  return fp_add(wfmt, a & 0xffffu, b & 0xffffu) | (fp_add(wfmt, a >> 16, b >> 16) << 16);
}

// THE REFERENCE: one atomic on its cell. Returns what a returning op returns
// (the value before), 0 for the others.
//   inc   new = old >= limit ? 0 : old + 1
//   dec   new = (old == 0 || old > limit) ? limit : old - 1
//   cas   new = old == compare ? operand : old
inline uint64_t apply(const op_t& o, uint32_t* cells) {
  const bool wide = is64(o.op);
  const uint64_t old = load_cell(cells, o.cell, wide), a = o.a;
  uint64_t v = old;
  switch (o.op) {
    case OP_ADD32: case OP_ADD64: case OP_ADDR32: case OP_ADDR64: v = old + a; break;
    case OP_AND: v = old & a; break;
    case OP_OR: v = old | a; break;
    case OP_XOR: v = old ^ a; break;
    case OP_MINI: v = (int32_t)a < (int32_t)old ? a : old; break;
    case OP_MAXI: v = (int32_t)a > (int32_t)old ? a : old; break;
    case OP_MINU: v = (uint32_t)a < (uint32_t)old ? a : old; break;
    case OP_MAXU: v = (uint32_t)a > (uint32_t)old ? a : old; break;
    case OP_FADD32: v = fp_add(egpu_cv::W_F32, (uint32_t)old, (uint32_t)a); break;
    case OP_PKF16: v = pk_add(egpu_cv::W_F16, (uint32_t)old, (uint32_t)a); break;
    case OP_PKBF16: v = pk_add(egpu_cv::W_BF16, (uint32_t)old, (uint32_t)a); break;
    case OP_FADD64: v = f64_of(f64_from(old) + f64_from(a)); break;
    case OP_FMIN64: v = f64_from(a) < f64_from(old) ? a : old; break;
    case OP_FMAX64: v = f64_from(a) > f64_from(old) ? a : old; break;
    case OP_INC: v = (uint32_t)old >= (uint32_t)a ? 0u : (uint32_t)old + 1u; break;
    case OP_DEC: v = ((uint32_t)old == 0u || (uint32_t)old > (uint32_t)a) ? (uint32_t)a : (uint32_t)old - 1u; break;
    case OP_SWAP: v = a; break;
    case OP_CAS32: case OP_CAS64: case OP_CLAIM: v = old == o.b ? a : old; break;
    default: return 0;
  }
  store_cell(cells, o.cell, wide, v);
  return returns(o.op) ? old : 0;
}

inline bool kind_ok(int kind) { return kind >= 0 && kind < EGPU_AT_NKINDS; }
inline bool rounds_ok(int rounds) { return rounds >= 1 && rounds <= EGPU_AT_MAX_ROUNDS; }
inline bool grid_work_ok(long long blocks, long long rounds) {
  return blocks * rounds <= EGPU_AT_GRID_MAX_WORK;
}

// One workgroup, one kind, one round, lanes in order 0..255.
struct workgroup {
  uint32_t init[EGPU_AT_WORDS], fin[EGPU_AT_WORDS];
  op_t ops[EGPU_AT_LANES][EGPU_AT_NSLOT];
  uint64_t ret[EGPU_AT_LANES][EGPU_AT_NSLOT];
};
inline void replay(int kind, uint32_t seed, int group, int round, workgroup* wg) {
  for (int w = 0; w < EGPU_AT_WORDS; ++w) wg->fin[w] = wg->init[w] = init_word(kind, seed, group, round, w);
  for (int tid = 0; tid < EGPU_AT_LANES; ++tid)
    for (int s = 0; s < EGPU_AT_NSLOT; ++s) {
      wg->ops[tid][s] = gen_op(kind, s, seed, group, round, tid);
      wg->ret[tid][s] = apply(wg->ops[tid][s], wg->fin);
    }
}
// the round sum of one wave: its lanes' terms plus every final word
inline uint32_t wave_round_sum(int kind, const workgroup& wg, int wave) {
  uint32_t sum = 0;
  for (int w = 0; w < EGPU_AT_WORDS; ++w) sum += final_term(kind, w, wg.fin[w]);
  for (int tid = 64 * wave; tid < 64 * wave + 64; ++tid)
    for (int s = 0; s < EGPU_AT_NSLOT; ++s)
      sum += lane_term(wg.ops[tid][s], tid, wg.ret[tid][s], wg.fin[wg.ops[tid][s].cell]);
  return sum;
}

// out[4 * group + wave][kind]; g_grid has no wave signature (0).
// Returns 0, or -1 when rounds is outside [1, EGPU_AT_MAX_ROUNDS].
inline int expected_all(uint32_t seed, int rounds, uint32_t out[EGPU_AT_PATTERNS][EGPU_AT_NKINDS]) {
  if (!rounds_ok(rounds)) return -1;
  workgroup* wg = new workgroup;
  for (int group = 0; group < EGPU_AT_GROUPS; ++group)
    for (int kind = 0; kind < EGPU_AT_NKINDS; ++kind) {
      uint32_t sig[4] = {0, 0, 0, 0};
      for (int r = 0; r < rounds && kind != K_G_GRID; ++r) {
        replay(kind, seed, group, r, wg);
        for (int wave = 0; wave < 4; ++wave) sig[wave] = round_step(sig[wave], wave_round_sum(kind, *wg, wave));
      }
      for (int wave = 0; wave < 4; ++wave) out[4 * group + wave][kind] = sig[wave];
    }
  delete wg;
  return 0;
}

// The closed form of the grid slice after `blocks` workgroups ran `rounds`
// rounds: what one workgroup of each group contributes to a zero cell, times
// how many workgroups of that group (workgroup % 4) the grid has. add: the sum;
// xor: the contribution if the count is odd; umax: the largest of the groups
// present; f64 add: the sum, exact within grid_work_ok. Returns 0 or -1.
inline int grid_expected(uint32_t seed, int blocks, int rounds, uint32_t out[EGPU_AT_WORDS]) {
  if (blocks < 1 || !rounds_ok(rounds) || !grid_work_ok(blocks, rounds)) return -1;
  for (int w = 0; w < EGPU_AT_WORDS; ++w) out[w] = 0;
  workgroup* wg = new workgroup;
  for (int group = 0; group < EGPU_AT_GROUPS && group < blocks; ++group) {
    const uint64_t count = (uint64_t)(blocks - group + 3) / 4;
    for (int r = 0; r < rounds; ++r) {
      replay(K_G_GRID, seed, group, r, wg);
      for (int s = 0; s < EGPU_AT_NSLOT; ++s) {
        const int op = slot_of(K_G_GRID, s).op;
        const bool wide = is64(op);
        for (int w = EGPU_AT_SLOT_WORDS * s; op != OP_NONE && w < EGPU_AT_SLOT_WORDS * (s + 1); w += wide ? 2 : 1) {
          const uint64_t c = load_cell(wg->fin, w, wide), have = load_cell(out, w, wide);
          const uint64_t v = op == OP_XOR ? have ^ ((count & 1) ? c : 0)
                           : op == OP_MAXU ? ((uint32_t)c > (uint32_t)have ? c : have)
                           : op == OP_FADD64 ? f64_of(f64_from(have) + (double)count * f64_from(c))
                                             : have + count * c;
          store_cell(out, w, wide, v);
        }
      }
    }
  }
  delete wg;
  return 0;
}

}  // namespace egpu_at
