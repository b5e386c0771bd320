// selftest_move_ref.h — host reference of the move sweep
// (egpu_selftest_move.hip).
//
// Host-only: plain C++17, no HIP call, no GPU type. The sweep moves data
// through the gfx950 data-movement paths (direct global-to-LDS loads, 128-bit
// LDS accesses, the transposing LDS reads, ds_bpermute / ds_permute, the
// permlane swaps and DPP) and folds what every lane received into one
// signature per kind. Data movement only permutes bits, so the reference is a
// generated source, a lane map per kind, and the fold.
//
// Shared with the kernel (EGPU_ST_FN): the generator, the per-round lane
// bijection and the fold. The LANE MAPS live here only: the device executes the
// instruction, the host says which source element every (lane, element) must
// have received. Every map below is what an MI355X showed (docs/HEALTH.md).
//
// A wave works in units of one TILE = 256 words = 64 lanes x 4 registers, four
// tiles per round (one 4 KiB slab). Inputs are a pure function of
// (kind, pattern, seed, round), pattern in [0, 16).
#pragma once

#include <cstdint>

#include "selftest_ref.h"

// The host reference moves 16 patterns x 10 kinds x 1024 words per round
// (about 4 ms); the bound keeps a probe's reference at about a second.
#define EGPU_MOVE_MAX_ROUNDS 256
#define EGPU_MOVE_PATTERNS 16
#define EGPU_MOVE_NKINDS 10
#define EGPU_MOVE_TILE_WORDS 256
#define EGPU_MOVE_TILES 4
#define EGPU_MOVE_SLAB_WORDS (EGPU_MOVE_TILE_WORDS * EGPU_MOVE_TILES)
// Global source of the direct-to-LDS kinds: a pattern half and its complement.
#define EGPU_MOVE_SRC_HALF 4096
#define EGPU_MOVE_SRC_WORDS (2 * EGPU_MOVE_SRC_HALF)
#define EGPU_MOVE_MAX_ELEMS 32  // elements a lane receives per tile, at most

namespace egpu_mv {

using egpu_st::acc_hash_step;
using egpu_st::lane_seed;
using egpu_st::mix32;

enum { K_G2L16 = 0, K_G2L4, K_B128, K_TR16, K_TR8, K_TR6, K_TR4, K_BPERM, K_SWAP, K_DPP };

EGPU_ST_FN constexpr bool is_g2l(int kind) { return kind == K_G2L16 || kind == K_G2L4; }
EGPU_ST_FN constexpr bool is_lane_kind(int kind) { return kind >= K_BPERM; }

// ---- generator
// word i of the global source buffer: mix, then the complement of the same
EGPU_ST_FN uint32_t src_word(uint32_t seed, uint32_t i) {
  const uint32_t g = mix32(seed * 0x9e3779b9u + (i & (EGPU_MOVE_SRC_HALF - 1)));
  return i < EGPU_MOVE_SRC_HALF ? g : ~g;
}

EGPU_ST_FN uint32_t kind_base(uint32_t seed, int pattern, int kind) {
  return lane_seed(seed, pattern, 64, 16 + kind);
}

// Where a direct-to-LDS round reads the source buffer, in words: a multiple of
// 4 (16 bytes), in [0, HALF - SLAB] by the modulo, plus HALF in odd rounds. So
// offset + SLAB_WORDS <= SRC_WORDS whatever the arguments.
EGPU_ST_FN uint32_t g2l_offset(uint32_t seed, int pattern, int kind, int round) {
  const uint32_t slots = (EGPU_MOVE_SRC_HALF - EGPU_MOVE_SLAB_WORDS) / 4 + 1;
  const uint32_t off = 4u * (mix32(kind_base(seed, pattern, kind) + (uint32_t)(round >> 1)) % slots);
  return off + ((round & 1) ? EGPU_MOVE_SRC_HALF : 0);
}

// Word w (0..1023) of the source slab of a round. Rounds 2k and 2k+1 are
// complements of each other, so every bit position that is moved sees both
// polarities in every pair of rounds.
EGPU_ST_FN uint32_t slab_word(uint32_t seed, int pattern, int kind, int round, uint32_t w) {
  if (is_g2l(kind)) return src_word(seed, g2l_offset(seed, pattern, kind, round) + w);
  const uint32_t g =
      mix32(kind_base(seed, pattern, kind) + (uint32_t)(round >> 1) * EGPU_MOVE_SLAB_WORDS + w);
  return (round & 1) ? ~g : g;
}

// The pattern of the wave whose slab a wave reads: wave (w + 1) & 3 of the same
// workgroup. Lane kinds move the wave's own registers.
EGPU_ST_FN constexpr int source_pattern(int kind, int pattern) {
  return is_lane_kind(kind) ? pattern : ((pattern & ~3) | ((pattern + 1) & 3));
}

// ---- per-round bijection of the 64 lanes: lane * odd + c mod 64
EGPU_ST_FN constexpr int lane_perm(int round, int lane) {
  return (lane * ((10 * round + 5) & 63) + ((17 * round + 3) & 63)) & 63;
}

// 16-byte slot a lane writes in the b128 kind (an involution of 0..63)
EGPU_ST_FN constexpr int b128_swizzle(int lane) { return lane ^ ((lane >> 3) & 7); }
// 16-byte slot a lane reads back after a direct-to-LDS load
EGPU_ST_FN constexpr int g2l_read_slot(int kind, int lane) {
  return kind == K_G2L16 ? 63 - lane : (lane + 32) & 63;
}

// ---- fold: distinct odd weights per (lane, tile, register), summed over the
// wave, then chained over the rounds
EGPU_ST_FN uint32_t reg_weight(int lane, int tile, int reg) {
  return (2u * (uint32_t)(lane * 16 + tile * 4 + reg) + 1u) * 0x01000193u;
}
EGPU_ST_FN uint32_t round_step(uint32_t sig, uint32_t round_sum) {
  return acc_hash_step(sig, (int)round_sum);
}

// ---------------------------------------------------------------- host only
// Geometry of a kind's map: element width in bits, elements a lane receives per
// tile through the map (ELEMS), and the number of source elements the map
// covers bijectively (REGION). Elements are packed little-endian in the lane's
// registers (element j at bit j * BITS) and in the tile, except tr6's source:
// element k of its 1024 is column k & 15 (6 bits at bit 6 * column) of the
// 16-byte row k >> 4, whose upper 32 bits are not read.
struct geometry {
  int bits, elems, region;
};
inline geometry geometry_of(int kind) {
  switch (kind) {
    case K_TR16: return {16, 8, 512};
    case K_TR8: return {8, 16, 1024};
    case K_TR6: return {6, 16, 1024};
    case K_TR4: return {4, 32, 2048};
    case K_DPP: return {32, 2, 128};  // registers 2 and 3 are broadcasts: dpp_bcast_lane
    default: return {32, 4, 256};
  }
}

inline int lane_perm_inverse(int round, int lane) {
  for (int l = 0; l < 64; ++l)
    if (lane_perm(round, l) == lane) return l;
  return -1;
}

// Source element index of element j of lane `lane` (block b = lane >> 4 of 16
// lanes, i = lane & 15). Lane kinds number their source register * 64 + lane.
//   g2l16, g2l4  word 4 * read_slot(lane) + j (the load itself is linear: the
//                hardware puts the lane's SIZE bytes at base + offset + lane * SIZE)
//   b128         word 4 * swizzle(lane) + j
//   tr16/8/4     two ds_read_b64_tr per tile, h = j / E (E = 64 / BITS elements
//                per read), e = j % E: element 64*E*h + 16*E*b + 16*e + i. The
//                16 lanes' 128 bytes are an E x 16 matrix and lane i receives
//                its column i.
//   tr6          one ds_read_b96_tr_b6: element 16 * (16*b + j) + i. Rows must be
//                16-byte aligned; lane i receives column i of its block's 16 rows.
//   bperm        registers 0, 1 ds_bpermute: lane_perm(lane); 2, 3 ds_permute:
//                the inverse.
//   swap         v_permlane16_swap (vdst = s0, src = s1): odd rows of vdst trade
//                with even rows of src; v_permlane32_swap (s2, s3): the upper
//                half of vdst trades with the lower half of src.
//   dpp          0: row_mirror of quad_perm:[1,2,3,0]; 1: row_half_mirror of
//                row_ror:3.
inline int map_index(int kind, int round, int lane, int j) {
  const int b = lane >> 4, i = lane & 15, row = lane >> 4;
  switch (kind) {
    case K_G2L16:
    case K_G2L4: return 4 * g2l_read_slot(kind, lane) + j;
    case K_B128: return 4 * b128_swizzle(lane) + j;
    case K_TR16:
    case K_TR8:
    case K_TR4: {
      const int e_per = 64 / geometry_of(kind).bits;
      return 64 * e_per * (j / e_per) + 16 * e_per * b + 16 * (j % e_per) + i;
    }
    case K_TR6: return 16 * (16 * b + j) + i;
    case K_BPERM:
      return 64 * j + (j < 2 ? lane_perm(round, lane) : lane_perm_inverse(round, lane));
    case K_SWAP:
      switch (j) {
        case 0: return (row & 1) ? 64 + lane - 16 : lane;
        case 1: return (row & 1) ? 64 + lane : lane + 16;
        case 2: return lane < 32 ? 128 + lane : 192 + lane - 32;
        default: return lane < 32 ? 128 + lane + 32 : 192 + lane;
      }
    default: {  // K_DPP
      if (j == 0) {
        const int m = lane ^ 15;
        return (m & ~3) | ((m + 1) & 3);
      }
      const int m = lane ^ 7;
      return 64 + ((m & ~15) | ((m - 3) & 15));
    }
  }
}

// dpp registers 2 (row_bcast:15) and 3 (row_bcast:31), full row and bank masks:
// the lane whose value lane `lane` receives. A lane with no source keeps its own.
inline int dpp_bcast_lane(int reg, int lane) {
  if (reg == 2) return lane < 16 ? lane : 16 * (lane >> 4) - 1;
  return lane < 32 ? lane : 31;
}

inline uint32_t tile_bits(const uint32_t tile[EGPU_MOVE_TILE_WORDS], int bit, int n) {
  uint64_t v = tile[bit >> 5];
  if ((bit >> 5) + 1 < EGPU_MOVE_TILE_WORDS) v |= (uint64_t)tile[(bit >> 5) + 1] << 32;
  return (uint32_t)(v >> (bit & 31)) & (n == 32 ? 0xffffffffu : (1u << n) - 1u);
}

inline int source_bit(int kind, int index) {
  return kind == K_TR6 ? 128 * (index >> 4) + 6 * (index & 15) : index * geometry_of(kind).bits;
}

// The four registers every lane receives from one tile: regs[4 * lane + reg].
inline void move_tile(int kind, int round, const uint32_t tile[EGPU_MOVE_TILE_WORDS],
                      uint32_t regs[256]) {
  const geometry g = geometry_of(kind);
  for (int i = 0; i < 256; ++i) regs[i] = 0;
  for (int lane = 0; lane < 64; ++lane) {
    for (int j = 0; j < g.elems; ++j) {
      const uint32_t v = tile_bits(tile, source_bit(kind, map_index(kind, round, lane, j)), g.bits);
      const int off = j * g.bits;
      regs[4 * lane + (off >> 5)] |= v << (off & 31);
      if ((off & 31) + g.bits > 32) regs[4 * lane + (off >> 5) + 1] |= v >> (32 - (off & 31));
    }
    if (kind == K_DPP)
      for (int reg = 2; reg < 4; ++reg) regs[4 * lane + reg] = tile[64 * reg + dpp_bcast_lane(reg, lane)];
  }
}

inline uint32_t expected_sig(uint32_t seed, int pattern, int kind, int rounds) {
  const int sp = source_pattern(kind, pattern);
  uint32_t tile[EGPU_MOVE_TILE_WORDS], regs[256], sig = 0;
  for (int r = 0; r < rounds; ++r) {
    uint32_t sum = 0;
    for (int t = 0; t < EGPU_MOVE_TILES; ++t) {
      for (int w = 0; w < EGPU_MOVE_TILE_WORDS; ++w)
        tile[w] = slab_word(seed, sp, kind, r, (uint32_t)(t * EGPU_MOVE_TILE_WORDS + w));
      move_tile(kind, r, tile, regs);
      for (int lane = 0; lane < 64; ++lane)
        for (int reg = 0; reg < 4; ++reg) sum += regs[4 * lane + reg] * reg_weight(lane, t, reg);
    }
    sig = round_step(sig, sum);
  }
  return sig;
}

inline bool rounds_ok(int rounds) { return rounds >= 1 && rounds <= EGPU_MOVE_MAX_ROUNDS; }
inline bool kind_ok(int kind) { return kind >= 0 && kind < EGPU_MOVE_NKINDS; }

// out[NKINDS * p + kind] = signature of `kind` for pattern p.
// Returns 0, or -1 when rounds is outside [1, EGPU_MOVE_MAX_ROUNDS].
inline int expected_all(uint32_t seed, int rounds,
                        uint32_t out[EGPU_MOVE_PATTERNS * EGPU_MOVE_NKINDS]) {
  if (!rounds_ok(rounds)) return -1;
  for (int p = 0; p < EGPU_MOVE_PATTERNS; ++p)
    for (int kind = 0; kind < EGPU_MOVE_NKINDS; ++kind)
      out[EGPU_MOVE_NKINDS * p + kind] = expected_sig(seed, p, kind, rounds);
  return 0;
}

}  // namespace egpu_mv
