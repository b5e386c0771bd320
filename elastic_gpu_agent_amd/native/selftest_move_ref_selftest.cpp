// Stand-alone check of selftest_move_ref.h, the host reference of the move
// sweep, meant to be built with -fsanitize=address,undefined and run directly
// (libegpu_kernels.so itself is never run under a sanitizer).
//
// Checks: every lane map is a bijection of the source region it claims and
// every index, source bit and global offset is in range; the per-round lane
// permutation and the swizzle are bijections; move_tile only permutes bits;
// flipping any single source bit of the region changes the fold; rounds 2k and
// 2k+1 are complements; expected_all at rounds 1 and EGPU_MOVE_MAX_ROUNDS into
// exact-size heap blocks.
//
// Build + run: python -m elastic_gpu_agent_amd.native.build_fuzz --selftest
#include <cstdint>
#include <cstdio>
#include <set>
#include <vector>

#include "selftest_move_ref.h"

namespace {

namespace mv = egpu_mv;

int failures = 0;

#define CHECK(cond, what)                                                       \
  do {                                                                          \
    if (!(cond)) {                                                              \
      fprintf(stderr, "FAIL %s:%d %s (%s)\n", __FILE__, __LINE__, #cond, what); \
      ++failures;                                                               \
    }                                                                           \
  } while (0)

void test_maps_are_bijections() {
  for (int kind = 0; kind < EGPU_MOVE_NKINDS; ++kind) {
    const mv::geometry g = mv::geometry_of(kind);
    CHECK(g.elems <= EGPU_MOVE_MAX_ELEMS && g.elems * g.bits <= 128, "a lane holds four registers");
    CHECK(64 * g.elems == g.region, "as many received elements as source elements");
    for (int round : {0, 1, 7, EGPU_MOVE_MAX_ROUNDS - 1}) {
      std::vector<int> hit(g.region, 0);
      for (int lane = 0; lane < 64; ++lane)
        for (int j = 0; j < g.elems; ++j) {
          const int idx = mv::map_index(kind, round, lane, j);
          CHECK(idx >= 0 && idx < g.region, "index inside the region");
          if (idx >= 0 && idx < g.region) hit[idx]++;
          const int bit = mv::source_bit(kind, idx);
          CHECK(bit >= 0 && bit + g.bits <= 32 * EGPU_MOVE_TILE_WORDS, "source bits inside the tile");
        }
      for (int h : hit) CHECK(h == 1, "every source element received exactly once");
    }
  }
  for (int reg = 2; reg < 4; ++reg)
    for (int lane = 0; lane < 64; ++lane) {
      const int from = mv::dpp_bcast_lane(reg, lane);
      CHECK(from >= 0 && from < 64, "broadcast source is a lane");
    }
}

void test_lane_helpers() {
  for (int round = 0; round < EGPU_MOVE_MAX_ROUNDS; ++round) {
    std::set<int> seen;
    for (int lane = 0; lane < 64; ++lane) {
      const int to = mv::lane_perm(round, lane);
      CHECK(to >= 0 && to < 64, "lane_perm in range");
      seen.insert(to);
      CHECK(mv::lane_perm(round, mv::lane_perm_inverse(round, lane)) == lane, "inverse");
    }
    CHECK(seen.size() == 64, "lane_perm is a bijection");
  }
  CHECK(mv::lane_perm(0, 1) != mv::lane_perm(1, 1), "the permutation changes with the round");
  std::set<int> slots, rd16, rd4;
  for (int lane = 0; lane < 64; ++lane) {
    slots.insert(mv::b128_swizzle(lane));
    CHECK(mv::b128_swizzle(mv::b128_swizzle(lane)) == lane, "swizzle is an involution");
    rd16.insert(mv::g2l_read_slot(mv::K_G2L16, lane));
    rd4.insert(mv::g2l_read_slot(mv::K_G2L4, lane));
  }
  CHECK(slots.size() == 64 && rd16.size() == 64 && rd4.size() == 64, "slot maps are bijections");
  CHECK(*slots.begin() == 0 && *slots.rbegin() == 63, "slots in range");
  std::set<uint32_t> weights;
  for (int lane = 0; lane < 64; ++lane)
    for (int t = 0; t < EGPU_MOVE_TILES; ++t)
      for (int reg = 0; reg < 4; ++reg) {
        const uint32_t w = mv::reg_weight(lane, t, reg);
        CHECK(w & 1u, "weights are odd");
        weights.insert(w);
      }
  CHECK(weights.size() == 64 * 16, "weights are distinct");
}

void test_generator() {
  for (uint32_t seed : {0u, 0x5eed1234u, 0xffffffffu})
    for (int p = 0; p < EGPU_MOVE_PATTERNS; ++p)
      for (int kind : {(int)mv::K_G2L16, (int)mv::K_G2L4})
        for (int round = 0; round < EGPU_MOVE_MAX_ROUNDS; ++round) {
          const uint32_t off = mv::g2l_offset(seed, p, kind, round);
          CHECK(off % 4 == 0, "16-byte aligned");
          CHECK(off + EGPU_MOVE_SLAB_WORDS <= EGPU_MOVE_SRC_WORDS, "slab inside the source buffer");
          CHECK((off >= EGPU_MOVE_SRC_HALF) == ((round & 1) != 0), "odd rounds read the complement half");
        }
  for (int kind = 0; kind < EGPU_MOVE_NKINDS; ++kind)
    for (uint32_t w : {0u, 1u, 255u, 256u, 1023u})
      CHECK(mv::slab_word(9, 3, kind, 6, w) == ~mv::slab_word(9, 3, kind, 7, w),
            "rounds 2k and 2k+1 are complements");
  for (int p = 0; p < EGPU_MOVE_PATTERNS; ++p) {
    const int sp = mv::source_pattern(mv::K_TR8, p);
    CHECK(sp != p && (sp >> 2) == (p >> 2), "the neighbour wave of the same workgroup");
    CHECK(mv::source_pattern(mv::K_DPP, p) == p, "lane kinds use their own pattern");
  }
}

uint32_t fold(const uint32_t regs[256]) {
  uint32_t sum = 0;
  for (int lane = 0; lane < 64; ++lane)
    for (int reg = 0; reg < 4; ++reg) sum += regs[4 * lane + reg] * mv::reg_weight(lane, 1, reg);
  return sum;
}

int popcount_all(const uint32_t* w, int n) {
  int c = 0;
  for (int i = 0; i < n; ++i) c += (int)egpu_st::popc32(w[i]);
  return c;
}

// Every source bit the map claims reaches exactly one register bit, and
// flipping it changes the fold.
void test_single_bit_flips() {
  for (int kind = 0; kind < EGPU_MOVE_NKINDS; ++kind) {
    const mv::geometry g = mv::geometry_of(kind);
    std::vector<uint32_t> tile(EGPU_MOVE_TILE_WORDS), regs(256), flipped(256);
    for (int w = 0; w < EGPU_MOVE_TILE_WORDS; ++w) tile[w] = mv::slab_word(1, 2, kind, 0, (uint32_t)w);
    mv::move_tile(kind, 0, tile.data(), regs.data());
    const uint32_t base = fold(regs.data());
    for (int idx = 0; idx < g.region; ++idx)
      for (int b = 0; b < g.bits; ++b) {
        const int bit = mv::source_bit(kind, idx) + b;
        tile[bit >> 5] ^= 1u << (bit & 31);
        mv::move_tile(kind, 0, tile.data(), flipped.data());
        tile[bit >> 5] ^= 1u << (bit & 31);
        int changed = 0;
        for (int i = 0; i < 256; ++i) changed += (int)egpu_st::popc32(regs[i] ^ flipped[i]);
        CHECK(changed == 1, "one source bit, one register bit");
        CHECK(fold(flipped.data()) != base, "a single bit flip changes the fold");
      }
    if (kind != mv::K_DPP && kind != mv::K_TR6)  // these two do not move all 8192 bits one to one
      CHECK(popcount_all(regs.data(), 256) == popcount_all(tile.data(), EGPU_MOVE_TILE_WORDS),
            "a move only permutes bits");
  }
}

// exact-size heap block, so ASan traps a write one word past the records
std::vector<uint32_t> expected(uint32_t seed, int rounds, int* rc) {
  std::vector<uint32_t> out(EGPU_MOVE_PATTERNS * EGPU_MOVE_NKINDS, 0xdeadbeefu);
  *rc = mv::expected_all(seed, rounds, out.data());
  return out;
}

void test_expected_all() {
  int rc1, rc2;
  const auto a = expected(42, 2, &rc1), b = expected(42, 2, &rc2);
  CHECK(rc1 == 0 && rc2 == 0, "valid arguments");
  CHECK(a == b, "same inputs, same records");
  const auto other = expected(43, 2, &rc1), more = expected(42, 3, &rc2);
  for (int i = 0; i < EGPU_MOVE_PATTERNS * EGPU_MOVE_NKINDS; ++i) {
    CHECK(a[i] != other[i], "the seed matters, also after a complement pair");
    CHECK(a[i] != more[i], "the round count matters");
  }
  for (int kind = 0; kind < EGPU_MOVE_NKINDS; ++kind) {
    std::set<uint32_t> sigs;
    for (int p = 0; p < EGPU_MOVE_PATTERNS; ++p) sigs.insert(a[EGPU_MOVE_NKINDS * p + kind]);
    CHECK(sigs.size() == EGPU_MOVE_PATTERNS, "16 distinct signatures per kind");
  }
  const auto top = expected(42, EGPU_MOVE_MAX_ROUNDS, &rc1);
  CHECK(rc1 == 0 && top != a, "the largest round count");
  for (uint32_t v : top) CHECK(v != 0xdeadbeefu, "every record written");
  const auto lo = expected(0, 0, &rc1);
  CHECK(rc1 != 0 && lo[0] == 0xdeadbeefu, "rounds 0 rejected, nothing written");
  expected(0, -1, &rc1);
  CHECK(rc1 != 0, "negative rounds rejected");
  expected(0, EGPU_MOVE_MAX_ROUNDS + 1, &rc1);
  CHECK(rc1 != 0, "rounds over the bound rejected");
}

}  // namespace

int main() {
  test_maps_are_bijections();
  test_lane_helpers();
  test_generator();
  test_single_bit_flips();
  test_expected_all();
  if (failures) {
    fprintf(stderr, "selftest_move_ref: %d check(s) failed\n", failures);
    return 1;
  }
  printf("selftest_move_ref: all checks passed\n");
  return 0;
}
