// Stand-alone check of selftest_ref.h, the host reference of the GPU
// self-test, meant to be built with -fsanitize=address,undefined and run
// directly (libegpu_kernels.so itself is never run under a sanitizer).
//
// Checks: determinism, the bound on `rounds`, that the 64 patterns give 64
// distinct records, the exactness bound of the MFMA accumulator, and a few
// literal signatures (the FMA literals are what std::fmaf gives: this file is
// compiled without any GPU toolchain in the way).
//
// Build + run: python -m elastic_gpu_agent_amd.native.build_fuzz --selftest
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <tuple>
#include <vector>

#include "selftest_ref.h"

namespace {

int failures = 0;

#define CHECK(cond, what)                                                       \
  do {                                                                          \
    if (!(cond)) {                                                              \
      fprintf(stderr, "FAIL %s:%d %s (%s)\n", __FILE__, __LINE__, #cond, what); \
      ++failures;                                                               \
    }                                                                           \
  } while (0)

// exact-size heap block, so ASan traps a write one word past the 64 records
std::vector<uint32_t> expected(uint32_t seed, int rounds, int* rc) {
  std::vector<uint32_t> out(EGPU_SELFTEST_PATTERNS * 3, 0xdeadbeefu);
  *rc = egpu_st::expected_all(seed, rounds, out.data());
  return out;
}

void test_determinism() {
  int rc1, rc2;
  const auto a = expected(42, 7, &rc1), b = expected(42, 7, &rc2);
  CHECK(rc1 == 0 && rc2 == 0, "valid arguments");
  CHECK(a == b, "same inputs, same records");
  const auto c = expected(43, 7, &rc1);
  CHECK(a != c, "the seed matters");
  const auto d = expected(42, 8, &rc1);
  CHECK(a != d, "rounds matters");
}

void test_rounds_bound() {
  int rc;
  const auto lo = expected(0, 0, &rc);
  CHECK(rc != 0, "rounds 0 rejected");
  CHECK(lo[0] == 0xdeadbeefu, "nothing written on error");
  expected(0, -1, &rc);
  CHECK(rc != 0, "negative rounds rejected");
  expected(0, EGPU_SELFTEST_MAX_ROUNDS + 1, &rc);
  CHECK(rc != 0, "rounds over the bound rejected");
  // the bound keeps the f32 accumulator exact: |acc| <= 144 * rounds
  CHECK(144ll * EGPU_SELFTEST_MAX_ROUNDS < (1ll << 24), "accumulator below 2^24");
  // and the worst case is really what the generator can reach at most
  for (uint32_t w = 0; w < 1u << 24; w += 4099)
    for (int j = 0; j < 8; ++j) {
      const int e = egpu_st::mfma_elem(w, j);
      CHECK(e >= -3 && e <= 3, "operand in [-3, 3]");
    }
}

void test_accumulator_range() {
  // at the largest round count that is still cheap here, every |D| entry is
  // within the analytic bound
  const int rounds = 64;
  std::vector<int32_t> d(1024);
  for (int p : {0, 17, 63}) {
    egpu_st::mfma_tile(7, p, rounds, d.data());
    for (int32_t v : d) CHECK(v <= 144 * rounds && v >= -144 * rounds, "|acc| <= 144*rounds");
  }
}

void test_patterns_distinct() {
  for (int rounds : {1, 4}) {
    int rc;
    const auto e = expected(0, rounds, &rc);
    std::set<uint32_t> ints, fmas, mfmas;
    std::set<std::tuple<uint32_t, uint32_t, uint32_t>> recs;
    for (int p = 0; p < EGPU_SELFTEST_PATTERNS; ++p) {
      ints.insert(e[3 * p]);
      fmas.insert(e[3 * p + 1]);
      mfmas.insert(e[3 * p + 2]);
      recs.insert(std::make_tuple(e[3 * p], e[3 * p + 1], e[3 * p + 2]));
    }
    CHECK(recs.size() == 64, "64 distinct records");
    CHECK(ints.size() == 64 && fmas.size() == 64 && mfmas.size() == 64,
          "every signature distinct on its own");
  }
}

void test_lane_swap_changes_signature() {
  // the lane weights make the reduction order-sensitive: exchanging the
  // values of two lanes changes the sum
  uint32_t v[64];
  for (int l = 0; l < 64; ++l) v[l] = egpu_st::int_chain(egpu_st::lane_seed(1, 2, l, 0), 3);
  auto sum = [&]() {
    uint32_t s = 0;
    for (int l = 0; l < 64; ++l) s += v[l] * egpu_st::lane_weight(l);
    return s;
  };
  const uint32_t before = sum();
  for (int a = 0; a < 64; ++a)
    for (int b = a + 1; b < 64; ++b) {
      std::swap(v[a], v[b]);
      CHECK(sum() != before, "swap detected");
      std::swap(v[a], v[b]);
    }
}

void test_literals() {
  int rc;
  const auto e = expected(0, 4, &rc);
  CHECK(e[0] == 0x3ea752ffu && e[1] == 0x29c8a963u && e[2] == 0x63d636beu, "seed 0 pattern 0");
  CHECK(e[3] == 0x5d888a1cu && e[4] == 0x59a04b97u && e[5] == 0x58faf12bu, "seed 0 pattern 1");
  const auto f = expected(0x1234abcdu, 5, &rc);
  CHECK(f[189] == 0xbb87c225u && f[190] == 0x2dac9d18u && f[191] == 0x89bb1e15u,
        "seed 0x1234abcd rounds 5 pattern 63");
  // one FMA step by hand: x, a, b in [1,2), result mantissa kept
  const uint32_t one = egpu_st::fma_chain(0, 1);
  CHECK(one == 0x000e5920u, "single fmaf step");
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1) {  // --print: the values behind the literals above
    int rc;
    const auto f = expected(0x1234abcdu, 5, &rc);
    printf("0x%08xu 0x%08xu 0x%08xu 0x%08xu\n", f[189], f[190], f[191],
           egpu_st::fma_chain(0, 1));
    return 0;
  }
  test_determinism();
  test_rounds_bound();
  test_accumulator_range();
  test_patterns_distinct();
  test_lane_swap_changes_signature();
  test_literals();
  if (failures) {
    fprintf(stderr, "selftest_ref: %d check(s) failed\n", failures);
    return 1;
  }
  printf("selftest_ref: all checks passed\n");
  return 0;
}
