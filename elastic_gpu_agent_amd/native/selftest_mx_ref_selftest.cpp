// Stand-alone check of selftest_mx_ref.h, the host reference of the matrix
// sweep, meant to be built with -fsanitize=address,undefined and run directly
// (libegpu_kernels.so itself is never run under a sanitizer).
//
// Checks: the decoders over every code of every format against values worked
// out here from the format definitions; that every element the generator
// emits decodes to the table entry its code names (so never a NaN or an
// infinity) and that no scale byte is 0xFF; packing and unpacking of
// fragments; the exactness bound; expected_all at rounds 1 and
// EGPU_MX_MAX_ROUNDS into exact-size heap blocks; and literal signatures.
//
// Build + run: python -m elastic_gpu_agent_amd.native.build_fuzz --selftest
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "selftest_mx_ref.h"

namespace {

namespace mx = egpu_mx;

int failures = 0;

#define CHECK(cond, what)                                                       \
  do {                                                                          \
    if (!(cond)) {                                                              \
      fprintf(stderr, "FAIL %s:%d %s (%s)\n", __FILE__, __LINE__, #cond, what); \
      ++failures;                                                               \
    }                                                                           \
  } while (0)

const double TABLE[8] = {0, 0.5, -1, 1.5, 2, -3, 4, -6};

// value of a sign / exponent / mantissa code, by the textbook formula
double by_formula(uint32_t code, int ebits, int mbits) {
  const int bias = (1 << (ebits - 1)) - 1;
  const int e = (int)((code >> mbits) & ((1u << ebits) - 1u));
  const double m = (double)(code & ((1u << mbits) - 1u)) / (double)(1u << mbits);
  const double v = e == 0 ? std::pow(2.0, 1 - bias) * m : std::pow(2.0, e - bias) * (1.0 + m);
  return (code >> (ebits + mbits)) & 1u ? -v : v;
}

void test_decoders_every_code() {
  // e2m1: the sixteen values of the OCP MX specification
  const double fp4[16] = {0, 0.5, 1, 1.5, 2, 3, 4, 6, -0.0, -0.5, -1, -1.5, -2, -3, -4, -6};
  for (uint32_t c = 0; c < 16; ++c) CHECK(mx::decode_e2m1(c) == fp4[c], "e2m1");
  // e2m3: no special codes; largest magnitude 7.5, smallest subnormal 0.125
  for (uint32_t c = 0; c < 64; ++c) CHECK(mx::decode_e2m3(c) == by_formula(c, 2, 3), "e2m3");
  CHECK(mx::decode_e2m3(0x1f) == 7.5 && mx::decode_e2m3(0x01) == 0.125, "e2m3 range");
  // e4m3fn: 0x7f and 0xff are NaN, everything else a number up to 448
  for (uint32_t c = 0; c < 256; ++c) {
    const double v = mx::decode_e4m3fn(c);
    if ((c & 0x7f) == 0x7f)
      CHECK(std::isnan(v), "e4m3fn NaN");
    else
      CHECK(v == by_formula(c, 4, 3), "e4m3fn");
  }
  CHECK(mx::decode_e4m3fn(0x7e) == 448.0 && mx::decode_e4m3fn(0x01) == std::ldexp(1.0, -9),
        "e4m3fn range");
  // e5m2: IEEE-like, exponent 31 is infinity (mantissa 0) or NaN
  for (uint32_t c = 0; c < 256; ++c) {
    const double v = mx::decode_e5m2(c);
    if (((c >> 2) & 31) == 31) {
      if (c & 3)
        CHECK(std::isnan(v), "e5m2 NaN");
      else
        CHECK(std::isinf(v) && (v < 0) == (c >= 128), "e5m2 infinity");
    } else {
      CHECK(v == by_formula(c, 5, 2), "e5m2");
    }
  }
  CHECK(mx::decode_e5m2(0x7b) == 57344.0, "e5m2 range");
  // e8m0: 2^(e - 127), 0xff is NaN
  for (uint32_t c = 0; c < 255; ++c)
    CHECK(mx::decode_e8m0(c) == std::ldexp(1.0, (int)c - 127), "e8m0");
  CHECK(std::isnan(mx::decode_e8m0(0xff)), "e8m0 NaN");
  // f16 and bf16: every code against the formula, specials apart
  for (uint32_t c = 0; c < 65536; ++c) {
    if (((c >> 10) & 31) != 31) CHECK(mx::decode_f16(c) == by_formula(c, 5, 10), "f16");
    if (((c >> 7) & 255) != 255) CHECK(mx::decode_bf16(c) == by_formula(c, 8, 7), "bf16");
  }
  CHECK(std::isinf(mx::decode_f16(0x7c00)) && std::isnan(mx::decode_f16(0x7e00)), "f16 specials");
  CHECK(std::isinf(mx::decode_bf16(0xff80)) && std::isnan(mx::decode_bf16(0x7fc0)),
        "bf16 specials");
  for (uint32_t c = 0; c < 256; ++c) CHECK(mx::decode(mx::F_I8, c) == (double)(int8_t)c, "i8");
}

void test_encode_tables() {
  const int fmts[7] = {mx::F_F16, mx::F_BF16, mx::F_I8, mx::F_E4M3, mx::F_E5M2, mx::F_E2M3,
                       mx::F_E2M1};
  for (int fmt : fmts)
    for (uint32_t c = 0; c < 8; ++c) {
      const uint32_t bits = mx::encode(fmt, c);
      CHECK(bits >> mx::fmt_bits(fmt) == 0, "encoding fits its width");
      const double want = fmt == mx::F_I8 ? 2 * TABLE[c] : TABLE[c];
      CHECK(mx::decode(fmt, bits) == want, "encoding decodes to the table entry");
      CHECK(mx::elem_x4(fmt, c) == (int)(4 * want), "elem_x4");
    }
}

template <int KIND> void check_generator_kind(uint32_t seed) {
  using T = mx::traits<KIND>;
  std::set<double> seen;
  std::set<int> da, db, signs;
  for (int p = 0; p < EGPU_MX_PATTERNS; ++p)
    for (int round : {0, 1, 2, EGPU_MX_MAX_ROUNDS - 1}) {
      const int sr = mx::round_scale(seed, p, KIND, round);
      CHECK(sr >= -40 && sr <= 40, "S_r in [-40, 40]");
      signs.insert(sr < 0 ? -1 : sr > 0 ? 1 : 0);
      for (int l = 0; l < 64; ++l) {
        mx::lane_regs r;
        mx::lane_operands<KIND>(seed, p, l, round, &r);
        for (int j = 0; j < T::E; ++j) {
          const double a = mx::decode(T::FA, mx::extract(r.a, j, mx::fmt_bits(T::FA)));
          const double b = mx::decode(T::FB, mx::extract(r.b, j, mx::fmt_bits(T::FB)));
          CHECK(std::isfinite(a) && std::isfinite(b), "no NaN, no infinity");
          const double scale = KIND == mx::K_I8 ? 2.0 : 1.0;
          CHECK(a == scale * TABLE[mx::elem_code(r.wa, j)], "A element is its table entry");
          CHECK(b == scale * TABLE[mx::elem_code(r.wb, j)], "B element is its table entry");
          seen.insert(a);
        }
        // nothing above the last element
        for (int i = (T::E * mx::fmt_bits(T::FA) + 31) / 32; i < 8; ++i)
          CHECK(r.a[i] == 0, "unused A registers are zero");
        for (int i = (T::E * mx::fmt_bits(T::FB) + 31) / 32; i < 8; ++i)
          CHECK(r.b[i] == 0, "unused B registers are zero");
        if (!T::SCALED) {
          CHECK(r.sa == 0 && r.sb == 0, "no scales for an unscaled kind");
          continue;
        }
        std::set<uint32_t> bytes_a, bytes_b;
        for (int i = 0; i < 4; ++i) {
          bytes_a.insert((r.sa >> (8 * i)) & 0xff);
          bytes_b.insert((r.sb >> (8 * i)) & 0xff);
        }
        CHECK(!bytes_a.count(0xff) && !bytes_b.count(0xff), "no 0xFF scale code");
        CHECK(bytes_a.size() == 4 && bytes_b.size() == 4, "filler bytes differ from the live one");
        const int ea = (int)((r.sa >> (8 * mx::SCALE_BYTE_A)) & 0xff) - 127 - sr;
        const int eb = (int)((r.sb >> (8 * mx::SCALE_BYTE_B)) & 0xff) - 127 + sr;
        CHECK((ea == 0 || ea == 1) && (eb == 0 || eb == 1), "da, db in {0, 1}");
        da.insert(ea);
        db.insert(eb);
      }
    }
  CHECK(seen.size() == 8, "all eight table entries occur");
  if (T::SCALED) {
    CHECK(da.size() == 2 && db.size() == 2, "both da and db values occur");
    CHECK(signs.count(-1) && signs.count(1), "S_r takes both signs");
  }
}

struct generator_fn {
  template <int KIND> void operator()() { check_generator_kind<KIND>(0x5eed1234u); }
};

void test_generator() {
  for (int kind = 0; kind < EGPU_MX_NKINDS; ++kind) {
    generator_fn f;
    CHECK(mx::for_kind(kind, f), "known kind");
  }
  generator_fn f;
  CHECK(!mx::for_kind(EGPU_MX_NKINDS, f) && !mx::for_kind(-1, f), "unknown kind");
}

// the accumulator really stays within the analytic bound, and on whole hash units
template <int KIND> void check_range(int rounds, long long per_round) {
  using T = mx::traits<KIND>;
  std::vector<double> d(1024);
  for (int p : {0, 9, 15}) {
    mx::tile<KIND>(7, p, rounds, d.data(), nullptr);
    for (int i = 0; i < T::M * T::M; ++i) {
      const double u = KIND == mx::K_I8 ? d[i] : d[i] * 4.0;
      CHECK(u == std::floor(u), "whole number of hash units");
      CHECK(std::fabs(u) <= (double)(per_round * rounds), "|acc| within the bound");
    }
  }
}

void test_exactness_bound() {
  const long long worst[EGPU_MX_NKINDS] = {2304, 4608, 2304, 2304, 4608, 36864, 36864, 36864, 36864};
  for (long long w : worst) CHECK(w * EGPU_MX_MAX_ROUNDS < (1ll << 24), "below 2^24");
  check_range<mx::K_F16>(16, worst[mx::K_F16]);
  check_range<mx::K_I8>(16, worst[mx::K_I8]);
  check_range<mx::K_FP8>(16, worst[mx::K_FP8]);
  check_range<mx::K_BF8>(16, worst[mx::K_BF8]);
  check_range<mx::K_BF16S>(16, worst[mx::K_BF16S]);
  check_range<mx::K_MXFP8>(16, worst[mx::K_MXFP8]);
  check_range<mx::K_MXFP6>(16, worst[mx::K_MXFP6]);
  check_range<mx::K_MXFP4>(16, worst[mx::K_MXFP4]);
  check_range<mx::K_MXMIX>(16, worst[mx::K_MXMIX]);
}

// exact-size heap block, so ASan traps a write one word past the records
std::vector<uint32_t> expected(uint32_t seed, int rounds, int* rc) {
  std::vector<uint32_t> out(EGPU_MX_PATTERNS * EGPU_MX_NKINDS, 0xdeadbeefu);
  *rc = mx::expected_all(seed, rounds, out.data());
  return out;
}

void test_expected_all() {
  int rc1, rc2;
  const auto a = expected(42, 1, &rc1), b = expected(42, 1, &rc2);
  CHECK(rc1 == 0 && rc2 == 0, "valid arguments");
  CHECK(a == b, "same inputs, same records");
  CHECK(a != expected(43, 1, &rc1), "the seed matters");
  for (int kind = 0; kind < EGPU_MX_NKINDS; ++kind) {
    std::set<uint32_t> sigs;
    for (int p = 0; p < EGPU_MX_PATTERNS; ++p) sigs.insert(a[EGPU_MX_NKINDS * p + kind]);
    CHECK(sigs.size() == EGPU_MX_PATTERNS, "16 distinct signatures per kind");
  }
  const auto top = expected(42, EGPU_MX_MAX_ROUNDS, &rc1);
  CHECK(rc1 == 0 && top != a, "the largest round count");
  for (uint32_t v : top) CHECK(v != 0xdeadbeefu, "every record written");
  const auto lo = expected(0, 0, &rc1);
  CHECK(rc1 != 0 && lo[0] == 0xdeadbeefu, "rounds 0 rejected, nothing written");
  expected(0, -1, &rc1);
  CHECK(rc1 != 0, "negative rounds rejected");
  expected(0, EGPU_MX_MAX_ROUNDS + 1, &rc1);
  CHECK(rc1 != 0, "rounds over the bound rejected");
}

void test_literals() {
  int rc;
  const auto e = expected(0, 4, &rc);
  const uint32_t want0[EGPU_MX_NKINDS] = {0xd31ca4dcu, 0xd2b496c9u, 0xef4fdafcu, 0x914ff51cu,
                                          0x086ca5e4u, 0x50e52c95u, 0xac3fc9f3u, 0xdac9186eu,
                                          0x814d2eb4u};
  for (int k = 0; k < EGPU_MX_NKINDS; ++k) CHECK(e[k] == want0[k], "seed 0 rounds 4 pattern 0");
  const auto f = expected(0x1234abcdu, 5, &rc);
  const uint32_t want15[EGPU_MX_NKINDS] = {0x0c45d149u, 0x3d85514fu, 0xfb3fee4fu, 0xd5463610u,
                                           0xc05dc16cu, 0xa0653b19u, 0x2e8e4650u, 0xa7af8ca7u,
                                           0xa4a98714u};
  for (int k = 0; k < EGPU_MX_NKINDS; ++k)
    CHECK(f[EGPU_MX_NKINDS * 15 + k] == want15[k], "seed 0x1234abcd rounds 5 pattern 15");
}

}  // namespace

int main() {
  test_decoders_every_code();
  test_encode_tables();
  test_generator();
  test_exactness_bound();
  test_expected_all();
  test_literals();
  if (failures) {
    fprintf(stderr, "selftest_mx_ref: %d check(s) failed\n", failures);
    return 1;
  }
  printf("selftest_mx_ref: all checks passed\n");
  return 0;
}
