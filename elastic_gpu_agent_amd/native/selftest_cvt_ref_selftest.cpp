// Stand-alone check of selftest_cvt_ref.h, the host reference of the
// conversion sweep, meant to be built with -fsanitize=address,undefined and run
// directly (libegpu_kernels.so itself is never run under a sanitizer).
//
// Checks: the group table fits the lane's register arrays; every decoder and
// the generic encoder are inverse on every finite code of every format; for
// every generated encode element the generic encoder agrees with the
// generator's closed form and the source is zero or a normal number of its
// format; every decode result is zero or normal; scales are in range with a
// zero mantissa; one wave and round covers every (code, sign, q) of the
// single-format kinds; `old` words of rounds 2k and 2k+1 are complements and
// survive where the layout says; fold weights are odd and distinct;
// expected_all at rounds 1 and EGPU_CVT_MAX_ROUNDS into exact-size heap blocks.
//
// Build + run: python -m elastic_gpu_agent_amd.native.build_fuzz --selftest
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <set>
#include <vector>

#include "selftest_cvt_ref.h"

namespace {

namespace cv = egpu_cv;

int failures = 0;

#define CHECK(cond, what)                                                       \
  do {                                                                          \
    if (!(cond)) {                                                              \
      fprintf(stderr, "FAIL %s:%d %s (%s)\n", __FILE__, __LINE__, #cond, what); \
      ++failures;                                                               \
    }                                                                           \
  } while (0)

void test_group_table() {
  for (int kind = 0; kind < EGPU_CVT_NKINDS; ++kind) {
    const int n = cv::n_groups(kind);
    CHECK(cv::src_base(kind, n) <= EGPU_CVT_NSRC, "sources fit");
    CHECK(cv::old_base(kind, n) <= EGPU_CVT_NOLD, "old words fit");
    CHECK(cv::res_base(kind, n) <= EGPU_CVT_NRES, "results fit");
    CHECK(cv::scale_lo(kind) <= cv::scale_hi(kind), "scale range");
  }
  CHECK(cv::res_base(cv::K_X16, 4) == 32 && cv::res_base(cv::K_PLAIN, 5) == 32, "mixed kinds fill 32");
}

bool wide_normal_or_zero(int wfmt, uint32_t bits) {
  const cv::format f = cv::wide(wfmt);
  const uint32_t ex = (bits >> f.mbits) & ((1u << f.ebits) - 1u);
  const uint32_t frac = bits & ((1u << f.mbits) - 1u);
  return (ex == 0 && frac == 0) || (ex != 0 && ex != (1u << f.ebits) - 1u);
}

void test_codecs_are_inverse() {
  for (int nf = cv::N_E4M3; nf <= cv::N_E2M1; ++nf) {
    const cv::format f = cv::narrow(nf);
    for (uint32_t sign = 0; sign < 2; ++sign)
      for (uint32_t mag = 0; mag <= (uint32_t)f.max_mag; ++mag) {
        const uint32_t code = (sign << (f.ebits + f.mbits)) | mag;
        const double v = cv::decode_narrow(nf, code);
        CHECK(std::isfinite(v), "finite codes decode to numbers");
        CHECK(cv::encode_rne(f, v) == code, "encode(decode(code)) == code");
        if (mag) CHECK(std::fabs(v) > std::fabs(cv::decode_narrow(nf, code - 1)), "codes are monotonic");
      }
    CHECK(cv::encode_rne(f, 1e30) == (uint32_t)f.max_mag, "saturates");
  }
  // literal values, from the OCP tables
  CHECK(cv::decode_narrow(cv::N_E4M3, 0x7E) == 448.0 && cv::decode_narrow(cv::N_E5M2, 0x7B) == 57344.0, "fp8 max");
  CHECK(cv::decode_narrow(cv::N_E2M3, 0x1F) == 7.5 && cv::decode_e3m2(0x1F) == 28.0, "fp6 max");
  CHECK(cv::decode_e3m2(0x01) == 0.0625 && cv::decode_narrow(cv::N_E2M1, 0x7) == 6.0, "bf6 min, fp4 max");
  CHECK(cv::encode_rne(cv::narrow(cv::N_E2M1), 2.5) == 4 && cv::encode_rne(cv::narrow(cv::N_E2M1), 5.0) == 6,
        "ties to even: 2.5 -> 2, 5 -> 4");
  CHECK(cv::encode_rne(cv::narrow(cv::N_E2M1), -0.25) == 0x8, "a tie at zero rounds to signed zero");
  for (int wf = cv::W_F32; wf <= cv::W_BF16; ++wf)
    for (uint32_t bits : {0x0u, 0x3c00u, 0x3f80u, 0x0401u, 0x7bffu, 0x7f7fu, 0x00800000u, 0x3f800001u}) {
      const uint32_t b = bits & (wf == cv::W_F32 ? 0xffffffffu : 0xffffu);
      if (wide_normal_or_zero(wf, b))
        CHECK(cv::encode_rne(cv::wide(wf), cv::decode_wide(wf, b)) == b, "wide round trip");
    }
}

void test_generator() {
  for (int kind = 0; kind < EGPU_CVT_NKINDS; ++kind)
    for (int pattern : {0, 15})
      for (int round : {0, 1, EGPU_CVT_MAX_ROUNDS - 1})
        for (int g = 0; g < cv::n_groups(kind); ++g) {
          const cv::group gr = cv::group_of(kind, g);
          const cv::format nf = cv::narrow(gr.nfmt), wf = cv::wide(gr.wfmt);
          const uint32_t gs = cv::group_seed(7, pattern, kind, g, round);
          std::set<uint32_t> seen;
          for (int lane = 0; lane < 64; ++lane) {
            const int S = cv::lane_scale(7, pattern, kind, round, lane);
            CHECK(S >= cv::scale_lo(kind) && S <= cv::scale_hi(kind), "scale in range");
            CHECK((cv::scale_bits(S) & 0x807fffffu) == 0 && cv::scale_exponent(cv::scale_bits(S)) == S,
                  "scale is a positive power of two");
            for (int j = 0; j < gr.elems; ++j) {
              const cv::element e = cv::gen_element(gs, nf, gr.elems, round, lane, j);
              CHECK(e.mag <= (uint32_t)nf.max_mag && e.q < 4 && e.sign < 2, "element in range");
              CHECK(e.mag < (uint32_t)nf.max_mag || e.q < 2, "never above the largest finite code");
              seen.insert((e.mag << 3) | (e.sign << 2) | (gr.dir == cv::ENC ? e.q : 0));
              if (gr.dir == cv::ENC) {
                const uint32_t w = cv::wide_bits(wf, nf, e, S);
                CHECK(wide_normal_or_zero(gr.wfmt, w), "source is zero or normal");
                const double v = std::ldexp(cv::decode_wide(gr.wfmt, w), -S);
                const double c = std::fabs(cv::decode_narrow(gr.nfmt, e.mag));
                const double up = e.mag < (uint32_t)nf.max_mag
                                      ? std::fabs(cv::decode_narrow(gr.nfmt, e.mag + 1))
                                      : c + (c - std::fabs(cv::decode_narrow(gr.nfmt, e.mag - 1)));
                CHECK(std::fabs(v) == c + e.q * (up - c) / 4 && std::signbit(v) == (e.sign != 0),
                      "source is c + q quarter gaps, times 2^S");
                CHECK(cv::encode_rne(nf, v) == cv::closed_form(nf, e), "encoder agrees with the closed form");
              } else {
                const double v = std::ldexp(cv::decode_narrow(gr.nfmt, cv::narrow_code(nf, e)), S);
                const uint32_t w = cv::encode_rne(wf, v);
                CHECK(wide_normal_or_zero(gr.wfmt, w) && cv::decode_wide(gr.wfmt, w) == v,
                      "decode result is exact, zero or normal");
              }
            }
          }
          if (gr.elems >= 16) {
            const size_t per_code = gr.dir == cv::ENC ? 4 : 1;
            const size_t want = 2 * (per_code * (size_t)(nf.max_mag + 1) - (gr.dir == cv::ENC ? 2 : 0));
            CHECK(seen.size() == want, "one wave, one round: every allowed (code, sign, q)");
          }
        }
}

void test_old_words_and_layout() {
  for (int kind = 0; kind < EGPU_CVT_NKINDS; ++kind) {
    cv::lane_io a, b;
    uint32_t ra[EGPU_CVT_NRES], rb[EGPU_CVT_NRES];
    CHECK(cv::lane_reference(kind, 3, 5, 17, 6, &a, ra) && cv::lane_reference(kind, 3, 5, 17, 7, &b, rb),
          "known kind");
    int o = 0;
    for (int g = 0; g < cv::n_groups(kind); ++g) {
      const cv::group gr = cv::group_of(kind, g);
      for (int i = 0; i < cv::n_old(gr); ++i, ++o) {
        CHECK(a.old[o] == ~b.old[o], "rounds 2k and 2k+1 carry complementary old words");
        const uint32_t keep = gr.pack == cv::P_WORD ? ~(0xffffu << (16 * (i & 1))) : ~(0xffu << (8 * (i & 3)));
        CHECK(((ra[cv::res_base(kind, g) + i] ^ a.old[o]) & keep) == 0, "untouched bits survive");
      }
    }
    for (int i = o; i < EGPU_CVT_NOLD; ++i) CHECK(a.old[i] == 0, "unused old words are zero");
    for (int i = cv::res_base(kind, cv::n_groups(kind)); i < EGPU_CVT_NRES; ++i)
      CHECK(ra[i] == 0, "unused result registers are zero");
  }
  cv::lane_io io;
  uint32_t res[EGPU_CVT_NRES];
  CHECK(!cv::lane_reference(EGPU_CVT_NKINDS, 0, 0, 0, 0, &io, res), "unknown kind rejected");
  std::set<uint32_t> weights;
  for (int lane = 0; lane < 64; ++lane)
    for (int reg = 0; reg < EGPU_CVT_NRES; ++reg) {
      CHECK(cv::reg_weight(lane, reg) & 1u, "weights are odd");
      weights.insert(cv::reg_weight(lane, reg));
    }
  CHECK(weights.size() == 64 * EGPU_CVT_NRES, "weights are distinct");
}

// exact-size heap block, so ASan traps a write one word past the records
std::vector<uint32_t> expected(uint32_t seed, int rounds, int* rc) {
  std::vector<uint32_t> out(EGPU_CVT_PATTERNS * EGPU_CVT_NKINDS, 0xdeadbeefu);
  *rc = cv::expected_all(seed, rounds, (uint32_t(*)[EGPU_CVT_NKINDS])out.data());
  return out;
}

void test_expected_all() {
  int rc1, rc2;
  const auto a = expected(42, 2, &rc1), b = expected(42, 2, &rc2);
  CHECK(rc1 == 0 && rc2 == 0, "valid arguments");
  CHECK(a == b, "same inputs, same records");
  const auto other = expected(43, 2, &rc1), more = expected(42, 3, &rc2);
  for (int i = 0; i < EGPU_CVT_PATTERNS * EGPU_CVT_NKINDS; ++i) {
    CHECK(a[i] != other[i], "the seed matters, also after a complement pair");
    CHECK(a[i] != more[i], "the round count matters");
  }
  for (int kind = 0; kind < EGPU_CVT_NKINDS; ++kind) {
    std::set<uint32_t> sigs;
    for (int p = 0; p < EGPU_CVT_PATTERNS; ++p) sigs.insert(a[EGPU_CVT_NKINDS * p + kind]);
    CHECK(sigs.size() == EGPU_CVT_PATTERNS, "16 distinct signatures per kind");
  }
  const auto top = expected(42, EGPU_CVT_MAX_ROUNDS, &rc1);
  CHECK(rc1 == 0 && top != a, "the largest round count");
  for (uint32_t v : top) CHECK(v != 0xdeadbeefu, "every record written");
  const auto lo = expected(0, 0, &rc1);
  CHECK(rc1 != 0 && lo[0] == 0xdeadbeefu, "rounds 0 rejected, nothing written");
  expected(0, -1, &rc1);
  CHECK(rc1 != 0, "negative rounds rejected");
  expected(0, EGPU_CVT_MAX_ROUNDS + 1, &rc1);
  CHECK(rc1 != 0, "rounds over the bound rejected");
}

}  // namespace

int main() {
  test_group_table();
  test_codecs_are_inverse();
  test_generator();
  test_old_words_and_layout();
  test_expected_all();
  if (failures) {
    fprintf(stderr, "selftest_cvt_ref: %d check(s) failed\n", failures);
    return 1;
  }
  printf("selftest_cvt_ref: all checks passed\n");
  return 0;
}
