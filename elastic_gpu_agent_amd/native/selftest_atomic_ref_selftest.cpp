// Stand-alone check of selftest_atomic_ref.h, the host reference of the atomic
// sweep, meant to be built with -fsanitize=address,undefined and run directly
// (libegpu_kernels.so itself is never run under a sanitizer).
//
// Checks: every generated cell lies inside its slot's 128 words (the kernel
// uses the same generator for its addresses); the slot table matches the kinds;
// FP fan-ins respect the exactness bound and no FP word is -0, NaN, infinite
// or subnormal; integer cells and operands of rounds 2k and 2k+1 are
// complements; literal values of the reference's inc/dec/cas rules; replaying
// the lanes in reverse leaves the same cells and the same wave sums; weights
// are odd and distinct; expected_all and grid_expected into exact-size heap
// blocks, the grid's closed form against a brute-force replay of every
// workgroup, and the blocks x rounds bound.
//
// Build + run: python -m elastic_gpu_agent_amd.native.build_fuzz --selftest
#include <cstdint>
#include <cstdio>
#include <memory>
#include <set>
#include <vector>

#include "selftest_atomic_ref.h"

namespace {

namespace at = egpu_at;

int failures = 0;

#define CHECK(cond, what)                                                       \
  do {                                                                          \
    if (!(cond)) {                                                              \
      fprintf(stderr, "FAIL %s:%d %s (%s)\n", __FILE__, __LINE__, #cond, what); \
      ++failures;                                                               \
    }                                                                           \
  } while (0)

bool fp_word_plain(int bits, int ebits, uint64_t w) {  // zero (+0 only) or a normal number
  const int mbits = bits - 1 - ebits;
  const uint64_t ex = (w >> mbits) & ((1ull << ebits) - 1);
  return w == 0 || (ex != 0 && ex != (1ull << ebits) - 1);
}
bool fp_plain(int op, uint64_t w) {
  switch (op) {
    case at::OP_FADD32: return fp_word_plain(32, 8, w);
    case at::OP_PKF16: return fp_word_plain(16, 5, w & 0xffff) && fp_word_plain(16, 5, w >> 16);
    case at::OP_PKBF16: return fp_word_plain(16, 8, w & 0xffff) && fp_word_plain(16, 8, w >> 16);
    default: return fp_word_plain(64, 11, w);
  }
}

void test_generator() {
  std::set<int> fans;
  for (int kind = 0; kind < EGPU_AT_NKINDS; ++kind)
    for (int group = 0; group < EGPU_AT_GROUPS; ++group)
      for (int round : {0, 1, 2, 5, EGPU_AT_MAX_ROUNDS - 1})
        for (int s = 0; s < EGPU_AT_NSLOT; ++s) {
          const at::slot st = at::slot_of(kind, s);
          const at::shape sp = at::shape_of(kind, s, group, round);
          const int fan = 1 << (sp.fl + sp.sl);
          if (st.op != at::OP_NONE) fans.insert(fan);
          if (at::is_fp_add(st.op)) CHECK(3 * (fan + 1) <= at::exact_limit(st.op), "FP fan-in within the exact range");
          if (at::returns(st.op)) CHECK(sp.sl == 0, "returning ops use wave-private cells");
          CHECK(!at::is_lds(kind) || (st.op != at::OP_FMIN64 && st.op != at::OP_FMAX64), "f64 min/max are global");
          int per_cell[EGPU_AT_WORDS] = {0};
          for (int tid = 0; tid < EGPU_AT_LANES; ++tid) {
            const at::op_t o = at::gen_op(kind, s, 7, group, round, tid);
            const int width = at::is64(st.op) ? 2 : 1;
            CHECK(o.cell >= EGPU_AT_SLOT_WORDS * s && o.cell + width <= EGPU_AT_SLOT_WORDS * (s + 1) &&
                      o.cell % width == 0, "cell inside its slot, aligned");
            CHECK(o.op == at::OP_NONE || o.op == st.op, "the slot's opcode or none");
            if (o.op == at::OP_NONE) continue;
            CHECK(++per_cell[o.cell] <= fan, "no more lanes on a cell than the shape says");
            if (st.op >= at::OP_FADD32 && st.op <= at::OP_FMAX64) {
              CHECK(fp_plain(st.op, o.a), "FP operand: no -0, NaN, infinity, subnormal");
              CHECK(kind == at::K_G_GRID || fp_plain(st.op, at::init_cell(kind, st.op, at::slot_seed(7, kind, s, group, round), round, o.cell)),
                    "FP initial cell likewise");
              if (st.op >= at::OP_FMIN64) CHECK(o.a != 0, "min/max exclude zero");
            } else if (st.op <= at::OP_MAXU && st.op != at::OP_AND && st.op != at::OP_OR) {
              const at::op_t other = at::gen_op(kind, s, 7, group, round ^ 1, tid);
              const uint64_t mask = at::is64(st.op) ? ~0ull : 0xffffffffull;
              CHECK(other.cell == o.cell && (other.a ^ o.a) == mask, "complement pair: same cell, complemented operand");
            }
            if (kind != at::K_G_GRID && !(st.op >= at::OP_FADD32 && st.op <= at::OP_FMAX64) &&
                st.op != at::OP_INC && st.op != at::OP_DEC && st.op != at::OP_CLAIM)
              CHECK((at::init_word(kind, 7, group, round, o.cell) ^ at::init_word(kind, 7, group, round ^ 1, o.cell)) == 0xffffffffu,
                    "complement pair: complemented initial cell");
          }
        }
  for (int f : {1, 2, 4, 16, 64, 128, 256}) CHECK(fans.count(f), "every fan-in occurs");
}

void test_reference_rules() {
  uint32_t c[2] = {5, 0};
  at::op_t o{at::OP_INC, 0, 5, 0, false};
  CHECK(at::apply(o, c) == 5 && c[0] == 0, "inc wraps to 0 at the limit");
  CHECK(at::apply(o, c) == 0 && c[0] == 1, "inc counts below it");
  o.op = at::OP_DEC;
  c[0] = 0;
  CHECK(at::apply(o, c) == 0 && c[0] == 5, "dec wraps to the limit at 0");
  c[0] = 9;
  CHECK(at::apply(o, c) == 9 && c[0] == 5, "dec wraps to the limit from above it");
  CHECK(at::apply(o, c) == 5 && c[0] == 4, "dec counts below it");
  c[0] = 0xffffffffu, c[1] = 0;
  o = at::op_t{at::OP_ADD64, 0, 1, 0, false};
  at::apply(o, c);
  CHECK(c[0] == 0 && c[1] == 1, "add u64 carries across bit 31/32");
  o = at::op_t{at::OP_CAS64, 0, 7, (1ull << 32), false};
  CHECK(at::apply(o, c) == (1ull << 32) && c[0] == 7 && c[1] == 0, "cas64 swaps on equal");
  CHECK(at::apply(o, c) == 7 && c[0] == 7, "cas64 leaves the cell on unequal");
  c[0] = at::f32_of(3);
  o = at::op_t{at::OP_FADD32, 0, at::f32_of(-2), 0, false};
  at::apply(o, c);
  CHECK(c[0] == 0x3F800000u, "3 + -2 = 1 in f32");
  CHECK(at::pk_add(egpu_cv::W_BF16, at::bf16_of(-3), at::bf16_of(3)) == 0, "x + -x is +0");
  CHECK(at::pk_add(egpu_cv::W_F16, at::f16_of(2) | (at::f16_of(-1) << 16), at::f16_of(3) | (at::f16_of(-3) << 16)) ==
            (0x4500u | (0xC400u << 16)), "packed f16: 5 and -4");
}

void test_order_independence_and_fold() {
  auto fwd = std::make_unique<at::workgroup>(), rev = std::make_unique<at::workgroup>();
  for (int kind = 0; kind < EGPU_AT_NKINDS; ++kind)
    for (int round : {0, 1, 3}) {
      at::replay(kind, 11, 2, round, fwd.get());
      for (int w = 0; w < EGPU_AT_WORDS; ++w) rev->fin[w] = rev->init[w] = fwd->init[w];
      for (int tid = EGPU_AT_LANES - 1; tid >= 0; --tid)
        for (int s = 0; s < EGPU_AT_NSLOT; ++s) {
          rev->ops[tid][s] = fwd->ops[tid][s];
          rev->ret[tid][s] = at::apply(rev->ops[tid][s], rev->fin);
        }
      for (int w = 0; w < EGPU_AT_WORDS; ++w)
        CHECK(at::slot_of(kind, w / EGPU_AT_SLOT_WORDS).op == at::OP_CLAIM ||
                  at::slot_of(kind, w / EGPU_AT_SLOT_WORDS).op == at::OP_SWAP || fwd->fin[w] == rev->fin[w],
              "reverse lane order, same final cells (claim and swap: whoever came last)");
      uint32_t a = 0, b = 0;
      for (int wave = 0; wave < 4; ++wave) {
        // a wave's sum is symmetric in its own lanes; all four together in all lanes
        a += at::wave_round_sum(kind, *fwd, wave), b += at::wave_round_sum(kind, *rev, wave);
        if (kind % 5 == at::K_L_RTN || kind % 5 == at::K_L_CAS)
          CHECK(at::wave_round_sum(kind, *fwd, wave) == at::wave_round_sum(kind, *rev, wave), "wave-private: per wave");
      }
      CHECK(a == b, "reverse lane order, same fold");
    }
  std::set<uint32_t> weights;
  for (int w = 0; w < EGPU_AT_WORDS; ++w) {
    CHECK(at::cell_weight(w) & 1u, "weights are odd");
    weights.insert(at::cell_weight(w));
  }
  CHECK(weights.size() == EGPU_AT_WORDS, "weights are distinct");
}

// exact-size heap blocks, so ASan traps a write one word past the end
void test_expected_and_grid() {
  std::vector<uint32_t> a(EGPU_AT_PATTERNS * EGPU_AT_NKINDS, 0xdeadbeefu), b = a, c = a;
  CHECK(at::expected_all(42, 2, (uint32_t(*)[EGPU_AT_NKINDS])a.data()) == 0, "valid arguments");
  CHECK(at::expected_all(42, 2, (uint32_t(*)[EGPU_AT_NKINDS])b.data()) == 0 && a == b, "same inputs, same records");
  CHECK(at::expected_all(43, EGPU_AT_MAX_ROUNDS, (uint32_t(*)[EGPU_AT_NKINDS])c.data()) == 0, "the largest round count");
  for (int p = 0; p < EGPU_AT_PATTERNS; ++p)
    for (int k = 0; k < EGPU_AT_NKINDS; ++k) {
      const int i = EGPU_AT_NKINDS * p + k;
      CHECK(k == at::K_G_GRID ? a[i] == 0 && c[i] == 0 : a[i] != c[i] && a[i] != 0xdeadbeefu, "seed and rounds matter");
    }
  std::vector<uint32_t> d(EGPU_AT_PATTERNS * EGPU_AT_NKINDS, 0xdeadbeefu);
  CHECK(at::expected_all(0, 0, (uint32_t(*)[EGPU_AT_NKINDS])d.data()) != 0 && d[0] == 0xdeadbeefu, "rounds 0 rejected");
  CHECK(at::expected_all(0, EGPU_AT_MAX_ROUNDS + 1, (uint32_t(*)[EGPU_AT_NKINDS])d.data()) != 0, "rounds over the bound rejected");

  // closed form against every workgroup replayed one after the other
  auto wg = std::make_unique<at::workgroup>();
  for (int blocks : {1, 3, 5, 9}) {
    std::vector<uint32_t> want(EGPU_AT_WORDS), brute(EGPU_AT_WORDS, 0);
    CHECK(at::grid_expected(9, blocks, 3, want.data()) == 0, "valid grid");
    for (int blk = 0; blk < blocks; ++blk)
      for (int r = 0; r < 3; ++r)
        for (int tid = 0; tid < EGPU_AT_LANES; ++tid)
          for (int s = 0; s < EGPU_AT_NSLOT; ++s) at::apply(at::gen_op(at::K_G_GRID, s, 9, blk % 4, r, tid), brute.data());
    CHECK(want == brute, "closed form of the grid cells");
  }
  std::vector<uint32_t> g(EGPU_AT_WORDS, 0xdeadbeefu);
  CHECK(at::grid_work_ok(1024, 16) && at::grid_work_ok(EGPU_AT_GRID_MAX_WORK, 1), "1024 x 16 fits");
  CHECK(!at::grid_work_ok(EGPU_AT_GRID_MAX_WORK + 1, 1) && !at::grid_work_ok(65536, 16), "the bound");
  CHECK(3.0 * 16777216.0 * 256.0 * EGPU_AT_GRID_MAX_WORK <= 9007199254740992.0 &&
            3.0 * 16777216.0 * 256.0 * (EGPU_AT_GRID_MAX_WORK + 1) > 9007199254740992.0, "the bound is 2^53 / (3 * 2^24 * 256)");
  CHECK(at::grid_expected(0, 65536, 16, g.data()) != 0 && g[0] == 0xdeadbeefu, "over the bound: nothing written");
  CHECK(at::grid_expected(0, 0, 2, g.data()) != 0, "blocks 0 rejected");
}

}  // namespace

int main() {
  test_generator();
  test_reference_rules();
  test_order_independence_and_fold();
  test_expected_and_grid();
  if (failures) {
    fprintf(stderr, "selftest_atomic_ref: %d check(s) failed\n", failures);
    return 1;
  }
  printf("selftest_atomic_ref: all checks passed\n");
  return 0;
}
