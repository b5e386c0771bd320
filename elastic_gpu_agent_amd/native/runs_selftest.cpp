// Stand-alone check of the ID-run codec in idruns.h and wirecore.h (RunBuilder,
// digest_field_runs, parse_runs / write_runs / expand_runs), meant to be built
// with -fsanitize=address,undefined and run directly (the pybind modules
// themselves are never run under a sanitizer). Companion of
// digest_stride_selftest.cpp.
//
// Every set goes through digest_field_runs, sorted and shuffled, and through
// a naive split / group / print written here: the runs fragment (or, where
// the set does not qualify, the literal list), the count and the hashed bytes
// must agree with the naive ones and with plain digest_field, and expanding
// the runs must give the literal list byte for byte. Wire inputs and
// fragments live in exact-size heap blocks so ASan traps a read of even one
// byte past the end; write_runs fills an exact-size block too.
//
// Build + run: python -m elastic_gpu_agent_amd.native.build_fuzz --selftest
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "selftest_util.h"
#include "wirecore.h"

namespace {

using namespace selftest;

// the format, from its description: "" where the set keeps its literal list
std::string naive_runs(const Ids& sorted) {
  struct R { std::string prefix; size_t width; unsigned long long start, count; };
  std::vector<R> runs;
  bool have = false;
  std::string pp;
  size_t pw = 0;
  unsigned long long pv = 0;
  for (auto& s : sorted) {
    size_t w = 0;
    while (w < s.size() && s[s.size() - 1 - w] >= '0' && s[s.size() - 1 - w] <= '9') ++w;
    if (w < 1 || w > 18) return "";
    for (unsigned char c : s)
      if (c < 0x20 || c >= 0x80 || c == '"' || c == '\\') return "";
    std::string prefix = s.substr(0, s.size() - w);
    unsigned long long v = strtoull(s.c_str() + s.size() - w, nullptr, 10);
    if (have && prefix == pp && w == pw && v == pv + 1) ++runs.back().count;
    else runs.push_back(R{prefix, w, v, 1});
    have = true; pp = prefix; pw = w; pv = v;
  }
  if (sorted.size() < 1024 || runs.size() > sorted.size() / 8) return "";
  std::string j = "[";
  for (size_t i = 0; i < runs.size(); ++i) {
    char tail[96];
    snprintf(tail, sizeof tail, "\",%zu,%llu,%llu]", runs[i].width, runs[i].start, runs[i].count);
    if (i) j += ",";
    j += "[\"" + runs[i].prefix + tail;
  }
  return j + "]";
}

Rng rnd{0x9E3779B97F4A7C15ull};

void check_set(Ids ids, const char* what) {
  Ids sorted = ids;
  std::sort(sorted.begin(), sorted.end(), id_less);
  const std::string want_list = naive_json(sorted);
  const std::string want_runs = naive_runs(sorted);
  Ids shuffled = ids;
  rnd.shuffle(shuffled);
  const Ids* orders[2] = {&sorted, &shuffled};
  wirecore::DigestScratch& sc = wirecore::digest_scratch();
  for (int o = 0; o < 2; ++o) {
    HeapCopy in(encode(*orders[o]));
    std::string ref_hex, ref_joined;
    {
      wirecore::ScratchGuard guard(sc);
      wirecore::DigestOut d = wirecore::digest_field(sc, in.p, in.n, 1, true, false, capture_digest);
      ref_hex = d.hex;
      ref_joined = last_joined;
      CHECK(std::string(sc.json.data(), d.json_len) == want_list, what);
    }
    wirecore::ScratchGuard guard(sc);
    bool is_runs = false;
    last_joined.clear();
    wirecore::DigestOut d =
        wirecore::digest_field_runs(sc, in.p, in.n, 1, capture_digest, &is_runs, nullptr);
    CHECK(ref_hex == d.hex, what);
    CHECK(ref_joined == last_joined, what);
    CHECK(d.count == sorted.size(), what);
    const std::string frag(sc.json.data(), d.json_len);
    CHECK(is_runs == !want_runs.empty(), what);
    if (is_runs) {
      CHECK(frag == want_runs, what);
      HeapCopy f(frag);
      try {
        wirecore::RunsPlan plan = wirecore::parse_runs((const char*)f.p, f.n, d.count);
        CHECK(plan.total == want_list.size(), what);
        char* out = (char*)malloc(plan.total);  // exact size: ASan guards both ends
        wirecore::write_runs(plan, out);
        CHECK(std::string(out, plan.total) == want_list, what);
        free(out);
        CHECK(wirecore::expand_runs((const char*)f.p, f.n, d.count) == want_list, what);
      } catch (const std::exception& e) {
        CHECK(false, e.what());
      }
    } else {
      CHECK(frag == want_list, what);
    }
  }
  // RunBuilder alone, as _fastwire.ids_to_runs drives it
  wirecore::RunBuilder rb;
  rb.reset(sorted.size() / wirecore::kRunsPerIds);
  for (auto& s : sorted) rb.add((const uint8_t*)s.data(), s.size());
  std::string j;
  if (rb.qualifies()) rb.to_json(j);
  CHECK(j == want_runs, what);
}

Ids seq(const char* fmt, unsigned long long from, size_t n) {
  Ids v;
  char b[96];
  for (size_t i = 0; i < n; ++i) {
    snprintf(b, sizeof b, fmt, from + i);
    v.push_back(b);
  }
  return v;
}

Ids cat(Ids a, const Ids& b) {
  a.insert(a.end(), b.begin(), b.end());
  return a;
}

void expect_reject(const std::string& frag, uint64_t count) {
  HeapCopy f(frag);
  bool threw = false;
  try {
    (void)wirecore::expand_runs((const char*)f.p, f.n, count);
  } catch (const std::runtime_error&) {
    threw = true;
  }
  CHECK(threw, frag.c_str());
}

}  // namespace

int main() {
  // around the minimum, one run, several prefixes, gaps, a duplicate
  check_set(seq("0-%06llu", 0, 1023), "1023");
  check_set(seq("0-%06llu", 0, 1024), "1024");
  check_set(seq("0-%06llu", 0, 1025), "1025");
  check_set(seq("0-%06llu", 0, 18432), "one run");
  check_set(cat(seq("0-%06llu", 0, 700), seq("1-%06llu", 0, 700)), "two gpus");
  check_set(cat(seq("0-%06llu", 0, 777), seq("0-%06llu", 778, 1222)), "gap");
  check_set(cat(seq("0-%06llu", 0, 2000), Ids{"0-000005"}), "duplicate");
  check_set(seq("0-%06llu", 99000, 2000), "rollover in the width");
  check_set(seq("7-%llu", 1, 1199), "width change, fragments when sorted");
  check_set(seq("a%04llu", 8000, 2000), "up to 9999");
  check_set(seq("a%018llu", 999999999999999000ull, 1000), "top of 18 digits");
  check_set(seq("a%018llu", 0, 1500), "18 digits");
  check_set(seq("a%019llu", 0, 1500), "19 digits");
  check_set(seq("%03llu", 0, 1000), "digits only");
  check_set(seq("%08llu", 0, 3000), "8 digits only, L = 8");
  // every stride length and the generic path
  check_set(seq("%llu", 1000, 2000), "L = 4");
  check_set(seq("10-%06llu", 0, 1500), "L = 9");
  check_set(seq("gpu-%012llu", 0, 1500), "L = 16");
  check_set(seq("gpu-long-prefix-%08llu", 0, 1500), "L = 24, generic");
  check_set(cat(cat(seq("0-%06llu", 0, 1500), seq("10-%06llu", 0, 1500)),
                seq("gpu-long-prefix-%08llu", 0, 1500)), "mixed lengths");
  check_set(seq("a:b:%05llu", 0, 1500), "colons in the prefix");
  // every stride length, sorted (the run's one or two words) and shuffled
  // (the radix output up to L = 8): consecutive IDs whose tails cross a
  // one-carry boundary (x9 -> y0) and a two-carry one (x99 -> y00). The
  // exception is L = 1: ten IDs are far below the 3 * kRunsMinIds wire bytes
  // at which digest_field_runs attaches a RunBuilder, so there only the
  // digest and the RunBuilder alone are compared, not `successor`.
  check_set(seq("%llu", 0, 10), "sweep L = 1");
  for (int L = 2; L <= 16; ++L) {
    Ids v;
    char b[32];
    if (L >= 4) {
      // 1500 IDs from 950: past 999 -> 1000; a letter in front from L = 5
      for (unsigned long long i = 950; i < 950 + 1500; ++i) {
        if (L == 4) snprintf(b, sizeof b, "%04llu", i);
        else snprintf(b, sizeof b, "a%0*llu", L - 1, i);
        v.push_back(b);
      }
    } else {
      // two or three bytes: every all-digit ID (09 -> 10, 099 -> 100), then
      // blocks with another byte in front; from the last ID of a block (99,
      // a9) no carry leads to the next. L = 3 takes letters up to 1500 IDs.
      // L = 2 takes every printable byte json.dumps leaves alone: 920 IDs,
      // too few to be stored as runs, but past the 768 entries from which
      // the walk runs with a RunBuilder and evaluates `successor`.
      for (int i = 0; i < (L == 2 ? 100 : 1000); ++i) {
        snprintf(b, sizeof b, "%0*d", L, i);
        v.push_back(b);
      }
      for (int c = L == 2 ? '!' : 'a'; c <= (L == 2 ? '~' : 'z') && v.size() < 1500; ++c) {
        if ((c >= '0' && c <= '9') || c == '"' || c == '\\') continue;
        for (int i = 0; i < (L == 2 ? 10 : 100); ++i) {
          snprintf(b, sizeof b, "%c%0*d", c, L - 1, i);
          v.push_back(b);
        }
      }
      if (L == 2) CHECK(encode(v).size() >= 3 * wirecore::kRunsMinIds, "sweep L = 2 is walked with runs");
    }
    snprintf(b, sizeof b, "sweep L = %d", L);
    check_set(v, b);
  }
  // not run-encodable somewhere in a large set
  check_set(cat(seq("0-%06llu", 0, 2000), Ids{"0-abc"}), "no digits");
  check_set(cat(seq("0-%06llu", 0, 2000), Ids{"0-\"1"}), "quote");
  check_set(cat(seq("0-%06llu", 0, 2000), Ids{std::string("0-\x01") + "1"}), "control byte");
  check_set(cat(seq("0-%06llu", 0, 2000), Ids{"\xc3\xa9" "1"}), "non-ascii");
  check_set(cat(seq("0-%06llu", 0, 2000), Ids{""}), "empty id");
  // runs at count / 8 and one over
  {
    Ids at, over;
    for (unsigned r = 0; r < 128; ++r) at = cat(at, seq("0-%06llu", r * 100, 8));
    check_set(at, "runs == count / 8");
    for (unsigned r = 0; r < 129; ++r) over = cat(over, seq("0-%06llu", r * 100, 8));
    over = cat(over, seq("0-%06llu", 90000, 6));
    check_set(over, "runs == count / 8 + 1");
  }
  // random sets: random gaps and prefixes
  for (int round = 0; round < 40; ++round) {
    Ids v;
    unsigned long long at = rnd() % 1000;
    const size_t n = 900 + rnd() % 3000;
    const unsigned gap_every = 2 + rnd() % 400;
    const char* fmts[] = {"0-%06llu", "%llu", "1-%05llu", "gpu-%012llu", "node-a/gpu-3/%07llu"};
    const char* fmt = fmts[rnd() % 5];
    for (size_t i = 0; i < n; ++i) {
      char b[96];
      snprintf(b, sizeof b, fmt, at);
      v.push_back(b);
      at += (rnd() % gap_every == 0) ? 1 + rnd() % 50 : 1;
    }
    check_set(v, "random");
  }

  // expand_runs: everything it must refuse
  expect_reject("[[\"0-\",6,0,2048]]", 2047);
  expect_reject("[[\"0-\",6,0,2048]]", 2049);
  expect_reject("[[\"0-\",6,0,1000],[\"0-\",6,2000,1000]]", 1000);
  expect_reject("[[\"0-\",6,999000,1001]]", 1001);
  expect_reject("[[\"0-\",1,9,2]]", 2);
  expect_reject("[[\"0-\",0,0,1]]", 1);
  expect_reject("[[\"0-\",19,0,1]]", 1);
  expect_reject("[[\"0-\",6,-1,5]]", 5);
  expect_reject("[[\"0-\",6,0,-5]]", 5);
  expect_reject("[[\"0-\",6,0.0,5]]", 5);
  expect_reject("[[\"0-\",6,0,5e0]]", 5);
  expect_reject("[[\"0-\",6,\"0\",5]]", 5);
  expect_reject("[[\"0-\",6,0,0]]", 0);
  expect_reject("[[\"0-\",6,0,5,1]]", 5);
  expect_reject("[[\"0-\",6,0]]", 0);
  expect_reject("[[\"0-\",06,0,5]]", 5);
  expect_reject("[[\"0\\u002d\",6,0,5]]", 5);
  expect_reject("[[\"0-\",6,0,5]]x", 5);
  expect_reject("[[\"0-\",18,0,600000]]", 600000);  // over kRunsMaxExpanded
  expect_reject("[[\"0-\",18,0,999999999999999999]]", 999999999999999999ull);
  expect_reject("[[\"0-\",6,0,99999999999999999999]]", 5);
  expect_reject("[[\"0-\",6,0,18446744073709551615]]", 18446744073709551615ull);
  expect_reject(std::string("[[\"") + std::string(5u << 20, 'p') + "\",1,0,1]]", 1);
  // counts that would wrap a sum: each run is within its width
  expect_reject("[[\"a\",18,0,999999999999999999],[\"a\",18,0,999999999999999999],"
                "[\"a\",18,0,999999999999999999]]", 2999999999999999997ull);
  {  // truncated at every byte
    const std::string good = "[[\"0-\",6,0,1000],[\"1-\",6,24,1048]]";
    CHECK(wirecore::expand_runs(good.data(), good.size(), 2048).size() ==
              2048 * 11 + 1, "good fragment");
    for (size_t k = 0; k < good.size(); ++k) expect_reject(good.substr(0, k), 2048);
  }
  CHECK(wirecore::expand_runs("[]", 2, 0) == "[]", "empty");
  CHECK(wirecore::expand_runs(" [ [ \"0-\" , 2 , 98 , 2 ] ] ", 27, 2) == "[\"0-98\",\"0-99\"]",
        "whitespace");

  if (failures) {
    fprintf(stderr, "%d check(s) failed\n", failures.load());
    return 1;
  }
  printf("runs selftest OK\n");
  return 0;
}
