// Stand-alone check of the hash memo in hashmemo.h and wirecore.h (HashMemo,
// digest_field_put, digest_field_runs), meant to be built with
// -fsanitize=address,undefined and run directly (the pybind modules
// themselves are never run under a sanitizer). Companion of runs_selftest.cpp.
//
// Every set goes through the Allocate-side digest and the PreStart-side
// digest with a memo, and through plain digest_field / digest_field_runs
// without one: hash, count, fragment and is_runs must agree whatever the memo
// holds, and the counters must show the puts, hits and misses the sets imply.
// The threaded case runs Allocate/PreStart pairs on distinct sets from four
// threads against one memo. Wire inputs live in exact-size heap blocks so
// ASan traps a read of even one byte past the end.
//
// Build + run: python -m elastic_gpu_agent_amd.native.build_fuzz --selftest
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "selftest_util.h"
#include "wirecore.h"

namespace {

using selftest::HeapCopy;
using selftest::Ids;
using selftest::encode;
using selftest::failures;

// stand-in for sha256 (no crypto library here); counts its calls per thread
thread_local int sha_calls = 0;
void fnv_digest(const void* data, size_t len, unsigned char md[32]) {
  ++sha_calls;
  selftest::fnv_digest(data, len, md);
}

Ids id_range(int gpu, size_t start, size_t n, int width = 6) {
  Ids ids;
  char b[48];
  for (size_t i = 0; i < n; ++i) {
    snprintf(b, sizeof b, "%d-%0*zu", gpu, width, start + i);
    ids.push_back(b);
  }
  return ids;
}

Ids shuffled(Ids ids, unsigned seed) {
  std::mt19937 rng(seed);
  std::shuffle(ids.begin(), ids.end(), rng);
  return ids;
}

struct Result {
  std::string hex, frag;
  size_t count;
  bool is_runs;
  bool operator==(const Result& o) const {
    return hex == o.hex && frag == o.frag && count == o.count && is_runs == o.is_runs;
  }
};

std::string allocate(const Ids& ids, wirecore::HashMemo* memo) {
  HeapCopy in(encode(ids));
  wirecore::DigestScratch& sc = wirecore::digest_scratch();
  wirecore::ScratchGuard guard(sc);
  wirecore::DigestOut d = wirecore::digest_field_put(sc, in.p, in.n, 1, fnv_digest, memo);
  CHECK(d.count == ids.size(), "allocate count");
  return d.hex;
}

Result prestart(const Ids& ids, wirecore::HashMemo* memo) {
  HeapCopy in(encode(ids));
  wirecore::DigestScratch& sc = wirecore::digest_scratch();
  wirecore::ScratchGuard guard(sc);
  bool is_runs = false;
  wirecore::DigestOut d =
      wirecore::digest_field_runs(sc, in.p, in.n, 1, fnv_digest, &is_runs, memo);
  return Result{d.hex, std::string(sc.json.data(), d.json_len), d.count, is_runs};
}

// Allocate then PreStart of one set against `memo`; everything must equal
// the memo-less results. Returns whether PreStart skipped its hash.
bool pair_case(const Ids& alloc_ids, const Ids& pre_ids, wirecore::HashMemo& memo,
               const char* what) {
  const std::string plain_hex = allocate(alloc_ids, nullptr);
  const Result plain = prestart(pre_ids, nullptr);
  CHECK(allocate(alloc_ids, &memo) == plain_hex, what);
  const int before = sha_calls;
  const Result got = prestart(pre_ids, &memo);
  const int hashed = sha_calls - before;
  CHECK(got == plain, what);
  CHECK(hashed <= 1, what);  // never hashed twice
  return hashed == 0;
}

void test_memo_itself() {
  wirecore::HashMemo m;
  char hex[9];
  CHECK(m.enabled() && m.stats().cap == wirecore::kMemoEntries, "default cap");
  CHECK(!m.take("a", hex), "empty take");
  m.put("a", "11111111");
  m.put("b", "22222222");
  m.put("a", "33333333");  // same key: one entry, refreshed
  CHECK(m.stats().entries == 2, "entries");
  CHECK(m.take("a", hex) && !strcmp(hex, "33333333"), "take a");
  CHECK(!m.take("a", hex), "consumed");
  m.configure(2);
  m.put("c", "44444444");
  m.put("d", "55555555");  // evicts b, the oldest
  CHECK(m.stats().evictions == 1, "evictions");
  CHECK(!m.take("b", hex), "evicted");
  CHECK(m.take("d", hex) && m.take("c", hex) && !strcmp(hex, "44444444"), "kept");
  // refreshed entry survives an eviction that takes the older one
  m.put("e", "66666666");
  m.put("f", "77777777");
  m.put("e", "88888888");
  m.put("g", "99999999");  // evicts f
  CHECK(!m.take("f", hex) && m.take("e", hex) && !strcmp(hex, "88888888"), "refresh order");
  // key length cap: exactly at the cap is stored, one over is not
  std::string at(wirecore::kMemoMaxKey, 'k'), over(wirecore::kMemoMaxKey + 1, 'k');
  const uint64_t puts = m.stats().puts;
  m.put(over, "aaaaaaaa");
  CHECK(m.stats().puts == puts && !m.take(over, hex), "over the cap");
  m.put(at, "bbbbbbbb");
  CHECK(m.take(at, hex) && !strcmp(hex, "bbbbbbbb"), "at the cap");
  // shrinking drops the oldest; 0 empties and turns off
  m.configure(8);
  for (int i = 0; i < 8; ++i) m.put(std::string(1, (char)('A' + i)), "cccccccc");
  m.configure(3);
  CHECK(m.stats().entries == 3 && m.take("H", hex) && !m.take("A", hex), "shrink");
  m.configure(0);
  CHECK(!m.enabled() && m.stats().entries == 0, "off");
  const wirecore::HashMemoStats off = m.stats();
  m.put("z", "dddddddd");
  CHECK(!m.take("z", hex), "off take");
  CHECK(m.stats().puts == off.puts && m.stats().misses == off.misses, "off counts nothing");
}

void test_pairs() {
  wirecore::HashMemo memo;
  // smallest set that qualifies, and one short of it
  CHECK(pair_case(id_range(0, 0, 1024), id_range(0, 0, 1024), memo, "1024"), "1024 hit");
  CHECK(!pair_case(id_range(0, 0, 1023), id_range(0, 0, 1023), memo, "1023"), "1023 no put");
  CHECK(memo.stats().puts == 1 && memo.stats().hits == 1, "counts");
  // orders: sorted/shuffled either side
  Ids big = id_range(0, 100, 18432);
  CHECK(pair_case(big, shuffled(big, 1), memo, "sorted, shuffled"), "hit");
  CHECK(pair_case(shuffled(big, 2), big, memo, "shuffled, sorted"), "hit");
  CHECK(pair_case(shuffled(big, 3), shuffled(big, 4), memo, "shuffled both"), "hit");
  // the hit consumed the entry
  const int before = sha_calls;
  Result again = prestart(shuffled(big, 5), &memo);
  CHECK(sha_calls - before == 1 && again == prestart(big, nullptr), "second PreStart hashes");
  // a set that differs by one gap
  Ids other(big.begin(), big.end());
  other.erase(other.begin() + 1000);
  other.push_back(id_range(0, 100 + 18432, 1)[0]);
  CHECK(!pair_case(big, other, memo, "one gap"), "miss");
  CHECK(prestart(big, &memo) == prestart(big, nullptr), "own entry still there");
  // wide IDs (two-word stride path), two prefixes, duplicates
  Ids wide = id_range(3, 5, 2048, 12);
  CHECK(pair_case(wide, shuffled(wide, 6), memo, "wide"), "hit");
  Ids two = id_range(0, 0, 1500);
  Ids more = id_range(1, 7, 1500);
  two.insert(two.end(), more.begin(), more.end());
  CHECK(pair_case(two, shuffled(two, 7), memo, "two prefixes"), "hit");
  Ids dup = id_range(0, 0, 2048);
  dup.push_back(dup[17]);
  std::sort(dup.begin(), dup.end());
  CHECK(pair_case(dup, shuffled(dup, 8), memo, "duplicate"), "hit");
  // large enough to try, does not qualify: an ID that is not run-encodable,
  // and a fragmented set; hashed once, list fragment as without the memo
  Ids bad = id_range(0, 0, 2048);
  bad.push_back("0-x");
  std::sort(bad.begin(), bad.end());
  CHECK(!pair_case(bad, shuffled(bad, 9), memo, "not run-encodable"), "no put");
  Ids frag;
  for (size_t k = 0; k < 1200; ++k) frag.push_back(id_range(0, 3 * k, 1)[0]);
  CHECK(!pair_case(frag, shuffled(frag, 10), memo, "fragmented"), "no put");
  // fragment over the key cap: 300 runs of 8
  Ids longkey;
  for (size_t k = 0; k < 300; ++k) {
    Ids r = id_range(0, 10 * k, 8);
    longkey.insert(longkey.end(), r.begin(), r.end());
  }
  const uint64_t puts = memo.stats().puts;
  CHECK(!pair_case(longkey, shuffled(longkey, 11), memo, "long key"), "not stored");
  CHECK(memo.stats().puts == puts, "long key put");
  CHECK(prestart(longkey, nullptr).frag.size() > wirecore::kMemoMaxKey, "long key is long");
  // memo off: the plain paths
  memo.configure(0);
  CHECK(!pair_case(big, big, memo, "off"), "off");
  // malformed input throws as without the memo and leaves it usable
  memo.configure(4);
  std::string trunc = encode(id_range(0, 0, 2048));
  trunc.resize(trunc.size() - 3);
  HeapCopy in(trunc);
  wirecore::DigestScratch& sc = wirecore::digest_scratch();
  bool threw = false, is_runs = false;
  try {
    wirecore::ScratchGuard guard(sc);
    wirecore::digest_field_put(sc, in.p, in.n, 1, fnv_digest, &memo);
  } catch (const std::runtime_error&) {
    threw = true;
  }
  CHECK(threw, "truncated allocate");
  threw = false;
  try {
    wirecore::ScratchGuard guard(sc);
    wirecore::digest_field_runs(sc, in.p, in.n, 1, fnv_digest, &is_runs, &memo);
  } catch (const std::runtime_error&) {
    threw = true;
  }
  CHECK(threw && memo.stats().entries == 0, "truncated prestart");
  CHECK(pair_case(big, big, memo, "after throw"), "hit");
}

void test_threads() {
  wirecore::HashMemo memo;
  std::vector<std::thread> threads;
  for (int t = 0; t < 4; ++t)
    threads.emplace_back([t, &memo] {
      for (int k = 0; k < 20; ++k) {
        Ids ids = id_range(t, 2000 * (size_t)k, 1024 + (size_t)k);
        CHECK(pair_case(ids, shuffled(ids, (unsigned)(t * 100 + k)), memo, "threaded"), "hit");
      }
    });
  for (auto& th : threads) th.join();
  wirecore::HashMemoStats s = memo.stats();
  CHECK(s.puts == 80 && s.hits == 80 && s.misses == 0 && s.entries == 0, "threaded counts");
  // churn at a tiny cap: evictions and misses race, results stay right
  memo.configure(2);
  threads.clear();
  for (int t = 0; t < 4; ++t)
    threads.emplace_back([t, &memo] {
      for (int k = 0; k < 20; ++k) {
        Ids ids = id_range(t, 2000 * (size_t)k, 1024);
        pair_case(ids, ids, memo, "threaded, cap 2");
      }
    });
  for (auto& th : threads) th.join();
  s = memo.stats();
  CHECK(s.entries <= 2 && s.hits + s.misses == 80 + 80, "cap 2 counts");
}

}  // namespace

int main() {
  test_memo_itself();
  test_pairs();
  test_threads();
  if (failures) {
    fprintf(stderr, "%d failure(s)\n", failures.load());
    return 1;
  }
  printf("hash_memo_selftest OK\n");
  return 0;
}
