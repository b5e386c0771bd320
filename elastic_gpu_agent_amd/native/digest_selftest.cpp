// Stand-alone check of the fused device-set digest in wirecore.h, meant to be
// built with -fsanitize=address,undefined and run directly (the pybind
// modules themselves are never run under a sanitizer).
//
// Every case goes through wirecore::digest_field and through a naive
// collect / sort / join reference written here; hash input, count, sorted
// spans and JSON fragment must agree. Inputs live in exact-size heap blocks
// so ASan traps any read past the end, and every truncation of a small
// message must throw or equal the reference for the shorter message.
//
// Build + run: python -m elastic_gpu_agent_amd.native.build_fuzz --selftest
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "selftest_util.h"
#include "wirecore.h"

namespace {

using namespace selftest;

// unknown fields of wire types 0, 1, 2, 5 and a non-LEN field 1
std::string unknown_fields() {
  std::string u;
  put_varint(u, 2 << 3 | 0); put_varint(u, 300);
  put_varint(u, 7 << 3 | 1); u += std::string("\1\2\3\4\5\6\7\10", 8);
  put_ld(u, 9, "0-zzz-not-an-id");
  put_varint(u, 4 << 3 | 5); u += std::string("\xaa\xbb\xcc\xdd", 4);
  put_varint(u, 1 << 3 | 0); put_varint(u, 5);
  return u;
}

// run the helper on `wire`; compare with the reference for `ids`
void expect_ids(const std::string& wire, std::vector<std::string> ids, const char* what) {
  std::sort(ids.begin(), ids.end());  // byte-wise, shorter prefix first
  std::string joined;
  for (size_t i = 0; i < ids.size(); ++i) {
    if (i) joined += ":";
    joined += ids[i];
  }
  HeapCopy in(wire);
  wirecore::DigestScratch& sc = wirecore::digest_scratch();
  for (int mode = 0; mode < 4; ++mode) {
    bool want_json = mode & 1, want_spans = mode & 2;
    wirecore::ScratchGuard guard(sc);
    wirecore::DigestOut d = wirecore::digest_field(sc, in.p, in.n, 1, want_json,
                                                   want_spans, capture_digest);
    CHECK(d.count == ids.size(), what);
    CHECK(last_joined == joined, what);
    CHECK(strlen(d.hex) == 8, what);
    if (want_json)
      CHECK(std::string(sc.json.data(), d.json_len) == naive_json(ids), what);
    if (want_spans) {
      CHECK(sc.spans.size() == ids.size(), what);
      for (size_t i = 0; i < sc.spans.size() && i < ids.size(); ++i)
        CHECK(std::string((const char*)sc.spans[i].first, sc.spans[i].second) == ids[i], what);
    }
  }
}

void expect_throw(const std::string& wire, const char* what) {
  HeapCopy in(wire);
  wirecore::DigestScratch& sc = wirecore::digest_scratch();
  bool threw = false;
  try {
    wirecore::ScratchGuard guard(sc);
    wirecore::digest_field(sc, in.p, in.n, 1, true, true, capture_digest);
  } catch (const std::runtime_error&) {
    threw = true;
  }
  CHECK(threw, what);
}

void run_case(const std::vector<std::string>& ids, const char* what) {
  expect_ids(encode(ids), ids, what);
  expect_ids(encode(ids, 1, unknown_fields()), ids, what);
}

}  // namespace

int main() {
  std::vector<std::string> sorted;
  for (int i = 0; i < 300; ++i) {
    char b[16];
    snprintf(b, sizeof b, "0-%04d", i);
    sorted.push_back(b);
  }
  std::vector<std::string> reversed(sorted.rbegin(), sorted.rend());
  std::vector<std::string> last_pair = sorted;
  std::swap(last_pair[298], last_pair[299]);

  run_case({}, "empty");
  run_case({"0-07"}, "single");
  run_case(sorted, "sorted");
  run_case(reversed, "reverse");
  run_case(last_pair, "sorted except last pair");
  run_case({"0-1", "0-1", "0-2", "0-2"}, "duplicates");
  run_case({"0-2", "0-1", "0-2", "0-1"}, "duplicates unsorted");
  run_case({"0-1", "0-10"}, "prefix neighbour");
  run_case({"0-10", "0-1"}, "prefix neighbour reversed");
  run_case({"", "0-1"}, "zero-length id");
  run_case({"0-1", ""}, "zero-length id last");
  run_case({"", ""}, "only zero-length ids");
  run_case({std::string(127, 'a'), std::string(128, 'a')}, "127/128");
  run_case({std::string(128, 'b'), std::string(127, 'a')}, "128/127");
  run_case({"0-\"q\"", "0-\\b", "0-\x1f", "\x1f\"\\"}, "json escapes");
  run_case({std::string(200, '"'), std::string(200, '\x1f')}, "fragment 6x input");

  // several wire ranges taken as one set (podresources: one ContainerDevices
  // entry per ID, IDs in field 2), the inversion falling between two ranges
  {
    std::vector<std::string> ids = {"1-5", "1-7", "1-3", "1-4"};
    std::vector<std::string> wires;
    for (auto& id : ids) {
      std::string w;
      put_ld(w, 1, "resource-name");
      put_ld(w, 2, id);
      wires.push_back(w);
    }
    std::vector<wirecore::Span> ranges;
    for (auto& w : wires) ranges.emplace_back((const uint8_t*)w.data(), w.size());
    wirecore::DigestScratch& sc = wirecore::digest_scratch();
    wirecore::ScratchGuard guard(sc);
    wirecore::DigestOut d = wirecore::digest_ranges(sc, ranges.data(), ranges.size(), 2,
                                                    true, true, capture_digest);
    CHECK(d.count == 4, "ranges");
    CHECK(last_joined == "1-3:1-4:1-5:1-7", "ranges");
    CHECK(std::string(sc.json.data(), d.json_len) == "[\"1-3\",\"1-4\",\"1-5\",\"1-7\"]", "ranges");
  }

  // a large call, then a small one: nothing of the first may show
  {
    std::vector<std::string> big;
    for (int i = 0; i < 20000; ++i) {
      char b[16];
      snprintf(b, sizeof b, "0-%06d", i);
      big.push_back(b);
    }
    run_case(big, "20000 sorted");
    run_case({"0-3", "0-1", "0-2"}, "3 after 20000");
    std::vector<std::string> shuffled = big;
    Rng{88172645463325252ull}.shuffle(shuffled);
    run_case(shuffled, "20000 shuffled");
    run_case({"0-3", "0-1", "0-2"}, "3 after 20000 shuffled");
    expect_throw(encode(big) + std::string("\x0a\x7f", 2), "big then truncated");
    run_case({}, "empty after a throw");
  }

  // scratch above the retention cap is given back
  {
    std::vector<std::string> huge(700000, "0-000000");
    expect_ids(encode(huge), huge, "above cap");
    wirecore::DigestScratch& sc = wirecore::digest_scratch();
    CHECK(sc.joined.capacity() <= wirecore::kScratchCap, "joined trimmed");
    CHECK(sc.json.capacity() <= wirecore::kScratchCap, "json trimmed");
    CHECK(sc.spans.capacity() * sizeof(wirecore::Span) <= wirecore::kScratchCap, "spans trimmed");
  }

  // every truncation of a small valid message
  {
    std::vector<std::string> ids = {"0-2", "", "0-1", std::string(130, 'x'), "0-3"};
    std::string msg, u = unknown_fields();
    std::vector<std::pair<size_t, size_t>> boundary;  // (offset, ids before it)
    boundary.emplace_back(0, 0);
    for (size_t i = 0; i < ids.size(); ++i) {
      put_ld(msg, 1, ids[i]);
      boundary.emplace_back(msg.size(), i + 1);
      if (i == 1) {
        // the unknown fields end on sub-field boundaries of their own; find
        // them by walking (this is test scaffolding, not the code under test)
        wirecore::Reader r{(const uint8_t*)u.data(), (const uint8_t*)u.data() + u.size()};
        while (!r.done()) {
          uint64_t tag = r.varint();
          r.skip(tag & 7);
          boundary.emplace_back(msg.size() + (r.p - (const uint8_t*)u.data()), i + 1);
        }
        msg += u;
      }
    }
    for (size_t k = 0; k <= msg.size(); ++k) {
      std::string cut = msg.substr(0, k);
      long nids = -1;
      for (auto& b : boundary)
        if (b.first == k) nids = (long)b.second;
      if (nids >= 0)
        expect_ids(cut, std::vector<std::string>(ids.begin(), ids.begin() + nids), "cut on boundary");
      else
        expect_throw(cut, "cut inside a field");
    }
    // overlong varint, and a length far beyond the buffer
    expect_throw(std::string("\x0a") + std::string(10, '\xff') + "\x01", "varint too long");
    expect_throw(std::string("\x0a") + std::string(9, '\xff') + "\x01", "length wraps");
  }

  if (failures) {
    fprintf(stderr, "digest selftest: %d failure(s)\n", failures.load());
    return 1;
  }
  printf("digest selftest OK\n");
  return 0;
}
