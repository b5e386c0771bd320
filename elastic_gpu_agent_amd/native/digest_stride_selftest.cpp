// Stand-alone check of the fixed-stride run and the radix fallback of the
// device-set digest in wirecore.h, meant to be built with
// -fsanitize=address,undefined and run directly (the pybind modules
// themselves are never run under a sanitizer). Companion of
// digest_selftest.cpp, which keeps the general cases.
//
// Every case goes through wirecore::digest_field / digest_ranges and through
// a naive collect / sort / join reference written here; hash input, count,
// sorted spans and JSON fragment must agree. Inputs live in exact-size heap
// blocks so ASan traps a read of even one byte past the end: a whole-word
// load of an ID shorter than 8 bytes at the end of a range is the trap this
// file is for.
//
// Build + run: python -m elastic_gpu_agent_amd.native.build_fuzz --selftest
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "selftest_util.h"
#include "wirecore.h"

namespace {

using namespace selftest;

// one unknown field of each kind the walker accepts: varint, fixed64,
// length-delimited, fixed32, and a field 1 that is not length-delimited
std::vector<std::string> unknown_kinds() {
  std::vector<std::string> k(5);
  put_varint(k[0], 2 << 3 | 0); put_varint(k[0], 300);
  put_varint(k[1], 7 << 3 | 1); k[1] += std::string("\1\2\3\4\5\6\7\10", 8);
  put_ld(k[2], 9, "0-zzz-not-an-id");
  put_varint(k[3], 4 << 3 | 5); k[3] += std::string("\xaa\xbb\xcc\xdd", 4);
  put_varint(k[4], 1 << 3 | 0); put_varint(k[4], 5);
  return k;
}

// `extra` goes in after entry number `at` (0 = before the first)
std::string encode_with(const Ids& ids, size_t at, const std::string& extra) {
  std::string out;
  for (size_t i = 0; i <= ids.size(); ++i) {
    if (i == at) out += extra;
    if (i < ids.size()) put_ld(out, 1, ids[i]);
  }
  return out;
}

// run the helper on `wire` in all four modes; compare with the reference
void expect_ids(const std::string& wire, Ids ids, const char* what, uint32_t field = 1) {
  std::sort(ids.begin(), ids.end(), id_less);
  std::string joined;
  for (size_t i = 0; i < ids.size(); ++i) {
    if (i) joined += ":";
    joined += ids[i];
  }
  const std::string json = naive_json(ids);
  HeapCopy in(wire);
  wirecore::DigestScratch& sc = wirecore::digest_scratch();
  for (int mode = 0; mode < 4; ++mode) {
    bool want_json = mode & 1, want_spans = mode & 2;
    wirecore::ScratchGuard guard(sc);
    wirecore::DigestOut d = wirecore::digest_field(sc, in.p, in.n, field, want_json,
                                                   want_spans, capture_digest);
    CHECK(d.count == ids.size(), what);
    CHECK(last_joined == joined, what);
    if (want_json) CHECK(std::string(sc.json.data(), d.json_len) == json, what);
    if (want_spans) {
      CHECK(sc.spans.size() == ids.size(), what);
      for (size_t i = 0; i < sc.spans.size() && i < ids.size(); ++i) {
        CHECK(sc.spans[i].first >= in.p && sc.spans[i].first + sc.spans[i].second <= in.p + in.n, what);
        CHECK(std::string((const char*)sc.spans[i].first, sc.spans[i].second) == ids[i], what);
      }
    }
  }
}

void expect_throw(const std::string& wire, const char* what) {
  HeapCopy in(wire);
  wirecore::DigestScratch& sc = wirecore::digest_scratch();
  for (int mode = 0; mode < 4; ++mode) {
    bool threw = false;
    try {
      wirecore::ScratchGuard guard(sc);
      wirecore::digest_field(sc, in.p, in.n, 1, mode & 1, mode & 2, capture_digest);
    } catch (const std::runtime_error&) {
      threw = true;
    }
    CHECK(threw, what);
  }
}

void run_case(const Ids& ids, const char* what) { expect_ids(encode(ids), ids, what); }

Rng rng{88172645463325252ull};

// n IDs of length L over `alphabet`, in random order (duplicates possible)
Ids random_ids(size_t n, size_t L, const std::string& alphabet) {
  Ids out;
  for (size_t i = 0; i < n; ++i) {
    std::string id(L, ' ');
    for (size_t k = 0; k < L; ++k) id[k] = alphabet[rng() % alphabet.size()];
    out.push_back(id);
  }
  return out;
}

Ids sorted_ids(size_t n, size_t L, const std::string& alphabet) {
  Ids out = random_ids(n, L, alphabet);
  std::sort(out.begin(), out.end(), id_less);
  return out;
}

const std::string kDigits = "0123456789-";

}  // namespace

int main() {
  char what[96];
  const std::vector<std::string> unknown = unknown_kinds();
  std::string all_unknown;
  for (auto& u : unknown) all_unknown += u;

  // sorted runs of every length around the stride limit, every small size;
  // the last entry always ends exactly at the end of the heap block
  for (size_t L = 1; L <= wirecore::kMaxStride + 1; ++L) {
    for (size_t n : {0, 1, 2, 3, 300}) {
      snprintf(what, sizeof what, "sorted L=%zu n=%zu", L, n);
      Ids ids = sorted_ids(n, L, kDigits);
      run_case(ids, what);
      // field 2 (podresources) takes the same path
      expect_ids(encode(ids, 2), ids, what, 2);
      // every entry followed by unknown fields: runs of one
      std::string broken;
      for (auto& id : ids) { put_ld(broken, 1, id); broken += all_unknown; }
      expect_ids(broken, ids, what);
    }
    // out of order at the start, in the middle, as the last entry
    Ids ids = sorted_ids(50, L, kDigits);
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    if (ids.size() >= 4) {
      snprintf(what, sizeof what, "inversion L=%zu", L);
      for (size_t at : {(size_t)0, ids.size() / 2, ids.size() - 2}) {
        Ids bad = ids;
        std::swap(bad[at], bad[at + 1]);
        run_case(bad, what);
      }
      Ids last_first = ids;
      std::rotate(last_first.begin(), last_first.end() - 1, last_first.end());
      run_case(last_first, what);
    }
    // duplicates inside a run
    Ids dup;
    for (auto& id : ids) { dup.push_back(id); dup.push_back(id); dup.push_back(id); }
    snprintf(what, sizeof what, "duplicates L=%zu", L);
    run_case(dup, what);
  }

  // IDs that differ only in their last bytes: for L > 8 the order is decided
  // by the second word alone
  for (size_t L = 4; L <= wirecore::kMaxStride; ++L) {
    Ids ids;
    for (int i = 0; i < 200; ++i) {
      char b[8];
      snprintf(b, sizeof b, "%03d", i);
      ids.push_back(std::string(L - 3, '0') + b);
    }
    snprintf(what, sizeof what, "common prefix L=%zu", L);
    run_case(ids, what);
    for (size_t at : {0, 99, 198}) {
      Ids bad = ids;
      std::swap(bad[at], bad[at + 1]);
      run_case(bad, what);
    }
  }

  // runs that change length in the middle, in byte order
  {
    Ids ids;
    for (int i = 0; i < 40; ++i) { char b[16]; snprintf(b, sizeof b, "10-%04d", i); ids.push_back(b); }
    for (int i = 0; i < 40; ++i) { char b[16]; snprintf(b, sizeof b, "9-%04d", i); ids.push_back(b); }
    for (int i = 0; i < 40; ++i) { char b[32]; snprintf(b, sizeof b, "9-9%03d-and-a-tail", i); ids.push_back(b); }
    run_case(ids, "length changes, sorted");
    std::reverse(ids.begin(), ids.end());
    run_case(ids, "length changes, reversed");
    run_case({"0-1", "0-10", "0-11", "0-2", "0-20"}, "prefix neighbours");
    run_case({"0-10", "0-11", "0-1"}, "shorter prefix after its extensions");
  }

  // a run broken at every position by each thing the generic reader owns
  {
    Ids ids = sorted_ids(12, 6, kDigits);
    std::vector<std::string> breakers = unknown;
    breakers.push_back(all_unknown);
    for (size_t bi = 0; bi < breakers.size(); ++bi)
      for (size_t at = 0; at <= ids.size(); ++at) {
        snprintf(what, sizeof what, "unknown kind %zu at %zu", bi, at);
        expect_ids(encode_with(ids, at, breakers[bi]), ids, what);
      }
    for (size_t at = 0; at <= ids.size(); ++at) {
      // an entry with a two-byte length: an ID of 128+ bytes
      for (char fill : {'!', 'z'}) {
        std::string longid(130, fill), e;
        put_ld(e, 1, longid);
        Ids all = ids;
        all.push_back(longid);
        expect_ids(encode_with(ids, at, e), all, "two-byte length");
      }
      // an entry whose tag is a two-byte varint (0x8A 0x00 = field 1, LEN)
      for (const char* odd : {"0-0000", "zzzzzz", "5"}) {
        std::string e("\x8a\x00", 2);
        put_varint(e, strlen(odd));
        e += odd;
        Ids all = ids;
        all.push_back(odd);
        expect_ids(encode_with(ids, at, e), all, "two-byte tag");
      }
      // an empty ID
      {
        std::string e;
        put_ld(e, 1, "");
        Ids all = ids;
        all.push_back("");
        expect_ids(encode_with(ids, at, e), all, "empty id");
      }
      // a length byte whose entry does not fit: must throw
      expect_throw(encode_with(ids, at, std::string("\x0a\x7f", 2)), "length beyond the range");
    }
  }

  // escaping: every special byte at every offset, one word and two words
  for (size_t L : {1, 3, 7, 8, 9, 12, 16}) {
    const std::string specials[] = {"\"", "\\", std::string(1, '\0'), "\x1f", "\x7f",
                                    "\x20", "\x21", "\x23", "\x5b", "\x5d", "\x80", "\xff",
                                    "\xc3\xa9", "\xe2\x82\xac"};
    for (auto& sp : specials)
      for (size_t off = 0; off + sp.size() <= L; ++off) {
        Ids ids;
        for (char base : {'a', 'b', 'c'}) {
          std::string id(L, base);
          ids.push_back(id);       // clean neighbour
          id.replace(off, sp.size(), sp);
          ids.push_back(id);
        }
        snprintf(what, sizeof what, "escape L=%zu off=%zu byte=%02x", L, off, (unsigned char)sp[0]);
        Ids s = ids;
        std::sort(s.begin(), s.end(), id_less);
        run_case(s, what);                           // the run
        std::reverse(s.begin(), s.end());
        run_case(s, what);                           // the fallback
      }
  }
  run_case(Ids(300, std::string(8, '"')), "every entry escaped, L=8");
  run_case(Ids(300, std::string(16, '\x01')), "every entry escaped, L=16");
  {
    Ids ids(300, std::string(5, '\x02'));
    ids.push_back(std::string(5, '\x01'));
    run_case(ids, "every entry escaped, fallback");
  }

  // every truncation of a small fixed-stride message
  for (size_t L : {1, 2, 5, 7, 8, 9, 16}) {
    Ids ids = sorted_ids(6, L, kDigits);
    std::string msg = encode(ids);
    for (size_t k = 0; k <= msg.size(); ++k) {
      snprintf(what, sizeof what, "cut L=%zu at %zu", L, k);
      if (k % (L + 2) == 0)
        expect_ids(msg.substr(0, k), Ids(ids.begin(), ids.begin() + k / (L + 2)), what);
      else
        expect_throw(msg.substr(0, k), what);
    }
    // the same with the set unsorted, so the fallback's walk sees the cut
    std::reverse(ids.begin(), ids.end());
    msg = encode(ids);
    for (size_t k = 0; k <= msg.size(); ++k) {
      snprintf(what, sizeof what, "cut reversed L=%zu at %zu", L, k);
      if (k % (L + 2) == 0)
        expect_ids(msg.substr(0, k), Ids(ids.begin(), ids.begin() + k / (L + 2)), what);
      else
        expect_throw(msg.substr(0, k), what);
    }
  }

  // shuffled fixed-width sets: the radix fallback (L <= 8) and the span sort
  {
    std::string any;
    for (int c = 0; c < 256; ++c) any.push_back((char)c);
    for (size_t L = 1; L <= 9; ++L)
      for (size_t n : {2, 3, 255, 256, 257, 2000}) {
        snprintf(what, sizeof what, "shuffled L=%zu n=%zu", L, n);
        Ids ids = random_ids(n, L, kDigits);
        run_case(ids, what);
        // key bytes 0x00 and 0xFF, and everything between
        run_case(random_ids(n, L, any), what);
        run_case(random_ids(n, L, std::string("\0\xff", 2)), what);
        // duplicates
        Ids dup = random_ids(n, L, "01");
        run_case(dup, what);
        // unknown fields between the shuffled entries
        std::string broken;
        for (auto& id : ids) { put_ld(broken, 1, id); broken += all_unknown; }
        expect_ids(broken, ids, what);
      }
    Ids big;
    for (int i = 0; i < 18432; ++i) { char b[16]; snprintf(b, sizeof b, "1-%06d", i); big.push_back(b); }
    rng.shuffle(big);
    run_case(big, "18432 shuffled");
    // mixed lengths keep the span sort
    Ids mixed = random_ids(300, 4, kDigits);
    Ids more = random_ids(300, 5, kDigits);
    mixed.insert(mixed.end(), more.begin(), more.end());
    mixed.push_back("");
    rng.shuffle(mixed);
    run_case(mixed, "mixed lengths shuffled");
    Ids last_differs = random_ids(300, 6, kDigits);
    last_differs.push_back("0-00000");
    run_case(last_differs, "one shorter id at the end");
  }

  // several ranges as one set (podresources: IDs in field 2), one ID per
  // range and many per range, sorted and not; each range its own heap block
  for (int shuffled = 0; shuffled < 2; ++shuffled)
    for (size_t per_range : {1, 7}) {
      Ids ids = sorted_ids(70, 4, kDigits);
      if (shuffled) rng.shuffle(ids);
      std::vector<HeapCopy*> blocks;
      std::vector<wirecore::Span> ranges;
      for (size_t i = 0; i < ids.size(); i += per_range) {
        std::string w;
        put_ld(w, 1, "resource-name");
        for (size_t k = i; k < i + per_range; ++k) put_ld(w, 2, ids[k]);
        blocks.push_back(new HeapCopy(w));
        ranges.emplace_back(blocks.back()->p, blocks.back()->n);
      }
      Ids want = ids;
      std::sort(want.begin(), want.end(), id_less);
      std::string joined;
      for (size_t i = 0; i < want.size(); ++i) joined += (i ? ":" : "") + want[i];
      wirecore::DigestScratch& sc = wirecore::digest_scratch();
      for (int mode = 0; mode < 4; ++mode) {
        wirecore::ScratchGuard guard(sc);
        wirecore::DigestOut d = wirecore::digest_ranges(sc, ranges.data(), ranges.size(), 2,
                                                        mode & 1, mode & 2, capture_digest);
        CHECK(d.count == want.size(), "ranges");
        CHECK(last_joined == joined, "ranges");
        if (mode & 1) CHECK(std::string(sc.json.data(), d.json_len) == naive_json(want), "ranges");
        if (mode & 2)
          for (size_t i = 0; i < sc.spans.size() && i < want.size(); ++i)
            CHECK(std::string((const char*)sc.spans[i].first, sc.spans[i].second) == want[i], "ranges");
      }
      for (auto* b : blocks) delete b;
    }

  // a field number whose tag is not one byte takes the generic reader only
  {
    Ids ids = sorted_ids(40, 6, kDigits);
    expect_ids(encode(ids, 16), ids, "field 16", 16);
    std::reverse(ids.begin(), ids.end());
    expect_ids(encode(ids, 16), ids, "field 16 reversed", 16);
  }

  // scratch reuse: a request above the retention cap, then a small one
  {
    Ids huge;
    huge.reserve(300000);
    for (int i = 0; i < 300000; ++i) { char b[16]; snprintf(b, sizeof b, "0-%06d", i); huge.push_back(b); }
    run_case(huge, "300000 sorted");
    run_case({"0-3", "0-1", "0-2"}, "3 after 300000 sorted");
    rng.shuffle(huge);
    run_case(huge, "300000 shuffled");
    wirecore::DigestScratch& sc = wirecore::digest_scratch();
    CHECK(sc.keys.capacity() * sizeof(uint64_t) <= wirecore::kScratchCap, "keys trimmed");
    CHECK(sc.joined.capacity() <= wirecore::kScratchCap, "joined trimmed");
    CHECK(sc.json.capacity() <= wirecore::kScratchCap, "json trimmed");
    run_case({"0-3", "0-1", "0-2"}, "3 after 300000 shuffled");
    run_case({"0-1", "0-2", "0-3"}, "3 sorted after 300000 shuffled");
    run_case({}, "empty after all that");
  }

  // two threads, each with its own scratch
  {
    auto worker = [](char gpu) {
      Ids ids;
      for (int i = 0; i < 3000; ++i) { char b[16]; snprintf(b, sizeof b, "%c-%05d", gpu, i); ids.push_back(b); }
      Ids shuffled = ids;
      std::reverse(shuffled.begin(), shuffled.begin() + 1500);
      for (int rep = 0; rep < 20; ++rep) {
        run_case(ids, "thread sorted");
        run_case(shuffled, "thread shuffled");
      }
    };
    std::thread a(worker, '3'), b(worker, '4');
    a.join();
    b.join();
  }

  if (failures) {
    fprintf(stderr, "digest stride selftest: %d failure(s)\n", failures.load());
    return 1;
  }
  printf("digest stride selftest OK\n");
  return 0;
}
