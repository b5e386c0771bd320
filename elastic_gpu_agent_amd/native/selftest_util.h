// selftest_util.h — what the stand-alone sanitizer self-tests of the digest
// (digest_selftest.cpp, digest_stride_selftest.cpp, runs_selftest.cpp,
// hash_memo_selftest.cpp) and the fuzz harness share: the stand-in hash, the
// wire encoders, and for the self-tests the failure counter, exact-size heap
// blocks, the naive references and a deterministic shuffle. Test scaffolding
// only; nothing here is shipped.
//
// The fuzz harness defines SELFTEST_UTIL_NO_CHECKS before the include and gets
// the hash and the encoders without the failure counter and CHECK.
#pragma once

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace selftest {

typedef std::vector<std::string> Ids;

// stand-in for sha256 (the programs link no crypto library): FNV-1a over
// every byte, so ASan sees a join that ran past its buffer
inline void fnv_digest(const void* data, size_t len, unsigned char md[32]) {
  uint64_t h = 1469598103934665603ull;
  for (size_t i = 0; i < len; ++i) h = (h ^ ((const uint8_t*)data)[i]) * 1099511628211ull;
  for (int i = 0; i < 32; ++i) md[i] = (unsigned char)(h >> (8 * (i & 7)));
}

inline void put_varint(std::string& out, uint64_t v) {
  while (v >= 0x80) {
    out.push_back((char)(v | 0x80));
    v >>= 7;
  }
  out.push_back((char)v);
}

inline void put_ld(std::string& out, uint32_t field, const std::string& payload) {
  put_varint(out, field << 3 | 2);
  put_varint(out, payload.size());
  out += payload;
}

// the IDs as LEN entries of `field`, each followed by `between`
inline std::string encode(const Ids& ids, uint32_t field = 1, const std::string& between = "") {
  std::string out;
  for (auto& id : ids) {
    put_ld(out, field, id);
    out += between;
  }
  return out;
}

#ifndef SELFTEST_UTIL_NO_CHECKS

inline std::atomic<int> failures{0};  // some cases run several threads

#define CHECK(cond, what)                                                       \
  do {                                                                          \
    if (!(cond)) {                                                              \
      fprintf(stderr, "FAIL %s:%d %s (%s)\n", __FILE__, __LINE__, #cond, what); \
      ++selftest::failures;                                                     \
    }                                                                           \
  } while (0)

// the "hash" keeps the joined bytes so two paths can be compared exactly
inline thread_local std::string last_joined;
inline void capture_digest(const void* data, size_t len, unsigned char md[32]) {
  last_joined.assign((const char*)data, len);
  fnv_digest(data, len, md);
}

struct HeapCopy {  // exact-size block: one byte past the end is poisoned
  uint8_t* p;
  size_t n;
  explicit HeapCopy(const std::string& s) : p((uint8_t*)malloc(s.size() ? s.size() : 1)), n(s.size()) {
    memcpy(p, s.data(), s.size());
  }
  HeapCopy(const HeapCopy&) = delete;
  ~HeapCopy() { free(p); }
};

inline bool id_less(const std::string& a, const std::string& b) {  // byte-wise, unsigned
  size_t m = std::min(a.size(), b.size());
  int c = m ? memcmp(a.data(), b.data(), m) : 0;
  return c ? c < 0 : a.size() < b.size();
}

// json.dumps(sorted, separators=(",", ":")) for byte strings
inline std::string naive_json(const Ids& sorted) {
  std::string j = "[";
  for (size_t i = 0; i < sorted.size(); ++i) {
    if (i) j += ",";
    j += "\"";
    for (unsigned char c : sorted[i]) {
      if (c == '"' || c == '\\') { j += '\\'; j += (char)c; }
      else if (c < 0x20) { char e[8]; snprintf(e, sizeof e, "\\u%04x", c); j += e; }
      else j += (char)c;
    }
    j += "\"";
  }
  return j + "]";
}

struct Rng {  // xorshift: deterministic
  uint64_t state;
  uint64_t operator()() {
    state ^= state << 13;
    state ^= state >> 7;
    state ^= state << 17;
    return state;
  }
  void shuffle(Ids& v) {
    for (size_t i = v.size(); i > 1; --i) std::swap(v[i - 1], v[(*this)() % i]);
  }
};

#endif  // SELFTEST_UTIL_NO_CHECKS

}  // namespace selftest
