// wirecore.h — protobuf wire-walking core shared by _fastwire and the
// standalone fuzz targets. Header-only; extracted verbatim from
// fastwire.cpp so fuzzing covers exactly the shipped parser.
#pragma once

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <iterator>
#include <list>
#include <mutex>
#include <stdexcept>
#include <string>
#include <string_view>
#include <unordered_map>
#include <utility>
#include <vector>

namespace wirecore {

struct Reader {
  const uint8_t* p;
  const uint8_t* end;

  bool done() const { return p >= end; }

  uint64_t varint() {
    // one-byte varints (tags, short lengths) are nearly all of them
    if (p < end && !(*p & 0x80)) return *p++;
    uint64_t result = 0;
    int shift = 0;
    while (p < end) {
      uint8_t b = *p++;
      result |= (uint64_t)(b & 0x7F) << shift;
      if (!(b & 0x80)) return result;
      shift += 7;
      if (shift >= 70) throw std::runtime_error("varint too long");
    }
    throw std::runtime_error("truncated varint");
  }

  void skip(uint32_t wire) {
    switch (wire) {
      case 0:
        varint();
        break;
      case 1:
        p += 8;
        break;
      case 2: {
        uint64_t n = varint();
        // compare against the REMAINING size: `p += n` with an attacker-
        // controlled 64-bit n can wrap the pointer past the `p > end`
        // check below (found by the libFuzzer harness: OOB read SEGV)
        if (n > (uint64_t)(end - p)) throw std::runtime_error("truncated field");
        p += n;
        break;
      }
      case 5:
        p += 4;
        break;
      default:
        throw std::runtime_error("bad wire type");
    }
    if (p > end) throw std::runtime_error("truncated field");
  }
};

// collect every field-1 LEN payload within [p, end)
inline void field1_spans(const uint8_t* p, const uint8_t* end,
                  std::vector<std::pair<const uint8_t*, size_t>>& out) {
  Reader r{p, end};
  while (!r.done()) {
    uint64_t tag = r.varint();
    uint32_t field = tag >> 3, wire = tag & 7;
    if (field == 1 && wire == 2) {
      uint64_t n = r.varint();
      if (n > (uint64_t)(r.end - r.p)) throw std::runtime_error("truncated");
      out.emplace_back(r.p, (size_t)n);
      r.p += n;
    } else {
      r.skip(wire);
    }
  }
}


// collect every field-N LEN payload within [p, end)
inline void spanN(const uint8_t* p, const uint8_t* end, uint32_t want,
                  std::vector<std::pair<const uint8_t*, size_t>>& out) {
  Reader r{p, end};
  while (!r.done()) {
    uint64_t tag = r.varint();
    uint32_t field = tag >> 3, wire = tag & 7;
    if (field == want && wire == 2) {
      uint64_t n = r.varint();
      if (n > (uint64_t)(r.end - r.p)) throw std::runtime_error("truncated");
      out.emplace_back(r.p, (size_t)n);
      r.p += n;
    } else {
      r.skip(wire);
    }
  }
}

// ---- fused device-set digest -----------------------------------------------
// hash = sha256(":".join(sorted ids))[:8]  (types.hash_device_ids). One pass
// over the field-`want` LEN entries of [p, end): walk the varints, compare
// each ID with its predecessor and write the ':'-joined bytes straight into
// one pre-sized buffer (the joined length never exceeds the input length: an
// entry costs tag + length varint >= 2 bytes on the wire and at most 1
// separator byte joined). Kubelet builds its ID lists from Go sets, so
// unsorted input is the production case: the pass then falls back to
// collect + sort + join with byte-wise, shorter-prefix-first ordering.
//
// Fixed-stride runs. The IDs of one resource have one width ("%d-%06d",
// "%d-%02d"), so a request is a long run of entries that share the one-byte
// tag and a one-byte length L <= kMaxStride. Where the reader stands on such
// a two-byte header the walk handles the maximal run of entries with that
// same header at stride L + 2 in a tight loop (DigestWriter::run): the
// predecessor compare is on big-endian words (one for L <= 8, two
// overlapping ones above), the room for the whole run is checked once, the
// joined bytes and the JSON literal are stored as whole words, and the bytes
// json.dumps escapes ('"', '\\', < 0x20) are found with a word-at-a-time
// test; an entry that has one goes through json_put_string. A run ends at the
// first byte that is not that header, or where a whole entry no longer fits
// in the range, and the generic reader carries on from there, so multi-byte
// tags or lengths, empty IDs, other fields and truncated entries are parsed,
// and rejected, by the generic code alone.
//
// Radix fallback. When the unsorted set has one length L <= 8 (and the caller
// does not want spans into the input), the IDs are loaded as left-aligned
// big-endian uint64 keys and sorted with an LSD byte radix sort that skips
// the byte positions at which all keys agree; the output is written from the
// keys. Unsigned order of the words is byte-wise order of the strings. Mixed
// lengths, L > 8 and want_spans keep the span sort.
//
// The scratch buffers are thread_local and reused, so a warm thread does not
// allocate; every call resets their lengths on entry, and capacity above
// kScratchCap is released on exit so one 295k-ID request does not pin
// megabytes per thread forever.
//
// The caller supplies the hash (sha256 over a buffer → 32 bytes) so this
// header keeps no dependency beyond the standard library.

using Span = std::pair<const uint8_t*, size_t>;
using Sha256Fn = void (*)(const void* data, size_t len, unsigned char md[32]);

constexpr size_t kScratchCap = 4u << 20;  // bytes retained per buffer
constexpr size_t kMaxStride = 16;         // longest ID the fixed-stride run takes
// whole-word stores may run up to 7 bytes past an ID; the buffers keep room
constexpr size_t kWordSlack = 8;

// 8 bytes loaded from memory -> integer whose top byte is the first byte
// in memory (its own inverse)
inline uint64_t word_to_be(uint64_t raw) {
#if defined(__BYTE_ORDER__) && __BYTE_ORDER__ == __ORDER_BIG_ENDIAN__
  return raw;
#else
  return __builtin_bswap64(raw);
#endif
}

// the first n <= 8 bytes at p, left-aligned big-endian, low bytes zero;
// reads exactly n bytes
inline uint64_t be_key_bytes(const uint8_t* p, size_t n) {
  uint64_t k = 0;
  for (size_t i = 0; i < n; ++i) k |= (uint64_t)p[i] << (56 - 8 * i);
  return k;
}

// true when any byte of w is '"', '\\' or < 0x20 (what json.dumps escapes);
// bytes >= 0x80 never match
inline bool word_needs_escape(uint64_t w) {
  const uint64_t k01 = 0x0101010101010101ull, k80 = 0x8080808080808080ull;
  uint64_t lt = (w - k01 * 0x20) & ~w;
  uint64_t q = w ^ (k01 * 0x22), b = w ^ (k01 * 0x5c);
  return ((lt | ((q - k01) & ~q) | ((b - k01) & ~b)) & k80) != 0;
}

// LSD byte radix sort of a[0..n) with b[0..n) as the second buffer; byte
// positions at which all keys agree are skipped. Returns the sorted buffer.
inline uint64_t* radix_sort_keys(uint64_t* a, uint64_t* b, size_t n) {
  uint64_t diff = 0;
  for (size_t i = 1; i < n; ++i) diff |= a[i] ^ a[0];
  for (int shift = 0; shift < 64; shift += 8) {
    if (!((diff >> shift) & 0xFF)) continue;
    size_t cnt[256] = {0};
    for (size_t i = 0; i < n; ++i) ++cnt[(a[i] >> shift) & 0xFF];
    size_t sum = 0;
    for (int c = 0; c < 256; ++c) {
      size_t t = cnt[c];
      cnt[c] = sum;
      sum += t;
    }
    for (size_t i = 0; i < n; ++i) b[cnt[(a[i] >> shift) & 0xFF]++] = a[i];
    std::swap(a, b);
  }
  return a;
}

inline bool span_less(const Span& a, const Span& b) {
  size_t m = a.second < b.second ? a.second : b.second;
  int c = m ? memcmp(a.first, b.first, m) : 0;
  if (c) return c < 0;
  return a.second < b.second;
}

// ---- ID runs ----------------------------------------------------------------
// The IDs of a resource are "<gpu>-<zero-padded index>", and kubelet hands out
// mostly consecutive ones, so a large sorted set is a handful of runs. The
// store keeps such a set as [[prefix, width, start, count], ...] (200 KB of
// literal list become ~20 bytes); the literal list stays the exchange format
// and expand_runs rebuilds it byte for byte.
//
// An ID is run-encodable when it ends in a maximal run of 1..18 ASCII digits
// (so the value fits a uint64) and holds no byte json.dumps would escape
// ('"', '\\', < 0x20, >= 0x80). Over the sorted set an ID with the prefix and
// width of its predecessor and value == previous + 1 extends the run; anything
// else (a duplicate, 9 -> 10, another prefix) starts one. A set is stored as
// runs only when every ID is run-encodable, it has >= kRunsMinIds IDs and at
// most count / kRunsPerIds runs: small sets keep their literal bytes and a
// fragmented set never grows.

constexpr size_t kRunsMinIds = 1024;
constexpr size_t kRunsPerIds = 8;
constexpr size_t kRunsMaxWidth = 18;

struct IdRun {
  size_t prefix_off, prefix_len;  // into RunBuilder::prefixes
  unsigned width;
  uint64_t start, count;
};

// Fed the sorted IDs one by one. The expected successor is kept as text, so
// an ID that extends the run costs one compare and an ASCII increment. The
// digest's word-at-a-time loops see "previous ID + 1 in the last digit" and
// "previous ID + 1 with one carry (x9 -> y0)" on the words they already hold
// and only report how many such IDs went by and the last of them (extend), so
// 99 of 100 consecutive IDs never reach add.
struct RunBuilder {
  std::vector<IdRun> runs;
  std::string prefixes;
  std::string next;  // the ID that would extend the last run
  bool has_next = false;
  bool ok = true;    // every ID so far is run-encodable, runs within max_runs
  size_t n = 0;
  size_t max_runs = 0;

  void reset(size_t run_cap) {
    runs.clear();
    prefixes.clear();
    has_next = false;
    ok = true;
    n = 0;
    max_runs = run_cap;
  }

  // `next` += 1 in its last `width` bytes; no successor at 99..9
  void advance() {
    const size_t w = runs.back().width;
    size_t i = next.size();
    for (size_t k = 0; k < w; ++k) {
      char& c = next[--i];
      if (c != '9') {
        ++c;
        return;
      }
      c = '0';
    }
    has_next = false;
  }

  // the last run grew by k IDs, each the decimal successor of the one before
  // it within the run's digits, the first of them being `next`; `last` is
  // the k-th
  void extend(size_t k, const uint8_t* last, size_t len) {
    if (!k || !ok || !has_next) return;
    runs.back().count += k;
    n += k;
    next.assign((const char*)last, len);
    advance();
  }

  void add(const uint8_t* id, size_t len) {
    if (!ok) return;
    ++n;
    if (has_next && len == next.size() && memcmp(id, next.data(), len) == 0) {
      ++runs.back().count;
      advance();
      return;
    }
    size_t w = 0;
    while (w < len && (unsigned)(id[len - 1 - w] - '0') < 10) ++w;
    if (w == 0 || w > kRunsMaxWidth || runs.size() >= max_runs) {
      ok = false;
      return;
    }
    const size_t plen = len - w;
    for (size_t i = 0; i < plen; ++i) {
      const uint8_t c = id[i];
      if (c < 0x20 || c >= 0x80 || c == '"' || c == '\\') {
        ok = false;
        return;
      }
    }
    uint64_t v = 0;
    for (size_t i = plen; i < len; ++i) v = v * 10 + (id[i] - '0');
    IdRun r;
    r.prefix_len = plen;
    r.width = (unsigned)w;
    r.start = v;
    r.count = 1;
    if (!runs.empty() && runs.back().prefix_len == plen &&
        memcmp(prefixes.data() + runs.back().prefix_off, id, plen) == 0) {
      r.prefix_off = runs.back().prefix_off;
    } else {
      r.prefix_off = prefixes.size();
      prefixes.append((const char*)id, plen);
    }
    runs.push_back(r);
    next.assign((const char*)id, len);
    has_next = true;
    advance();
  }

  bool qualifies() const {
    return ok && n >= kRunsMinIds && runs.size() * kRunsPerIds <= n;
  }

  // compact JSON: [["0-",6,0,18432]]
  void to_json(std::string& out) const {
    out.clear();
    out.push_back('[');
    char num[24];
    for (size_t i = 0; i < runs.size(); ++i) {
      const IdRun& r = runs[i];
      if (i) out.push_back(',');
      out.append("[\"");
      out.append(prefixes, r.prefix_off, r.prefix_len);
      out.append("\",");
      const uint64_t f[3] = {r.width, r.start, r.count};
      for (int k = 0; k < 3; ++k) {
        char* e = num + sizeof num;
        uint64_t v = f[k];
        do {
          *--e = (char)('0' + v % 10);
          v /= 10;
        } while (v);
        out.append(e, num + sizeof num - e);
        out.push_back(k < 2 ? ',' : ']');
      }
    }
    out.push_back(']');
  }
};

// The strings are used as raw storage: size() is the high-water mark of what
// was ever needed (so growing zero-fills only new bytes), and each call
// tracks its own used lengths locally. Bytes past those lengths are stale
// and never read.
struct DigestScratch {
  std::string joined;
  std::string json;
  std::vector<Span> spans;
  std::vector<uint64_t> keys;  // radix fallback: n keys + n for the passes
  RunBuilder runs;             // digest_field_runs and the two memo digests

  void trim() {
    if (joined.capacity() > kScratchCap) std::string().swap(joined);
    if (json.capacity() > kScratchCap) std::string().swap(json);
    if (spans.capacity() * sizeof(Span) > kScratchCap) std::vector<Span>().swap(spans);
    if (keys.capacity() * sizeof(uint64_t) > kScratchCap) std::vector<uint64_t>().swap(keys);
    if (runs.runs.capacity() * sizeof(IdRun) > kScratchCap) std::vector<IdRun>().swap(runs.runs);
    if (runs.prefixes.capacity() > kScratchCap) std::string().swap(runs.prefixes);
    if (runs.next.capacity() > kScratchCap) std::string().swap(runs.next);
  }
};

inline DigestScratch& digest_scratch() {
  static thread_local DigestScratch s;
  return s;
}

// releases oversized scratch on every exit path (exceptions included)
struct ScratchGuard {
  DigestScratch& s;
  explicit ScratchGuard(DigestScratch& sc) : s(sc) { s.spans.clear(); }
  ~ScratchGuard() { s.trim(); }
};

// json.dumps-equivalent string literal for an ID, written at `out`, which
// must have room for 6 * n + 2 bytes (every byte escaped as \u00XX plus the
// quotes). Bytes >= 0x20 other than '"' and '\\' are copied as they are.
inline char* json_put_string(char* out, const uint8_t* sp, size_t n) {
  *out++ = '"';
  size_t j = 0;
  while (j < n) {
    size_t run = j;
    while (run < n) {
      uint8_t c = sp[run];
      if (c == '"' || c == '\\' || c < 0x20) break;
      ++run;
    }
    memcpy(out, sp + j, run - j);  // bulk copy of the clean run
    out += run - j;
    j = run;
    if (j < n) {
      uint8_t c = sp[j++];
      if (c == '"' || c == '\\') {
        *out++ = '\\';
        *out++ = (char)c;
      } else {
        static const char kHex[] = "0123456789abcdef";
        *out++ = '\\';
        *out++ = 'u';
        *out++ = '0';
        *out++ = '0';
        *out++ = kHex[c >> 4];
        *out++ = kHex[c & 15];
      }
    }
  }
  *out++ = '"';
  return out;
}

struct DigestOut {
  char hex[9];
  size_t count;
  size_t json_len;    // bytes of scratch.json holding the fragment
  size_t joined_len;  // bytes of scratch.joined holding the ':'-joined IDs
};

// the first 8 hex characters of sha(data[0, len)), NUL-terminated
inline void hash_hex8(Sha256Fn sha, const void* data, size_t len, char hex[9]) {
  unsigned char md[32];
  sha(data, len, md);
  static const char kHex[] = "0123456789abcdef";
  for (int i = 0; i < 4; ++i) {
    hex[2 * i] = kHex[md[i] >> 4];
    hex[2 * i + 1] = kHex[md[i] & 15];
  }
  hex[8] = 0;
}

// writer over the two scratch strings; keeps its cursors in locals
struct DigestWriter {
  DigestScratch& s;
  bool want_json;
  RunBuilder* rb;     // also split the IDs into runs (may be null)
  char *jo, *jo_end;  // joined cursor / end of storage
  char *js, *js_end;  // json cursor / end of storage

  DigestWriter(DigestScratch& sc, size_t in_bytes, bool json, RunBuilder* runs = nullptr)
      : s(sc), want_json(json), rb(runs) {
    // the joined bytes never outgrow the input: an entry takes >= 2 wire
    // bytes beyond its payload and <= 1 separator byte joined
    if (s.joined.size() < in_bytes + 1 + kWordSlack) s.joined.resize(in_bytes + 1 + kWordSlack);
    jo = &s.joined[0];
    jo_end = jo + s.joined.size();
    js = js_end = nullptr;
    if (want_json) {
      // '[' + per ID two quotes and a comma (n + 3 <= 1.5 * (n + 2)) + ']';
      // IDs holding quotes or control bytes can need more: json_room grows
      size_t est = in_bytes + in_bytes / 2 + 16 + kWordSlack;
      if (s.json.size() < est) s.json.resize(est);
      js = &s.json[0];
      js_end = js + s.json.size();
    }
    restart();
  }

  void restart() {
    jo = &s.joined[0];
    if (rb) rb->reset(rb->max_runs);
    if (want_json) {
      js = &s.json[0];
      *js++ = '[';
    }
  }

  void json_room(size_t need) {
    if ((size_t)(js_end - js) >= need) return;
    size_t used = js - &s.json[0];
    s.json.resize(std::max(s.json.size() * 2, used + need));
    js = &s.json[0] + used;
    js_end = &s.json[0] + s.json.size();
  }

  // The cursors are copied into locals around the stores: a store through a
  // char* may alias the members, which would then be reloaded after each.
  void put(const Span& id, bool first) {
    const size_t n = id.second;
    char* j = jo;
    if ((size_t)(jo_end - j) < n + 1) throw std::runtime_error("digest overflow");
    if (!first) *j++ = ':';
    memcpy(j, id.first, n);
    jo = j + n;
    if (rb) rb->add(id.first, n);
    if (want_json) {
      json_room(6 * n + 4);  // literal + comma + closing bracket
      char* q = js;
      if (!first) *q++ = ',';
      js = json_put_string(q, id.first, n);
    }
  }

  // Fixed-stride run: the entries at r.p that all start with the two bytes
  // (tagbyte, L), 1 <= L <= kMaxStride, each wholly inside the range. The
  // caller has already put the run's first entry, `prev`, so every entry
  // here is preceded by a separator. Stops at the first byte that is not
  // such an entry and leaves r.p there; `prev` and `count` follow. Returns
  // false at an entry smaller than its predecessor.
  bool run(Reader& r, uint8_t tagbyte, size_t L, Span& prev, size_t& count,
           std::vector<Span>* spans) {
    const size_t stride = L + 2;
    const uint8_t* p = r.p;
    const uint8_t* const end = r.end;
    const size_t maxn = (size_t)(end - p) / stride;
    if (maxn == 0 || p[0] != tagbyte || p[1] != L) return true;
    // room for the whole run, once: per entry a separator and L bytes
    // (joined), a comma, two quotes and L bytes (JSON), plus the word slack
    if ((size_t)(jo_end - jo) < maxn * (L + 1) + kWordSlack)
      throw std::runtime_error("digest overflow");
    if (want_json) json_room(maxn * (L + 3) + 1 + kWordSlack);
    char* j = jo;
    char* q = js;
    const bool json = want_json;
    const uint8_t* last = nullptr;
    size_t n = 0;
    bool in_order = true;
    // runs: an entry that is its predecessor with the last digit one higher
    // is only counted; every other one goes through RunBuilder::add
    RunBuilder* rbl = rb && rb->ok ? rb : nullptr;
    size_t matched = 0;
    if (L <= 8) {
      const int sh = 64 - 8 * (int)L;
      const uint64_t unit = 1ull << sh;
      // x9 -> y0 in the last two bytes: + 256 units - 9 units
      const uint64_t carry = 247 * unit;
      const int sh1 = L >= 2 ? sh + 8 : sh;  // the digit before the last
      const uint64_t mask = ~0ull << (64 - 8 * L);
      // the bytes past the ID must not look like bytes to escape
      const uint64_t pad = ~mask & 0x3030303030303030ull;
      uint64_t pk = be_key_bytes(prev.first, L);
      while ((size_t)(end - p) >= stride && p[0] == tagbyte && p[1] == L) {
        const uint8_t* pay = p + 2;
        uint64_t raw = 0;
        if ((size_t)(end - pay) >= 8)
          memcpy(&raw, pay, 8);
        else
          memcpy(&raw, pay, L);  // the last entries of a range: L bytes only
        const uint64_t key = word_to_be(raw) & mask;
        if (key < pk) {
          in_order = false;
          break;
        }
        if (rbl) {
          const uint64_t d = key - pk;
          const unsigned d0 = (unsigned)((pk >> sh) & 0xFF) - '0';
          if ((d == unit && d0 < 9) ||
              (d == carry && d0 == 9 && L >= 2 &&
               (unsigned)(((pk >> sh1) & 0xFF) - '0') < 9)) {
            ++matched;
          } else {
            rbl->extend(matched, last, L);
            matched = 0;
            rbl->add(pay, L);
            if (!rbl->ok) rbl = nullptr;
          }
        }
        pk = key;
        *j = ':';
        memcpy(j + 1, &raw, 8);
        j += L + 1;
        if (json) {
          if (word_needs_escape(key | pad)) {
            js = q;
            json_room(6 * L + 4 + ((size_t)(end - p) / stride) * (L + 3) + kWordSlack);
            q = js;
            *q++ = ',';
            q = json_put_string(q, pay, L);
          } else {
            q[0] = ',';
            q[1] = '"';
            memcpy(q + 2, &raw, 8);
            q[L + 2] = '"';
            q += L + 3;
          }
        }
        if (spans) spans->emplace_back(pay, L);
        last = pay;
        ++n;
        p += stride;
      }
    } else {
      // two overlapping words: the first 8 bytes, then the last 8
      const size_t off = L - 8;
      uint64_t raw;
      memcpy(&raw, prev.first, 8);
      uint64_t ph = word_to_be(raw);
      memcpy(&raw, prev.first + off, 8);
      uint64_t pl = word_to_be(raw);
      while ((size_t)(end - p) >= stride && p[0] == tagbyte && p[1] == L) {
        const uint8_t* pay = p + 2;
        uint64_t rh, rl;
        memcpy(&rh, pay, 8);
        memcpy(&rl, pay + off, 8);
        const uint64_t kh = word_to_be(rh), kl = word_to_be(rl);
        if (kh < ph || (kh == ph && kl < pl)) {
          in_order = false;
          break;
        }
        if (rbl) {
          const uint64_t d = kl - pl;
          const unsigned d0 = (unsigned)(pl & 0xFF) - '0';
          if (kh == ph && ((d == 1 && d0 < 9) ||
                           (d == 247 && d0 == 9 &&
                            (unsigned)(((pl >> 8) & 0xFF) - '0') < 9))) {
            ++matched;
          } else {
            rbl->extend(matched, last, L);
            matched = 0;
            rbl->add(pay, L);
            if (!rbl->ok) rbl = nullptr;
          }
        }
        ph = kh;
        pl = kl;
        *j = ':';
        memcpy(j + 1, &rh, 8);
        memcpy(j + 1 + off, &rl, 8);
        j += L + 1;
        if (json) {
          if (word_needs_escape(kh) || word_needs_escape(kl)) {
            js = q;
            json_room(6 * L + 4 + ((size_t)(end - p) / stride) * (L + 3) + kWordSlack);
            q = js;
            *q++ = ',';
            q = json_put_string(q, pay, L);
          } else {
            q[0] = ',';
            q[1] = '"';
            memcpy(q + 2, &rh, 8);
            memcpy(q + 2 + off, &rl, 8);
            q[L + 2] = '"';
            q += L + 3;
          }
        }
        if (spans) spans->emplace_back(pay, L);
        last = pay;
        ++n;
        p += stride;
      }
    }
    if (rbl) rbl->extend(matched, last, L);
    jo = j;
    js = q;
    r.p = p;
    count += n;
    if (last) prev = Span{last, L};
    return in_order;
  }

  // Radix fallback output: the n sorted left-aligned big-endian keys of IDs
  // of length 1 <= L <= 8, written after restart().
  void put_keys(const uint64_t* keys, size_t n, size_t L) {
    if ((size_t)(jo_end - jo) < n * (L + 1) + kWordSlack)
      throw std::runtime_error("digest overflow");
    if (want_json) json_room(n * (L + 3) + 1 + kWordSlack);
    char* j = jo;
    char* q = js;
    const uint64_t pad = L == 8 ? 0 : (0x3030303030303030ull >> (8 * L));
    RunBuilder* rbl = rb && rb->ok ? rb : nullptr;
    size_t matched = 0;
    const int sh = 64 - 8 * (int)L;
    const uint64_t unit = 1ull << sh;
    const uint64_t carry = 247 * unit;  // x9 -> y0, as in run()
    const int sh1 = L >= 2 ? sh + 8 : sh;
    uint8_t id[8];  // the previous key's bytes, when IDs went by uncounted
    for (size_t i = 0; i < n; ++i) {
      const uint64_t key = keys[i];
      const uint64_t raw = word_to_be(key);
      if (i) *j++ = ':';
      memcpy(j, &raw, 8);
      j += L;
      if (rbl) {
        const uint64_t pk = i ? keys[i - 1] : 0;
        const uint64_t d = key - pk;
        const unsigned d0 = (unsigned)((pk >> sh) & 0xFF) - '0';
        if (i && ((d == unit && d0 < 9) ||
                  (d == carry && d0 == 9 && L >= 2 &&
                   (unsigned)(((pk >> sh1) & 0xFF) - '0') < 9))) {
          ++matched;
        } else {
          if (matched) {
            const uint64_t praw = word_to_be(pk);
            memcpy(id, &praw, 8);
            rbl->extend(matched, id, L);
            matched = 0;
          }
          memcpy(id, &raw, 8);
          rbl->add(id, L);
          if (!rbl->ok) rbl = nullptr;
        }
      }
      if (want_json) {
        if (i) *q++ = ',';
        if (word_needs_escape(key | pad)) {
          uint8_t id[8];
          memcpy(id, &raw, 8);
          js = q;
          json_room(6 * L + 4 + (n - i) * (L + 3) + kWordSlack);
          q = json_put_string(js, id, L);
        } else {
          q[0] = '"';
          memcpy(q + 1, &raw, 8);
          q[L + 1] = '"';
          q += L + 2;
        }
      }
    }
    if (rbl && matched) {
      const uint64_t praw = word_to_be(keys[n - 1]);
      memcpy(id, &praw, 8);
      rbl->extend(matched, id, L);
    }
    jo = j;
    js = q;
  }

  // a null `sha` leaves the hash out (hex stays empty)
  DigestOut finish(size_t count, Sha256Fn sha) {
    DigestOut out;
    out.json_len = 0;
    if (want_json) {
      json_room(1);
      *js++ = ']';
      out.json_len = js - &s.json[0];
    }
    out.hex[0] = 0;
    out.count = count;
    out.joined_len = jo - &s.joined[0];
    if (sha) hash_hex8(sha, s.joined.data(), out.joined_len, out.hex);
    return out;
  }
};

// Digest of the field-`want` LEN entries of every range in
// ranges[0..nranges), taken as one ID set. `want_json` also builds the JSON
// array fragment of the sorted IDs into scratch.json[0, json_len);
// `want_spans` leaves the sorted spans in scratch.spans. Results in the
// scratch stay valid until the next digest on this thread; the caller owns
// the ScratchGuard.
inline DigestOut digest_ranges(DigestScratch& s, const Span* ranges, size_t nranges,
                               uint32_t want, bool want_json, bool want_spans,
                               Sha256Fn sha, RunBuilder* runs = nullptr) {
  size_t in_bytes = 0;
  for (size_t i = 0; i < nranges; ++i) in_bytes += ranges[i].second;
  DigestWriter w(s, in_bytes, want_json, runs);
  bool sorted = true, have_prev = false;
  Span prev{nullptr, 0};
  size_t count = 0;
  // the fixed-stride run needs the tag to be one byte
  const bool stride_ok = want < 16;
  const uint8_t tagbyte = (uint8_t)((want << 3) | 2);
  std::vector<Span>* const run_spans = want_spans ? &s.spans : nullptr;
  for (size_t ri = 0; ri < nranges && sorted; ++ri) {
    Reader r{ranges[ri].first, ranges[ri].first + ranges[ri].second};
    while (!r.done()) {
      if (stride_ok && (size_t)(r.end - r.p) >= 3 && r.p[0] == tagbyte) {
        const size_t L = r.p[1];
        if (L - 1 < kMaxStride && (size_t)(r.end - r.p) >= L + 2) {
          // the run's first entry meets a predecessor of any length
          Span cur{r.p + 2, L};
          if (have_prev && span_less(cur, prev)) {
            sorted = false;
            break;
          }
          w.put(cur, !have_prev);
          if (want_spans) s.spans.push_back(cur);
          r.p += L + 2;
          prev = cur;
          have_prev = true;
          ++count;
          if (!w.run(r, tagbyte, L, prev, count, run_spans)) {
            sorted = false;
            break;
          }
          continue;
        }
      }
      uint64_t tag = r.varint();
      uint32_t field = tag >> 3, wire = tag & 7;
      if (field == want && wire == 2) {
        uint64_t n = r.varint();
        if (n > (uint64_t)(r.end - r.p)) throw std::runtime_error("truncated");
        Span cur{r.p, (size_t)n};
        r.p += n;
        if (have_prev && span_less(cur, prev)) {
          sorted = false;
          break;
        }
        w.put(cur, !have_prev);
        if (want_spans) s.spans.push_back(cur);
        prev = cur;
        have_prev = true;
        ++count;
      } else {
        r.skip(wire);
      }
    }
  }
  if (!sorted) {
    // unsorted: collect every span (re-walking from the start keeps every
    // bounds check of the walk), sort byte-wise shorter-prefix-first, join
    s.spans.clear();
    for (size_t ri = 0; ri < nranges; ++ri)
      spanN(ranges[ri].first, ranges[ri].first + ranges[ri].second, want, s.spans);
    count = s.spans.size();
    w.restart();
    // one length 1 <= L <= 8 throughout: sort big-endian words, not spans
    size_t L = count && !want_spans ? s.spans[0].second : 0;
    if (L > 8) L = 0;
    for (size_t i = 1; i < count && L; ++i)
      if (s.spans[i].second != L) L = 0;
    if (L) {
      if (s.keys.size() < 2 * count) s.keys.resize(2 * count);
      uint64_t* keys = s.keys.data();
      // spans come in range order; a whole-word load must stay in its range
      size_t i = 0;
      for (size_t ri = 0; ri < nranges && i < count; ++ri) {
        const uint8_t* lo = ranges[ri].first;
        const uint8_t* hi = lo + ranges[ri].second;
        const uint64_t mask = ~0ull << (64 - 8 * L);
        for (; i < count; ++i) {
          const uint8_t* id = s.spans[i].first;
          if (id < lo || id >= hi) break;
          if ((size_t)(hi - id) >= 8) {
            uint64_t raw;
            memcpy(&raw, id, 8);
            keys[i] = word_to_be(raw) & mask;
          } else {
            keys[i] = be_key_bytes(id, L);
          }
        }
      }
      for (; i < count; ++i) keys[i] = be_key_bytes(s.spans[i].first, L);
      w.put_keys(radix_sort_keys(keys, keys + count, count), count, L);
    } else {
      // a lambda, not the function's address: std::sort inlines the compare
      std::sort(s.spans.begin(), s.spans.end(),
                [](const Span& a, const Span& b) { return span_less(a, b); });
      for (size_t i = 0; i < count; ++i) w.put(s.spans[i], i == 0);
    }
  }
  return w.finish(count, sha);
}

inline DigestOut digest_field(DigestScratch& s, const uint8_t* p, size_t len,
                              uint32_t want, bool want_json, bool want_spans,
                              Sha256Fn sha) {
  Span range{p, len};
  return digest_ranges(s, &range, 1, want, want_json, want_spans, sha);
}

// digest_field for a caller that stores runs: scratch.json[0, json_len) holds
// the runs fragment and *is_runs is set when the set qualifies, the literal
// list fragment otherwise. A set that qualifies never has its literal list
// built. One that is large enough to try and then does not qualify (an ID
// that is not run-encodable, too many runs) is walked a second time for the
// list, without hashing again.
inline DigestOut digest_field_runs(DigestScratch& s, const uint8_t* p, size_t len,
                                   uint32_t want, Sha256Fn sha, bool* is_runs) {
  *is_runs = false;
  // an entry takes >= 3 wire bytes (tag, length, one digit)
  if (len < 3 * kRunsMinIds) return digest_field(s, p, len, want, true, false, sha);
  Span range{p, len};
  s.runs.reset(len / (3 * kRunsPerIds));
  DigestOut d = digest_ranges(s, &range, 1, want, false, false, sha, &s.runs);
  if (s.runs.qualifies() && s.runs.n == d.count) {
    s.runs.to_json(s.json);
    d.json_len = s.json.size();
    *is_runs = true;
    return d;
  }
  DigestOut l = digest_ranges(s, &range, 1, want, true, false, nullptr);
  d.json_len = l.json_len;
  return d;
}

// ---- hash memo ----------------------------------------------------------------
// Allocate and PreStart hash the same device set moments apart. For a set
// that qualifies as runs, the runs fragment is an exact name of the sorted
// list (expand_runs rebuilds it byte for byte), so equal fragments mean equal
// joined bytes and equal hashes: Allocate leaves fragment -> hash here and
// PreStart takes it instead of hashing again. A hit removes the entry, so
// every skipped hash stands for one hash Allocate really computed.
//
// Bounds: at most `cap` entries (kMemoEntries by default, 0 = off), keys of
// at most kMemoMaxKey bytes (a longer fragment is not stored and its PreStart
// hashes), so the memo holds about 1 MiB of keys at the most. At the cap the
// oldest entry goes. One mutex guards it: digests run without the GIL on
// several server threads, and the critical sections are a lookup and a copy
// of ~100 bytes.

constexpr size_t kMemoEntries = 256;
constexpr size_t kMemoMaxKey = 4096;

struct HashMemoStats {
  uint64_t puts = 0, hits = 0, misses = 0, evictions = 0;
  size_t entries = 0, cap = 0;
};

class HashMemo {
 public:
  // 0 turns the memo off and empties it; a smaller cap drops the oldest
  void configure(size_t entries) {
    std::lock_guard<std::mutex> g(mu_);
    cap_ = entries;
    while (order_.size() > cap_) drop_oldest();
  }

  // unlocked peek for the callers' fast path; put and take check again
  bool enabled() const { return cap_.load(std::memory_order_relaxed) != 0; }

  void put(std::string_view key, const char hex[8]) {
    if (key.size() > kMemoMaxKey) return;
    std::lock_guard<std::mutex> g(mu_);
    if (!cap_) return;
    ++stats_.puts;
    auto it = index_.find(key);
    if (it != index_.end()) {
      // the same set again: one entry, now the newest
      memcpy(it->second->hex, hex, 8);
      order_.splice(order_.end(), order_, it->second);
      return;
    }
    if (order_.size() >= cap_) {
      drop_oldest();
      ++stats_.evictions;
    }
    order_.emplace_back();
    Entry& e = order_.back();
    e.key.assign(key.data(), key.size());
    memcpy(e.hex, hex, 8);
    index_.emplace(std::string_view(e.key), std::prev(order_.end()));
  }

  // on a hit copies the hash (NUL-terminated) and removes the entry
  bool take(std::string_view key, char hex[9]) {
    std::lock_guard<std::mutex> g(mu_);
    if (!cap_) return false;
    auto it = key.size() <= kMemoMaxKey ? index_.find(key) : index_.end();
    if (it == index_.end()) {
      ++stats_.misses;
      return false;
    }
    ++stats_.hits;
    memcpy(hex, it->second->hex, 8);
    hex[8] = 0;
    auto node = it->second;
    index_.erase(it);  // before the node that owns the key's bytes
    order_.erase(node);
    return true;
  }

  HashMemoStats stats() {
    std::lock_guard<std::mutex> g(mu_);
    HashMemoStats s = stats_;
    s.entries = order_.size();
    s.cap = cap_;
    return s;
  }

 private:
  struct Entry {
    std::string key;
    char hex[8];
  };

  void drop_oldest() {
    index_.erase(std::string_view(order_.front().key));
    order_.pop_front();
  }

  std::mutex mu_;
  std::atomic<size_t> cap_{kMemoEntries};
  std::list<Entry> order_;  // oldest first; the index's keys view these nodes
  std::unordered_map<std::string_view, std::list<Entry>::iterator> index_;
  HashMemoStats stats_;
};

// Allocate side: digest_field(want_json = false) for a caller that feeds the
// memo. A field large enough to hold a set that qualifies is walked with the
// scratch RunBuilder, hashed as ever, and where the set does qualify its
// fragment -> hash is put. The result never differs from digest_field's.
inline DigestOut digest_field_put(DigestScratch& s, const uint8_t* p, size_t len,
                                  uint32_t want, Sha256Fn sha, HashMemo* memo) {
  if (len < 3 * kRunsMinIds || !memo || !memo->enabled())
    return digest_field(s, p, len, want, false, false, sha);
  Span range{p, len};
  s.runs.reset(len / (3 * kRunsPerIds));
  DigestOut d = digest_ranges(s, &range, 1, want, false, false, sha, &s.runs);
  if (s.runs.qualifies() && s.runs.n == d.count) {
    s.runs.to_json(s.json);
    memo->put(s.json, d.hex);
  }
  return d;
}

// PreStart side: digest_field_runs for a caller that consults the memo. The
// walk leaves the hash out; a set that qualifies takes its hash from the
// memo, and on a miss the joined bytes the walk left in the scratch are
// hashed. A set that does not qualify is hashed from those same bytes before
// the second walk builds its list, so no set is walked more often than by
// digest_field_runs and none is hashed twice.
inline DigestOut digest_field_runs_take(DigestScratch& s, const uint8_t* p, size_t len,
                                        uint32_t want, Sha256Fn sha, bool* is_runs,
                                        HashMemo* memo) {
  if (len < 3 * kRunsMinIds || !memo || !memo->enabled())
    return digest_field_runs(s, p, len, want, sha, is_runs);
  *is_runs = false;
  Span range{p, len};
  s.runs.reset(len / (3 * kRunsPerIds));
  DigestOut d = digest_ranges(s, &range, 1, want, false, false, nullptr, &s.runs);
  if (s.runs.qualifies() && s.runs.n == d.count) {
    s.runs.to_json(s.json);
    d.json_len = s.json.size();
    *is_runs = true;
    if (!memo->take(s.json, d.hex)) hash_hex8(sha, s.joined.data(), d.joined_len, d.hex);
    return d;
  }
  hash_hex8(sha, s.joined.data(), d.joined_len, d.hex);
  DigestOut l = digest_ranges(s, &range, 1, want, true, false, nullptr);
  d.json_len = l.json_len;
  return d;
}

// ---- runs -> literal list ----------------------------------------------------
// parse_runs checks a runs fragment against the ID count its record states
// and sizes the expansion; write_runs then fills exactly plan.total bytes.
// Nothing is allocated for the expansion before every check has passed:
// counts must sum to expected_count, start + count <= 10^width, width in
// 1..18, total <= kScratchCap. Prefix spans point into the fragment.

struct RunsPlan {
  struct Run {
    const char* prefix;
    size_t prefix_len;
    unsigned width;
    uint64_t start, count;
  };
  std::vector<Run> runs;
  size_t total = 2;  // "[]"
};

namespace runs_detail {

inline void ws(const char*& p, const char* end) {
  while (p < end && (*p == ' ' || *p == '\t' || *p == '\n' || *p == '\r')) ++p;
}

inline void expect(const char*& p, const char* end, char c) {
  ws(p, end);
  if (p >= end || *p != c) throw std::runtime_error("runs: malformed fragment");
  ++p;
}

// a JSON non-negative integer below 10^18: digits only, no leading zero
inline uint64_t uint_field(const char*& p, const char* end) {
  ws(p, end);
  const char* b = p;
  uint64_t v = 0;
  while (p < end && (unsigned)(*p - '0') < 10) {
    if (p - b >= 18) throw std::runtime_error("runs: number too long");
    v = v * 10 + (uint64_t)(*p - '0');
    ++p;
  }
  if (p == b || (p - b > 1 && *b == '0'))
    throw std::runtime_error("runs: not a non-negative integer");
  if (p < end && (*p == '.' || *p == 'e' || *p == 'E'))
    throw std::runtime_error("runs: not an integer");
  return v;
}

}  // namespace runs_detail

inline RunsPlan parse_runs(const char* frag, size_t len, uint64_t expected_count) {
  using namespace runs_detail;
  static const uint64_t kPow10[19] = {
      1ull, 10ull, 100ull, 1000ull, 10000ull, 100000ull, 1000000ull, 10000000ull,
      100000000ull, 1000000000ull, 10000000000ull, 100000000000ull, 1000000000000ull,
      10000000000000ull, 100000000000000ull, 1000000000000000ull, 10000000000000000ull,
      100000000000000000ull, 1000000000000000000ull};
  RunsPlan plan;
  const char* p = frag;
  const char* const end = frag + len;
  uint64_t left = expected_count;
  expect(p, end, '[');
  ws(p, end);
  if (p < end && *p == ']') {
    ++p;
  } else {
    for (;;) {
      RunsPlan::Run r;
      expect(p, end, '[');
      expect(p, end, '"');
      r.prefix = p;
      while (p < end && *p != '"') {
        const unsigned char c = (unsigned char)*p;
        if (c < 0x20 || c >= 0x80 || c == '\\') throw std::runtime_error("runs: bad prefix");
        ++p;
      }
      r.prefix_len = (size_t)(p - r.prefix);
      expect(p, end, '"');
      expect(p, end, ',');
      const uint64_t width = uint_field(p, end);
      expect(p, end, ',');
      r.start = uint_field(p, end);
      expect(p, end, ',');
      r.count = uint_field(p, end);
      expect(p, end, ']');
      if (width < 1 || width > kRunsMaxWidth) throw std::runtime_error("runs: bad width");
      r.width = (unsigned)width;
      if (r.count < 1 || r.count > left) throw std::runtime_error("runs: count mismatch");
      left -= r.count;
      // r.start, r.count < 10^18 each: the sum fits a uint64
      if (r.start + r.count > kPow10[width]) throw std::runtime_error("runs: past the width");
      // r.count <= kScratchCap from here on, so the product cannot wrap
      if (r.count > kScratchCap) throw std::runtime_error("runs: too large");
      const uint64_t per = (uint64_t)r.prefix_len + width + 3;  // quotes, comma
      if (per > kScratchCap || r.count * per > kScratchCap - plan.total)
        throw std::runtime_error("runs: too large");
      plan.total += (size_t)(r.count * per);
      plan.runs.push_back(r);
      ws(p, end);
      if (p < end && *p == ',') {
        ++p;
        continue;
      }
      expect(p, end, ']');
      break;
    }
    plan.total -= 1;  // no comma after the last ID
  }
  ws(p, end);
  if (p != end) throw std::runtime_error("runs: trailing bytes");
  if (left) throw std::runtime_error("runs: count mismatch");
  return plan;
}

// the literal list fragment, json.dumps(ids, separators=(",", ":")), into
// out[0, plan.total)
inline void write_runs(const RunsPlan& plan, char* out) {
  char* q = out;
  *q++ = '[';
  bool first = true;
  for (const RunsPlan::Run& r : plan.runs) {
    char digits[kRunsMaxWidth];
    uint64_t v = r.start;
    for (unsigned i = r.width; i-- > 0;) {
      digits[i] = (char)('0' + v % 10);
      v /= 10;
    }
    for (uint64_t k = 0; k < r.count; ++k) {
      if (!first) *q++ = ',';
      first = false;
      *q++ = '"';
      memcpy(q, r.prefix, r.prefix_len);
      q += r.prefix_len;
      memcpy(q, digits, r.width);
      q += r.width;
      *q++ = '"';
      for (unsigned i = r.width; i-- > 0;) {  // digits += 1
        if (digits[i] != '9') {
          ++digits[i];
          break;
        }
        digits[i] = '0';
      }
    }
  }
  *q++ = ']';
  if ((size_t)(q - out) != plan.total) throw std::logic_error("runs: size mismatch");
}

inline std::string expand_runs(const char* frag, size_t len, uint64_t expected_count) {
  RunsPlan plan = parse_runs(frag, len, expected_count);
  std::string out(plan.total, '\0');
  write_runs(plan, &out[0]);
  return out;
}

}  // namespace wirecore
