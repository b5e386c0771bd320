// wirecore.h — protobuf wire-walking core shared by _fastwire and the
// standalone fuzz targets. Header-only; extracted verbatim from
// fastwire.cpp so fuzzing covers exactly the shipped parser.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
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

// The strings are used as raw storage: size() is the high-water mark of what
// was ever needed (so growing zero-fills only new bytes), and each call
// tracks its own used lengths locally. Bytes past those lengths are stale
// and never read.
struct DigestScratch {
  std::string joined;
  std::string json;
  std::vector<Span> spans;
  std::vector<uint64_t> keys;  // radix fallback: n keys + n for the passes

  void trim() {
    if (joined.capacity() > kScratchCap) std::string().swap(joined);
    if (json.capacity() > kScratchCap) std::string().swap(json);
    if (spans.capacity() * sizeof(Span) > kScratchCap) std::vector<Span>().swap(spans);
    if (keys.capacity() * sizeof(uint64_t) > kScratchCap) std::vector<uint64_t>().swap(keys);
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
  size_t json_len;  // bytes of scratch.json holding the fragment
};

// writer over the two scratch strings; keeps its cursors in locals
struct DigestWriter {
  DigestScratch& s;
  bool want_json;
  char *jo, *jo_end;  // joined cursor / end of storage
  char *js, *js_end;  // json cursor / end of storage

  DigestWriter(DigestScratch& sc, size_t in_bytes, bool json)
      : s(sc), want_json(json) {
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
    if (L <= 8) {
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
    for (size_t i = 0; i < n; ++i) {
      const uint64_t key = keys[i];
      const uint64_t raw = word_to_be(key);
      if (i) *j++ = ':';
      memcpy(j, &raw, 8);
      j += L;
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
    jo = j;
    js = q;
  }

  DigestOut finish(size_t count, Sha256Fn sha) {
    DigestOut out;
    out.json_len = 0;
    if (want_json) {
      json_room(1);
      *js++ = ']';
      out.json_len = js - &s.json[0];
    }
    unsigned char md[32];
    sha(s.joined.data(), jo - &s.joined[0], md);
    static const char kHex[] = "0123456789abcdef";
    for (int i = 0; i < 4; ++i) {
      out.hex[2 * i] = kHex[md[i] >> 4];
      out.hex[2 * i + 1] = kHex[md[i] & 15];
    }
    out.hex[8] = 0;
    out.count = count;
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
                               Sha256Fn sha) {
  size_t in_bytes = 0;
  for (size_t i = 0; i < nranges; ++i) in_bytes += ranges[i].second;
  DigestWriter w(s, in_bytes, want_json);
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

}  // namespace wirecore
