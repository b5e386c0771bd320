// wirecore.h — the protobuf wire reader and the fused device-set digest of
// _fastwire: Reader and spans_of walk LEN fields, DigestWriter / digest_ranges
// hash (and print) an ID set in one pass, and digest_field, digest_field_put
// and digest_field_runs are the entry points of the Allocate and PreStart
// handlers. Header-only, standard library only, shared with the fuzz targets
// and the sanitizer self-tests so they run exactly the shipped code. The
// ID-run codec (idruns.h) and the hash memo (hashmemo.h) come with it.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "hashmemo.h"
#include "idruns.h"

namespace wirecore {

using Span = std::pair<const uint8_t*, size_t>;

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

// collect every field-`want` LEN payload within [p, end)
inline void spans_of(const uint8_t* p, const uint8_t* end, uint32_t want,
                     std::vector<Span>& out) {
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

// ---- fixed-stride keys ---------------------------------------------------------
// An ID of the run's one length L as the words DigestWriter::run and put_keys
// compare, test and store. Both key types offer the same operations: load (an
// entry inside [.., end)), load_exact (exactly L bytes), less (byte-wise
// order), successor (b is a plus one in the last digit, or plus one with one
// carry, x9 -> y0, the digit before it below 9: the IDs RunBuilder only
// counts), needs_escape (a byte json.dumps escapes) and store (whole words,
// up to kWordSlack - 1 bytes past the ID).

// 1 <= L <= 8: one left-aligned big-endian word
struct NarrowKey {
  struct Val {
    uint64_t raw;  // as loaded; the bytes past the ID are whatever followed it
    uint64_t key;  // big-endian, the bytes past the ID zero
  };
  size_t L;
  int sh;  // shift of the last byte
  uint64_t mask;
  uint64_t pad;  // the bytes past the ID must not look like bytes to escape

  explicit NarrowKey(size_t len)
      : L(len), sh(64 - 8 * (int)len), mask(~0ull << sh),
        pad(~mask & 0x3030303030303030ull) {}

  static Val of(uint64_t key) { return Val{word_to_be(key), key}; }

  // a whole-word load where 8 bytes remain in the range, L bytes otherwise
  // (the last entries of a range)
  Val load(const uint8_t* id, const uint8_t* end) const {
    uint64_t raw = 0;
    if ((size_t)(end - id) >= 8)
      memcpy(&raw, id, 8);
    else
      memcpy(&raw, id, L);
    return Val{raw, word_to_be(raw) & mask};
  }
  Val load_exact(const uint8_t* id) const { return of(be_key_bytes(id, L)); }

  bool less(const Val& a, const Val& b) const { return a.key < b.key; }
  // on the right-aligned words: the last digit is the low byte, and x9 -> y0
  // adds 256 - 9 (at L = 1 the byte before the last is 0, never a digit)
  bool successor(const Val& a, const Val& b) const {
    const uint64_t t = a.key >> sh;
    const uint64_t d = (b.key >> sh) - t;
    const unsigned d0 = (unsigned)(t & 0xFF) - '0';
    return (d == 1 && d0 < 9) ||
           (d == 247 && d0 == 9 && (unsigned)(((t >> 8) & 0xFF) - '0') < 9);
  }
  bool needs_escape(const Val& v) const { return word_needs_escape(v.key | pad); }
  void store(char* out, const Val& v) const { memcpy(out, &v.raw, 8); }
};

// 9 <= L <= kMaxStride: two overlapping words, the first 8 bytes and the last 8
struct WideKey {
  struct Val {
    uint64_t rh, rl;  // as loaded
    uint64_t kh, kl;  // big-endian
  };
  size_t L, off;

  explicit WideKey(size_t len) : L(len), off(len - 8) {}

  // both words lie inside the ID
  Val load_exact(const uint8_t* id) const {
    Val v;
    memcpy(&v.rh, id, 8);
    memcpy(&v.rl, id + off, 8);
    v.kh = word_to_be(v.rh);
    v.kl = word_to_be(v.rl);
    return v;
  }
  Val load(const uint8_t* id, const uint8_t*) const { return load_exact(id); }

  bool less(const Val& a, const Val& b) const {
    return a.kh < b.kh || (a.kh == b.kh && a.kl < b.kl);
  }
  bool successor(const Val& a, const Val& b) const {
    const uint64_t d = b.kl - a.kl;
    const unsigned d0 = (unsigned)(a.kl & 0xFF) - '0';
    return a.kh == b.kh && ((d == 1 && d0 < 9) ||
                            (d == 247 && d0 == 9 && (unsigned)(((a.kl >> 8) & 0xFF) - '0') < 9));
  }
  bool needs_escape(const Val& v) const {
    return word_needs_escape(v.kh) || word_needs_escape(v.kl);
  }
  void store(char* out, const Val& v) const {
    memcpy(out, &v.rh, 8);
    memcpy(out + off, &v.rl, 8);
  }
};

// the JSON literal of an ID without bytes to escape; the closing quote goes
// in after the whole-word store, which may cover its place
template <class K>
inline char* put_literal(const K& k, char* q, const typename K::Val& v) {
  q[0] = '"';
  k.store(q + 1, v);
  q[k.L + 1] = '"';
  return q + k.L + 2;
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
  RunBuilder runs;             // digest_field_split

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
    const size_t maxn = (size_t)(r.end - r.p) / stride;
    if (maxn == 0 || r.p[0] != tagbyte || r.p[1] != L) return true;
    // room for the whole run, once: per entry a separator and L bytes
    // (joined), a comma, two quotes and L bytes (JSON), plus the word slack
    if ((size_t)(jo_end - jo) < maxn * (L + 1) + kWordSlack)
      throw std::runtime_error("digest overflow");
    if (want_json) json_room(maxn * (L + 3) + 1 + kWordSlack);
    // One loop for both key widths. The cursors are copied into locals around
    // the stores, and so is everything else the loop reads: a store through a
    // char* may alias the members and the captures, which would then be
    // reloaded after each.
    auto walk = [&](const auto k) {
      const size_t len = k.L, step = len + 2;
      const uint8_t tag = tagbyte;
      std::vector<Span>* const sp = spans;
      const uint8_t* p = r.p;
      const uint8_t* const end = r.end;
      char* j = jo;
      char* q = js;
      const bool json = want_json;
      const uint8_t* last = nullptr;
      size_t n = 0;
      bool in_order = true;
      // runs: an entry that is its predecessor's successor is only counted;
      // every other one goes through RunBuilder::add
      RunBuilder* rbl = rb && rb->ok ? rb : nullptr;
      size_t matched = 0;
      auto pv = k.load_exact(prev.first);
      while ((size_t)(end - p) >= step && p[0] == tag && p[1] == len) {
        const uint8_t* pay = p + 2;
        const auto v = k.load(pay, end);
        if (k.less(v, pv)) {
          in_order = false;
          break;
        }
        if (rbl) {
          if (k.successor(pv, v)) {
            ++matched;
          } else {
            rbl->extend(matched, last, len);
            matched = 0;
            rbl->add(pay, len);
            if (!rbl->ok) rbl = nullptr;
          }
        }
        pv = v;
        *j = ':';
        k.store(j + 1, v);
        j += len + 1;
        if (json) {
          if (k.needs_escape(v)) {
            js = q;
            json_room(6 * len + 4 + ((size_t)(end - p) / step) * (len + 3) + kWordSlack);
            q = js;
            *q++ = ',';
            q = json_put_string(q, pay, len);
          } else {
            *q = ',';
            q = put_literal(k, q + 1, v);
          }
        }
        if (sp) sp->emplace_back(pay, len);
        last = pay;
        ++n;
        p += step;
      }
      if (rbl) rbl->extend(matched, last, len);
      jo = j;
      js = q;
      r.p = p;
      count += n;
      if (last) prev = Span{last, len};
      return in_order;
    };
    return L <= 8 ? walk(NarrowKey(L)) : walk(WideKey(L));
  }

  // Radix fallback output: the n sorted left-aligned big-endian keys of IDs
  // of length 1 <= L <= 8, written after restart().
  void put_keys(const uint64_t* keys, size_t n, size_t L) {
    if ((size_t)(jo_end - jo) < n * (L + 1) + kWordSlack)
      throw std::runtime_error("digest overflow");
    if (want_json) json_room(n * (L + 3) + 1 + kWordSlack);
    char* j = jo;
    char* q = js;
    const NarrowKey k(L);
    RunBuilder* rbl = rb && rb->ok ? rb : nullptr;
    size_t matched = 0;
    uint8_t id[8];  // a key's bytes, for the RunBuilder and the escape detour
    for (size_t i = 0; i < n; ++i) {
      const NarrowKey::Val v = NarrowKey::of(keys[i]);
      if (i) *j++ = ':';
      k.store(j, v);
      j += L;
      if (rbl) {
        if (i && k.successor(NarrowKey::of(keys[i - 1]), v)) {
          ++matched;
        } else {
          if (matched) {
            k.store((char*)id, NarrowKey::of(keys[i - 1]));
            rbl->extend(matched, id, L);
            matched = 0;
          }
          k.store((char*)id, v);
          rbl->add(id, L);
          if (!rbl->ok) rbl = nullptr;
        }
      }
      if (want_json) {
        if (i) *q++ = ',';
        if (k.needs_escape(v)) {
          k.store((char*)id, v);
          js = q;
          json_room(6 * L + 4 + (n - i) * (L + 3) + kWordSlack);
          q = json_put_string(js, id, L);
        } else {
          q = put_literal(k, q, v);
        }
      }
    }
    if (rbl && matched) {
      k.store((char*)id, NarrowKey::of(keys[n - 1]));
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
      spans_of(ranges[ri].first, ranges[ri].first + ranges[ri].second, want, s.spans);
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
      const NarrowKey k(L);
      size_t i = 0;
      for (size_t ri = 0; ri < nranges && i < count; ++ri) {
        const uint8_t* lo = ranges[ri].first;
        const uint8_t* hi = lo + ranges[ri].second;
        for (; i < count; ++i) {
          const uint8_t* id = s.spans[i].first;
          if (id < lo || id >= hi) break;
          keys[i] = k.load(id, hi).key;
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

// The walk of the two digests below: [p, p + len) with the scratch
// RunBuilder, hashed where `sha` is given. True when the set qualifies as
// runs; its fragment is then in scratch.json (and no literal list was built).
inline bool digest_field_split(DigestScratch& s, const uint8_t* p, size_t len,
                               uint32_t want, Sha256Fn sha, DigestOut& d) {
  Span range{p, len};
  s.runs.reset(len / (3 * kRunsPerIds));
  d = digest_ranges(s, &range, 1, want, false, false, sha, &s.runs);
  if (!s.runs.qualifies() || s.runs.n != d.count) return false;
  s.runs.to_json(s.json);
  return true;
}

// Allocate side: digest_field(want_json = false) for a caller that feeds the
// memo. A field large enough to hold a set that qualifies is walked with the
// scratch RunBuilder, hashed as ever, and where the set does qualify its
// fragment -> hash is put. The result never differs from digest_field's.
inline DigestOut digest_field_put(DigestScratch& s, const uint8_t* p, size_t len,
                                  uint32_t want, Sha256Fn sha, HashMemo* memo) {
  // an entry takes >= 3 wire bytes (tag, length, one digit)
  if (len < 3 * kRunsMinIds || !memo || !memo->enabled())
    return digest_field(s, p, len, want, false, false, sha);
  DigestOut d;
  if (digest_field_split(s, p, len, want, sha, d)) memo->put(s.json, d.hex);
  return d;
}

// PreStart side: digest_field for a caller that stores runs. Where the set
// qualifies, scratch.json[0, json_len) holds the runs fragment and *is_runs is
// set; its literal list is never built. Otherwise the fragment is the literal
// list: a field too small to qualify goes straight to digest_field, and a set
// large enough to try that then does not qualify (an ID that is not
// run-encodable, too many runs) is walked a second time for the list.
// The first walk leaves the hash out. A set that qualifies takes its hash from
// `memo` (may be null) when that is enabled and holds it; every other set is
// hashed from the joined bytes that walk left in the scratch, once.
inline DigestOut digest_field_runs(DigestScratch& s, const uint8_t* p, size_t len,
                                   uint32_t want, Sha256Fn sha, bool* is_runs,
                                   HashMemo* memo) {
  *is_runs = false;
  if (len < 3 * kRunsMinIds) return digest_field(s, p, len, want, true, false, sha);
  DigestOut d;
  if (digest_field_split(s, p, len, want, nullptr, d)) {
    d.json_len = s.json.size();
    *is_runs = true;
    if (!(memo && memo->enabled() && memo->take(s.json, d.hex)))
      hash_hex8(sha, s.joined.data(), d.joined_len, d.hex);
    return d;
  }
  hash_hex8(sha, s.joined.data(), d.joined_len, d.hex);
  Span range{p, len};
  d.json_len = digest_ranges(s, &range, 1, want, true, false, nullptr).json_len;
  return d;
}

}  // namespace wirecore
