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

  void trim() {
    if (joined.capacity() > kScratchCap) std::string().swap(joined);
    if (json.capacity() > kScratchCap) std::string().swap(json);
    if (spans.capacity() * sizeof(Span) > kScratchCap) std::vector<Span>().swap(spans);
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
    if (s.joined.size() < in_bytes + 1) s.joined.resize(in_bytes + 1);
    jo = &s.joined[0];
    jo_end = jo + s.joined.size();
    js = js_end = nullptr;
    if (want_json) {
      // '[' + per ID two quotes and a comma (n + 3 <= 1.5 * (n + 2)) + ']';
      // IDs holding quotes or control bytes can need more: json_room grows
      size_t est = in_bytes + in_bytes / 2 + 16;
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

  void put(const Span& id, bool first) {
    if ((size_t)(jo_end - jo) < id.second + 1) throw std::runtime_error("digest overflow");
    if (!first) *jo++ = ':';
    memcpy(jo, id.first, id.second);
    jo += id.second;
    if (want_json) {
      json_room(6 * id.second + 4);  // literal + comma + closing bracket
      if (!first) *js++ = ',';
      js = json_put_string(js, id.first, id.second);
    }
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
  for (size_t ri = 0; ri < nranges && sorted; ++ri) {
    Reader r{ranges[ri].first, ranges[ri].first + ranges[ri].second};
    while (!r.done()) {
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
    // a lambda, not the function's address: std::sort inlines the compare
    std::sort(s.spans.begin(), s.spans.end(),
              [](const Span& a, const Span& b) { return span_less(a, b); });
    count = s.spans.size();
    w.restart();
    for (size_t i = 0; i < count; ++i) w.put(s.spans[i], i == 0);
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
