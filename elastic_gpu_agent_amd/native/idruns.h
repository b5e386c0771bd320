// idruns.h — the ID-run codec: RunBuilder splits a sorted device set into
// runs of consecutive IDs and prints the runs fragment the store keeps;
// parse_runs / write_runs / expand_runs turn a stored fragment back into the
// literal list. Header-only, standard library only; wirecore.h's digest feeds
// the RunBuilder, _fastwire and the fuzz targets call the parser.
//
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
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

namespace wirecore {

constexpr size_t kRunsMinIds = 1024;
constexpr size_t kRunsPerIds = 8;
constexpr size_t kRunsMaxWidth = 18;
constexpr size_t kRunsMaxExpanded = 4u << 20;  // bytes a fragment may expand to

struct IdRun {
  size_t prefix_off, prefix_len;  // into RunBuilder::prefixes
  unsigned width;
  uint64_t start, count;
};

// Fed the sorted IDs one by one. The expected successor is kept as text, so
// an ID that extends the run costs one compare and an ASCII increment. The
// digest's word-at-a-time loop sees "previous ID + 1 in the last digit" and
// "previous ID + 1 with one carry (x9 -> y0)" on the words it already holds
// and only reports how many such IDs went by and the last of them (extend), so
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

// ---- runs -> literal list ----------------------------------------------------
// parse_runs checks a runs fragment against the ID count its record states
// and sizes the expansion; write_runs then fills exactly plan.total bytes.
// Nothing is allocated for the expansion before every check has passed:
// counts must sum to expected_count, start + count <= 10^width, width in
// 1..18, total <= kRunsMaxExpanded. Prefix spans point into the fragment.

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
      // r.count <= kRunsMaxExpanded from here on, so the product cannot wrap
      if (r.count > kRunsMaxExpanded) throw std::runtime_error("runs: too large");
      const uint64_t per = (uint64_t)r.prefix_len + width + 3;  // quotes, comma
      if (per > kRunsMaxExpanded || r.count * per > kRunsMaxExpanded - plan.total)
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
