// libFuzzer harness over the native parsers that face untrusted bytes
// (VERDICT round-1 weak #9: the C++ frame/HPACK parser is root-adjacent
// attack surface in kube-system and had only replay-style garbage tests).
//
// One binary, target selected by the first input byte — keeps a single
// corpus exercising every parser:
//   0: HPACK header-block decode (h2core.h — the code in _etransport)
//   1: Huffman string decode
//   2: protobuf wire walk (wirecore.h spans_of — the code in _fastwire)
//   3: AllocateRequest digest (outer field1 → wirecore.h digest_field per
//      container: the fused walk/check/join/hash helper behind _fastwire),
//      and the same set through digest_field_runs: where it comes back as ID
//      runs, expanding them must give the literal list fragment; and once
//      more through the Allocate and PreStart digests with a hash memo
//      (hashmemo.h): digest with memo == digest without
//   4: minijson parse (OCI config/state parsing in egpu-hook); the same
//      bytes, read as a 16-bit ID count and a runs fragment, through
//      idruns.h parse_runs / write_runs (what the store reads back)
//   5: devfilter OCI device-rule extraction + eBPF program build
//
// Build + run: python -m elastic_gpu_agent_amd.native.build_fuzz
//              (clang -fsanitize=fuzzer,address from /opt/rocm's LLVM)
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "h2core.h"
#include "minijson.h"
#define SELFTEST_UTIL_NO_CHECKS  // the hash and the encoders only
#include "selftest_util.h"
#include "wirecore.h"

// devfilter's parser + program builder (no kernel interaction in build)
#include "devfilter.h"

namespace {

void fuzz_hpack(const uint8_t* data, size_t size) {
  h2core::HpackDecoder dec;
  std::vector<std::pair<std::string, std::string>> out;
  (void)dec.decode(data, size, &out);
}

void fuzz_huffman(const uint8_t* data, size_t size) {
  std::string out;
  (void)h2core::huffman_decode(data, size, &out);
}

void fuzz_wire(const uint8_t* data, size_t size) {
  std::vector<wirecore::Span> spans;
  try {
    wirecore::spans_of(data, data + size, 1, spans);
  } catch (const std::runtime_error&) {
  }
  // every reported span must stay inside the input
  for (auto& s : spans) {
    if (s.first < data || s.first + s.second > data + size) __builtin_trap();
  }
}

// the stand-in for sha256 reads every joined byte, so ASan sees any join
// that ran past its buffer
constexpr wirecore::Sha256Fn sum_digest = selftest::fnv_digest;

// the shipped digest: outer field1 -> per container the fused walk / order
// check / join / hash helper, JSON fragment and sorted spans included
void fuzz_wire_nested(const uint8_t* data, size_t size) {
  std::vector<wirecore::Span> outer;
  wirecore::DigestScratch& sc = wirecore::digest_scratch();
  try {
    wirecore::spans_of(data, data + size, 1, outer);
    for (auto& o : outer) {
      // without spans an unsorted fixed-width set takes the radix fallback,
      // with spans the span sort: hash and fragment must not differ
      std::string hex_no_spans, json_no_spans;
      {
        wirecore::ScratchGuard guard(sc);
        wirecore::DigestOut d = wirecore::digest_field(
            sc, o.first, o.second, 1, /*want_json=*/true, /*want_spans=*/false, sum_digest);
        hex_no_spans = d.hex;
        json_no_spans.assign(sc.json.data(), d.json_len);
      }
      wirecore::ScratchGuard guard(sc);
      wirecore::DigestOut d = wirecore::digest_field(
          sc, o.first, o.second, 1, /*want_json=*/true, /*want_spans=*/true, sum_digest);
      if (hex_no_spans != d.hex) __builtin_trap();
      if (json_no_spans != std::string(sc.json.data(), d.json_len)) __builtin_trap();
      if (d.count != sc.spans.size()) __builtin_trap();
      if (d.json_len < 2 || d.json_len > sc.json.size()) __builtin_trap();
      if (sc.json[0] != '[' || sc.json[d.json_len - 1] != ']') __builtin_trap();
      for (size_t i = 0; i < sc.spans.size(); ++i) {
        auto& s = sc.spans[i];
        if (s.first < data || s.first + s.second > data + size) __builtin_trap();
        // sorted, byte-wise, shorter prefix first
        if (i && wirecore::span_less(s, sc.spans[i - 1])) __builtin_trap();
      }
      // runs: same hash and count; expand(compress(set)) is the list fragment
      const size_t count = d.count;
      bool is_runs = false;
      wirecore::DigestOut r =
          wirecore::digest_field_runs(sc, o.first, o.second, 1, sum_digest, &is_runs, nullptr);
      if (hex_no_spans != r.hex || r.count != count) __builtin_trap();
      if (r.json_len > sc.json.size()) __builtin_trap();
      if (is_runs) {
        if (count < wirecore::kRunsMinIds) __builtin_trap();
        if (wirecore::expand_runs(sc.json.data(), r.json_len, count) != json_no_spans)
          __builtin_trap();
      } else if (json_no_spans != std::string(sc.json.data(), r.json_len)) {
        __builtin_trap();
      }
      // hash memo: Allocate's digest puts, PreStart's takes (or hashes); the
      // second PreStart finds the entry consumed. All equal the plain ones.
      const std::string runs_json(sc.json.data(), r.json_len);
      static wirecore::HashMemo memo;
      const uint64_t hits = memo.stats().hits;
      wirecore::DigestOut a =
          wirecore::digest_field_put(sc, o.first, o.second, 1, sum_digest, &memo);
      if (hex_no_spans != a.hex || a.count != count) __builtin_trap();
      for (int pass = 0; pass < 2; ++pass) {
        bool memo_runs = false;
        wirecore::DigestOut t = wirecore::digest_field_runs(
            sc, o.first, o.second, 1, sum_digest, &memo_runs, &memo);
        if (hex_no_spans != t.hex || t.count != count || memo_runs != is_runs)
          __builtin_trap();
        if (runs_json != std::string(sc.json.data(), t.json_len)) __builtin_trap();
      }
      // a hit needs a set that qualifies with a fragment within the key cap
      const bool storable = is_runs && runs_json.size() <= wirecore::kMemoMaxKey;
      if (memo.stats().hits - hits != (storable ? 1u : 0u)) __builtin_trap();
      if (memo.stats().entries != 0) __builtin_trap();
    }
  } catch (const std::runtime_error&) {
  }
}

void fuzz_minijson(const uint8_t* data, size_t size) {
  std::string text((const char*)data, size);
  auto v = minijson::parse(text);
  if (v && v->is_obj()) {
    // exercise navigation on whatever parsed
    (void)v->get("linux").get("resources").get("devices").is_arr();
    (void)v->get("process").get("env").is_arr();
    (void)v->get("pid").as_int(0);
  }
}

// arbitrary bytes as a stored runs fragment: parse_runs must refuse or size
// the expansion exactly; the block is exact-size so ASan sees either end
void fuzz_runs_expand(const uint8_t* data, size_t size) {
  if (size < 2) return;
  const uint64_t count = data[0] | (uint64_t)data[1] << 8;
  try {
    wirecore::RunsPlan plan = wirecore::parse_runs((const char*)data + 2, size - 2, count);
    if (plan.total > wirecore::kRunsMaxExpanded) __builtin_trap();
    char* out = (char*)malloc(plan.total);
    wirecore::write_runs(plan, out);
    if (out[0] != '[' || out[plan.total - 1] != ']') __builtin_trap();
    free(out);
  } catch (const std::runtime_error&) {
  }
}

void fuzz_devfilter(const uint8_t* data, size_t size) {
  std::string config((const char*)data, size);
  bool found = false;
  auto rules = devfilter::parse_oci_device_rules(config, &found);
  if (rules.size() > 512) rules.resize(512);  // bound program size
  auto prog = devfilter::build_prog(rules, false);
  if (prog.empty()) __builtin_trap();  // must always emit a valid program
}

}  // namespace

extern "C" int LLVMFuzzerInitialize(int*, char***) {
  h2core::trie_init();  // etransport calls this at module load
  return 0;
}

extern "C" int LLVMFuzzerTestOneInput(const uint8_t* data, size_t size) {
  if (size < 1) return 0;
  uint8_t sel = data[0] % 6;
  ++data;
  --size;
  switch (sel) {
    case 0: fuzz_hpack(data, size); break;
    case 1: fuzz_huffman(data, size); break;
    case 2: fuzz_wire(data, size); break;
    case 3: fuzz_wire_nested(data, size); break;
    case 4: fuzz_minijson(data, size); fuzz_runs_expand(data, size); break;
    case 5: fuzz_devfilter(data, size); break;
  }
  return 0;
}
