// _fastwire: C++ accelerators for the two protobuf shapes that can carry
// hundreds of thousands of fake-device IDs when gpu-memory runs at 1-MiB
// units (288 GiB ⇒ 294,912 IDs per GPU):
//
//   decode_string_list(buf)    repeated string field 1 (PreStartContainerRequest,
//                              ContainerAllocateRequest bodies)
//   decode_nested_string_lists(buf)
//                              repeated message field 1, each holding repeated
//                              string field 1 (AllocateRequest shape) →
//                              list of lists of str
//   encode_device_list(ids, suffix)
//                              ListAndWatchResponse body: for each id emit a
//                              field-1 Device submessage = (field-1 string id)
//                              + caller-precomputed suffix bytes (health +
//                              topology), all length-prefixed.
//
// Pure wire-format code — semantics identical to protos/protowire.py (the
// test-suite cross-checks them); ~30-40× faster on large ID sets.

#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <openssl/evp.h>

#include <algorithm>
#include <cerrno>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "bindfx.h"
#include "wirecore.h"

namespace py = pybind11;

namespace {

using wirecore::DigestOut;
using wirecore::DigestScratch;
using wirecore::Reader;
using wirecore::ScratchGuard;
using wirecore::Span;
using wirecore::span_less;
using wirecore::spans_of;

py::list decode_string_list(py::bytes data) {
  char* buf;
  Py_ssize_t len;
  PyBytes_AsStringAndSize(data.ptr(), &buf, &len);
  std::vector<Span> spans;
  spans_of((const uint8_t*)buf, (const uint8_t*)buf + len, 1, spans);
  py::list out;
  for (auto& s : spans)
    out.append(py::str((const char*)s.first, s.second));
  return out;
}

py::list decode_nested_string_lists(py::bytes data) {
  char* buf;
  Py_ssize_t len;
  PyBytes_AsStringAndSize(data.ptr(), &buf, &len);
  std::vector<Span> outer;
  spans_of((const uint8_t*)buf, (const uint8_t*)buf + len, 1, outer);
  py::list out;
  for (auto& o : outer) {
    std::vector<Span> inner;
    spans_of(o.first, o.first + o.second, 1, inner);
    py::list ids;
    for (auto& s : inner)
      ids.append(py::str((const char*)s.first, s.second));
    out.append(ids);
  }
  return out;
}

void put_varint(std::string& out, uint64_t v) {
  while (v >= 0x80) {
    out.push_back((char)(v | 0x80));
    v >>= 7;
  }
  out.push_back((char)v);
}

size_t varint_size(uint64_t v) {
  size_t n = 1;
  while (v >= 0x80) {
    v >>= 7;
    ++n;
  }
  return n;
}

py::bytes encode_device_list(const std::vector<std::string>& ids, py::bytes suffix_b) {
  char* sbuf;
  Py_ssize_t slen;
  PyBytes_AsStringAndSize(suffix_b.ptr(), &sbuf, &slen);
  std::string out;
  size_t est = 0;
  for (auto& id : ids) est += id.size() + slen + 10;
  out.reserve(est);
  for (auto& id : ids) {
    // device submessage: field 1 (ID string) + suffix
    size_t body = 1 + varint_size(id.size()) + id.size() + slen;
    out.push_back(0x0A);  // ListAndWatchResponse.devices (field 1, LEN)
    put_varint(out, body);
    out.push_back(0x0A);  // Device.ID (field 1, LEN)
    put_varint(out, id.size());
    out.append(id);
    out.append(sbuf, slen);
  }
  return py::bytes(out);
}

// repeated string field 1 (PreStartContainerRequest / inner container bodies)
std::string encode_string_list_raw(const std::vector<std::string>& ids) {
  std::string out;
  size_t est = 0;
  for (auto& id : ids) est += id.size() + 6;
  out.reserve(est);
  for (auto& id : ids) {
    out.push_back(0x0A);
    put_varint(out, id.size());
    out.append(id);
  }
  return out;
}

py::bytes encode_string_list(const std::vector<std::string>& ids) {
  return py::bytes(encode_string_list_raw(ids));
}

// AllocateRequest shape: repeated message field 1 wrapping repeated string 1
py::bytes encode_nested_string_lists(const std::vector<std::vector<std::string>>& lists) {
  std::string out;
  for (auto& ids : lists) {
    std::string inner = encode_string_list_raw(ids);
    out.push_back(0x0A);
    put_varint(out, inner.size());
    out.append(inner);
  }
  return py::bytes(out);
}

// ---- Allocate request digest (hash + count without materializing IDs) ----
// The reference-exact gpu-memory contract (1-MiB units) makes Allocate
// requests carry up to ~295k device IDs. The Allocate handler only needs the
// device-set HASH (sha256 of ":".join(sorted ids), first 8 hex chars —
// types.hash_device_ids) and the COUNT, so this computes both straight off
// the wire: no 73k-element Python lists, no Python sort/join/sha. Byte-wise
// span comparison matches Python's code-point string order because UTF-8 is
// order-preserving. GIL released during parse/sort/hash.

void sha256_evp(const void* data, size_t len, unsigned char md[32]) {
  unsigned int mdlen = 0;
  EVP_Digest(data, len, md, &mdlen, EVP_sha256(), nullptr);
}

// fragment -> hash of the large sets Allocate has digested and PreStart has
// not yet taken (hashmemo.h); one per process
wirecore::HashMemo g_hash_memo;

std::vector<std::pair<std::string, size_t>> digest_raw(const uint8_t* p, size_t len) {
  // container requests are few (one per container); only the per-container
  // ID walk is hot
  std::vector<Span> outer;
  spans_of(p, p + len, 1, outer);
  std::vector<std::pair<std::string, size_t>> result;
  result.reserve(outer.size());
  DigestScratch& sc = wirecore::digest_scratch();
  for (auto& o : outer) {
    ScratchGuard guard(sc);
    DigestOut d = wirecore::digest_field_put(sc, o.first, o.second, 1, sha256_evp,
                                             &g_hash_memo);
    result.emplace_back(std::string(d.hex, 8), d.count);
  }
  return result;
}

py::list digest_allocate_request(py::bytes data) {
  char* buf;
  Py_ssize_t len;
  PyBytes_AsStringAndSize(data.ptr(), &buf, &len);
  std::vector<std::pair<std::string, size_t>> result;
  {
    py::gil_scoped_release rel;
    result = digest_raw((const uint8_t*)buf, (size_t)len);
  }
  py::list out;
  for (auto& r : result)
    out.append(py::make_tuple(py::str(r.first), (long long)r.second));
  return out;
}

// PreStartContainerRequest digest: the handler needs the SORTED ID list
// (persisted in the reference's on-disk record format) plus the device-set
// hash; one C++ pass hashes (sorting the spans when kubelet sent them
// unsorted), then materializes the sorted Python strings exactly once.
py::tuple decode_prestart_digest(py::bytes data) {
  char* buf;
  Py_ssize_t len;
  PyBytes_AsStringAndSize(data.ptr(), &buf, &len);
  DigestScratch& sc = wirecore::digest_scratch();
  ScratchGuard guard(sc);
  DigestOut d;
  {
    py::gil_scoped_release rel;
    d = wirecore::digest_field(sc, (const uint8_t*)buf, (size_t)len, 1, false, true,
                               sha256_evp);
  }
  py::list out;
  for (auto& s : sc.spans) out.append(py::str((const char*)s.first, s.second));
  return py::make_tuple(out, py::str(d.hex, 8));
}

// PreStart digest v2: hash + count + the sorted ID list PRE-SERIALIZED as a
// JSON array fragment. The handler needs the list only to persist the
// reference-format record {"Hash","List","ResourceName"}; building 73k
// Python strings (then json.dumps-ing them back) cost ~8 ms per 72-GiB pod
// at the 1-MiB contract unit. PodInfo.val() splices this fragment verbatim,
// so the IDs never exist as Python objects on the hot path.
py::tuple decode_prestart_digest2(py::bytes data) {
  char* buf;
  Py_ssize_t len;
  PyBytes_AsStringAndSize(data.ptr(), &buf, &len);
  DigestScratch& sc = wirecore::digest_scratch();
  ScratchGuard guard(sc);
  DigestOut d;
  {
    py::gil_scoped_release rel;
    d = wirecore::digest_field(sc, (const uint8_t*)buf, (size_t)len, 1, true, false,
                               sha256_evp);
  }
  return py::make_tuple(py::str(d.hex, 8), (long long)d.count,
                        py::bytes(sc.json.data(), d.json_len));
}

// PreStart digest v3: as v2, but a large set of consecutive IDs comes back as
// its runs fragment ([[prefix, width, start, count], ...], is_runs = True)
// and its literal list is never built: the store keeps the runs, and
// expand_runs rebuilds the list for the few readers that want it. Sets that
// do not qualify (idruns.h) come back exactly as from v2. A set that qualifies
// and was digested by Allocate just before takes its hash from the memo
// (hashmemo.h) instead of hashing the same bytes again.
py::tuple decode_prestart_digest3(py::bytes data) {
  char* buf;
  Py_ssize_t len;
  PyBytes_AsStringAndSize(data.ptr(), &buf, &len);
  DigestScratch& sc = wirecore::digest_scratch();
  ScratchGuard guard(sc);
  DigestOut d;
  bool is_runs = false;
  {
    py::gil_scoped_release rel;
    d = wirecore::digest_field_runs(sc, (const uint8_t*)buf, (size_t)len, 1, sha256_evp,
                                    &is_runs, &g_hash_memo);
  }
  return py::make_tuple(py::str(d.hex, 8), (long long)d.count,
                        py::bytes(sc.json.data(), d.json_len), is_runs);
}

void hash_memo_configure(long long entries) {
  if (entries < 0) throw std::invalid_argument("hash memo: negative entry cap");
  g_hash_memo.configure((size_t)entries);
}

py::dict hash_memo_stats() {
  wirecore::HashMemoStats s = g_hash_memo.stats();
  py::dict d;
  d["puts"] = s.puts;
  d["hits"] = s.hits;
  d["misses"] = s.misses;
  d["evictions"] = s.evictions;
  d["entries"] = s.entries;
  d["cap"] = s.cap;
  return d;
}

// The runs fragment of an already sorted list of IDs (a Device built from
// Python strings), or None when the set does not qualify.
py::object ids_to_runs(py::list ids) {
  const size_t n = ids.size();
  if (n < wirecore::kRunsMinIds) return py::none();
  std::vector<Span> spans;
  spans.reserve(n);
  for (size_t i = 0; i < n; ++i) {
    Py_ssize_t sz;
    // the UTF-8 form is cached in the str object, which the list keeps alive
    const char* s = PyUnicode_AsUTF8AndSize(PyList_GET_ITEM(ids.ptr(), i), &sz);
    if (!s) throw py::error_already_set();
    spans.emplace_back((const uint8_t*)s, (size_t)sz);
  }
  std::string out;
  bool ok;
  {
    py::gil_scoped_release rel;
    wirecore::RunBuilder rb;
    rb.reset(n / wirecore::kRunsPerIds);
    for (auto& s : spans) rb.add(s.first, s.second);
    ok = rb.qualifies();
    if (ok) rb.to_json(out);
  }
  if (!ok) return py::none();
  return py::bytes(out);
}

// runs fragment + the record's ID count -> the literal list fragment, byte
// for byte what decode_prestart_digest2 returns for that set
py::bytes expand_runs(py::bytes frag, long long count) {
  char* buf;
  Py_ssize_t len;
  PyBytes_AsStringAndSize(frag.ptr(), &buf, &len);
  if (count < 0) throw std::runtime_error("runs: negative count");
  wirecore::RunsPlan plan;
  {
    py::gil_scoped_release rel;
    plan = wirecore::parse_runs(buf, (size_t)len, (uint64_t)count);
  }
  PyObject* out = PyBytes_FromStringAndSize(nullptr, (Py_ssize_t)plan.total);
  if (!out) throw py::error_already_set();
  py::bytes result = py::reinterpret_steal<py::bytes>(out);
  char* dst = PyBytes_AS_STRING(out);
  {
    py::gil_scoped_release rel;
    wirecore::write_runs(plan, dst);
  }
  return result;
}

// ---- podresources List digest --------------------------------------------
// ListPodResourcesResponse walker: per (pod, container, resource) compute the
// device-set hash + count straight off the wire. The locator's job is "which
// pod holds this hashed set"; at the 1-MiB contract unit a loaded node's
// List response carries millions of device IDs — materializing them as
// Python strings and re-hashing per locate() costs tens of ms.
// Shapes: ListPodResourcesResponse{1: PodResources{1 name, 2 namespace,
// 3 ContainerResources{1 name, 2 ContainerDevices{1 resource_name,
// 2 device_ids}}}} (k8s v1alpha1; ref pkg/podresources/v1alpha1/api.proto).
py::list podresources_digest(py::bytes data) {
  char* buf;
  Py_ssize_t len;
  PyBytes_AsStringAndSize(data.ptr(), &buf, &len);
  struct Row {
    std::string ns, pod, container, resource, hash;
    size_t count;
  };
  std::vector<Row> rows;
  {
    py::gil_scoped_release rel;
    DigestScratch& sc = wirecore::digest_scratch();
    std::vector<Span> pods;
    spans_of((const uint8_t*)buf, (const uint8_t*)buf + len, 1, pods);
    for (auto& pspan : pods) {
      std::vector<Span> f;
      std::string pod_name, pod_ns;
      f.clear();
      spans_of(pspan.first, pspan.first + pspan.second, 1, f);
      if (!f.empty()) pod_name.assign((const char*)f[0].first, f[0].second);
      f.clear();
      spans_of(pspan.first, pspan.first + pspan.second, 2, f);
      if (!f.empty()) pod_ns.assign((const char*)f[0].first, f[0].second);
      std::vector<Span> containers;
      spans_of(pspan.first, pspan.first + pspan.second, 3, containers);
      for (auto& cspan : containers) {
        f.clear();
        spans_of(cspan.first, cspan.first + cspan.second, 1, f);
        std::string cname;
        if (!f.empty()) cname.assign((const char*)f[0].first, f[0].second);
        std::vector<Span> devs;
        spans_of(cspan.first, cspan.first + cspan.second, 2, devs);
        // group the ContainerDevices entries per resource_name (a container
        // may list a resource in one entry pre-1.21 or one entry per ID
        // after); the digest walks each group's entries as one ID set
        std::vector<std::pair<std::string, std::vector<Span>>> groups;
        for (auto& dspan : devs) {
          f.clear();
          spans_of(dspan.first, dspan.first + dspan.second, 1, f);
          std::string res;
          if (!f.empty()) res.assign((const char*)f[0].first, f[0].second);
          bool found = false;
          for (auto& g : groups)
            if (g.first == res) {
              g.second.push_back(dspan);
              found = true;
              break;
            }
          if (!found)
            groups.emplace_back(res, std::vector<Span>{dspan});
        }
        for (auto& g : groups) {
          auto& ranges = g.second;
          ScratchGuard guard(sc);
          DigestOut d = wirecore::digest_ranges(sc, ranges.data(), ranges.size(), 2,
                                                false, false, sha256_evp);
          if (d.count == 0) continue;
          rows.push_back(Row{pod_ns, pod_name, cname, g.first,
                             std::string(d.hex, 8), d.count});
        }
      }
    }
  }
  py::list out;
  for (auto& r : rows)
    out.append(py::make_tuple(py::str(r.ns), py::str(r.pod), py::str(r.container),
                              py::str(r.resource), py::str(r.hash),
                              (long long)r.count));
  return out;
}

// ---- GetPreferredAllocation digest (per-GPU counts + on-demand extract) ----
// At the reference-exact 1-MiB gpu-memory contract kubelet sends the FULL
// free-ID pool (≈295k IDs, ~3 MB) as available_deviceIDs on every pod
// admission; decoding that into Python strings plus a Python group-by cost
// ~300 ms per call. The policy only needs per-GPU availability COUNTS to
// choose a GPU; the chosen GPU's lexicographically-first `size` IDs are then
// extracted and emitted as an already-encoded response body without ever
// materializing Python strings.

struct PreferredContainer {
  std::vector<Span> available;
  std::vector<Span> must_include;
  long long size = 0;
};

// parse leading "<int>-" GPU prefix of an ID span; -1 when malformed
long long gpu_prefix(const uint8_t* p, size_t n) {
  long long v = 0;
  size_t i = 0;
  while (i < n && p[i] >= '0' && p[i] <= '9') {
    v = v * 10 + (p[i] - '0');
    ++i;
  }
  if (i == 0 || i >= n || p[i] != '-') return -1;
  return v;
}

void parse_preferred(const uint8_t* p, size_t len,
                     std::vector<PreferredContainer>& out) {
  std::vector<Span> outer;
  spans_of(p, p + len, 1, outer);
  out.resize(outer.size());
  for (size_t i = 0; i < outer.size(); ++i) {
    Reader r{outer[i].first, outer[i].first + outer[i].second};
    while (!r.done()) {
      uint64_t tag = r.varint();
      uint32_t field = tag >> 3, wire = tag & 7;
      if ((field == 1 || field == 2) && wire == 2) {
        uint64_t n = r.varint();
        if (n > (uint64_t)(r.end - r.p)) throw std::runtime_error("truncated");
        auto& vec = field == 1 ? out[i].available : out[i].must_include;
        vec.emplace_back(r.p, (size_t)n);
        r.p += n;
      } else if (field == 3 && wire == 0) {
        out[i].size = (long long)r.varint();
      } else {
        r.skip(wire);
      }
    }
  }
}

py::list preferred_digest(py::bytes data) {
  char* buf;
  Py_ssize_t len;
  PyBytes_AsStringAndSize(data.ptr(), &buf, &len);
  std::vector<PreferredContainer> containers;
  std::vector<std::vector<std::pair<long long, size_t>>> counts_all;
  {
    py::gil_scoped_release rel;
    parse_preferred((const uint8_t*)buf, (size_t)len, containers);
    counts_all.resize(containers.size());
    for (size_t i = 0; i < containers.size(); ++i) {
      // small flat map: node GPU counts are ≤ tens of entries
      auto& counts = counts_all[i];
      for (auto& s : containers[i].available) {
        long long g = gpu_prefix(s.first, s.second);
        bool found = false;
        for (auto& kv : counts)
          if (kv.first == g) {
            ++kv.second;
            found = true;
            break;
          }
        if (!found) counts.emplace_back(g, 1);
      }
    }
  }
  py::list out;
  for (size_t i = 0; i < containers.size(); ++i) {
    py::dict counts;
    for (auto& kv : counts_all[i])
      counts[py::int_(kv.first)] = py::int_((long long)kv.second);
    py::list must;
    for (auto& s : containers[i].must_include)
      must.append(py::str((const char*)s.first, s.second));
    out.append(py::make_tuple(counts, must, containers[i].size));
  }
  return out;
}

// Encoded ContainerPreferredAllocationResponse body (repeated string 1) of
// the lexicographically-first `n` available IDs of GPU `gpu` in container
// `index` — same order the Python path produces (groups sorted, then [:n]).
py::bytes preferred_extract(py::bytes data, size_t index, long long gpu, size_t n) {
  char* buf;
  Py_ssize_t len;
  PyBytes_AsStringAndSize(data.ptr(), &buf, &len);
  std::string out;
  {
    py::gil_scoped_release rel;
    std::vector<PreferredContainer> containers;
    parse_preferred((const uint8_t*)buf, (size_t)len, containers);
    if (index >= containers.size()) throw std::runtime_error("bad container index");
    std::vector<Span> group;
    for (auto& s : containers[index].available)
      if (gpu_prefix(s.first, s.second) == gpu) group.push_back(s);
    // a lambda, not the function's address: the sorts inline the compare
    auto cmp = [](const Span& a, const Span& b) { return span_less(a, b); };
    if (n < group.size()) {
      std::nth_element(group.begin(), group.begin() + n, group.end(), cmp);
      group.resize(n);
    }
    std::sort(group.begin(), group.end(), cmp);
    size_t est = 0;
    for (auto& s : group) est += s.second + 6;
    out.reserve(est);
    for (auto& s : group) {
      out.push_back(0x0A);
      put_varint(out, s.second);
      out.append((const char*)s.first, s.second);
    }
  }
  return py::bytes(out);
}

// ---- AllocateResponse encoder (the Allocate hot path's response half) ----
// Byte-identical to protos.deviceplugin.AllocateResponse.encode (MessageSpec
// policy: non-repeated strings/bools omitted when empty/false; map entries
// omit empty keys/values; dict insertion order preserved) — the differential
// test in tests/test_fastpath.py asserts exact equality.

std::string dict_str(const py::dict& d, const char* key) {
  if (d.contains(key)) {
    py::object v = d[key];
    if (!v.is_none()) return v.cast<std::string>();
  }
  return {};
}

void put_str_field(std::string& out, uint8_t tag, const std::string& s) {
  if (s.empty()) return;
  out.push_back((char)tag);
  put_varint(out, s.size());
  out.append(s);
}

void encode_str_map(std::string& out, uint8_t tag, const py::dict& map) {
  for (auto kv : map) {
    std::string k = kv.first.cast<std::string>();
    std::string v = kv.second.cast<std::string>();
    std::string entry;
    put_str_field(entry, 0x0A, k);  // map entry key (1)
    put_str_field(entry, 0x12, v);  // map entry value (2)
    out.push_back((char)tag);
    put_varint(out, entry.size());
    out.append(entry);
  }
}

py::bytes encode_allocate_response(py::dict resp) {
  std::string out;
  out.reserve(512);
  if (!resp.contains("container_responses")) return py::bytes(out);
  for (auto cr_h : resp["container_responses"].cast<py::list>()) {
    py::dict cr = cr_h.cast<py::dict>();
    std::string c;
    c.reserve(384);
    if (cr.contains("envs"))
      encode_str_map(c, 0x0A, cr["envs"].cast<py::dict>());  // envs (1)
    if (cr.contains("mounts")) {
      for (auto m_h : cr["mounts"].cast<py::list>()) {  // mounts (2)
        py::dict m = m_h.cast<py::dict>();
        std::string b;
        put_str_field(b, 0x0A, dict_str(m, "container_path"));
        put_str_field(b, 0x12, dict_str(m, "host_path"));
        if (m.contains("read_only") && m["read_only"].cast<bool>()) {
          b.push_back(0x18);  // read_only (3, varint)
          b.push_back(0x01);
        }
        c.push_back(0x12);
        put_varint(c, b.size());
        c.append(b);
      }
    }
    if (cr.contains("devices")) {
      for (auto d_h : cr["devices"].cast<py::list>()) {  // devices (3)
        py::dict d = d_h.cast<py::dict>();
        std::string b;
        put_str_field(b, 0x0A, dict_str(d, "container_path"));
        put_str_field(b, 0x12, dict_str(d, "host_path"));
        put_str_field(b, 0x1A, dict_str(d, "permissions"));
        c.push_back(0x1A);
        put_varint(c, b.size());
        c.append(b);
      }
    }
    if (cr.contains("annotations"))
      encode_str_map(c, 0x22, cr["annotations"].cast<py::dict>());  // (4)
    out.push_back(0x0A);  // AllocateResponse.container_responses (1)
    put_varint(out, c.size());
    out.append(c);
  }
  return py::bytes(out);
}

// ---- file effects of a bind and of a GC pass (bindfx.h) ----------------------
// The arguments are copied out of the Python objects first; the syscalls run
// with the GIL released. A failure becomes OSError with its errno and path.

[[noreturn]] void raise_oserror(const bindfx::SysError& e) {
  errno = e.err;
  PyErr_SetFromErrnoWithFilename(PyExc_OSError, e.path.c_str());
  throw py::error_already_set();
}

void make_links(const std::vector<std::pair<std::string, std::string>>& pairs) {
  try {
    py::gil_scoped_release rel;
    bindfx::make_links(pairs);
  } catch (const bindfx::SysError& e) {
    raise_oserror(e);
  }
}

void atomic_write(const std::string& path, py::bytes data) {
  char* buf;
  Py_ssize_t len;
  PyBytes_AsStringAndSize(data.ptr(), &buf, &len);
  try {
    py::gil_scoped_release rel;
    bindfx::atomic_write(path, buf, (size_t)len);
  } catch (const bindfx::SysError& e) {
    raise_oserror(e);
  }
}

void unlink_many(const std::vector<std::string>& paths) {
  try {
    py::gil_scoped_release rel;
    bindfx::unlink_many(paths);
  } catch (const bindfx::SysError& e) {
    raise_oserror(e);
  }
}

}  // namespace

PYBIND11_MODULE(_fastwire, m) {
  m.doc() = "wire-format accelerators for large fake-device ID sets";
  m.def("decode_string_list", &decode_string_list);
  m.def("decode_nested_string_lists", &decode_nested_string_lists);
  m.def("encode_device_list", &encode_device_list);
  m.def("encode_string_list", &encode_string_list);
  m.def("encode_nested_string_lists", &encode_nested_string_lists);
  m.def("encode_allocate_response", &encode_allocate_response);
  m.def("digest_allocate_request", &digest_allocate_request);
  m.def("decode_prestart_digest", &decode_prestart_digest);
  m.def("decode_prestart_digest2", &decode_prestart_digest2);
  m.def("decode_prestart_digest3", &decode_prestart_digest3);
  m.def("ids_to_runs", &ids_to_runs);
  m.def("expand_runs", &expand_runs);
  m.def("preferred_digest", &preferred_digest);
  m.def("podresources_digest", &podresources_digest);
  m.def("preferred_extract", &preferred_extract);
  m.def("hash_memo_configure", &hash_memo_configure, py::arg("entries"));
  m.def("hash_memo_stats", &hash_memo_stats);
  m.attr("HASH_MEMO_ENTRIES") = (long long)wirecore::kMemoEntries;
  m.attr("HASH_MEMO_MAX_KEY") = (long long)wirecore::kMemoMaxKey;
  m.def("make_links", &make_links, py::arg("pairs"));
  m.def("atomic_write", &atomic_write, py::arg("path"), py::arg("data"));
  m.def("unlink_many", &unlink_many, py::arg("paths"));
}
