// Stand-alone check of h2frame.h — the receive buffer, the frame parser and
// the header/flow-control byte work of the native transport — meant to be
// built with -fsanitize=address,undefined and run directly (the pybind
// module itself is never run under a sanitizer). CPU only, no Python.
//
// Bytes reach the code the way they do in service: through a socketpair and
// RecvBuf::read_more. The feeder decides how many bytes each read() sees, so
// every buffer transition (growth, compaction, shrink) is hit on purpose and
// the frame views are compared byte for byte with what was sent. Inputs that
// are parsed in place live in exact-size heap blocks so ASan traps any read
// past the end. Expected wire bytes are literals recorded from the transport
// before this header was split out of it, not values computed here.
//
// Build + run: python -m elastic_gpu_agent_amd.native.build_fuzz --selftest
#include <csignal>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <sys/socket.h>
#include <thread>
#include <vector>

#include "h2frame.h"

using namespace h2frame;

namespace {

int failures = 0;

#define CHECK(cond, what)                                              \
  do {                                                                 \
    if (!(cond)) {                                                     \
      fprintf(stderr, "FAIL %s:%d %s (%s)\n", __FILE__, __LINE__, #cond, what); \
      ++failures;                                                      \
    }                                                                  \
  } while (0)

// exact-size heap copy: one byte past the end is an ASan report
std::unique_ptr<uint8_t[]> exact(const std::string& s) {
  std::unique_ptr<uint8_t[]> p(new uint8_t[s.size()]);
  if (!s.empty()) memcpy(p.get(), s.data(), s.size());
  return p;
}

std::string frame_bytes(uint32_t len_field, uint8_t type, uint8_t flags, uint32_t sid,
                        const std::string& body) {
  uint8_t h[9];
  put_frame_header(h, len_field, type, flags, sid);
  return std::string((const char*)h, 9) + body;
}

std::string frame_bytes(uint8_t type, uint8_t flags, uint32_t sid, const std::string& body) {
  return frame_bytes((uint32_t)body.size(), type, flags, sid, body);
}

std::string pattern(size_t n, uint32_t seed) {
  std::string s(n, '\0');
  for (size_t i = 0; i < n; ++i) {
    seed = seed * 1664525u + 1013904223u;
    s[i] = (char)(seed >> 24);
  }
  return s;
}

// Feeds `stream` to a RecvBuf through a socketpair, one chunk per read():
// a chunk ends at the next offset in `cuts`, after `chunk` bytes, or at the
// end of the stream. fill() is the server's loop with the write in front.
struct Feeder {
  Feeder(std::string s, std::vector<size_t> c, size_t chunk_size)
      : stream(std::move(s)), cuts(std::move(c)), chunk(chunk_size) {
    if (socketpair(AF_UNIX, SOCK_STREAM, 0, fds) != 0) abort();
  }
  ~Feeder() { close(fds[0]); close(fds[1]); }

  bool fill(size_t need) {
    while (buf.avail() < need) {
      if (pos == stream.size()) return false;  // the peer has no more to say
      size_t end = std::min(stream.size(), pos + chunk);
      for (size_t c : cuts)
        if (c > pos && c < end) end = c;
      if (write(fds[1], stream.data() + pos, end - pos) != (ssize_t)(end - pos)) abort();
      pos = end;
      ssize_t r = buf.read_more(fds[0], need);
      if (r < 0 && errno == EINTR) continue;
      if (r <= 0) return false;
      ++reads;
    }
    return true;
  }

  bool next(Frame* f, bool* oversize) {
    return next_frame(buf, [this](size_t n) { return fill(n); }, f, oversize);
  }

  std::string stream;
  std::vector<size_t> cuts;
  size_t chunk;
  size_t pos = 0, reads = 0;
  int fds[2];
  RecvBuf buf;
};

struct Parsed {
  uint8_t type, flags;
  uint32_t sid;
  std::string body;
  bool operator==(const Parsed& o) const {
    return type == o.type && flags == o.flags && sid == o.sid && body == o.body;
  }
};

std::vector<Parsed> parse_all(Feeder& fd) {
  std::vector<Parsed> out;
  Frame f;
  bool oversize;
  while (fd.next(&f, &oversize))
    out.push_back({f.type, f.flags, f.sid, std::string((const char*)f.body, f.len)});
  CHECK(!oversize, "stream ended by EOF, not by an oversize frame");
  return out;
}

// ---------------------------------------------------------------- framing
void test_delivery() {
  std::vector<Parsed> want = {
      {F_DATA, FLAG_END_STREAM, 1, std::string("\0\0\0\0\2hi", 7)},
      {F_SETTINGS, FLAG_ACK, 0, ""},  // 0-length frame
      {F_HEADERS, FLAG_END_HEADERS | FLAG_END_STREAM, 0x7fffffff, "\x88\x0f\x10"},
      {F_PING, 0, 0, "12345678"},
      {F_DATA, 0, 3, ""},  // 0-length frame at the very end
  };
  std::string stream;
  for (auto& p : want) stream += frame_bytes(p.type, p.flags, p.sid, p.body);
  // the reserved bit of the stream id is masked off
  stream[2 * 9 + 7 + 5] = (char)0xff;

  Feeder whole(stream, {}, stream.size());
  auto a = parse_all(whole);
  CHECK(a == want, "one write");
  CHECK(whole.reads == 1, "one write is one read");

  Feeder bytewise(stream, {}, 1);
  auto b = parse_all(bytewise);
  CHECK(b == want, "1 byte per write");
  CHECK(bytewise.reads == stream.size(), "each read saw one byte");

  // a header split between two reads, and a body split from its header
  Feeder split(stream, {4, 9 + 7 + 9 + 9 + 2}, stream.size());
  CHECK(parse_all(split) == want, "header split between two reads");
  CHECK(split.reads == 3, "three reads");
}

void test_buffer_transitions() {
  // compaction: the consumed prefix (frame A) is at least the live bytes
  // when B's body needs room, so the second fill of B memmoves B's header
  // and first body bytes to the front; f.body must be read after that
  {
    std::string a = pattern(200000, 1), b = pattern(100000, 2);
    std::string stream = frame_bytes(F_DATA, 0, 1, a) + frame_bytes(F_DATA, 0, 3, b);
    Feeder fd(stream, {9 + a.size() + 9 + 10}, 64 * 1024);
    Frame f;
    bool oversize;
    CHECK(fd.next(&f, &oversize) && f.len == a.size() && !memcmp(f.body, a.data(), a.size()),
          "frame A");
    size_t cap = fd.buf.capacity();
    CHECK(cap == RecvBuf::kInitCap, "first allocation");
    CHECK(fd.buf.avail() == 19, "B's header and 10 body bytes are live");
    CHECK(fd.next(&f, &oversize) && f.sid == 3 && f.len == b.size(), "frame B");
    CHECK(!memcmp(f.body, b.data(), b.size()), "B's body after the move");
    CHECK(fd.buf.capacity() == cap, "compacted, not reallocated");
  }
  // growth with a consumed prefix smaller than the live bytes: no
  // compaction, live data + need > capacity reallocates and carries them
  {
    std::string x = pattern(10, 3), y = pattern(400000, 4);
    std::string stream = frame_bytes(F_DATA, 0, 1, x) + frame_bytes(F_DATA, 0, 3, y);
    Feeder fd(stream, {19 + 9 + 1000}, 64 * 1024);
    Frame f;
    bool oversize;
    CHECK(fd.next(&f, &oversize) && !memcmp(f.body, x.data(), x.size()), "frame X");
    CHECK(fd.buf.avail() == 1009, "Y's header and 1000 body bytes are live");
    CHECK(fd.next(&f, &oversize) && f.len == y.size(), "frame Y");
    CHECK(!memcmp(f.body, y.data(), y.size()), "Y's body after the reallocation");
    CHECK(fd.buf.capacity() == 2 * RecvBuf::kInitCap, "capacity doubled");
  }
  // shrink: one frame above kRetainCap, then small traffic. The read that
  // ends the big frame also brings 4 bytes of the next header, so the
  // shrinking reallocation has live bytes to carry.
  {
    std::string big = pattern(RecvBuf::kRetainCap + 1, 5), small = pattern(7, 6);
    std::string stream = frame_bytes(F_DATA, 0, 1, big) + frame_bytes(F_PING, 0, 0, small) +
                         frame_bytes(F_DATA, FLAG_END_STREAM, 1, small);
    Feeder fd(stream, {9 + big.size() + 4}, 64 * 1024);
    Frame f;
    bool oversize;
    CHECK(fd.next(&f, &oversize) && f.len == big.size(), "big frame");
    CHECK(!memcmp(f.body, big.data(), big.size()), "big body, grown chunk by chunk");
    CHECK(fd.buf.capacity() > RecvBuf::kRetainCap, "capacity above the retain cap");
    CHECK(fd.buf.avail() == 4, "4 live header bytes");
    CHECK(fd.next(&f, &oversize) && f.type == F_PING && f.len == 7 &&
              !memcmp(f.body, small.data(), 7),
          "small frame across the shrink");
    CHECK(fd.buf.capacity() == RecvBuf::kInitCap, "capacity came back down");
    CHECK(fd.next(&f, &oversize) && f.type == F_DATA && f.flags == FLAG_END_STREAM &&
              !memcmp(f.body, small.data(), 7),
          "traffic after the shrink");
    CHECK(!fd.next(&f, &oversize) && !oversize, "end of stream");
  }
}

void test_length_limit() {
  // The length field has 24 bits, so the most a header can announce is
  // 16 MiB - 1. That is below next_frame's 64 MiB refusal, which no input
  // can therefore reach: `oversize` stays false and the parser asks for the
  // body. Here the peer sends the header alone and goes away.
  std::string stream = frame_bytes(0xffffff, F_DATA, 0, 1, "");
  CHECK(stream.size() == 9 && stream.substr(0, 3) == "\xff\xff\xff", "largest length field");
  Feeder fd(stream, {}, 9);
  Frame f;
  bool oversize = true;
  CHECK(!fd.next(&f, &oversize), "unfinished frame");
  CHECK(!oversize, "16 MiB - 1 is not oversize");
  CHECK(fd.reads == 1 && fd.buf.avail() == 9, "the header is all that was read, and it stays");
  CHECK(fd.buf.capacity() == RecvBuf::kInitCap, "no room made for a body that never came");
}

// ---------------------------------------------------------------- parsing
void test_strip_padding() {
  struct Case {
    const char* name;
    uint8_t flags;
    bool priority;
    std::string body;
    bool ok;
    std::string want;
  };
  const uint8_t PP = FLAG_PADDED | FLAG_PRIORITY;
  std::vector<Case> cases = {
      {"no pad", 0, true, "abc", true, "abc"},
      {"pad 0", FLAG_PADDED, true, std::string("\0ab", 3), true, "ab"},
      {"pad == remaining", FLAG_PADDED, true, "\2xy", true, ""},
      {"pad > remaining", FLAG_PADDED, true, "\3xy", false, ""},
      {"empty padded frame", FLAG_PADDED, true, "", false, ""},
      {"empty padded DATA frame", FLAG_PADDED, false, "", false, ""},
      {"pad byte only", FLAG_PADDED, false, std::string("\0", 1), true, ""},
      {"PRIORITY, 4 bytes", FLAG_PRIORITY, true, "abcd", false, ""},
      {"PRIORITY, 5 bytes", FLAG_PRIORITY, true, "abcde", true, ""},
      {"PADDED+PRIORITY", PP, true, std::string("\1PRIORhi\0", 9), true, "hi"},
      {"PADDED+PRIORITY, 5 bytes", PP, true, std::string("\0PRIO", 5), false, ""},
      {"PADDED+PRIORITY, pad too long", PP, true, std::string("\3PRIORhi", 8), false, ""},
      {"DATA ignores the PRIORITY bit", FLAG_PRIORITY, false, "abcd", true, "abcd"},
  };
  for (auto& c : cases) {
    auto mem = exact(c.body);
    Frame f;
    f.type = F_HEADERS;
    f.flags = c.flags;
    f.body = mem.get();
    f.len = c.body.size();
    const uint8_t* p = nullptr;
    size_t n = 0;
    bool ok = strip_padding(f, c.priority, &p, &n);
    CHECK(ok == c.ok, c.name);
    if (ok && c.ok) CHECK(std::string((const char*)p, n) == c.want, c.name);
  }
}

void test_first_grpc_message() {
  std::string full = std::string("\0\0\0\0\3abc", 8);
  struct Case { const char* name; std::string body; std::string want; };
  std::vector<Case> cases = {
      {"n = 0", "", ""},
      {"n = 4", full.substr(0, 4), ""},
      {"exact length", full, "abc"},
      {"one byte short", full.substr(0, 7), ""},
      {"one byte extra", full + "Z", "abc"},
      {"empty message", std::string("\0\0\0\0\0", 5), ""},
      {"length near 2^32", std::string("\0\xff\xff\xff\xff", 5) + "ab", ""},
  };
  for (auto& c : cases) {
    auto mem = exact(c.body);
    const uint8_t* msg = nullptr;
    size_t n = 99;
    first_grpc_message(mem.get(), c.body.size(), &msg, &n);
    CHECK(std::string((const char*)msg, n) == c.want, c.name);
  }
}

void test_settings() {
  // MAX_FRAME = 32768, INITIAL_WINDOW = 100000
  std::string two("\0\5\0\0\x80\0" "\0\4\0\1\x86\xa0", 12);
  struct Case { size_t len; uint32_t max_frame; int64_t window; };
  // a trailing partial entry is ignored
  for (Case c : {Case{0, 16384, 65535}, Case{5, 16384, 65535}, Case{6, 32768, 65535},
                 Case{11, 32768, 65535}, Case{12, 32768, 100000}}) {
    auto mem = exact(two.substr(0, c.len));
    uint32_t max_frame = 16384;
    int64_t window = DEFAULT_WINDOW;
    int64_t delta = apply_settings(mem.get(), c.len, &max_frame, &window);
    CHECK(max_frame == c.max_frame, "max_frame");
    CHECK(window == c.window, "initial window");
    CHECK(delta == c.window - DEFAULT_WINDOW, "delta");
  }
  // the window may shrink, the last entry wins, unknown ids are skipped
  std::string three("\0\4\0\1\x11\x70" "\0\x99\1\2\3\4" "\0\4\0\0\xea\x60", 18);
  auto mem = exact(three);
  uint32_t max_frame = 16384;
  int64_t window = DEFAULT_WINDOW;
  CHECK(apply_settings(mem.get(), 18, &max_frame, &window) == 60000 - 65535, "negative delta");
  CHECK(window == 60000 && max_frame == 16384, "last INITIAL_WINDOW wins");

  Frame f;
  uint32_t inc = 77;
  auto w = exact(std::string("\x80\0\1\0", 4));
  f.body = w.get();
  f.len = 4;
  CHECK(window_increment(f, &inc) && inc == 256, "reserved bit masked");
  f.len = 3;
  CHECK(!window_increment(f, &inc), "3-byte WINDOW_UPDATE ignored");
  auto w5 = exact(std::string("\0\0\1\0\0", 5));
  f.body = w5.get();
  f.len = 5;
  CHECK(!window_increment(f, &inc), "5-byte WINDOW_UPDATE ignored");

  CHECK(send_budget(100, 50, 16384) == 50, "stream window binds");
  CHECK(send_budget(40, 50, 16384) == 40, "connection window binds");
  CHECK(send_budget(1 << 20, 1 << 20, 16384) == 16384, "max frame binds");
  CHECK(send_budget(-5, 50, 16384) == -5, "a negative window stays negative");
}

// ---------------------------------------------------------------- builders
template <size_t N>
std::string lit(const uint8_t (&a)[N]) { return std::string((const char*)a, N); }

void test_wire_literals() {
  // recorded from the server's first write and from ClientCore::connect()
  static const uint8_t kServerPreamble[] = {
      0x00, 0x00, 0x12, 0x04, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x05, 0x00, 0x10, 0x00,
      0x00, 0x00, 0x04, 0x02, 0x00, 0x00, 0x00, 0x00, 0x03, 0x00, 0x00, 0x04, 0x00, 0x00,
      0x00, 0x04, 0x08, 0x00, 0x00, 0x00, 0x00, 0x00, 0x01, 0xff, 0x00, 0x01};
  static const uint8_t kClientFrames[] = {
      0x00, 0x00, 0x0c, 0x04, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x05, 0x00,
      0x10, 0x00, 0x00, 0x00, 0x04, 0x02, 0x00, 0x00, 0x00, 0x00, 0x00, 0x04,
      0x08, 0x00, 0x00, 0x00, 0x00, 0x00, 0x01, 0xff, 0x00, 0x01};
  uint8_t out[kMaxPreamble + 1];
  out[kMaxPreamble] = 0xa5;
  size_t n = put_preamble(out, /*client=*/false);
  CHECK(std::string((const char*)out, n) == lit(kServerPreamble), "server preamble");
  n = put_preamble(out, /*client=*/true);
  CHECK(n == kMaxPreamble - 6 && out[kMaxPreamble] == 0xa5, "client preamble length");
  CHECK(std::string((const char*)out, n) ==
            std::string("PRI * HTTP/2.0\r\n\r\nSM\r\n\r\n", 24) + lit(kClientFrames),
        "client preamble");

  // recorded from a unary OK response and from an "unknown method" error
  // whose path held '%', 0x01 and 0xff
  static const uint8_t kRespHdr[] = {0x88, 0x0f, 0x10, 0x10, 0x61, 0x70, 0x70, 0x6c, 0x69, 0x63,
                                     0x61, 0x74, 0x69, 0x6f, 0x6e, 0x2f, 0x67, 0x72, 0x70, 0x63};
  static const uint8_t kOkTrailer[] = {0x00, 0x0b, 0x67, 0x72, 0x70, 0x63, 0x2d, 0x73,
                                       0x74, 0x61, 0x74, 0x75, 0x73, 0x01, 0x30};
  static const uint8_t kErrFields[] = {
      0x00, 0x0b, 0x67, 0x72, 0x70, 0x63, 0x2d, 0x73, 0x74, 0x61, 0x74, 0x75, 0x73, 0x01, 0x32,
      0x00, 0x0c, 0x67, 0x72, 0x70, 0x63, 0x2d, 0x6d, 0x65, 0x73, 0x73, 0x61, 0x67, 0x65, 0x1b,
      0x75, 0x6e, 0x6b, 0x6e, 0x6f, 0x77, 0x6e, 0x20, 0x6d, 0x65, 0x74, 0x68, 0x6f, 0x64, 0x20,
      0x2f, 0x61, 0x25, 0x32, 0x35, 0x62, 0x25, 0x30, 0x31, 0x25, 0x46, 0x46};
  static const uint8_t kErrFrameHeader[] = {0x00, 0x00, 0x4d, 0x01, 0x05, 0x00, 0x00, 0x00, 0x01};
  static const uint8_t kDataFrameHeader[] = {0x00, 0x00, 0x08, 0x00, 0x00, 0x00, 0x00, 0x00, 0x03};
  CHECK(lit(kRespHdrBlock) == lit(kRespHdr), "kRespHdrBlock");
  CHECK(lit(kOkTrailerBlock) == lit(kOkTrailer), "kOkTrailerBlock");
  std::string message = "unknown method /a%b\x01\xff";
  CHECK(status_trailer_fields(2, message) == lit(kErrFields), "status_trailer_fields");
  CHECK(error_trailer_block(2, message) == lit(kRespHdr) + lit(kErrFields),
        "error_trailer_block");
  uint8_t h[9];
  put_frame_header(h, 0x4d, F_HEADERS, FLAG_END_HEADERS | FLAG_END_STREAM, 1);
  CHECK(lit(h) == lit(kErrFrameHeader), "HEADERS frame header");
  put_frame_header(h, 8, F_DATA, 0, 3);
  CHECK(lit(h) == lit(kDataFrameHeader), "DATA frame header");
  uint8_t g[5];
  put_grpc_prefix(g, 3);
  CHECK(lit(g) == std::string("\0\0\0\0\3", 5), "gRPC prefix");

  // RFC 7540 §6.9 and §6.7 layouts
  uint8_t w[13];
  put_window_update(w, 5, 0x01020304);
  CHECK(lit(w) == std::string("\0\0\4\x08\0\0\0\0\5\1\2\3\4", 13), "WINDOW_UPDATE");
  uint8_t p[17];
  put_ping_ack(p, (const uint8_t*)"ABCDEFGH");
  CHECK(lit(p) == std::string("\0\0\x08\6\1\0\0\0\0", 9) + "ABCDEFGH", "PING ack");

  // a 127-byte grpc-message needs the HPACK integer continuation
  std::string fields = status_trailer_fields(13, std::string(127, 'm'));
  CHECK(fields.substr(16 + 14, 3) == std::string("\x7f\0m", 3), "hpack_put_int at the limit");
}

void test_percent() {
  std::string all;
  for (int i = 0; i < 256; ++i) all.push_back((char)i);
  std::string enc = percent_encode(all);
  for (unsigned char c : enc) CHECK(c >= 0x20 && c <= 0x7e, "encoded text is printable ASCII");
  CHECK(percent_decode(enc) == all, "round trip of all 256 byte values");
  CHECK(percent_decode(percent_encode(all + all)) == all + all, "escape at the very end");
  // an escape cut short by the end of the input stays as it is
  std::string longish(40, 'x');
  for (const char* tail : {"%", "%4", "%%", "%4%"}) {
    std::string in = longish + tail;
    std::string want = in;
    if (std::string(tail) == "%4%") want = longish + "\x04";  // strtol("4%") as before
    CHECK(percent_decode(in) == want, tail);
  }
  CHECK(percent_decode("") == "" && percent_encode("") == "", "empty");
  CHECK(percent_decode("a%41b") == "aAb", "escape in the middle");
}

// ---------------------------------------------------------------- sending
void test_payload_iov() {
  const uint8_t prefix[5] = {'p', 'q', 'r', 's', 't'};
  auto msg = exact("XYZ");
  std::string whole = "pqrstXYZ";
  for (size_t off = 0; off <= 6; ++off) {
    for (size_t n = 0; n <= 7; ++n) {
      if (off + n > whole.size()) continue;  // callers never ask past the end
      struct iovec iov[2];
      int k = payload_iov(iov, prefix, msg.get(), off, n);
      CHECK(k >= 0 && k <= 2 && (k > 0) == (n > 0), "iovec count");
      std::string got;
      for (int i = 0; i < k; ++i) {
        CHECK(iov[i].iov_len > 0, "no empty iovec");
        got.append((const char*)iov[i].iov_base, iov[i].iov_len);
      }
      CHECK(got == whole.substr(off, n), "concatenation equals the slice");
    }
  }
}

void test_writev_all() {
  int fds[2];
  if (socketpair(AF_UNIX, SOCK_STREAM, 0, fds) != 0) abort();
  int tiny = 1;  // the kernel rounds this up to its minimum
  setsockopt(fds[1], SOL_SOCKET, SO_SNDBUF, &tiny, sizeof(tiny));
  std::string a = pattern(9, 8), b = pattern(5, 9), c = pattern(1000003, 10), d = pattern(1, 11);
  std::string sent = a + b + c + d, got;
  std::thread reader([&]() {
    char buf[1531];  // odd-sized reads so writes end inside an iovec
    ssize_t r;
    while ((r = read(fds[0], buf, sizeof(buf))) > 0) got.append(buf, r);
  });
  struct iovec iov[4] = {{(void*)a.data(), a.size()}, {(void*)b.data(), b.size()},
                         {(void*)c.data(), c.size()}, {(void*)d.data(), d.size()}};
  CHECK(writev_all(fds[1], iov, 4), "writev_all");
  close(fds[1]);
  reader.join();
  CHECK(got == sent, "received bytes equal sent bytes");
  // a peer that is gone is a false, not a signal
  struct iovec one{(void*)a.data(), a.size()};
  close(fds[0]);
  if (socketpair(AF_UNIX, SOCK_STREAM, 0, fds) != 0) abort();
  close(fds[0]);
  CHECK(!writev_all(fds[1], &one, 1), "write to a closed peer");
  close(fds[1]);
  CHECK(writev_all(-1, &one, 0), "nothing to write");
}

void test_cap_retained() {
  std::string s(RecvBuf::kRetainCap + 1, 'x');
  cap_retained(s);
  CHECK(s.empty() && s.capacity() < 64, "oversized string given back");
  std::string t(1000, 'y');
  cap_retained(t);
  CHECK(t.size() == 1000, "small string kept");
}

}  // namespace

int main() {
  signal(SIGPIPE, SIG_IGN);
  test_delivery();
  test_buffer_transitions();
  test_length_limit();
  test_strip_padding();
  test_first_grpc_message();
  test_settings();
  test_wire_literals();
  test_percent();
  test_payload_iov();
  test_writev_all();
  test_cap_retained();
  if (failures) {
    fprintf(stderr, "h2frame selftest: %d failure(s)\n", failures);
    return 1;
  }
  printf("h2frame selftest OK\n");
  return 0;
}
