// h2frame.h — HTTP/2 framing and gRPC byte work shared by the server
// connection and the client in etransport.cpp, and by the stand-alone
// sanitizer self-test (h2frame_selftest.cpp). Header-only and free of
// Python; extracted verbatim from etransport.cpp like h2core.h, so the
// self-test exercises EXACTLY the code that runs as root in kube-system.
#pragma once

#include <algorithm>
#include <arpa/inet.h>
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <sys/uio.h>
#include <unistd.h>

#include "h2core.h"

namespace h2frame {

// ---------------------------------------------------------------- constants
constexpr uint8_t F_DATA = 0x0, F_HEADERS = 0x1, F_PRIORITY = 0x2, F_RST = 0x3,
                  F_SETTINGS = 0x4, F_PING = 0x6, F_GOAWAY = 0x7, F_WINUP = 0x8,
                  F_CONT = 0x9;
constexpr uint8_t FLAG_END_STREAM = 0x1, FLAG_ACK = 0x1, FLAG_END_HEADERS = 0x4,
                  FLAG_PADDED = 0x8, FLAG_PRIORITY = 0x20;
constexpr uint16_t S_HEADER_TABLE_SIZE = 0x1, S_MAX_CONCURRENT = 0x3,
                   S_INITIAL_WINDOW = 0x4, S_MAX_FRAME = 0x5;
constexpr int64_t DEFAULT_WINDOW = 65535;
constexpr int64_t RECV_WINDOW = 32ll * 1024 * 1024;
constexpr uint32_t OUR_MAX_FRAME = 1024 * 1024;
constexpr uint32_t OUR_MAX_CONCURRENT = 1024;
constexpr char kPreface[] = "PRI * HTTP/2.0\r\n\r\nSM\r\n\r\n";
constexpr size_t kPrefaceLen = sizeof(kPreface) - 1;

// precomputed response blocks (mirror egrpc/server.py: :status 200 indexed,
// content-type literal w/ static name index 31; grpc-status literal)
constexpr uint8_t kRespHdrBlock[] = {
    0x88, 0x0f, 0x10, 16, 'a','p','p','l','i','c','a','t','i','o','n','/','g','r','p','c'};
constexpr uint8_t kOkTrailerBlock[] = {
    0x00, 0x0b, 'g','r','p','c','-','s','t','a','t','u','s', 0x01, '0'};

// ---------------------------------------------------------------- builders
inline void put_frame_header(uint8_t* p, uint32_t len, uint8_t type, uint8_t flags,
                             uint32_t sid) {
  p[0] = len >> 16; p[1] = len >> 8; p[2] = len;
  p[3] = type; p[4] = flags;
  uint32_t s = htonl(sid);
  memcpy(p + 5, &s, 4);
}

inline void put_grpc_prefix(uint8_t* p, size_t msg_len) {
  p[0] = 0;
  uint32_t len = htonl((uint32_t)msg_len);
  memcpy(p + 1, &len, 4);
}

// one whole WINDOW_UPDATE frame, 13 bytes
inline void put_window_update(uint8_t* p, uint32_t sid, uint32_t inc) {
  put_frame_header(p, 4, F_WINUP, 0, sid);
  inc = htonl(inc);
  memcpy(p + 9, &inc, 4);
}

// the 17-byte answer to a PING carrying `opaque8`
inline void put_ping_ack(uint8_t* p, const uint8_t* opaque8) {
  put_frame_header(p, 8, F_PING, FLAG_ACK, 0);
  memcpy(p + 9, opaque8, 8);
}

// What either side says first: our SETTINGS and the connection window
// grant. The client puts the connection preface in front and leaves
// MAX_CONCURRENT out. Returns the length written, kMaxPreamble at most.
constexpr size_t kMaxPreamble = kPrefaceLen + 9 + 18 + 13;
inline size_t put_preamble(uint8_t* out, bool client) {
  uint8_t* p = out;
  if (client) { memcpy(p, kPreface, kPrefaceLen); p += kPrefaceLen; }
  put_frame_header(p, client ? 12 : 18, F_SETTINGS, 0, 0); p += 9;
  auto put_setting = [&](uint16_t k, uint32_t v) {
    p[0] = k >> 8; p[1] = k; uint32_t nv = htonl(v); memcpy(p + 2, &nv, 4); p += 6;
  };
  put_setting(S_MAX_FRAME, OUR_MAX_FRAME);
  put_setting(S_INITIAL_WINDOW, (uint32_t)RECV_WINDOW);
  if (!client) put_setting(S_MAX_CONCURRENT, OUR_MAX_CONCURRENT);
  put_window_update(p, 0, (uint32_t)(RECV_WINDOW - DEFAULT_WINDOW));
  return p + 13 - out;
}

inline std::string percent_encode(const std::string& msg) {
  std::string out;
  for (unsigned char c : msg) {
    if (c >= 0x20 && c <= 0x7e && c != '%') out.push_back(c);
    else {
      char buf[4];
      snprintf(buf, sizeof(buf), "%%%02X", c);
      out += buf;
    }
  }
  return out;
}

// grpc-message is percent-encoded; decode minimally (an escape cut short
// by the end of the input stays as it is)
inline std::string percent_decode(const std::string& msg) {
  std::string dec;
  for (size_t i = 0; i < msg.size(); ++i) {
    if (msg[i] == '%' && i + 2 < msg.size()) {
      dec.push_back((char)strtol(msg.substr(i + 1, 2).c_str(), nullptr, 16));
      i += 2;
    } else dec.push_back(msg[i]);
  }
  return dec;
}

inline void hpack_put_int(std::string* out, uint64_t v, int prefix, uint8_t flags) {
  uint64_t limit = (1u << prefix) - 1;
  if (v < limit) { out->push_back((char)(flags | v)); return; }
  out->push_back((char)(flags | limit));
  v -= limit;
  while (v >= 128) { out->push_back((char)(0x80 | (v & 0x7f))); v >>= 7; }
  out->push_back((char)v);
}

// grpc-status + grpc-message literals only — NO pseudo-headers. Used both
// as a trailers-only response (see error_trailer_block) and as real
// trailers after response HEADERS already went out: a :status in trailers
// is a protocol error to strict HTTP/2 clients (grpc-go kubelet) and
// escalates an application error into connection teardown (advisor
// finding, round 1 — this is the native twin of the egrpc/server.py fix).
inline std::string status_trailer_fields(int code, const std::string& message) {
  std::string out;
  std::string code_s = std::to_string(code);
  out.push_back((char)0x00);
  std::string n1 = "grpc-status";
  hpack_put_int(&out, n1.size(), 7, 0);
  out += n1;
  hpack_put_int(&out, code_s.size(), 7, 0);
  out += code_s;
  std::string msg = percent_encode(message);
  out.push_back((char)0x00);
  std::string n2 = "grpc-message";
  hpack_put_int(&out, n2.size(), 7, 0);
  out += n2;
  hpack_put_int(&out, msg.size(), 7, 0);
  out += msg;
  return out;
}

// :status 200 + content-type prefix for a trailers-only error response
// (no HEADERS were sent yet for this stream)
inline std::string error_trailer_block(int code, const std::string& message) {
  std::string out((const char*)kRespHdrBlock, sizeof(kRespHdrBlock));
  out += status_trailer_fields(code, message);
  return out;
}

// ---------------------------------------------------------------- buffers
// Receive buffer shared by the server connection and the client: read()
// lands directly in its tail and frames are handed out as views into it, so
// a warm connection neither allocates nor copies per request. Capacity is
// kept across requests; above kRetainCap (one huge ListAndWatch snapshot or
// GetPreferredAllocation pool) it is given back once the traffic is small
// again.
//
// A view handed out by head() dies at the next read_more(): that call may
// overwrite, move or reallocate the storage.
class RecvBuf {
 public:
  static constexpr size_t kInitCap = 256 * 1024;
  static constexpr size_t kMinRead = 64 * 1024;
  static constexpr size_t kRetainCap = 4u << 20;

  RecvBuf() = default;
  RecvBuf(const RecvBuf&) = delete;
  RecvBuf& operator=(const RecvBuf&) = delete;
  ~RecvBuf() { free(data_); }

  size_t avail() const { return end_ - pos_; }
  size_t capacity() const { return cap_; }
  const uint8_t* head() const { return data_ + pos_; }
  void consume(size_t n) { pos_ += n; }
  void clear() { pos_ = end_ = 0; }

  // one read() into the tail, after making room for `need` contiguous
  // bytes from head(); returns what read() returned
  ssize_t read_more(int fd, size_t need) {
    size_t live = end_ - pos_;
    if (live == 0) pos_ = end_ = 0;
    size_t room = std::max(need > live ? need - live : (size_t)0, kMinRead);
    size_t req = live + room;
    if (cap_ > kRetainCap && req <= kRetainCap / 2) {
      reallocate(std::max(req, kInitCap));
    } else if (cap_ - end_ < room) {
      // compact only when the consumed prefix dominates; otherwise grow
      if (pos_ > 0 && pos_ >= live) {
        memmove(data_, data_ + pos_, live);
        pos_ = 0;
        end_ = live;
      }
      if (cap_ - end_ < room)
        reallocate(std::max({live + room, cap_ * 2, kInitCap}));
    }
    ssize_t r = ::read(fd, data_ + end_, cap_ - end_);
    if (r > 0) end_ += (size_t)r;
    return r;
  }

 private:
  // new storage holding only the live bytes, at the front
  void reallocate(size_t ncap) {
    size_t live = end_ - pos_;
    uint8_t* n = (uint8_t*)malloc(ncap);
    if (!n) throw std::bad_alloc();
    if (live) memcpy(n, data_ + pos_, live);
    free(data_);
    data_ = n;
    cap_ = ncap;
    pos_ = 0;
    end_ = live;
  }

  uint8_t* data_ = nullptr;
  size_t cap_ = 0, pos_ = 0, end_ = 0;
};

// one received frame; `body` points into a RecvBuf (see the lifetime note)
struct Frame {
  uint8_t type = 0, flags = 0;
  uint32_t sid = 0;
  const uint8_t* body = nullptr;
  size_t len = 0;
};

// parse the frame at the buffer head once `fill` has made it contiguous;
// fill(n) returns false (server) or throws (client) on I/O failure
template <class Fill>
bool next_frame(RecvBuf& buf, Fill&& fill, Frame* f, bool* oversize) {
  *oversize = false;
  if (!fill(9)) return false;
  const uint8_t* h = buf.head();
  uint32_t len = h[0] << 16 | h[1] << 8 | h[2];
  f->type = h[3];
  f->flags = h[4];
  uint32_t s;
  memcpy(&s, h + 5, 4);
  f->sid = ntohl(s) & 0x7fffffff;
  if (len > 64u * 1024 * 1024) { *oversize = true; return false; }  // refuse absurd frames
  if (!fill(9 + (size_t)len)) return false;
  f->body = buf.head() + 9;  // re-read: the second fill may have moved it
  f->len = len;
  buf.consume(9 + (size_t)len);
  return true;
}

// writev() until every byte is out; the iovec array is consumed
inline bool writev_all(int fd, struct iovec* iov, int cnt) {
  while (cnt > 0) {
    ssize_t w = ::writev(fd, iov, cnt);
    if (w <= 0) {
      if (w < 0 && errno == EINTR) continue;
      return false;
    }
    size_t left = (size_t)w;
    while (cnt > 0 && left >= iov->iov_len) {
      left -= iov->iov_len;
      ++iov;
      --cnt;
    }
    if (cnt > 0 && left) {
      iov->iov_base = (uint8_t*)iov->iov_base + left;
      iov->iov_len -= left;
    }
  }
  return true;
}

// iovecs for bytes [off, off+n) of the logical payload prefix5 ++ msg
inline int payload_iov(struct iovec* iov, const uint8_t* prefix5, const uint8_t* msg,
                       size_t off, size_t n) {
  int k = 0;
  if (off < 5 && n) {
    size_t m = std::min(n, 5 - off);
    iov[k].iov_base = (void*)(prefix5 + off);
    iov[k].iov_len = m;
    ++k;
    off += m;
    n -= m;
  }
  if (n) {
    iov[k].iov_base = (void*)(msg + (off - 5));
    iov[k].iov_len = n;
    ++k;
  }
  return k;
}

// keep a reused string's capacity bounded (same policy as RecvBuf)
inline void cap_retained(std::string& s) {
  if (s.capacity() > RecvBuf::kRetainCap) std::string().swap(s);
}

// ---------------------------------------------------------------- parsing
// What a HEADERS or DATA frame carries once the pad-length byte, the
// PRIORITY fields (HEADERS only, hence `priority`) and the padding are
// off: a view into f.body. False when the frame is malformed.
inline bool strip_padding(const Frame& f, bool priority, const uint8_t** p, size_t* n) {
  size_t off = 0, pad = 0;
  // an empty padded frame has no pad-length byte to read
  if (f.flags & FLAG_PADDED) { pad = f.len ? f.body[0] : 0; off = 1; }
  if (priority && (f.flags & FLAG_PRIORITY)) off += 5;
  if (off > f.len || pad > f.len - off) return false;
  *p = f.body + off;
  *n = f.len - off - pad;
  return true;
}

// view of the first gRPC message in `body`; empty when incomplete
inline void first_grpc_message(const uint8_t* body, size_t n,
                               const uint8_t** msg, size_t* msg_len) {
  *msg = body;
  *msg_len = 0;
  if (n < 5) return;
  uint32_t len;
  memcpy(&len, body + 1, 4);
  len = ntohl(len);
  if (5 + (size_t)len > n) return;
  *msg = body + 5;
  *msg_len = len;
}

// Walks a SETTINGS payload (a trailing partial entry is ignored) and
// updates the peer's max frame size and initial window in place. Returns
// how far the initial window moved: every open stream's send window moves
// with it (RFC 7540 §6.9.2), which is the caller's to apply.
inline int64_t apply_settings(const uint8_t* body, size_t n, uint32_t* max_frame,
                              int64_t* initial_window) {
  int64_t before = *initial_window;
  for (size_t off = 0; off + 6 <= n; off += 6) {
    uint16_t k = body[off] << 8 | body[off + 1];
    uint32_t v;
    memcpy(&v, body + off + 2, 4);
    v = ntohl(v);
    if (k == S_MAX_FRAME) *max_frame = v;
    else if (k == S_INITIAL_WINDOW) *initial_window = v;
  }
  return *initial_window - before;
}

// increment of a WINDOW_UPDATE frame; false (ignore it) when malformed
inline bool window_increment(const Frame& f, uint32_t* inc) {
  if (f.len != 4) return false;
  memcpy(inc, f.body, 4);
  *inc = ntohl(*inc) & 0x7fffffff;
  return true;
}

// how many payload bytes the next DATA frame may carry; <= 0 means wait
inline int64_t send_budget(int64_t conn_window, int64_t stream_window,
                           uint32_t max_frame) {
  return std::min({conn_window, stream_window, (int64_t)max_frame});
}

}  // namespace h2frame
