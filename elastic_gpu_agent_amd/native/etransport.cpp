// _etransport — C++ data plane for the egrpc server (gRPC over HTTP/2 on
// unix sockets).
//
// The Python implementation in egrpc/server.py is the semantic reference
// (same frame handling, flow control and dispatch rules; it remains in-tree
// for differential testing via EGPU_PY_TRANSPORT=1). This core exists purely
// for latency: frame I/O, HPACK decoding and response assembly run without
// the interpreter; the GIL is taken only to invoke the Python handler.
// Measured: ~3-4× lower unary RTT than the Python loop on the same host.
//
// HPACK tables are generated from egrpc/hpack.py (hpack_tables.h) — the
// table the test-suite validates against libnghttp2.

#include <pybind11/pybind11.h>

#include <cxxabi.h>

#include <algorithm>
#include <arpa/inet.h>
#include <atomic>
#include <cerrno>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <csignal>
#include <execinfo.h>
#include <sys/socket.h>
#include <sys/uio.h>
#include <sys/un.h>
#include <thread>
#include <unistd.h>
#include <unordered_map>
#include <vector>

#include "hpack_tables.h"

namespace py = pybind11;

namespace {

// The pybind-free byte work: frames, buffers, header blocks (h2frame.h),
// HPACK and Huffman (h2core.h, which it includes). Included inside the
// unnamed namespace, as h2core.h always was here: every system header the
// two need is already in above, so only their own code lands here, with
// internal linkage. The module then exports none of it, nothing in the
// process can interpose it, and the hot-path calls (read_more, HPACK
// decode) stay direct and inlinable instead of going through the PLT.
#include "h2frame.h"

using namespace h2frame;
using h2core::HpackDecoder;
using h2core::trie_init;

// gRPC status of a failed call; default-constructed it is "none"
struct Status {
  Status() = default;
  Status(int c, std::string m) : failed(true), code(c), message(std::move(m)) {}
  bool failed = false;
  int code = 0;
  std::string message;
};

// GIL held. Copies a Python bytes object into *out; anything else is
// status 13 (INTERNAL) with the text `what`.
Status take_bytes(py::handle obj, std::string* out, const char* what) {
  char* rb;
  Py_ssize_t rn;
  if (PyBytes_AsStringAndSize(obj.ptr(), &rb, &rn) == 0) {
    out->assign(rb, rn);
    return {};
  }
  PyErr_Clear();
  return {13, what};
}

// false when the path does not fit a sockaddr_un
bool unix_addr(const std::string& path, sockaddr_un* addr) {
  *addr = sockaddr_un{};
  addr->sun_family = AF_UNIX;
  if (path.size() >= sizeof(addr->sun_path)) return false;
  strcpy(addr->sun_path, path.c_str());
  return true;
}

// ---------------------------------------------------------------- streams
struct StreamState {
  uint32_t id = 0;
  std::string path;
  std::string data;  // request body; unused when one DATA frame carries it all
  bool data_reserved = false;
  std::string header_accum;
  bool end_stream = false;
  bool end_headers = true;
  py::object ctx;  // Python ServerContext (set at dispatch; GIL to touch)
};

struct Handler {
  py::object fn;  // callable(request_bytes, ctx) -> bytes | iterator of bytes
  bool streaming = false;
};

class Connection;

struct CoreShared {
  std::unordered_map<std::string, Handler> handlers;
  py::object context_factory;   // callable() -> ctx
  py::object error_introspect;  // callable(exc) -> (code:int, message:str)
  std::atomic<bool> stopping{false};
  std::atomic<int> live_threads{0};  // conn + streaming threads in flight

  ~CoreShared() {
    // the last shared_ptr may be dropped from a connection thread that does
    // not hold the GIL; python members must be released under it
    if (!Py_IsInitialized()) {
      // interpreter gone: leak the references rather than crash
      for (auto& kv : handlers) kv.second.fn.release();
      context_factory.release();
      error_introspect.release();
      return;
    }
    py::gil_scoped_acquire gil;
    handlers.clear();
    context_factory = py::object();
    error_introspect = py::object();
  }
};

// ---------------------------------------------------------------- connection
class Connection : public std::enable_shared_from_this<Connection> {
 public:
  Connection(int fd, std::shared_ptr<CoreShared> core)
      : fd_(fd), core_(std::move(core)) {}

  void run() {
    try {
      run_inner();
    } catch (abi::__forced_unwind&) {
      // pthread_exit during interpreter finalization: must propagate
      throw;
    } catch (...) {
      // defensive: no other exception may escape a detached thread
    }
    finish();
  }

  // Runs `body` on a detached thread that is counted in live_threads (what
  // stop() drains) and keeps `conn` alive: a raw pointer would dangle once
  // the client disconnects and the server prunes the connection. `after`
  // runs once body is over, but not when the thread is being unwound.
  template <class Body, class After>
  static void launch_counted(std::shared_ptr<Connection> conn, Body body, After after) {
    conn->core_->live_threads.fetch_add(1);
    auto core = conn->core_;
    std::thread([conn, core, body, after]() {
      try {
        body();
      } catch (abi::__forced_unwind&) {
        core->live_threads.fetch_sub(1);
        throw;  // pthread_exit (interpreter finalization)
      } catch (...) {
        // a stray exception in a detached thread would std::terminate the
        // whole process; drop the connection instead
        conn->close_now();
      }
      after();
      core->live_threads.fetch_sub(1);
    }).detach();
  }

  void run_inner() {
    if (!expect_preface()) { return; }
    uint8_t hello[kMaxPreamble];  // our SETTINGS + connection window grant
    send_raw(hello, put_preamble(hello, /*client=*/false));
    while (!closed_.load()) {
      Frame f;
      if (!read_frame(&f)) break;
      process_frame(f, /*defer=*/false);
      while (!deferred_.empty()) {
        uint32_t id = deferred_.front();
        deferred_.pop_front();
        dispatch_buffered(id);
      }
      // bound per-connection recv-deficit bookkeeping: entries accumulate one
      // per stream id; safe to drop whenever no stream is open (conn thread
      // owns this map exclusively)
      if (stream_recv_deficit_.size() > 4096) {
        std::lock_guard<std::mutex> lk(streams_mu_);
        if (streams_.empty()) stream_recv_deficit_.clear();
      }
    }
  }

  void close_now() {
    closed_.store(true);
    ::shutdown(fd_, SHUT_RDWR);
  }

  bool closed() const { return closed_.load(); }

 private:
  // ---- io ----
  bool fill(size_t need) {
    while (buf_.avail() < need) {
      ssize_t r = buf_.read_more(fd_, need);
      if (r < 0 && errno == EINTR) continue;
      if (r <= 0) return false;
    }
    return true;
  }

  // f->body is a view into buf_: it dies at the next read_frame(), and
  // anything that can pump (send_message(pump=true), hence dispatch of a
  // unary call) reads frames. Finish with the view, or copy, before that.
  bool read_frame(Frame* f) {
    bool oversize;
    return next_frame(buf_, [this](size_t n) { return fill(n); }, f, &oversize);
  }

  void send_raw(const void* data, size_t n) {
    struct iovec iov{(void*)data, n};
    send_iov(&iov, 1);
  }

  void send_iov(struct iovec* iov, int cnt) {
    std::lock_guard<std::mutex> lk(write_mu_);
    if (!writev_all(fd_, iov, cnt)) closed_.store(true);
  }

  // ---- frame processing (mirrors egrpc/server.py) ----
  void process_frame(const Frame& f, bool defer) {
    const uint8_t type = f.type, flags = f.flags;
    const uint32_t sid = f.sid;
    const uint8_t* body = f.body;
    const size_t blen = f.len;
    switch (type) {
      case F_SETTINGS:
        if (!(flags & FLAG_ACK)) {
          {
            std::lock_guard<std::mutex> lk(win_mu_);
            int64_t delta =
                apply_settings(body, blen, &peer_max_frame_, &peer_initial_window_);
            for (auto& kv : stream_send_windows_) kv.second += delta;
            win_cv_.notify_all();
          }
          uint8_t ack[9];
          put_frame_header(ack, 0, F_SETTINGS, FLAG_ACK, 0);
          send_raw(ack, 9);
        }
        break;
      case F_PING:
        if (!(flags & FLAG_ACK) && blen == 8) {
          uint8_t p[17];
          put_ping_ack(p, body);
          send_raw(p, 17);
        }
        break;
      case F_WINUP: {
        uint32_t inc;
        if (!window_increment(f, &inc)) break;
        std::lock_guard<std::mutex> lk(win_mu_);
        if (sid == 0) conn_send_window_ += inc;
        else stream_window_ref(sid) += inc;
        win_cv_.notify_all();
        break;
      }
      case F_HEADERS: {
        StreamState* stp;
        {
          std::lock_guard<std::mutex> lk(streams_mu_);
          stp = &streams_[sid];
        }
        auto& st = *stp;
        st.id = sid;
        const uint8_t* block;
        size_t block_len;
        if (!strip_padding(f, /*priority=*/true, &block, &block_len)) {
          std::lock_guard<std::mutex> lk(streams_mu_);
          auto it = streams_.find(sid);
          if (it != streams_.end()) drop_stream(it);
          break;
        }
        st.end_stream = st.end_stream || (flags & FLAG_END_STREAM);
        if (flags & FLAG_END_HEADERS) {
          // the view is done with once decoded; dispatch may pump
          decode_headers(st, block, block_len);
          if (st.end_stream) queue_dispatch(sid, defer);
        } else {
          st.end_headers = false;
          st.header_accum.assign((const char*)block, block_len);
          cont_sid_ = sid;
        }
        break;
      }
      case F_CONT: {
        StreamState* stp = find_stream(cont_sid_);
        if (!stp) break;
        auto& st = *stp;
        st.header_accum.append((const char*)body, blen);
        if (flags & FLAG_END_HEADERS) {
          st.end_headers = true;
          decode_headers(st, (const uint8_t*)st.header_accum.data(),
                         st.header_accum.size());
          st.header_accum.clear();
          cont_sid_ = 0;
          if (st.end_stream) queue_dispatch(st.id, defer);
        }
        break;
      }
      case F_DATA: {
        StreamState* stp = find_stream(sid);
        if (!stp) break;
        auto& st = *stp;
        const uint8_t* chunk;
        size_t chunk_len;
        if (!strip_padding(f, /*priority=*/false, &chunk, &chunk_len)) break;
        if (blen) replenish(sid, blen, flags & FLAG_END_STREAM);
        bool end = flags & FLAG_END_STREAM;
        if (end && !defer && st.data.empty()) {
          // whole body in one frame: dispatch straight from the view. The
          // handler's bytes object is built before anything can pump.
          st.end_stream = true;
          dispatch(st, chunk, chunk_len);
          break;  // `chunk` and `st` are dead here
        }
        st.data.append((const char*)chunk, chunk_len);
        if (!st.data_reserved && st.data.size() >= 5) {
          // size the body once from the gRPC length prefix, bounded by what
          // flow control lets the peer have in flight
          st.data_reserved = true;
          uint32_t mlen;
          memcpy(&mlen, st.data.data() + 1, 4);
          size_t want = 5 + (size_t)ntohl(mlen);
          if (!end) st.data.reserve(std::min(want, (size_t)RECV_WINDOW));
        }
        if (end) {
          st.end_stream = true;
          queue_dispatch(sid, defer);
        }
        break;
      }
      case F_RST: {
        std::lock_guard<std::mutex> lk(streams_mu_);
        auto it = streams_.find(sid);
        if (it != streams_.end()) {
          cancel_ctx(it->second);
          drop_stream(it);
        }
        break;
      }
      case F_GOAWAY:
        closed_.store(true);
        break;
      default:
        break;  // PRIORITY / PUSH_PROMISE / unknown: ignore
    }
  }

  void decode_headers(StreamState& st, const uint8_t* block, size_t n) {
    std::vector<std::pair<std::string, std::string>> hdrs;
    if (!decoder_.decode(block, n, &hdrs)) {
      closed_.store(true);  // HPACK state is unrecoverable per-connection
      return;
    }
    for (auto& h : hdrs)
      if (h.first == ":path") st.path = h.second;
  }

  void replenish(uint32_t sid, size_t consumed, bool stream_done) {
    conn_recv_deficit_ += consumed;
    stream_recv_deficit_[sid] += consumed;
    uint8_t upd[2 * 13];
    size_t upd_len = 0;
    auto add = [&](uint32_t id, uint32_t inc) {
      put_window_update(upd + upd_len, id, inc);
      upd_len += 13;
    };
    if (conn_recv_deficit_ >= RECV_WINDOW / 2) {
      add(0, (uint32_t)conn_recv_deficit_);
      conn_recv_deficit_ = 0;
    }
    if (stream_recv_deficit_[sid] >= RECV_WINDOW / 2 && !stream_done) {
      add(sid, (uint32_t)stream_recv_deficit_[sid]);
      stream_recv_deficit_[sid] = 0;
    }
    if (upd_len) send_raw(upd, upd_len);
  }

  int64_t& stream_window_ref(uint32_t sid) {
    auto it = stream_send_windows_.find(sid);
    if (it == stream_send_windows_.end())
      it = stream_send_windows_.emplace(sid, peer_initial_window_).first;
    return it->second;
  }

  // ---- sending with flow control ----
  // One gRPC message (5-byte prefix + msg) as DATA frames, straight from the
  // caller's memory: per frame one writev of frame header, prefix part and
  // message part. pump=true may only be used from the connection thread; it
  // reads frames while the window is closed, so every earlier frame view is
  // dead once this returns.
  bool send_message(uint32_t sid, const uint8_t* msg, size_t msg_len, bool pump) {
    uint8_t prefix[5];
    put_grpc_prefix(prefix, msg_len);
    size_t off = 0, total = 5 + msg_len;
    while (off < total) {
      int64_t avail;
      {
        std::lock_guard<std::mutex> lk(win_mu_);
        avail = send_budget(conn_send_window_, stream_window_ref(sid), peer_max_frame_);
      }
      if (avail <= 0) {
        if (closed_.load()) return false;
        if (pump) {
          Frame f;
          if (!read_frame(&f)) { closed_.store(true); return false; }
          process_frame(f, /*defer=*/true);
        } else {
          std::unique_lock<std::mutex> lk(win_mu_);
          win_cv_.wait_for(lk, std::chrono::milliseconds(100));
        }
        continue;
      }
      size_t n = std::min((size_t)avail, total - off);
      uint8_t hdr[9];
      put_frame_header(hdr, n, F_DATA, 0, sid);
      struct iovec iov[3];
      iov[0].iov_base = hdr;
      iov[0].iov_len = 9;
      int cnt = 1 + payload_iov(iov + 1, prefix, msg, off, n);
      send_iov(iov, cnt);
      {
        std::lock_guard<std::mutex> lk(win_mu_);
        conn_send_window_ -= n;
        stream_window_ref(sid) -= n;
      }
      off += n;
    }
    return true;
  }

  void send_headers_frame(uint32_t sid, const uint8_t* block, size_t n, uint8_t flags) {
    uint8_t hdr[9];
    put_frame_header(hdr, n, F_HEADERS, flags, sid);
    struct iovec iov[2] = {{hdr, 9}, {(void*)block, n}};
    send_iov(iov, 2);
  }

  void send_trailers(uint32_t sid, const uint8_t* block, size_t n) {
    send_headers_frame(sid, block, n, FLAG_END_HEADERS | FLAG_END_STREAM);
  }

  void send_error(uint32_t sid, int code, const std::string& msg) {
    std::string block = error_trailer_block(code, msg);
    send_trailers(sid, (const uint8_t*)block.data(), block.size());
  }

  void send_unary_response(uint32_t sid, const uint8_t* msg, size_t msg_len) {
    size_t payload_len = 5 + msg_len;
    bool fits;
    {
      std::lock_guard<std::mutex> lk(win_mu_);
      fits = (int64_t)payload_len <=
             send_budget(conn_send_window_, stream_window_ref(sid), peer_max_frame_);
    }
    if (fits) {
      // one write: headers + data + trailers, the message sent in place
      uint8_t head[9 + sizeof(kRespHdrBlock) + 9 + 5];
      uint8_t tail[9 + sizeof(kOkTrailerBlock)];
      uint8_t* p = head;
      put_frame_header(p, sizeof(kRespHdrBlock), F_HEADERS, FLAG_END_HEADERS, sid);
      p += 9;
      memcpy(p, kRespHdrBlock, sizeof(kRespHdrBlock));
      p += sizeof(kRespHdrBlock);
      put_frame_header(p, payload_len, F_DATA, 0, sid);
      p += 9;
      put_grpc_prefix(p, msg_len);
      put_frame_header(tail, sizeof(kOkTrailerBlock), F_HEADERS,
                       FLAG_END_HEADERS | FLAG_END_STREAM, sid);
      memcpy(tail + 9, kOkTrailerBlock, sizeof(kOkTrailerBlock));
      struct iovec iov[3] = {{head, sizeof(head)}, {(void*)msg, msg_len},
                             {tail, sizeof(tail)}};
      send_iov(iov, 3);
      std::lock_guard<std::mutex> lk(win_mu_);
      conn_send_window_ -= payload_len;
      stream_window_ref(sid) -= payload_len;
    } else {
      send_headers_frame(sid, kRespHdrBlock, sizeof(kRespHdrBlock), FLAG_END_HEADERS);
      send_message(sid, msg, msg_len, /*pump=*/true);
      send_trailers(sid, kOkTrailerBlock, sizeof(kOkTrailerBlock));
    }
  }

  // ---- dispatch ----
  using StreamMap = std::unordered_map<uint32_t, StreamState>;

  // the entry stays put until it is erased (unordered_map never moves nodes)
  StreamState* find_stream(uint32_t sid) {
    std::lock_guard<std::mutex> lk(streams_mu_);
    auto it = streams_.find(sid);
    return it == streams_.end() ? nullptr : &it->second;
  }

  // Erase one stream; the caller holds streams_mu_. The GIL must be held to
  // drop py objects, and with the interpreter gone the reference is leaked
  // rather than touched.
  void drop_stream(StreamMap::iterator it) {
    py::object& ctx = it->second.ctx;
    if (ctx && Py_IsInitialized()) {
      py::gil_scoped_acquire gil;
      ctx = py::object();
    } else {
      ctx.release();
    }
    streams_.erase(it);
  }

  void queue_dispatch(uint32_t sid, bool defer) {
    if (defer) deferred_.push_back(sid);
    else dispatch_buffered(sid);
  }

  // dispatch a stream whose body was accumulated in st.data
  void dispatch_buffered(uint32_t sid) {
    if (StreamState* st = find_stream(sid))
      dispatch(*st, (const uint8_t*)st->data.data(), st->data.size());
  }

  void cancel_ctx(StreamState& st) {
    if (!st.ctx || st.ctx.is_none()) return;
    if (!Py_IsInitialized()) return;
    py::gil_scoped_acquire gil;
    try {
      st.ctx.attr("cancelled").attr("set")();
    } catch (...) {}
    st.ctx = py::object();
  }

  // `body` is the stream's whole request body: st.data, or a frame view
  // that is only valid until the handler's bytes object has been built
  void dispatch(StreamState& st, const uint8_t* body, size_t body_len) {
    auto it = core_->handlers.find(st.path);
    uint32_t sid = st.id;
    if (it == core_->handlers.end()) {
      send_error(sid, 2 /*UNKNOWN*/, "unknown method " + st.path);
      erase_stream(sid);
      return;
    }
    const uint8_t* req;
    size_t req_len;
    first_grpc_message(body, body_len, &req, &req_len);
    if (it->second.streaming) {
      // streaming handlers run on their own thread. All py::object copies are
      // made AND destroyed under the GIL: the thread owns a heap pack and
      // deletes it while holding the GIL.
      struct Pack {
        py::object fn, ctx;
        std::string request;
      };
      Pack* pack = nullptr;
      {
        py::gil_scoped_acquire gil;
        pack = new Pack{it->second.fn, core_->context_factory(),
                        std::string((const char*)req, req_len)};
        st.ctx = pack->ctx;
      }
      Connection* self = this;  // kept alive by the launcher's shared_ptr
      launch_counted(
          shared_from_this(),
          [self, pack, sid]() {
            self->run_streaming(pack->fn, pack->ctx, pack->request, sid);
          },
          [pack]() {
            if (Py_IsInitialized()) {
              py::gil_scoped_acquire gil;
              delete pack;
            }
          });
      return;
    }
    // unary: inline on the connection thread. The response is copied once
    // into a buffer this connection keeps, so the handler's result can be
    // dropped under the GIL already held and then sent without it.
    std::string& response = resp_buf_;
    Status err;
    {
      py::gil_scoped_acquire gil;
      try {
        py::object ctx = core_->context_factory();
        st.ctx = ctx;
        py::object result = it->second.fn(py::bytes((const char*)req, req_len), ctx);
        err = take_bytes(result, &response, "handler returned non-bytes");
      } catch (py::error_already_set& e) {
        err = introspect_error(e);
      }
    }
    if (err.failed) send_error(sid, err.code, err.message);
    else send_unary_response(sid, (const uint8_t*)response.data(), response.size());
    cap_retained(response);
    erase_stream(sid);
  }

  Status introspect_error(py::error_already_set& e) {
    // core_->error_introspect(exc_value) -> (code, message); GIL held
    try {
      py::object val = e.value();
      py::object r = core_->error_introspect(val);
      auto t = r.cast<py::tuple>();
      return {t[0].cast<int>(), t[1].cast<std::string>()};
    } catch (...) {
      return {2, "handler error"};
    }
  }

  void run_streaming(py::object& fn, py::object& ctx_ref, const std::string& request, uint32_t sid) {
    py::object ctx;
    {
      py::gil_scoped_acquire gil;
      ctx = ctx_ref;
    }
    send_headers_frame(sid, kRespHdrBlock, sizeof(kRespHdrBlock), FLAG_END_HEADERS);
    Status err;
    py::object iter;
    {
      py::gil_scoped_acquire gil;
      try {
        iter = py::iter(fn(py::bytes(request), ctx));
      } catch (py::error_already_set& e) {
        err = introspect_error(e);
      }
    }
    while (!err.failed && !closed_.load()) {
      std::string item;
      bool done = false;
      {
        py::gil_scoped_acquire gil;
        try {
          py::object obj = py::reinterpret_steal<py::object>(PyIter_Next(iter.ptr()));
          if (obj) err = take_bytes(obj, &item, "stream yielded non-bytes");
          else if (PyErr_Occurred()) throw py::error_already_set();
          else done = true;
        } catch (py::error_already_set& e) {
          err = introspect_error(e);
        }
      }
      if (done || err.failed) break;
      if (!send_message(sid, (const uint8_t*)item.data(), item.size(), /*pump=*/false))
        break;
    }
    {
      // drop the iterator/ctx with the GIL held
      py::gil_scoped_acquire gil;
      iter = py::object();
      ctx = py::object();
    }
    if (closed_.load()) { erase_stream(sid); return; }
    if (err.failed) {
      // response HEADERS already went out at the top: emit TRAILERS without
      // pseudo-headers (a second :status is a protocol error to grpc-go)
      std::string block = status_trailer_fields(err.code, err.message);
      send_trailers(sid, (const uint8_t*)block.data(), block.size());
    } else {
      send_trailers(sid, kOkTrailerBlock, sizeof(kOkTrailerBlock));
    }
    erase_stream(sid);
  }

  void erase_stream(uint32_t sid) {
    {
      std::lock_guard<std::mutex> lk(streams_mu_);
      auto it = streams_.find(sid);
      if (it != streams_.end()) drop_stream(it);
    }
    std::lock_guard<std::mutex> lk(win_mu_);
    stream_send_windows_.erase(sid);
  }

  bool expect_preface() {
    if (!fill(kPrefaceLen)) return false;
    bool ok = memcmp(buf_.head(), kPreface, kPrefaceLen) == 0;
    buf_.consume(kPrefaceLen);
    return ok;
  }

  void finish() {
    closed_.store(true);
    {
      std::lock_guard<std::mutex> lk(streams_mu_);
      while (!streams_.empty()) {
        cancel_ctx(streams_.begin()->second);
        drop_stream(streams_.begin());
      }
    }
    {
      std::lock_guard<std::mutex> lk(win_mu_);
      win_cv_.notify_all();
    }
    ::close(fd_);
  }

  int fd_;
  std::shared_ptr<CoreShared> core_;
  RecvBuf buf_;
  std::string resp_buf_;  // unary response in flight (connection thread only)
  std::atomic<bool> closed_{false};
  HpackDecoder decoder_;
  std::unordered_map<uint32_t, StreamState> streams_;
  std::deque<uint32_t> deferred_;
  uint32_t cont_sid_ = 0;
  // flow control
  uint32_t peer_max_frame_ = 16384;
  int64_t peer_initial_window_ = DEFAULT_WINDOW;
  int64_t conn_send_window_ = DEFAULT_WINDOW;
  std::unordered_map<uint32_t, int64_t> stream_send_windows_;
  int64_t conn_recv_deficit_ = 0;
  std::unordered_map<uint32_t, int64_t> stream_recv_deficit_;
  std::mutex win_mu_;
  std::condition_variable win_cv_;
  std::mutex write_mu_;
  std::mutex streams_mu_;
};

// ---------------------------------------------------------------- server
class ServerCore {
 public:
  ServerCore() : core_(std::make_shared<CoreShared>()) {}

  void add_handler(const std::string& path, py::object fn, bool streaming) {
    core_->handlers[path] = Handler{std::move(fn), streaming};
  }

  void set_context_factory(py::object f) { core_->context_factory = std::move(f); }
  void set_error_introspect(py::object f) { core_->error_introspect = std::move(f); }

  void bind_unix(const std::string& path) {
    ::unlink(path.c_str());
    listen_fd_ = ::socket(AF_UNIX, SOCK_STREAM, 0);
    if (listen_fd_ < 0) throw std::runtime_error("socket() failed");
    sockaddr_un addr;
    if (!unix_addr(path, &addr)) throw std::runtime_error("socket path too long");
    if (::bind(listen_fd_, (sockaddr*)&addr, sizeof(addr)) != 0)
      throw std::runtime_error("bind() failed: " + path);
    if (::listen(listen_fd_, 128) != 0) throw std::runtime_error("listen() failed");
    path_ = path;
  }

  // Pre-fork mode: accept on a listening fd inherited from the parent
  // (multiple worker processes accept on the SAME fd; the kernel load-
  // balances connections). The parent owns the socket path — stop() must
  // not unlink it, so path_ stays empty.
  void adopt_fd(int fd) {
    listen_fd_ = fd;
    path_.clear();
  }

  void start() {
    // A stop() from another thread can come between bind and start (a plugin
    // server stopped while its own thread is still bringing it up). The
    // accept thread must then not be created: stop() has already done its
    // join, and a joinable std::thread left in a ServerCore aborts the
    // process when the object is destroyed.
    std::lock_guard<std::mutex> stop_lk(stop_mu_);
    if (stopped_ || accept_thread_.joinable()) return;
    accept_thread_ = std::thread([this]() { accept_loop(); });
  }

  void stop() {
    // idempotent + thread-safe: shutdown paths (signal handler, watch loop,
    // test teardown) may race
    std::lock_guard<std::mutex> stop_lk(stop_mu_);
    if (stopped_) return;
    stopped_ = true;
    core_->stopping.store(true);
    if (listen_fd_ >= 0) {
      ::shutdown(listen_fd_, SHUT_RDWR);
      ::close(listen_fd_);
      listen_fd_ = -1;
    }
    {
      std::lock_guard<std::mutex> lk(conns_mu_);
      for (auto& c : conns_) c->close_now();
    }
    if (accept_thread_.joinable()) accept_thread_.join();
    if (!path_.empty()) ::unlink(path_.c_str());
    // Drain detached connection/streaming threads (they exit promptly once
    // their sockets are shut down). Without this, interpreter finalization
    // can force-unwind a thread that holds a pybind GIL scope, whose
    // destructor then aborts the process. stop() is called WITHOUT the GIL
    // (call_guard), so in-flight Python handlers can finish.
    for (int i = 0; i < 500 && core_->live_threads.load() > 0; ++i) {
      struct timespec ts {0, 10 * 1000 * 1000};  // 10 ms
      nanosleep(&ts, nullptr);
    }
  }

  ~ServerCore() {
    // stop() must have been called from Python; guard anyway. The accept
    // thread never takes the GIL, so joining it here is safe.
    core_->stopping.store(true);
    if (listen_fd_ >= 0) {
      ::shutdown(listen_fd_, SHUT_RDWR);
      ::close(listen_fd_);
    }
    if (accept_thread_.joinable()) accept_thread_.join();
  }

 private:
  void accept_loop() {
    while (!core_->stopping.load()) {
      int fd = ::accept(listen_fd_, nullptr, nullptr);
      if (fd < 0) return;
      auto conn = std::make_shared<Connection>(fd, core_);
      {
        std::lock_guard<std::mutex> lk(conns_mu_);
        conns_.push_back(conn);
        if (conns_.size() > 64) {  // prune finished connections
          conns_.erase(
              std::remove_if(conns_.begin(), conns_.end(),
                             [](const std::shared_ptr<Connection>& c) {
                               return c->closed();
                             }),
              conns_.end());
        }
      }
      Connection* c = conn.get();
      Connection::launch_counted(conn, [c]() { c->run(); }, []() {});
    }
  }

  std::shared_ptr<CoreShared> core_;
  int listen_fd_ = -1;
  std::string path_;
  std::thread accept_thread_;
  std::mutex conns_mu_;
  std::vector<std::shared_ptr<Connection>> conns_;
  std::mutex stop_mu_;
  bool stopped_ = false;
};


// ---------------------------------------------------------------- client
// Blocking unary client connection. Python owns reconnect policy; this core
// owns one connected socket and performs whole unary calls with the GIL
// released. Streaming calls stay on the Python client implementation.
class ClientCore {
 public:
  explicit ClientCore(const std::string& path) : path_(path) {}

  ~ClientCore() { close_fd(); }

  void connect() {
    close_fd();
    fd_ = ::socket(AF_UNIX, SOCK_STREAM, 0);
    if (fd_ < 0) throw std::runtime_error("socket() failed");
    sockaddr_un addr;
    if (!unix_addr(path_, &addr)) {
      close_fd();
      throw std::runtime_error("socket path too long");
    }
    if (::connect(fd_, (sockaddr*)&addr, sizeof(addr)) != 0) {
      close_fd();
      throw std::runtime_error("connect failed: " + path_);
    }
    buf_.clear();
    next_stream_ = 1;
    decoder_ = HpackDecoder();
    peer_max_frame_ = 16384;
    peer_initial_window_ = DEFAULT_WINDOW;
    conn_send_window_ = DEFAULT_WINDOW;
    conn_recv_deficit_ = 0;
    uint8_t hello[kMaxPreamble];  // preface + SETTINGS + window grant
    write_all(hello, put_preamble(hello, /*client=*/true));
  }

  bool connected() const { return fd_ >= 0; }

  void close_fd() {
    if (fd_ >= 0) { ::close(fd_); fd_ = -1; }
  }

  // returns (grpc_status, response_bytes, grpc_message). Transport failures
  // throw std::runtime_error (Python resets + maps to UNAVAILABLE).
  py::tuple call_unary(py::bytes header_block_b, py::bytes message_b, double timeout_s) {
    // the arguments keep both bytes objects alive for the whole call, so the
    // request is sent from the caller's memory with the GIL released
    char *hb, *mb;
    Py_ssize_t hn, mn;
    if (PyBytes_AsStringAndSize(header_block_b.ptr(), &hb, &hn) != 0 ||
        PyBytes_AsStringAndSize(message_b.ptr(), &mb, &mn) != 0)
      throw py::error_already_set();
    int status = 0;
    const uint8_t* data = nullptr;
    size_t data_len = 0;
    std::string grpc_message, err;
    {
      py::gil_scoped_release release;
      try {
        do_call((const uint8_t*)hb, (size_t)hn, (const uint8_t*)mb, (size_t)mn,
                timeout_s, &status, &data, &data_len, &grpc_message);
      } catch (const std::exception& e) {
        err = e.what();
      }
    }
    if (!err.empty()) {
      cap_retained(rdata_);
      throw std::runtime_error(err);
    }
    // `data` points into rdata_, which lives until the next call
    py::tuple out = py::make_tuple(status, py::bytes((const char*)data, data_len),
                                   grpc_message);
    cap_retained(rdata_);
    return out;
  }

 private:
  void set_timeout(double seconds) {
    timeval tv{};
    if (seconds > 0) {
      tv.tv_sec = (time_t)seconds;
      tv.tv_usec = (suseconds_t)((seconds - tv.tv_sec) * 1e6);
    }
    setsockopt(fd_, SOL_SOCKET, SO_RCVTIMEO, &tv, sizeof(tv));
  }

  void write_all(const void* data, size_t n) {
    struct iovec iov{(void*)data, n};
    writev_all_or_throw(&iov, 1);
  }

  void writev_all_or_throw(struct iovec* iov, int cnt) {
    if (!writev_all(fd_, iov, cnt)) throw std::runtime_error("connection lost (write)");
  }

  bool fill(size_t need) {
    while (buf_.avail() < need) {
      ssize_t r = buf_.read_more(fd_, need);
      if (r == 0) throw std::runtime_error("connection closed");
      if (r < 0) {
        if (errno == EINTR) continue;
        if (errno == EAGAIN || errno == EWOULDBLOCK)
          throw std::runtime_error("timeout");
        throw std::runtime_error("connection lost (read)");
      }
    }
    return true;
  }

  // f->body is a view into buf_ and dies at the next read_frame()
  void read_frame(Frame* f) {
    bool oversize;
    if (!next_frame(buf_, [this](size_t n) { return fill(n); }, f, &oversize))
      throw std::runtime_error("oversize frame");
  }

  // conn-level frames; returns true if consumed
  bool handle_conn_frame(const Frame& f, int64_t* active_stream_window) {
    if (f.type == F_SETTINGS) {
      if (!(f.flags & FLAG_ACK)) {
        *active_stream_window +=
            apply_settings(f.body, f.len, &peer_max_frame_, &peer_initial_window_);
        uint8_t ack[9];
        put_frame_header(ack, 0, F_SETTINGS, FLAG_ACK, 0);
        write_all(ack, 9);
      }
      return true;
    }
    if (f.type == F_PING) {
      if (!(f.flags & FLAG_ACK) && f.len == 8) {
        uint8_t p[17];
        put_ping_ack(p, f.body);
        write_all(p, 17);
      }
      return true;
    }
    if (f.type == F_WINUP && f.sid == 0) {
      uint32_t inc;
      if (window_increment(f, &inc)) conn_send_window_ += inc;
      return true;
    }
    if (f.type == F_GOAWAY) throw std::runtime_error("server sent GOAWAY");
    return false;
  }

  void do_call(const uint8_t* header_block, size_t header_len, const uint8_t* message,
               size_t message_len, double timeout_s, int* status,
               const uint8_t** data, size_t* data_len, std::string* grpc_message) {
    set_timeout(timeout_s);
    uint32_t sid = next_stream_;
    next_stream_ += 2;
    int64_t stream_window = peer_initial_window_;

    // HEADERS ride in the first DATA frame's writev; every DATA frame is one
    // iovec group: frame header, its share of the 5-byte gRPC prefix, and
    // its share of the caller's bytes in place
    uint8_t prefix[5];
    put_grpc_prefix(prefix, message_len);
    uint8_t hhdr[9];
    put_frame_header(hhdr, header_len, F_HEADERS, FLAG_END_HEADERS, sid);
    bool headers_sent = false;
    size_t off = 0, total = 5 + message_len;
    while (true) {
      int64_t avail = send_budget(conn_send_window_, stream_window, peer_max_frame_);
      if (avail <= 0) {
        if (!headers_sent) {
          struct iovec hv[2] = {{hhdr, 9}, {(void*)header_block, header_len}};
          writev_all_or_throw(hv, 2);
          headers_sent = true;
        }
        Frame f;
        read_frame(&f);
        if (!handle_conn_frame(f, &stream_window)) {
          uint32_t inc;
          if (f.type == F_WINUP && f.sid == sid) {
            if (window_increment(f, &inc)) stream_window += inc;
          } else if (f.type == F_RST) {
            throw std::runtime_error("stream reset during send");
          }
        }
        continue;
      }
      size_t n = std::min(total - off, (size_t)avail);
      bool last = off + n >= total;
      uint8_t dhdr[9];
      put_frame_header(dhdr, n, F_DATA, last ? FLAG_END_STREAM : 0, sid);
      struct iovec iov[5];
      int cnt = 0;
      if (!headers_sent) {
        iov[cnt++] = {hhdr, 9};
        iov[cnt++] = {(void*)header_block, header_len};
        headers_sent = true;
      }
      iov[cnt++] = {dhdr, 9};
      cnt += payload_iov(iov + cnt, prefix, message, off, n);
      writev_all_or_throw(iov, cnt);
      conn_send_window_ -= n;
      stream_window -= n;
      off += n;
      if (last) break;
    }

    // response: DATA accumulates in a buffer this client keeps
    std::string& rdata = rdata_;
    rdata.clear();
    std::vector<std::pair<std::string, std::string>> headers;
    while (true) {
      Frame f;
      read_frame(&f);
      if (handle_conn_frame(f, &stream_window)) continue;
      const uint8_t type = f.type, flags = f.flags;
      const uint8_t* body = f.body;
      size_t blen = f.len;
      if (f.sid != sid) continue;
      if (type == F_HEADERS || type == F_CONT) {
        // a CONTINUATION carries neither padding nor PRIORITY fields
        if (type == F_HEADERS && !strip_padding(f, /*priority=*/true, &body, &blen))
          throw std::runtime_error("bad hpack from server");
        if (!decoder_.decode(body, blen, &headers))
          throw std::runtime_error("bad hpack from server");
        if (flags & FLAG_END_STREAM) {
          int st = 0;
          std::string msg;
          for (auto& h : headers) {
            if (h.first == "grpc-status") st = atoi(h.second.c_str());
            else if (h.first == "grpc-message") msg = h.second;
          }
          // `*data` is a view into rdata
          first_grpc_message((const uint8_t*)rdata.data(), rdata.size(), data, data_len);
          *status = st;
          *grpc_message = percent_decode(msg);
          return;
        }
      } else if (type == F_DATA) {
        rdata.append((const char*)body, blen);
        if (blen) {
          conn_recv_deficit_ += blen;
          if (conn_recv_deficit_ >= RECV_WINDOW / 2) {
            uint8_t f2[2 * 13];
            put_window_update(f2, 0, (uint32_t)conn_recv_deficit_);
            put_window_update(f2 + 13, sid, (uint32_t)conn_recv_deficit_);
            write_all(f2, sizeof(f2));
            conn_recv_deficit_ = 0;
          }
        }
        if (flags & FLAG_END_STREAM)
          throw std::runtime_error("stream ended without trailers");
      } else if (type == F_RST) {
        throw std::runtime_error("stream reset");
      }
    }
  }

  std::string path_;
  int fd_ = -1;
  RecvBuf buf_;
  std::string rdata_;  // response body of the call in flight
  uint32_t next_stream_ = 1;
  HpackDecoder decoder_;
  uint32_t peer_max_frame_ = 16384;
  int64_t peer_initial_window_ = DEFAULT_WINDOW;
  int64_t conn_send_window_ = DEFAULT_WINDOW;
  int64_t conn_recv_deficit_ = 0;
};

void fatal_backtrace(int sig) {
  void* frames[64];
  int n = backtrace(frames, 64);
  fprintf(stderr, "[etransport] FATAL signal %d, backtrace:\n", sig);
  backtrace_symbols_fd(frames, n, 2);
  signal(sig, SIG_DFL);
  raise(sig);
}

}  // namespace

// test hook: the C++ HPACK decoder exposed for the differential fuzz suite
class HpackTester {
 public:
  py::list decode(py::bytes data) {
    std::string raw = data;
    std::vector<std::pair<std::string, std::string>> out;
    if (!dec_.decode((const uint8_t*)raw.data(), raw.size(), &out))
      throw std::runtime_error("hpack decode failed");
    py::list result;
    for (auto& h : out)
      result.append(py::make_tuple(py::bytes(h.first), py::bytes(h.second)));
    return result;
  }

 private:
  HpackDecoder dec_;
};

PYBIND11_MODULE(_etransport, m) {
  trie_init();
  if (const char* dbg = getenv("EGPU_ETRANSPORT_DEBUG"); dbg && dbg[0] == '1') {
    // crash diagnostics for pool boxes without a debugger
    signal(SIGSEGV, fatal_backtrace);
    signal(SIGABRT, fatal_backtrace);
  }
  m.doc() = "C++ data plane for the egrpc server";
  py::class_<HpackTester>(m, "HpackTester")
      .def(py::init<>())
      .def("decode", &HpackTester::decode);
  py::class_<ClientCore>(m, "ClientCore")
      .def(py::init<const std::string&>())
      .def("connect", &ClientCore::connect, py::call_guard<py::gil_scoped_release>())
      .def("connected", &ClientCore::connected)
      .def("close", &ClientCore::close_fd)
      .def("call_unary", &ClientCore::call_unary);
  py::class_<ServerCore>(m, "ServerCore")
      .def(py::init<>())
      .def("add_handler", &ServerCore::add_handler)
      .def("set_context_factory", &ServerCore::set_context_factory)
      .def("set_error_introspect", &ServerCore::set_error_introspect)
      .def("bind_unix", &ServerCore::bind_unix)
      .def("adopt_fd", &ServerCore::adopt_fd)
      .def("start", &ServerCore::start, py::call_guard<py::gil_scoped_release>())
      .def("stop", &ServerCore::stop, py::call_guard<py::gil_scoped_release>());
}
