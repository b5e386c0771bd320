"""The native transport hands frames around as views into its receive buffer
and sends messages in place with writev. These tests drive a real ServerCore
over a unix socket with every framing the view lifetime rules have to
survive, and compare each exchange with the same exchange against the Python
transport (the semantic reference).

The handler answers with the request's length and sha256, so any byte that
was read from a buffer after it moved shows up as a wrong digest."""
import hashlib
import os
import socket
import struct

import pytest

from elastic_gpu_agent_amd import egrpc
from elastic_gpu_agent_amd.egrpc import core, hpack

BIG = 3 << 20  # 3 MiB


def digest_of(req: bytes) -> bytes:
    return struct.pack(">Q", len(req)) + hashlib.sha256(req).digest()


def blob(n: int, seed: int = 0) -> bytes:
    """n deterministic bytes with no short period (so a frame-sized shift or a
    repeated chunk changes the sha)."""
    out = bytearray()
    h = hashlib.sha256(b"blob%d" % seed).digest()
    while len(out) < n:
        out += h
        h = hashlib.sha256(h).digest()
    return bytes(out[:n])


def digest_handler(request: bytes, context) -> bytes:
    return digest_of(request)


def big_handler(request: bytes, context) -> bytes:
    # 3 MiB that depend on the request: a response built from a dead request
    # view would differ
    return blob(BIG - len(request), seed=len(request)) + request


def _start_server(sock: str) -> egrpc.Server:
    s = egrpc.Server()
    s.add_service("t.Views", {
        "Digest": egrpc.unary_unary(digest_handler),
        "Big": egrpc.unary_unary(big_handler),
    })
    s.bind_unix(sock)
    s.start()
    return s


@pytest.fixture(scope="module")
def servers(tmp_path_factory):
    """(native socket, python socket): the same service on both transports."""
    from helpers import short_tmp_base

    import tempfile

    with tempfile.TemporaryDirectory(prefix="egpu-tv-",
                                     dir=short_tmp_base("egpu-tv-")) as tmp:
        native = _start_server(os.path.join(tmp, "n.sock"))
        assert native._native is not None, "_etransport must be built"
        mp = pytest.MonkeyPatch()
        mp.setenv("EGPU_PY_TRANSPORT", "1")
        try:
            python = _start_server(os.path.join(tmp, "p.sock"))
        finally:
            mp.undo()
        assert python._native is None
        try:
            yield os.path.join(tmp, "n.sock"), os.path.join(tmp, "p.sock")
        finally:
            native.stop()
            python.stop()


# ---- through ClientCore -----------------------------------------------------

SIZES = [
    0, 1,
    16379, 16380,  # either side of the default 16,384 frame after the prefix
    65530, 65531,  # either side of the default 65,535 window
    core.OUR_MAX_FRAME - 5, core.OUR_MAX_FRAME - 4,  # one DATA frame -> two
    BIG,
]


@pytest.mark.parametrize("warm", [False, True], ids=["fresh", "warm"])
@pytest.mark.parametrize("size", SIZES)
def test_clientcore_request_sizes(servers, size, warm):
    """fresh: the request leaves before the server's SETTINGS arrive, so the
    default frame size and window apply; warm: the server's 1-MiB frames."""
    req = blob(size, seed=size)
    got = []
    for sock in servers:
        ch = egrpc.Channel(sock)
        assert ch._native is not None
        try:
            call = ch.unary_unary("/t.Views/Digest")
            if warm:
                assert call(b"w", timeout=10.0) == digest_of(b"w")
            got.append(call(req, timeout=20.0))
        finally:
            ch.close()
    assert got[0] == digest_of(req)
    assert got[0] == got[1]


def test_clientcore_large_small_large_one_connection(servers):
    """Compaction and capacity retention: a large call, 1,000 small ones and
    a large one again, all on one connection."""
    big1, big2 = blob(BIG, seed=1), blob(BIG + 4097, seed=2)
    smalls = [blob(i % 97, seed=i) for i in range(1000)]
    got = []
    for sock in servers:
        ch = egrpc.Channel(sock)
        try:
            call = ch.unary_unary("/t.Views/Digest")
            res = [call(big1, timeout=20.0)]
            res += [call(s, timeout=10.0) for s in smalls]
            res.append(call(big2, timeout=20.0))
            got.append(res)
        finally:
            ch.close()
    assert got[0] == [digest_of(big1)] + [digest_of(s) for s in smalls] + [digest_of(big2)]
    assert got[0] == got[1]


def test_clientcore_large_response(servers):
    """3 MiB back through ClientCore (which advertises a 32-MiB window, so
    the server sends it in 1-MiB frames from the handler's bytes in place)."""
    req = blob(1000, seed=9)
    got = []
    for sock in servers:
        ch = egrpc.Channel(sock)
        try:
            call = ch.unary_unary("/t.Views/Big")
            got.append(call(req, timeout=20.0))
            got.append(call(b"", timeout=20.0))
        finally:
            ch.close()
    assert got[0] == big_handler(req, None) and got[1] == big_handler(b"", None)
    assert got[:2] == got[2:]


# ---- raw-socket client ------------------------------------------------------

def _headers_block(path: bytes) -> bytes:
    return hpack.encode_headers([
        (b":method", b"POST"), (b":scheme", b"http"), (b":path", path),
        (b":authority", b"localhost"), (b"content-type", b"application/grpc"),
        (b"te", b"trailers"),
    ])


DIGEST, BIGPATH = b"/t.Views/Digest", b"/t.Views/Big"


class RawH2:
    """A minimal HTTP/2 client that sends exactly the frames it is told to.
    It advertises the protocol defaults (65,535 window, 16,384 frames) and
    grants window only as it consumes DATA."""

    def __init__(self, path: str):
        self.sock = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
        self.sock.settimeout(20.0)
        self.sock.connect(path)
        self.sock.sendall(core.PREFACE + core.settings_frame([]))
        self.buf = bytearray()
        self.decoder = hpack.Decoder()
        self.ping_acks = []
        self.streams = {}  # sid -> {"data", "headers", "done"}

    def close(self):
        self.sock.close()

    def send(self, *chunks: bytes):
        """each chunk goes out in a write of its own"""
        for c in chunks:
            self.sock.sendall(c)

    @staticmethod
    def frame(ftype: int, flags: int, sid: int, body: bytes = b"") -> bytes:
        return core.frame_header(len(body), ftype, flags, sid) + body

    def headers(self, sid: int, path: bytes, flags=core.FLAG_END_HEADERS) -> bytes:
        return self.frame(core.HEADERS, flags, sid, _headers_block(path))

    def data_frames(self, sid: int, message: bytes, chunk: int, end=True):
        """DATA frames of `chunk` payload bytes carrying the gRPC-framed message"""
        payload = core.grpc_frame(message)
        frames = []
        for off in range(0, len(payload), chunk):
            last = off + chunk >= len(payload)
            frames.append(self.frame(core.DATA,
                                     core.FLAG_END_STREAM if (last and end) else 0,
                                     sid, payload[off:off + chunk]))
        return frames

    def _read_frame(self):
        hdr = core.read_exact(self.sock, 9, self.buf)
        length, ftype, flags, sid = core.parse_frame_header(hdr)
        body = core.read_exact(self.sock, length, self.buf) if length else b""
        return ftype, flags, sid, bytes(body)

    def read_responses(self, sids):
        """-> {sid: (grpc_status, first message or None, DATA frame count)}"""
        for sid in sids:
            self.streams.setdefault(sid, {"data": bytearray(), "headers": [],
                                          "done": False, "frames": 0})
        while not all(self.streams[s]["done"] for s in sids):
            ftype, flags, sid, body = self._read_frame()
            if ftype == core.SETTINGS:
                if not flags & core.FLAG_ACK:
                    self.sock.sendall(core.settings_frame([], flags=core.FLAG_ACK))
            elif ftype == core.PING:
                if flags & core.FLAG_ACK:
                    self.ping_acks.append(body)
            elif ftype in (core.HEADERS, core.CONTINUATION) and sid in self.streams:
                st = self.streams[sid]
                st["headers"] += self.decoder.decode(body)
                if flags & core.FLAG_END_STREAM:
                    st["done"] = True
            elif ftype == core.DATA and sid in self.streams:
                st = self.streams[sid]
                st["data"] += body
                st["frames"] += 1
                if body:
                    self.sock.sendall(core.window_update(0, len(body))
                                      + core.window_update(sid, len(body)))
            elif ftype in (core.RST_STREAM, core.GOAWAY):
                raise AssertionError(f"server sent frame type {ftype}")
        out = {}
        for sid in sids:
            st = self.streams[sid]
            hmap = dict(st["headers"])
            msgs = list(core.parse_grpc_frames(bytes(st["data"])))
            out[sid] = (int(hmap.get(b"grpc-status", b"-1")),
                        msgs[0] if msgs else None, st["frames"])
        return out


def both(servers, script):
    """run script(conn) against the native and the Python server; the native
    result is returned after checking that the two agree"""
    results = []
    for sock in servers:
        conn = RawH2(sock)
        try:
            results.append(script(conn))
        finally:
            conn.close()
    assert results[0] == results[1], "native and Python transports disagree"
    return results[0]


def _strip_frame_counts(res):
    return {sid: (st, msg) for sid, (st, msg, _n) in res.items()}


def test_raw_one_byte_data_frames(servers):
    msg = blob(300, seed=3)

    def script(c):
        c.send(c.headers(1, DIGEST) + b"".join(c.data_frames(1, msg, 1)))
        return _strip_frame_counts(c.read_responses([1]))

    assert both(servers, script) == {1: (0, digest_of(msg))}


def test_raw_one_byte_data_frames_one_write_each(servers):
    """the same, each frame in its own write: the 5-byte prefix arrives over
    five frames and five reads"""
    msg = blob(40, seed=4)

    def script(c):
        c.send(c.headers(1, DIGEST), *c.data_frames(1, msg, 1))
        return _strip_frame_counts(c.read_responses([1]))

    assert both(servers, script) == {1: (0, digest_of(msg))}


def test_raw_frame_headers_split_across_writes(servers):
    msg = blob(100_000, seed=5)

    def script(c):
        c.send(c.headers(1, DIGEST))
        for f in c.data_frames(1, msg, 16384):
            c.send(f[:4], f[4:16], f[16:])  # header cut at 4; 7 body bytes with its rest
        res = c.read_responses([1])
        # the connection is still in step afterwards
        c.send(c.headers(3, DIGEST) + b"".join(c.data_frames(3, b"after", 16384)))
        res.update(c.read_responses([3]))
        return _strip_frame_counts(res)

    assert both(servers, script) == {1: (0, digest_of(msg)), 3: (0, digest_of(b"after"))}


def test_raw_padded_data_frames(servers):
    """pad length 0, an ordinary pad, and a frame that is nothing but padding
    (pad length equal to the remaining length)"""
    msg = blob(5000, seed=6)
    payload = core.grpc_frame(msg)

    def padded(sid, chunk, pad, flags=0):
        return RawH2.frame(core.DATA, core.FLAG_PADDED | flags, sid,
                           bytes([pad]) + chunk + b"\xee" * pad)

    def script(c):
        c.send(c.headers(1, DIGEST)
               + padded(1, payload[:3], 0)         # pad 0, prefix split
               + padded(1, payload[3:2000], 17)
               + padded(1, b"", 255)                # only padding
               + padded(1, payload[2000:], 0)
               + padded(1, b"", 9, core.FLAG_END_STREAM))  # END_STREAM on pure padding
        return _strip_frame_counts(c.read_responses([1]))

    assert both(servers, script) == {1: (0, digest_of(msg))}


def test_raw_padded_single_frame(servers):
    """the whole message in ONE padded END_STREAM frame: the view dispatch
    must drop the pad-length byte and the padding"""
    msg = blob(3000, seed=7)
    payload = core.grpc_frame(msg)

    def script(c):
        c.send(c.headers(1, DIGEST)
               + RawH2.frame(core.DATA, core.FLAG_PADDED | core.FLAG_END_STREAM, 1,
                             bytes([200]) + payload + b"\xdd" * 200))
        return _strip_frame_counts(c.read_responses([1]))

    assert both(servers, script) == {1: (0, digest_of(msg))}


def test_raw_ping_and_window_update_between_data(servers):
    msg = blob(50_000, seed=8)

    def script(c):
        out = bytearray(c.headers(1, DIGEST))
        for i, f in enumerate(c.data_frames(1, msg, 4096)):
            out += RawH2.frame(core.PING, 0, 0, struct.pack(">Q", i))
            out += core.window_update(0, 1000) + core.window_update(1, 1000)
            out += f
        c.send(bytes(out))
        res = _strip_frame_counts(c.read_responses([1]))
        # every PING before the response was acknowledged, in order
        n = len(c.data_frames(1, msg, 4096))
        assert c.ping_acks == [struct.pack(">Q", i) for i in range(n)]
        return res

    assert both(servers, script) == {1: (0, digest_of(msg))}


def test_raw_headers_plus_continuation(servers):
    msg = blob(20_000, seed=10)
    block = _headers_block(DIGEST)

    def script(c):
        a, b_, c_ = block[:5], block[5:6], block[6:]
        c.send(RawH2.frame(core.HEADERS, 0, 1, a),
               RawH2.frame(core.CONTINUATION, 0, 1, b_),
               RawH2.frame(core.CONTINUATION, core.FLAG_END_HEADERS, 1, c_),
               b"".join(c.data_frames(1, msg, 16384)))
        return _strip_frame_counts(c.read_responses([1]))

    assert both(servers, script) == {1: (0, digest_of(msg))}


def test_raw_two_streams_interleaved(servers):
    m1, m3 = blob(40_000, seed=11), blob(33_333, seed=12)

    def script(c):
        f1 = c.data_frames(1, m1, 3000)
        f3 = c.data_frames(3, m3, 3000)
        out = bytearray(c.headers(1, DIGEST) + c.headers(3, DIGEST))
        for i in range(max(len(f1), len(f3))):
            if i < len(f1):
                out += f1[i]
            if i < len(f3):
                out += f3[i]
        c.send(bytes(out))
        return _strip_frame_counts(c.read_responses([1, 3]))

    assert both(servers, script) == {1: (0, digest_of(m1)), 3: (0, digest_of(m3))}


def test_raw_large_response_default_window(servers):
    """3 MiB to a client that only ever grants the default 65,535 window: the
    server has to read this client's WINDOW_UPDATEs from inside the dispatch
    of stream 1. Stream 3's whole request is already in the server's receive
    buffer by then, so it is parsed during that pump and dispatched after."""
    r1, m3 = blob(777, seed=13), blob(60_000, seed=14)

    def script(c):
        c.send(c.headers(1, BIGPATH) + b"".join(c.data_frames(1, r1, 16384))
               + c.headers(3, DIGEST) + b"".join(c.data_frames(3, m3, 16384)))
        res = c.read_responses([1, 3])
        # flow control held: no DATA frame above the 16,384 default
        assert res[1][2] >= (BIG + 5) // 16384
        return _strip_frame_counts(res)

    assert both(servers, script) == {1: (0, big_handler(r1, None)),
                                     3: (0, digest_of(m3))}
