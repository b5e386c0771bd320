"""egrpc transport tests: self-talk, wire interop with grpcio (both
directions), streaming, large messages (flow control), errors, latency."""
import os
import threading
import time
from concurrent import futures

import grpc
import pytest

from elastic_gpu_agent_amd import egrpc
from elastic_gpu_agent_amd.egrpc import core as ecore


def echo_handler(request: bytes, context) -> bytes:
    return request


def fail_handler(request: bytes, context):
    context.abort(grpc.StatusCode.INVALID_ARGUMENT, "nope µ")  # non-ascii msg


def stream_handler(request: bytes, context):
    for i in range(5):
        yield f"chunk-{i}".encode() + request


def stream_fail_handler(request, context):
    yield b"first"
    raise RuntimeError("boom mid-stream")


@pytest.fixture(params=["native", "python"])
def eserver(request, tmp_path, monkeypatch):
    """Differential fixture: every test in this file runs against BOTH the
    C++ data plane (default) and the pure-Python reference implementation."""
    if request.param == "python":
        monkeypatch.setenv("EGPU_PY_TRANSPORT", "1")
    sock = str(tmp_path / "egrpc.sock")
    s = egrpc.Server()
    s.add_service("t.Test", {
        "Echo": egrpc.unary_unary(echo_handler),
        "Fail": egrpc.unary_unary(fail_handler),
        "Stream": egrpc.unary_stream(stream_handler),
        "StreamFail": egrpc.unary_stream(stream_fail_handler),
    })
    s.bind_unix(sock)
    s.start()
    yield sock, s
    s.stop()


# ---- egrpc client ↔ egrpc server -------------------------------------------

def test_self_unary(eserver):
    sock, _ = eserver
    ch = egrpc.Channel(sock)
    echo = ch.unary_unary("/t.Test/Echo")
    assert echo(b"hello") == b"hello"
    assert echo(b"") == b""
    for size in (1, 100, 65535, 65536, 1 << 20, 5 << 20):
        blob = bytes(i & 0xFF for i in range(size))
        assert echo(blob) == blob
    ch.close()


def test_large_request_as_first_call(eserver):
    """Regression: a >64 KiB request as the FIRST RPC on a fresh channel —
    the server's SETTINGS INITIAL_WINDOW_SIZE delta must apply to the stream
    already mid-send (RFC 7540 §6.9.2); this used to deadlock."""
    sock, _ = eserver
    ch = egrpc.Channel(sock)
    blob = os.urandom(800_000)
    assert ch.unary_unary("/t.Test/Echo")(blob, timeout=10.0) == blob
    ch.close()


def test_self_error(eserver):
    sock, _ = eserver
    ch = egrpc.Channel(sock)
    fail = ch.unary_unary("/t.Test/Fail")
    with pytest.raises(egrpc.EgrpcError) as ei:
        fail(b"x")
    assert ei.value.code() == egrpc.INVALID_ARGUMENT
    assert "nope" in ei.value.details()
    # channel still usable after an error
    assert ch.unary_unary("/t.Test/Echo")(b"ok") == b"ok"
    ch.close()


def test_self_stream(eserver):
    sock, _ = eserver
    ch = egrpc.Channel(sock)
    stream = ch.unary_stream("/t.Test/Stream")
    items = list(stream(b"!"))
    assert items == [f"chunk-{i}".encode() + b"!" for i in range(5)]
    ch.close()


def test_unknown_method(eserver):
    sock, _ = eserver
    ch = egrpc.Channel(sock)
    with pytest.raises(egrpc.EgrpcError) as ei:
        ch.unary_unary("/t.Test/Nope")(b"")
    assert ei.value.code() == egrpc.UNKNOWN
    ch.close()


# ---- grpcio client ↔ egrpc server (the kubelet direction) ------------------

def test_grpcio_client_against_egrpc_server(eserver):
    sock, _ = eserver
    ch = grpc.insecure_channel(f"unix://{sock}")
    echo = ch.unary_unary("/t.Test/Echo")
    assert echo(b"from-grpcio") == b"from-grpcio"
    # large payload exercises WINDOW_UPDATE handling against a real stack
    blob = os.urandom(3 << 20)
    assert echo(blob) == blob
    # repeated calls on one connection (dynamic HPACK state on their side)
    for i in range(50):
        assert echo(f"msg-{i}".encode()) == f"msg-{i}".encode()
    # error mapping
    with pytest.raises(grpc.RpcError) as ei:
        ch.unary_unary("/t.Test/Fail")(b"x")
    assert ei.value.code() == grpc.StatusCode.INVALID_ARGUMENT
    assert "nope" in ei.value.details()
    # streaming
    items = list(ch.unary_stream("/t.Test/Stream")(b"?"))
    assert len(items) == 5 and items[0] == b"chunk-0?"
    # custom metadata (their encoder may huffman + dynamic-index these)
    meta = [("x-custom-header", "Some Value With Spaces!"), ("x-n", "42")]
    for _ in range(3):
        assert echo(b"meta", metadata=meta) == b"meta"
    ch.close()


def test_grpcio_concurrent_streams(eserver):
    """A live ListAndWatch stream must not block unary calls on the SAME
    grpc connection (kubelet multiplexes)."""
    sock, _ = eserver
    ch = grpc.insecure_channel(f"unix://{sock}")

    slow_items = []
    done = threading.Event()

    def consume():
        for it in ch.unary_stream("/t.Test/Stream")(b"s"):
            slow_items.append(it)
            time.sleep(0.05)
        done.set()

    t = threading.Thread(target=consume, daemon=True)
    t.start()
    time.sleep(0.02)
    # unary calls interleaved with the active stream
    echo = ch.unary_unary("/t.Test/Echo")
    for i in range(5):
        assert echo(b"inter") == b"inter"
    assert done.wait(5)
    assert len(slow_items) == 5
    ch.close()


# ---- egrpc client ↔ grpcio server ------------------------------------------

@pytest.fixture
def gserver(tmp_path):
    sock = str(tmp_path / "grpcio.sock")

    def echo(req, ctx):
        return req

    def fail(req, ctx):
        ctx.abort(grpc.StatusCode.FAILED_PRECONDITION, "denied ü")

    def stream(req, ctx):
        for i in range(4):
            yield f"s{i}".encode() + req

    handler = grpc.method_handlers_generic_handler("t.Test", {
        "Echo": grpc.unary_unary_rpc_method_handler(echo),
        "Fail": grpc.unary_unary_rpc_method_handler(fail),
        "Stream": grpc.unary_stream_rpc_method_handler(stream),
    })
    s = grpc.server(futures.ThreadPoolExecutor(max_workers=4),
                    options=[("grpc.max_receive_message_length", 32 << 20)])
    s.add_generic_rpc_handlers((handler,))
    s.add_insecure_port(f"unix://{sock}")
    s.start()
    yield sock
    s.stop(grace=0.2)


def test_egrpc_client_against_grpcio_server(gserver):
    ch = egrpc.Channel(gserver)
    echo = ch.unary_unary("/t.Test/Echo")
    assert echo(b"hi") == b"hi"
    blob = os.urandom(2 << 20)  # > default 64KB windows: we must honor
    assert echo(blob) == blob   # grpcio's WINDOW_UPDATE pacing
    with pytest.raises(egrpc.EgrpcError) as ei:
        ch.unary_unary("/t.Test/Fail")(b"")
    assert ei.value.code() == egrpc.FAILED_PRECONDITION
    assert "denied" in ei.value.details()
    items = list(ch.unary_stream("/t.Test/Stream")(b"z"))
    assert items == [b"s0z", b"s1z", b"s2z", b"s3z"]
    # connection reuse across many calls (grpcio server hpack state)
    for i in range(50):
        assert echo(str(i).encode()) == str(i).encode()
    ch.close()


def test_timeout_against_grpcio_server(tmp_path):
    def sleepy(req, ctx):
        time.sleep(2.0)
        return req

    sock = str(tmp_path / "sleepy.sock")
    handler = grpc.method_handlers_generic_handler(
        "t.Test", {"Sleepy": grpc.unary_unary_rpc_method_handler(sleepy)})
    s = grpc.server(futures.ThreadPoolExecutor(max_workers=2))
    s.add_generic_rpc_handlers((handler,))
    s.add_insecure_port(f"unix://{sock}")
    s.start()
    try:
        ch = egrpc.Channel(sock)
        with pytest.raises(egrpc.EgrpcError) as ei:
            ch.unary_unary("/t.Test/Sleepy")(b"", timeout=0.3)
        assert ei.value.code() == egrpc.DEADLINE_EXCEEDED
        ch.close()
    finally:
        s.stop(grace=0)


# ---- reconnect & latency ----------------------------------------------------

def test_client_reconnects_after_server_restart(tmp_path):
    sock = str(tmp_path / "r.sock")
    s1 = egrpc.Server()
    s1.add_service("t.Test", {"Echo": egrpc.unary_unary(echo_handler)})
    s1.bind_unix(sock)
    s1.start()
    ch = egrpc.Channel(sock)
    echo = ch.unary_unary("/t.Test/Echo")
    assert echo(b"1") == b"1"
    s1.stop()
    with pytest.raises(egrpc.EgrpcError):
        echo(b"2")
    s2 = egrpc.Server()
    s2.add_service("t.Test", {"Echo": egrpc.unary_unary(echo_handler)})
    s2.bind_unix(sock)
    s2.start()
    assert echo(b"3") == b"3"  # lazy reconnect
    s2.stop()
    ch.close()


def test_latency_beats_grpcio_floor(eserver, tmp_path):
    """The entire point: ~100-300µs p50 round trips where grpcio costs ~1ms+.

    The bound targets the native data plane; the pure-Python reference
    transport is held to the same one (it used to skip itself here).

    CI containers are noisy, so the bound is relative: a raw unix-socket
    echo server measured in the same process/load window sets the floor, and
    egrpc must stay within a small multiple of it (grpcio is ~30× the raw
    floor on this host class)."""
    import socket as socketlib

    # raw-socket echo baseline under current load
    raw_path = str(tmp_path / "raw.sock")
    srv = socketlib.socket(socketlib.AF_UNIX, socketlib.SOCK_STREAM)
    srv.bind(raw_path)
    srv.listen(1)

    def serve_echo():
        conn, _ = srv.accept()
        while True:
            data = conn.recv(4096)
            if not data:
                return
            conn.sendall(data)

    t = threading.Thread(target=serve_echo, daemon=True)
    t.start()
    cl = socketlib.socket(socketlib.AF_UNIX, socketlib.SOCK_STREAM)
    cl.connect(raw_path)
    raw = []
    for _ in range(1500):
        t0 = time.perf_counter()
        cl.sendall(b"x" * 64)
        cl.recv(4096)
        raw.append(time.perf_counter() - t0)
    raw.sort()
    raw_p50 = raw[len(raw) // 2] * 1e6
    cl.close()
    srv.close()

    sock, _ = eserver
    ch = egrpc.Channel(sock)
    echo = ch.unary_unary("/t.Test/Echo")
    for _ in range(300):
        echo(b"warm")
    lat = []
    for _ in range(2000):
        t0 = time.perf_counter()
        echo(b"ping")
        lat.append(time.perf_counter() - t0)
    lat.sort()
    p50 = lat[len(lat) // 2] * 1e6
    bound = max(900.0, raw_p50 * 12)
    assert p50 < bound, (
        f"egrpc p50 {p50:.0f}µs vs raw-socket p50 {raw_p50:.0f}µs "
        f"(bound {bound:.0f}µs) — transport regression"
    )
    ch.close()


def test_grpcio_midstream_error_is_trailers_only(eserver):
    """A handler raising AFTER items were yielded (response HEADERS already
    sent) must surface as a per-RPC error with proper TRAILERS — no second
    :status pseudo-header (grpc-go/grpcio treat that as a protocol error
    and tear the whole connection down; advisor finding, round 1, fixed in
    both the Python and native servers)."""
    sock, _ = eserver
    ch = grpc.insecure_channel(f"unix://{sock}")
    it = ch.unary_stream("/t.Test/StreamFail")(b"x")
    got = []
    with pytest.raises(grpc.RpcError) as ei:
        for item in it:
            got.append(item)
    assert got == [b"first"]
    assert ei.value.code() == grpc.StatusCode.UNKNOWN
    assert "boom mid-stream" in (ei.value.details() or "")
    # the CONNECTION must survive the per-stream error
    assert ch.unary_unary("/t.Test/Echo")(b"still-alive") == b"still-alive"
    ch.close()
