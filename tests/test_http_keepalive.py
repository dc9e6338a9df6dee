"""The exporter's HTTP server (native/exporter/http_server.cpp) keeps
connections alive and serves them from one poll() loop: persistence,
pipelining, isolation from silent and slow clients, the connection cap and
shutdown, against the real binary with the mock backend."""

import os
import socket
import subprocess
import time

import pytest

from mi355x_gpu_hpa.exporter import EXPORTER_BIN, ExporterProcess

# HttpServer::kMaxConnections
MAX_CONNECTIONS = 64


@pytest.fixture(scope="module")
def exporter():
    if not os.path.exists(EXPORTER_BIN):
        pytest.skip("exporter not built")
    with ExporterProcess(mock_devices=8, interval_ms=100) as exp:
        yield exp


def connect(exp, rcvbuf=None):
    s = socket.socket()
    if rcvbuf:
        s.setsockopt(socket.SOL_SOCKET, socket.SO_RCVBUF, rcvbuf)
    s.settimeout(3)
    s.connect(("127.0.0.1", exp.port))
    return s


def request(path, version="1.1", extra=""):
    return f"GET {path} HTTP/{version}\r\nHost: x\r\n{extra}\r\n".encode()


def read_response(s, buf=b""):
    """One response by Content-Length: (head, body, bytes read past it)."""
    while b"\r\n\r\n" not in buf:
        data = s.recv(65536)
        assert data, f"connection closed inside the headers: {buf!r}"
        buf += data
    head, rest = buf.split(b"\r\n\r\n", 1)
    length = None
    for line in head.split(b"\r\n")[1:]:
        k, v = line.split(b":", 1)
        if k.strip().lower() == b"content-length":
            length = int(v)
    assert length is not None
    while len(rest) < length:
        data = s.recv(65536)
        assert data, "connection closed inside the body"
        rest += data
    return head, rest[:length], rest[length:]


def is_closed(s):
    """True when the server has closed: the next read sees EOF."""
    s.settimeout(2)
    try:
        return s.recv(1) == b""
    except ConnectionResetError:
        return True


def test_two_requests_on_one_socket(exporter):
    s = connect(exporter)
    for _ in range(2):
        s.sendall(request("/metrics"))
        head, body, extra = read_response(s)
        assert head.startswith(b"HTTP/1.1 200 OK")
        assert b"connection: keep-alive" in head.lower()
        assert b"text/plain; version=0.0.4" in head
        assert body.count(b"\ndcgm_gpu_utilization{") == 8 and extra == b""
    s.sendall(request("/healthz"))
    head, body, _ = read_response(s)
    assert body == b"ok\n" and b"text/plain; charset=utf-8" in head
    s.close()


@pytest.mark.parametrize("version,extra", [
    ("1.1", "Connection: close\r\n"),
    ("1.1", "connection: Keep-Alive, CLOSE\r\n"),
    ("1.0", ""),
])
def test_close_and_http10_requests_get_closed(exporter, version, extra):
    s = connect(exporter)
    s.sendall(request("/healthz", version, extra))
    head, body, _ = read_response(s)
    assert head.startswith(b"HTTP/1.1 200 OK") and body == b"ok\n"
    assert b"connection: close" in head.lower()
    assert is_closed(s)
    s.close()


def test_status_codes_unchanged(exporter):
    s = connect(exporter)
    for path, status, body in [("/readyz", b"200 OK", b"ready\n"),
                               ("/nope", b"404 Not Found", b"see /metrics\n")]:
        s.sendall(request(path))
        head, got, _ = read_response(s)
        assert head.startswith(b"HTTP/1.1 " + status) and got == body
    s.sendall(b"POST /metrics HTTP/1.1\r\nHost: x\r\n\r\n")
    head, got, _ = read_response(s)
    assert head.startswith(b"HTTP/1.1 405 ") and got == b"GET only\n"
    s.close()


def test_unterminated_requests_are_answered_and_closed(exporter):
    # oversize: answered from its first line once the buffer limit is hit
    s = connect(exporter)
    s.sendall(b"GET /healthz" + b"a" * 8000)
    head, body, _ = read_response(s)
    assert head.startswith(b"HTTP/1.1 200 OK") and body == b"ok\n"
    assert b"connection: close" in head.lower()
    assert is_closed(s)
    s.close()
    # a client that stops sending before the blank line
    s = connect(exporter)
    s.sendall(b"GET /healthz HTTP/1.1\r\n")
    s.shutdown(socket.SHUT_WR)
    head, body, _ = read_response(s)
    assert body == b"ok\n" and b"connection: close" in head.lower()
    assert is_closed(s)
    s.close()


def test_idle_and_silent_connections_do_not_delay_others(exporter):
    idle = connect(exporter)
    idle.sendall(request("/healthz"))
    read_response(idle)                 # now an idle kept-alive connection
    silent = connect(exporter)          # connected, never sends
    half = connect(exporter)
    half.sendall(b"GET /metrics HTTP/1.1\r\nHost:")   # stuck mid-request
    for path, marker in [("/metrics", b"dcgm_gpu_utilization{"),
                         ("/healthz", b"ok\n")]:
        t0 = time.monotonic()
        s = connect(exporter)
        s.sendall(request(path, extra="Connection: close\r\n"))
        _, body, _ = read_response(s)
        dt = time.monotonic() - t0
        s.close()
        assert marker in body
        assert dt < 0.5, f"{path} took {dt:.3f}s behind a silent client"
    # the idle connection is still good
    idle.sendall(request("/healthz"))
    assert read_response(idle)[1] == b"ok\n"
    for s in (idle, silent, half):
        s.close()


def test_pipelined_requests_answered_in_order(exporter):
    s = connect(exporter)
    s.sendall(request("/healthz") + request("/metrics") + request("/nope"))
    head1, body1, rest = read_response(s)
    head2, body2, rest = read_response(s, rest)
    head3, body3, rest = read_response(s, rest)
    assert body1 == b"ok\n"
    assert head2.startswith(b"HTTP/1.1 200") and b"dcgm_gpu_temp{" in body2
    assert head3.startswith(b"HTTP/1.1 404") and rest == b""
    s.close()


def test_pipelined_flood_is_answered_completely(exporter):
    """Far more pipelined output than the socket buffers hold: the server
    keeps it as pending output and every response arrives whole."""
    n = 24
    s = connect(exporter, rcvbuf=2048)
    s.sendall(request("/metrics") * n)
    time.sleep(0.05)            # let the server run into the full socket
    rest = b""
    for _ in range(n):
        head, body, rest = read_response(s, rest)
        assert head.startswith(b"HTTP/1.1 200 OK") and len(body) > 40000
        assert body.count(b"\ndcgm_gpu_utilization{") == 8
    assert rest == b""
    s.close()


def test_slow_reader_gets_the_whole_body_while_others_are_served(exporter):
    slow = connect(exporter, rcvbuf=2048)
    slow.sendall(request("/metrics"))
    # headers first, then the body in small sips
    buf = b""
    while b"\r\n\r\n" not in buf:
        buf += slow.recv(512)
    head, got = buf.split(b"\r\n\r\n", 1)
    length = int([l.split(b":")[1] for l in head.split(b"\r\n")
                  if l.lower().startswith(b"content-length")][0])
    assert length > 40000
    served_meanwhile = 0
    while len(got) < length:
        data = slow.recv(4096)
        assert data, "server dropped the slow reader"
        got += data
        if served_meanwhile < 3 and len(got) < length // 2:
            t0 = time.monotonic()
            other = connect(exporter)
            other.sendall(request("/healthz"))
            assert read_response(other)[1] == b"ok\n"
            assert time.monotonic() - t0 < 0.5
            other.close()
            served_meanwhile += 1
            time.sleep(0.01)
    assert served_meanwhile == 3
    assert len(got) == length and got.endswith(b"\n")
    assert got.count(b"\ndcgm_gpu_utilization{") == 8
    # and the connection is still usable
    slow.sendall(request("/healthz"))
    assert read_response(slow)[1] == b"ok\n"
    slow.close()


def test_more_connections_than_the_cap(exporter):
    socks = [connect(exporter) for _ in range(MAX_CONNECTIONS + 16)]
    try:
        # the newest connection is served; so is a fresh one
        socks[-1].sendall(request("/healthz"))
        assert read_response(socks[-1])[1] == b"ok\n"
        assert "dcgm_gpu_utilization" in exporter.scrape()
        # the longest-idle ones made room
        assert is_closed(socks[0])
    finally:
        for s in socks:
            s.close()
    assert "dcgm_gpu_utilization" in exporter.scrape()


def test_sigterm_with_open_connections_exits_promptly():
    if not os.path.exists(EXPORTER_BIN):
        pytest.skip("exporter not built")
    with ExporterProcess(mock_devices=1, interval_ms=100) as exp:
        kept = connect(exp)
        kept.sendall(request("/healthz"))
        read_response(kept)
        silent = connect(exp)
        t0 = time.monotonic()
        exp.proc.terminate()
        try:
            rc = exp.proc.wait(timeout=2)
        except subprocess.TimeoutExpired:
            pytest.fail("exporter still running 2 s after SIGTERM")
        assert rc == 0 and time.monotonic() - t0 < 2
        assert is_closed(kept)
        kept.close()
        silent.close()
