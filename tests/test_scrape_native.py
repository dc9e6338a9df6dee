"""The native scrape client and parser (native/control/scrape_client.cpp)
against their specification: parse_prometheus_text() for the parser, and
small in-test socket servers for the client's connection handling."""

import math
import shutil
import socket
import subprocess
import tempfile
import threading
import time
from pathlib import Path

import pytest

from mi355x_gpu_hpa.control import scraper as sc
from mi355x_gpu_hpa.control.scraper import (
    NativeClient,
    NativeScrapeError,
    Scraper,
    ScrapeTarget,
    native_parse_prometheus_text,
    parse_prometheus_text,
)
from mi355x_gpu_hpa.exporter import ExporterProcess

REPO = Path(__file__).resolve().parent.parent
NATIVE = REPO / "native"
FIXTURES = sorted((REPO / "tests" / "fixtures").glob("*.prom"))
BENCH_FAMILIES = ("dcgm_gpu_utilization\ndcgm_gpu_temp\n"
                  "amd_xgmi_total_bytes_per_second\n"
                  "amd_exporter_samples_total\n")


@pytest.fixture(scope="module", autouse=True)
def built():
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    subprocess.run(["make", "-C", str(NATIVE), "exporter"],
                   check=True, capture_output=True)
    assert sc.native_available()


def key(samples):
    """Samples as comparable tuples; NaN compares equal to NaN."""
    return [(s.name, s.labels, "NaN" if math.isnan(s.value) else s.value)
            for s in samples]


def assert_same_parse(text):
    want = parse_prometheus_text(text)
    got = native_parse_prometheus_text(text)
    assert key(got) == key(want)
    return want


# --- parser: differential against the Python function ----------------------

@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: p.name)
def test_fixture_files(path):
    assert len(assert_same_parse(path.read_text())) > 10


@pytest.fixture(scope="module")
def live_bodies():
    """/metrics of --mock 1 and --mock 8, full and narrowed to the bench's
    four families."""
    bodies = {}
    with tempfile.NamedTemporaryFile("w", suffix=".csv") as mf:
        mf.write(BENCH_FAMILIES)
        mf.flush()
        for n in (1, 8):
            with ExporterProcess(mock_devices=n, interval_ms=100) as exp:
                bodies[f"mock{n}-full"] = exp.scrape()
            with ExporterProcess(mock_devices=n, interval_ms=100,
                                 metric_file=mf.name) as exp:
                bodies[f"mock{n}-narrow"] = exp.scrape()
    return bodies


@pytest.mark.parametrize(
    "which", ["mock1-full", "mock1-narrow", "mock8-full", "mock8-narrow"])
def test_live_mock_output(live_bodies, which):
    want = assert_same_parse(live_bodies[which])
    n = 8 if "mock8" in which else 1
    assert sum(s.name == "dcgm_gpu_utilization" for s in want) == n


EDGE_CASES = {
    "escaped_quote_backslash": 'm{a="x\\"y",b="c\\\\d",c="e\\nf"} 1\n',
    "replace_passes_in_sequence": 'm{a="\\\\\\""} 1\n',
    "escaped_quote_keeps_value_open": 'm{a="x\\",b="y"} 1\n',
    "empty_label_set": "m{} 2\n",
    "no_label_block": "m 2\n",
    "label_junk_between": 'm{ a="1" ,, 9b="2", c = "3", d="4"} 5\n',
    "duplicate_label": 'm{a="1",a="2",b="3"} 5\n',
    "brace_in_value": 'm{a="}"} 1\nn{a="{"} 1\n',
    "trailing_timestamp": 'm{a="b"} 2 1700000000000\nn 3 -5\n',
    "two_trailing_fields": "m 1 2 3\n",
    "inf_nan": "a +Inf\nb -Inf\nc Inf\nd NaN\ne +NaN\nf -NaN\n",
    "bad_spellings": "a inf\nb nan\nc Infinity\nd 0x10\ne .5\nf 1e\ng 1_0\n",
    "exponents": "a 1e3\nb -2.5E-2\nc +7.\nd 1.e2\ne 1e999\nf 1e-999\n"
                 "g 123456789012345678901234567890\nh 0.1\n",
    "crlf": 'a{x="1"} 1\r\nb 2\r\n',
    "other_line_ends": "a 1\rb 2\x0bc 3\x0cd 4\x1ce 5\x1df 6\x1eg 7\x1fh 8\n",
    "whitespace": "  a\t 1  \n\tb{x=\"1\"}   2\t3\t\n\x1fc 4\x1f\n",
    "no_value": 'm\nn{a="b"}\no \n',
    "no_space_before_value": 'm{a="b"}1\n',
    "truncated_last_line": 'a{x="1"} 1\nb{x="2',
    "truncated_value": "a 1\nb 2.",
    "empty": "",
    "only_comments": "# HELP m x\n# TYPE m gauge\n\n   \n#\n",
    "bad_names": "9m 1\n-m 1\n:m 1\n_m 1\nm-n 1\nm.n 1\n",
    "nul_bytes": 'm{a="x\x00y"} 1\nn\x00 2\n',
    "non_ascii_comment_and_value":
        '# HELP m caf\u00e9 \u2014 x\nm{a="\u00e9\u4e2d"} 1\n',
    # Unicode whitespace, digits and line ends: Python's rules apply
    "nbsp_separator": "m\u00a01\n",
    "nbsp_stripped": "\u00a0m 1\u00a0\n\u2003# c\n",
    "arabic_digits": "m \u0661\u0662\n",
    "unicode_line_ends": 'a{x="1\u2028b 2"} 3\nc 4\u0085d 5\u2029e 6\n',
}


@pytest.mark.parametrize("name", sorted(EDGE_CASES))
def test_edge_case(name):
    assert_same_parse(EDGE_CASES[name])


def test_edge_cases_are_not_vacuous():
    """The cases above that are meant to yield samples do."""
    n = {k: len(parse_prometheus_text(v)) for k, v in EDGE_CASES.items()}
    assert n["escaped_quote_backslash"] == 1 and n["inf_nan"] == 6
    assert n["exponents"] == 8 and n["crlf"] == 2 and n["other_line_ends"] == 6
    assert n["no_value"] == 0 and n["truncated_last_line"] == 1 and n["empty"] == 0
    assert n["nbsp_separator"] == 1 and n["arabic_digits"] == 1


def test_every_truncation_of_a_body(live_bodies):
    body = live_bodies["mock1-narrow"]
    for cut in range(len(body) + 1):
        assert_same_parse(body[:cut])


# --- client: connection handling against an in-test server ----------------

BODY = b'up{job="x"} 1\nload 0.5\n'


class MiniServer:
    """A tiny HTTP server that counts the connections it accepts."""

    def __init__(self, mode="keepalive", port=0):
        self.mode = mode
        self.accepted = 0
        self.requests = 0
        self._conns = []
        self._lsock = socket.socket()
        self._lsock.setsockopt(socket.SOL_SOCKET, socket.SO_REUSEADDR, 1)
        self._lsock.bind(("127.0.0.1", port))
        self._lsock.listen(8)
        self.port = self._lsock.getsockname()[1]
        self.url = f"http://127.0.0.1:{self.port}/metrics"
        self._thread = threading.Thread(target=self._accept, daemon=True)
        self._thread.start()

    def _accept(self):
        while True:
            try:
                conn, _ = self._lsock.accept()
            except OSError:
                return
            self.accepted += 1
            self._conns.append(conn)
            threading.Thread(target=self._serve, args=(conn,),
                             daemon=True).start()

    def _serve(self, conn):
        buf = b""
        try:
            while True:
                data = conn.recv(4096)
                if not data:
                    return
                buf += data
                while b"\r\n\r\n" in buf:
                    buf = buf.split(b"\r\n\r\n", 1)[1]
                    self.requests += 1
                    if not self._respond(conn):
                        return
        except OSError:
            pass
        finally:
            conn.close()

    def _respond(self, conn):
        head = b"HTTP/1.1 200 OK\r\nContent-Type: text/plain\r\n"
        length = b"Content-Length: %d\r\n" % len(BODY)
        if self.mode == "keepalive":
            conn.sendall(head + length + b"\r\n" + BODY)
            return True
        if self.mode == "close":
            conn.sendall(head + length + b"Connection: close\r\n\r\n" + BODY)
        elif self.mode == "eof":
            conn.sendall(b"HTTP/1.0 200 OK\r\n\r\n" + BODY)
        elif self.mode == "chunked":
            conn.sendall(head + b"Transfer-Encoding: chunked\r\n\r\n%x\r\n"
                         % len(BODY) + BODY + b"\r\n0\r\n\r\n")
        elif self.mode == "stall":
            conn.sendall(head + b"Content-Length: 1000\r\n\r\n" + BODY)
            conn.recv(1)    # until the client gives up and closes
        return False

    def stop(self):
        try:
            self._lsock.shutdown(socket.SHUT_RDWR)   # wakes accept()
        except OSError:
            pass
        self._lsock.close()
        for c in self._conns:
            try:
                c.shutdown(socket.SHUT_RDWR)
            except OSError:
                pass
            c.close()
        self._thread.join(timeout=2)


@pytest.fixture()
def server(request):
    servers = []

    def make(mode="keepalive", port=0):
        s = MiniServer(mode, port)
        servers.append(s)
        return s

    yield make
    for s in servers:
        s.stop()


WANT = parse_prometheus_text(BODY.decode())


def client_for(srv, timeout_s=2.0):
    return NativeClient("127.0.0.1", srv.port, "/metrics",
                        f"127.0.0.1:{srv.port}", timeout_s)


def test_two_scrapes_reuse_the_connection(server):
    srv = server("keepalive")
    c = client_for(srv)
    assert key(c.fetch()) == key(WANT)
    assert key(c.fetch()) == key(WANT)
    assert srv.accepted == 1 and srv.requests == 2
    assert c.connects == 1
    c.close()


@pytest.mark.parametrize("mode", ["close", "eof"])
def test_server_that_closes_after_each_response(server, mode):
    srv = server(mode)
    c = client_for(srv)
    assert key(c.fetch()) == key(WANT)
    assert key(c.fetch()) == key(WANT)
    assert srv.accepted == 2
    c.close()


def test_restarted_server_is_recovered_by_one_retry(server):
    srv = server("keepalive")
    c = client_for(srv)
    assert key(c.fetch()) == key(WANT)
    srv.stop()
    srv2 = server("keepalive", port=srv.port)
    assert key(c.fetch()) == key(WANT)
    assert srv2.accepted == 1 and c.connects == 2
    c.close()


def test_dead_port_is_an_error(server):
    srv = server("keepalive")
    c = client_for(srv, timeout_s=0.5)
    assert key(c.fetch()) == key(WANT)
    srv.stop()
    with pytest.raises(NativeScrapeError) as e:
        c.fetch()
    assert e.value.code < 0
    c.close()


def test_stall_mid_body_ends_at_the_timeout(server):
    srv = server("stall")
    c = client_for(srv, timeout_s=0.3)
    t0 = time.monotonic()
    with pytest.raises(NativeScrapeError) as e:
        c.fetch()
    dt = time.monotonic() - t0
    assert e.value.code == -3
    assert 0.25 < dt < 1.5
    c.close()


# --- Scraper on top of the client -----------------------------------------

def test_scraper_uses_native_and_serves_last_samples_when_down(server):
    srv = server("keepalive")
    s = Scraper([ScrapeTarget(srv.url, node="n7", extra_labels={"zone": "z"})],
                timeout_s=0.5)
    assert s.native
    first = s.scrape_once()
    assert [x.name for x in first] == ["up", "load"]
    assert first[0].labels == {"job": "x", "node": "n7", "zone": "z"}
    second = s.scrape_once()
    assert srv.accepted == 1
    # fresh objects every scrape: callers mutate the labels
    assert second[0] is not first[0] and second[0].labels is not first[0].labels
    assert s.last_scrape_duration_s > 0
    srv.stop()
    assert key(s.scrape_once()) == key(second)
    s.close()


def test_scraper_opt_out(server, monkeypatch):
    srv = server("keepalive")
    targets = [ScrapeTarget(srv.url)]
    off = Scraper(targets, native=False)
    assert not off.native
    a = off.scrape_once()
    b = off.scrape_once()
    assert srv.accepted == 2            # urllib: a connection per scrape
    on = Scraper(targets)
    assert key(on.scrape_once()) == key(a) == key(b)
    for v in ("0", "false", "off"):
        monkeypatch.setenv(sc.NATIVE_ENV, v)
        assert not Scraper(targets).native
    monkeypatch.setenv(sc.NATIVE_ENV, "1")
    assert Scraper(targets).native
    on.close()


def test_scraper_falls_back_for_chunked_and_odd_urls(server):
    srv = server("chunked")
    s = Scraper([ScrapeTarget(srv.url)])
    want = [(n, dict(l, node="node0"), v) for n, l, v in key(WANT)]
    assert key(s.scrape_once()) == want     # via urllib
    assert key(s.scrape_once()) == want
    assert srv.accepted == 3    # one native attempt, then urllib's two
    assert sc._native_target("https://h:1/metrics") is None
    assert sc._native_target("http://u:p@h:1/metrics") is None
    assert sc._native_target("http://h:1/m?x=1") == ("h", 1, "/m?x=1", "h:1")
    assert sc._native_target("http://h/") == ("h", 80, "/", "h")


def test_scraper_equivalence_against_mock_exporter():
    """Native path and opt-out path return equal sample lists for one tick
    (the tick is pinned by a sampling interval longer than the test)."""
    with ExporterProcess(mock_devices=8, interval_ms=600000) as exp:
        targets = [ScrapeTarget(exp.url, node="node0")]
        py = Scraper(targets, native=False)
        nat = Scraper(targets)
        assert nat.native
        a, b, c = py.scrape_once(), nat.scrape_once(), py.scrape_once()
        assert len(a) > 100
        # series that count the scrapes themselves move between requests
        moving = {(x.name, tuple(sorted(x.labels.items())))
                  for x, z in zip(a, c) if key([x]) != key([z])}
        assert len(moving) < 5

        def still(samples):
            return [k for k, s in zip(key(samples), samples)
                    if (s.name, tuple(sorted(s.labels.items()))) not in moving]

        assert [k[:2] for k in key(a)] == [k[:2] for k in key(b)]
        assert still(a) == still(b) == still(c)
        nat.close()


def test_selftest_binary(live_bodies, tmp_path):
    """The ASan+UBSan self-test program, alone and on a rendered body:
    exit 0, nothing on stderr."""
    subprocess.run(["make", "-C", str(NATIVE), "scrape-selftest"],
                   check=True, capture_output=True)
    body = tmp_path / "mock1.prom"
    body.write_text(live_bodies["mock1-full"])
    for args in ([], [str(body)]):
        p = subprocess.run([str(NATIVE / "build" / "scrape-selftest")] + args,
                           capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        assert p.stderr == ""
