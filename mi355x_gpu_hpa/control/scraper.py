"""scraper.py — Prometheus text-format scrape client + parser.

The harness's stand-in for Prometheus's scrape loop (reference scrape
config: kube-prometheus-stack-values.yaml:3-16, 1 s interval with the
``node`` relabel). Scrapes exporter /metrics endpoints over HTTP, parses the
text exposition format into Samples, and applies the node relabel the
reference does in Prometheus config (``__meta_kubernetes_pod_node_name`` ->
``node``; here: a static node label per target, same effect).

Like a real Prometheus, the scraper keeps one HTTP/1.1 connection per target
open between scrapes. Fetch and parse run in native code
(native/control/scrape_client.cpp, libmi355x_scrape.so) whenever the library
is built and the target is a plain ``http://host:port/path`` URL; otherwise,
or with ``native=False`` / ``MI355X_SCRAPE_NATIVE=0``, each scrape goes
through ``urllib`` and ``parse_prometheus_text``, which is also the
specification of the native parser.
"""

from __future__ import annotations

import ctypes
import os
import re
import time
import urllib.parse
import urllib.request
from array import array
from dataclasses import dataclass
from typing import Dict, List, Optional

from .. import NATIVE_BUILD
from .promql import Sample

SCRAPE_LIB = NATIVE_BUILD / "libmi355x_scrape.so"
# Set to 0/false/off/no to keep every Scraper on the urllib path (A/B runs).
NATIVE_ENV = "MI355X_SCRAPE_NATIVE"

_LINE_RE = re.compile(
    r"^(?P<name>[a-zA-Z_:][a-zA-Z0-9_:]*)"
    r"(?:\{(?P<labels>[^}]*)\})?\s+"
    r"(?P<value>[+-]?(?:\d+\.?\d*(?:[eE][+-]?\d+)?|Inf|NaN))"
    r"(?:\s+(?P<ts>-?\d+))?$"
)
_LABEL_RE = re.compile(r'([a-zA-Z_][a-zA-Z0-9_]*)="((?:[^"\\]|\\.)*)"')


def parse_prometheus_text(text: str) -> List[Sample]:
    out: List[Sample] = []
    for line in text.splitlines():
        line = line.strip()
        if not line or line.startswith("#"):
            continue
        m = _LINE_RE.match(line)
        if not m:
            continue
        labels = {}
        if m.group("labels"):
            for lm in _LABEL_RE.finditer(m.group("labels")):
                labels[lm.group(1)] = lm.group(2).replace('\\"', '"').replace(
                    "\\\\", "\\"
                )
        v = m.group("value")
        value = float("inf") if v == "Inf" else float("nan") if v == "NaN" else float(v)
        out.append(Sample(m.group("name"), labels, value))
    return out


# --- native client (scrape_client.h) ---------------------------------------

_OK, _DEFER, _ERR_UNSUPPORTED = 0, 1, -5


class _Result(ctypes.Structure):
    _fields_ = [
        ("n_samples", ctypes.c_int32),
        ("n_strings", ctypes.c_int32),
        ("arena_len", ctypes.c_int32),
        ("body_len", ctypes.c_int32),
        ("http_status", ctypes.c_int32),
        ("connects", ctypes.c_int32),
        ("values", ctypes.c_void_p),
        ("label_counts", ctypes.c_void_p),
        ("arena", ctypes.c_void_p),
        ("body", ctypes.c_void_p),
    ]


_lib = None
_lib_tried = False


def _load_native():
    """The scrape library, or None when it is not built."""
    global _lib, _lib_tried
    if not _lib_tried:
        _lib_tried = True
        try:
            lib = ctypes.CDLL(str(SCRAPE_LIB))
        except OSError:
            return None
        lib.mi355x_scrape_open.restype = ctypes.c_void_p
        lib.mi355x_scrape_open.argtypes = [
            ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p,
            ctypes.c_double]
        lib.mi355x_scrape_close.restype = None
        lib.mi355x_scrape_close.argtypes = [ctypes.c_void_p]
        lib.mi355x_scrape_fetch.argtypes = [
            ctypes.c_void_p, ctypes.POINTER(_Result)]
        lib.mi355x_scrape_parse.argtypes = [
            ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int,
            ctypes.POINTER(_Result)]
        _lib = lib
    return _lib


def native_available() -> bool:
    return _load_native() is not None


def _native_enabled_by_env() -> bool:
    return os.environ.get(NATIVE_ENV, "1").strip().lower() not in (
        "0", "false", "off", "no")


def _samples_from_result(res: _Result) -> List[Sample]:
    """Build Samples from the flat result: one split of the string arena,
    no text is scanned again."""
    n = res.n_samples
    if n == 0:
        return []
    strs = ctypes.string_at(res.arena, res.arena_len).decode().split("\n")
    if len(strs) != res.n_strings + 1:
        raise ValueError("scrape library returned an inconsistent arena")
    counts = array("i")
    counts.frombytes(ctypes.string_at(res.label_counts, 4 * n))
    values = array("d")
    values.frombytes(ctypes.string_at(res.values, 8 * n))
    out: List[Sample] = []
    i = 0
    for k, v in zip(counts, values):
        j = i + 1 + 2 * k
        out.append(Sample(strs[i],
                          dict(zip(strs[i + 1:j:2], strs[i + 2:j:2])), v))
        i = j
    return out


class NativeScrapeError(OSError):
    """A native fetch failed; ``code`` is the library's error code."""

    def __init__(self, code: int, http_status: int = 0):
        super().__init__(f"native scrape failed: code {code}"
                         + (f", HTTP {http_status}" if http_status else ""))
        self.code = code
        self.http_status = http_status


class NativeClient:
    """One target's persistent connection plus the native parser."""

    def __init__(self, host: str, port: int, path: str = "/metrics",
                 host_header: str = "", timeout_s: float = 2.0):
        lib = _load_native()
        if lib is None:
            raise OSError(f"{SCRAPE_LIB} missing; run `make -C native exporter`")
        self._lib = lib
        self._res = _Result()
        self._h = lib.mi355x_scrape_open(
            host.encode(), port, path.encode(), host_header.encode(),
            float(timeout_s))
        if not self._h:
            raise ValueError(f"bad scrape target {host!r}:{port}")

    @property
    def connects(self) -> int:
        """Connections opened so far (as of the last fetch)."""
        return self._res.connects

    def _finish(self, rc: int) -> List[Sample]:
        res = self._res
        if rc == _OK:
            return _samples_from_result(res)
        if rc == _DEFER:
            return parse_prometheus_text(
                ctypes.string_at(res.body, res.body_len).decode())
        raise NativeScrapeError(rc, res.http_status)

    def fetch(self) -> List[Sample]:
        return self._finish(
            self._lib.mi355x_scrape_fetch(self._h, ctypes.byref(self._res)))

    def parse(self, data: bytes) -> List[Sample]:
        return self._finish(self._lib.mi355x_scrape_parse(
            self._h, data, len(data), ctypes.byref(self._res)))

    def close(self) -> None:
        if self._h:
            self._lib.mi355x_scrape_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 — interpreter shutdown
            pass


_parse_client: Optional[NativeClient] = None


def native_parse_prometheus_text(text: str) -> List[Sample]:
    """parse_prometheus_text through the native parser (tests, tools)."""
    global _parse_client
    if _parse_client is None:
        _parse_client = NativeClient("127.0.0.1", 1)
    return _parse_client.parse(text.encode())


def _native_target(url: str):
    """(host, port, path, host_header) for a plain http://host:port/path
    URL, else None."""
    try:
        u = urllib.parse.urlsplit(url)
        port = u.port
    except ValueError:
        return None
    if u.scheme != "http" or not u.hostname or u.username or u.password \
            or u.fragment:
        return None
    path = (u.path or "/") + ("?" + u.query if u.query else "")
    if any(c <= " " or c > "~" for c in path + u.netloc):
        return None
    return u.hostname, port or 80, path, u.netloc


@dataclass
class ScrapeTarget:
    url: str                      # http://host:port/metrics
    node: str = "node0"           # the relabel's node label
    extra_labels: Optional[Dict[str, str]] = None


class Scraper:
    """Scrapes a set of targets; keeps the latest sample set per target."""

    def __init__(self, targets: List[ScrapeTarget], timeout_s: float = 2.0,
                 native: Optional[bool] = None):
        """``native=None`` uses the native client where it can, unless the
        MI355X_SCRAPE_NATIVE environment variable turns it off; ``False``
        keeps this scraper on urllib + parse_prometheus_text."""
        self.targets = targets
        self.timeout_s = timeout_s
        self.last: Dict[str, List[Sample]] = {}
        self.last_scrape_duration_s: float = 0.0
        if native is None:
            native = _native_enabled_by_env()
        self.native = bool(native) and native_available()
        # url -> (timeout the client was opened with, client); None marks a
        # target the native client cannot serve
        self._clients: Dict[str, Optional[tuple]] = {}

    def _client(self, url: str) -> Optional[NativeClient]:
        entry = self._clients.get(url, False)
        if entry and entry[0] != self.timeout_s:
            entry[1].close()
            entry = False
        if entry is False:
            spec = _native_target(url)
            entry = None
            if spec is not None:
                host, port, path, host_header = spec
                entry = (self.timeout_s, NativeClient(
                    host, port, path, host_header, self.timeout_s))
            self._clients[url] = entry
        return entry[1] if entry else None

    def _fetch_python(self, url: str) -> List[Sample]:
        with urllib.request.urlopen(url, timeout=self.timeout_s) as r:
            text = r.read().decode()
        return parse_prometheus_text(text)

    def _fetch(self, url: str) -> List[Sample]:
        client = self._client(url) if self.native else None
        if client is None:
            return self._fetch_python(url)
        try:
            return client.fetch()
        except NativeScrapeError as e:
            if e.code != _ERR_UNSUPPORTED:
                raise
            # a response framing the native client does not speak
            # (chunked): this target stays on urllib from here on
            client.close()
            self._clients[url] = None
            return self._fetch_python(url)

    def close(self) -> None:
        """Drop the kept connections (they reopen on the next scrape)."""
        for entry in self._clients.values():
            if entry:
                entry[1].close()
        self._clients.clear()

    def scrape_once(self) -> List[Sample]:
        t0 = time.monotonic()
        merged: List[Sample] = []
        for t in self.targets:
            try:
                samples = self._fetch(t.url)
            except Exception:
                # target down: keep serving its last samples (staleness is
                # handled upstream; Prometheus marks them stale after 5 min)
                merged.extend(self.last.get(t.url, []))
                continue
            for s in samples:
                s.labels.setdefault("node", t.node)
                if t.extra_labels:
                    for k, v in t.extra_labels.items():
                        s.labels.setdefault(k, v)
            self.last[t.url] = samples
            merged.extend(samples)
        self.last_scrape_duration_s = time.monotonic() - t0
        return merged
