// scrape_client.cpp — keep-alive HTTP/1.1 scrape client + Prometheus text
// parser behind the C ABI in scrape_client.h (libmi355x_scrape.so).
//
// The control loop scrapes one exporter per tick. Doing that with a fresh
// TCP connection and a Python HTTP stack per scrape costs several times
// what the exporter needs to render the body; a real Prometheus keeps its
// connection open, and so does this client.

#include "scrape_client.h"

#include <fcntl.h>
#include <netdb.h>
#include <netinet/in.h>
#include <netinet/tcp.h>
#include <poll.h>
#include <sys/socket.h>
#include <unistd.h>

#include <cerrno>
#include <charconv>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

namespace {

// A response larger than this is refused (the unfiltered 8-GPU body is
// about 58 KB).
constexpr size_t kMaxBodyBytes = 64u << 20;
// Response headers must fit in this much.
constexpr size_t kMaxHeaderBytes = 64u << 10;

// ---------------------------------------------------------------- parser

// Python's str.splitlines() boundaries within ASCII.
inline bool is_linesep(unsigned char c)
{
    return c == '\n' || c == '\r' || c == 0x0b || c == 0x0c ||
           (c >= 0x1c && c <= 0x1e);
}

// Python's str.isspace() / re \s within ASCII.
inline bool is_ws(unsigned char c)
{
    return c == ' ' || (c >= 0x09 && c <= 0x0d) || (c >= 0x1c && c <= 0x1f);
}

inline bool is_alpha(unsigned char c)
{
    return (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z');
}
inline bool is_digit(unsigned char c) { return c >= '0' && c <= '9'; }
inline bool name_start(unsigned char c) { return is_alpha(c) || c == '_' || c == ':'; }
inline bool name_char(unsigned char c) { return name_start(c) || is_digit(c); }
inline bool label_start(unsigned char c) { return is_alpha(c) || c == '_'; }
inline bool label_char(unsigned char c) { return label_start(c) || is_digit(c); }

struct Parsed {
    std::vector<double> values;
    std::vector<int32_t> label_counts;
    int32_t n_strings = 0;
    std::string arena;   // every string followed by '\n'
    std::string scratch;

    void clear()
    {
        values.clear();
        label_counts.clear();
        n_strings = 0;
        arena.clear();
    }
    void end_string()
    {
        arena += '\n';
        ++n_strings;
    }
    void add_string(const char* b, const char* e)
    {
        arena.append(b, e);
        end_string();
    }
    // value.replace('\\"', '"').replace('\\\\', '\\'): two passes, each
    // left to right over non-overlapping matches, as Python does them.
    void add_unescaped(const char* b, const char* e)
    {
        if (!std::memchr(b, '\\', (size_t)(e - b))) {
            add_string(b, e);
            return;
        }
        scratch.clear();
        for (const char* p = b; p < e;) {
            if (*p == '\\' && p + 1 < e && p[1] == '"') {
                scratch += '"';
                p += 2;
            } else {
                scratch += *p++;
            }
        }
        const char* s = scratch.data();
        const char* se = s + scratch.size();
        while (s < se) {
            if (*s == '\\' && s + 1 < se && s[1] == '\\') {
                arena += '\\';
                s += 2;
            } else {
                arena += *s++;
            }
        }
        end_string();
    }
};

// [+-]?(\d+\.?\d*([eE][+-]?\d+)?|Inf|NaN) at p; returns the end of the
// match or nullptr, and the value as Python's float() gives it.
const char* match_value(const char* p, const char* e, double* out)
{
    const char* start = p;
    bool neg = false;
    if (p < e && (*p == '+' || *p == '-')) {
        neg = *p == '-';
        ++p;
    }
    if (e - p >= 3 && !std::memcmp(p, "Inf", 3)) {
        *out = neg ? -std::numeric_limits<double>::infinity()
                   : std::numeric_limits<double>::infinity();
        return p + 3;
    }
    if (e - p >= 3 && !std::memcmp(p, "NaN", 3)) {
        *out = std::numeric_limits<double>::quiet_NaN();
        return p + 3;
    }
    const char* num = p;
    if (p >= e || !is_digit((unsigned char)*p)) return nullptr;
    while (p < e && is_digit((unsigned char)*p)) ++p;
    if (p < e && *p == '.') ++p;
    while (p < e && is_digit((unsigned char)*p)) ++p;
    if (p < e && (*p == 'e' || *p == 'E')) {
        const char* t = p + 1;
        if (t < e && (*t == '+' || *t == '-')) ++t;
        if (t < e && is_digit((unsigned char)*t)) {
            while (t < e && is_digit((unsigned char)*t)) ++t;
            p = t;
        }
    }
    double v = 0.0;
    auto r = std::from_chars(num, p, v);
    if (r.ec != std::errc() || r.ptr != p) {
        // out of double's range: strtod rounds to +-inf / 0 as float() does
        std::string tmp(start, p);
        *out = std::strtod(tmp.c_str(), nullptr);
        return p;
    }
    *out = neg ? -v : v;
    return p;
}

// _LABEL_RE.finditer over the text between the braces.
int parse_labels(const char* p, const char* le, Parsed* out)
{
    int n = 0;
    while (p < le) {
        if (!label_start((unsigned char)*p)) {
            ++p;
            continue;
        }
        const char* k = p;
        const char* q = p + 1;
        while (q < le && label_char((unsigned char)*q)) ++q;
        if (q + 1 < le && q[0] == '=' && q[1] == '"') {
            const char* v = q + 2;
            const char* r = v;
            bool closed = false;
            while (r < le) {
                if (*r == '"') {
                    closed = true;
                    break;
                }
                if (*r == '\\') {
                    if (r + 1 >= le) break;   // `\` needs a following char
                    r += 2;
                } else {
                    ++r;
                }
            }
            if (closed) {
                out->add_string(k, q);
                out->add_unescaped(v, r);
                ++n;
                p = r + 1;
                continue;
            }
        }
        ++p;   // no match here: the regex retries one char further on
    }
    return n;
}

inline bool has_high(const char* p, const char* e)
{
    for (; p < e; ++p)
        if ((unsigned char)*p >= 0x80) return true;
    return false;
}

// One stripped, non-empty line against _LINE_RE. Returns false when the
// line has a non-ASCII byte where Python's Unicode rules for whitespace
// and digits could apply (anywhere but a comment or the label block).
bool parse_line(const char* p, const char* e, Parsed* out)
{
    if (*p == '#') return true;
    if ((unsigned char)*p >= 0x80 || (unsigned char)e[-1] >= 0x80) return false;
    if (!name_start((unsigned char)*p)) return true;
    const char* name = p;
    ++p;
    while (p < e && name_char((unsigned char)*p)) ++p;
    const char* name_end = p;
    const char* lb = nullptr;
    const char* le = nullptr;
    if (p < e && *p == '{') {
        // \{[^}]*\} ends at the first '}', quoted or not
        const char* r = (const char*)std::memchr(p + 1, '}', (size_t)(e - p - 1));
        if (!r) return true;
        lb = p + 1;
        le = r;
        p = r + 1;
    }
    if (has_high(p, e)) return false;
    if (p >= e || !is_ws((unsigned char)*p)) return true;
    while (p < e && is_ws((unsigned char)*p)) ++p;
    double value;
    p = match_value(p, e, &value);
    if (!p) return true;
    if (p < e) {
        // optional timestamp: \s+-?\d+ and then the end of the line
        if (!is_ws((unsigned char)*p)) return true;
        while (p < e && is_ws((unsigned char)*p)) ++p;
        if (p < e && *p == '-') ++p;
        if (p >= e || !is_digit((unsigned char)*p)) return true;
        while (p < e && is_digit((unsigned char)*p)) ++p;
        if (p != e) return true;
    }
    out->add_string(name, name_end);
    int n = (lb && lb < le) ? parse_labels(lb, le, out) : 0;
    out->label_counts.push_back(n);
    out->values.push_back(value);
    return true;
}

// U+0085, U+2028 and U+2029 are line boundaries to str.splitlines().
bool has_unicode_linesep(const char* buf, size_t len)
{
    const unsigned char* b = (const unsigned char*)buf;
    size_t i = 0;
    while (i < len) {
        if (len - i >= 8) {
            uint64_t w;
            std::memcpy(&w, b + i, 8);
            if (!(w & 0x8080808080808080ull)) {
                i += 8;
                continue;
            }
        }
        unsigned char c = b[i];
        if (c == 0xC2 && i + 1 < len && b[i + 1] == 0x85) return true;
        if (c == 0xE2 && i + 2 < len && b[i + 1] == 0x80 &&
            (b[i + 2] == 0xA8 || b[i + 2] == 0xA9))
            return true;
        ++i;
    }
    return false;
}

int parse_text(const char* buf, size_t len, Parsed* out)
{
    out->clear();
    if (has_unicode_linesep(buf, len)) return MI355X_SCRAPE_DEFER;
    const char* p = buf;
    const char* end = buf + len;
    while (p < end) {
        const char* e = p;
        while (e < end && !is_linesep((unsigned char)*e)) ++e;
        const char* b = p;
        const char* t = e;
        while (b < t && is_ws((unsigned char)*b)) ++b;
        while (t > b && is_ws((unsigned char)t[-1])) --t;
        if (b < t && !parse_line(b, t, out)) {
            out->clear();
            return MI355X_SCRAPE_DEFER;
        }
        p = e + 1;
    }
    return MI355X_SCRAPE_OK;
}

// ---------------------------------------------------------------- client

struct Handle {
    std::string host, path, host_header, request;
    int port = 0;
    int timeout_ms = 2000;
    int fd = -1;
    int connects = 0;
    int http_status = 0;
    std::string rx;       // raw response: headers + body
    Parsed parsed;
    char tmp[65536];

    void close_fd()
    {
        if (fd >= 0) ::close(fd);
        fd = -1;
    }
};

int do_connect(Handle* h)
{
    addrinfo hints;
    std::memset(&hints, 0, sizeof(hints));
    hints.ai_family = AF_UNSPEC;
    hints.ai_socktype = SOCK_STREAM;
    addrinfo* res = nullptr;
    std::string port = std::to_string(h->port);
    if (getaddrinfo(h->host.c_str(), port.c_str(), &hints, &res) != 0 || !res)
        return MI355X_SCRAPE_ERR_CONNECT;
    int fd = -1;
    for (addrinfo* ai = res; ai; ai = ai->ai_next) {
        fd = ::socket(ai->ai_family, ai->ai_socktype | SOCK_NONBLOCK | SOCK_CLOEXEC,
                      ai->ai_protocol);
        if (fd < 0) continue;
        int rc = ::connect(fd, ai->ai_addr, ai->ai_addrlen);
        if (rc != 0 && errno == EINPROGRESS) {
            pollfd p{fd, POLLOUT, 0};
            int pr;
            do {
                pr = ::poll(&p, 1, h->timeout_ms);
            } while (pr < 0 && errno == EINTR);
            int soerr = 0;
            socklen_t sl = sizeof(soerr);
            if (pr == 1 && getsockopt(fd, SOL_SOCKET, SO_ERROR, &soerr, &sl) == 0 &&
                soerr == 0)
                rc = 0;
        }
        if (rc == 0) break;
        ::close(fd);
        fd = -1;
    }
    freeaddrinfo(res);
    if (fd < 0) return MI355X_SCRAPE_ERR_CONNECT;
    // blocking from here on; the socket timeouts bound every send and recv
    int fl = fcntl(fd, F_GETFL, 0);
    fcntl(fd, F_SETFL, fl & ~O_NONBLOCK);
    int one = 1;
    setsockopt(fd, IPPROTO_TCP, TCP_NODELAY, &one, sizeof(one));
    timeval tv{h->timeout_ms / 1000, (h->timeout_ms % 1000) * 1000};
    setsockopt(fd, SOL_SOCKET, SO_RCVTIMEO, &tv, sizeof(tv));
    setsockopt(fd, SOL_SOCKET, SO_SNDTIMEO, &tv, sizeof(tv));
    h->fd = fd;
    ++h->connects;
    return MI355X_SCRAPE_OK;
}

bool ieq_prefix(const char* p, const char* e, const char* lit)
{
    for (; *lit; ++lit, ++p) {
        if (p >= e) return false;
        char c = *p;
        if (c >= 'A' && c <= 'Z') c = (char)(c - 'A' + 'a');
        if (c != *lit) return false;
    }
    return true;
}

bool icontains(const char* p, const char* e, const char* lit)
{
    for (; p < e; ++p)
        if (ieq_prefix(p, e, lit)) return true;
    return false;
}

// recv once into rx. Returns bytes read, 0 on EOF, or a negative error.
long recv_some(Handle* h, bool* dead)
{
    ssize_t n;
    do {
        n = ::recv(h->fd, h->tmp, sizeof(h->tmp), 0);
    } while (n < 0 && errno == EINTR);
    if (n > 0) {
        h->rx.append(h->tmp, (size_t)n);
        return (long)n;
    }
    if (n == 0) {
        *dead = true;
        return 0;
    }
    if (errno == EAGAIN || errno == EWOULDBLOCK) return MI355X_SCRAPE_ERR_TIMEOUT;
    *dead = errno == ECONNRESET || errno == EPIPE;
    return MI355X_SCRAPE_ERR_IO;
}

// One GET on the open connection. *stale is set when the failure is what
// a dead kept connection looks like: the send failed, or the first read
// saw EOF or a reset before any byte of a response.
int round_trip(Handle* h, bool* stale, const char** body, size_t* body_len)
{
    *stale = false;
    size_t off = 0;
    while (off < h->request.size()) {
        ssize_t n = ::send(h->fd, h->request.data() + off, h->request.size() - off,
                           MSG_NOSIGNAL);
        if (n < 0 && errno == EINTR) continue;
        if (n < 0 && (errno == EAGAIN || errno == EWOULDBLOCK))
            return MI355X_SCRAPE_ERR_TIMEOUT;
        if (n <= 0) {
            *stale = true;
            return MI355X_SCRAPE_ERR_IO;
        }
        off += (size_t)n;
    }

    h->rx.clear();
    h->http_status = 0;
    size_t hdr_end = std::string::npos;
    while (hdr_end == std::string::npos) {
        bool dead = false;
        size_t scan_from = h->rx.size() < 3 ? 0 : h->rx.size() - 3;
        long n = recv_some(h, &dead);
        if (n <= 0) {
            if (dead && h->rx.empty()) *stale = true;
            return n < 0 ? (int)n : MI355X_SCRAPE_ERR_IO;
        }
        size_t pos = h->rx.find("\r\n\r\n", scan_from);
        if (pos != std::string::npos)
            hdr_end = pos + 4;
        else if (h->rx.size() > kMaxHeaderBytes)
            return MI355X_SCRAPE_ERR_HTTP;
    }

    // status line: HTTP/1.x NNN
    const char* p = h->rx.data();
    const char* he = p + hdr_end;
    if (hdr_end < 12 || std::memcmp(p, "HTTP/1.", 7) != 0 || !is_digit((unsigned char)p[7]) ||
        p[8] != ' ' || !is_digit((unsigned char)p[9]) || !is_digit((unsigned char)p[10]) ||
        !is_digit((unsigned char)p[11]))
        return MI355X_SCRAPE_ERR_HTTP;
    bool close_after = p[7] == '0';
    h->http_status = (p[9] - '0') * 100 + (p[10] - '0') * 10 + (p[11] - '0');

    long long content_length = -1;
    bool chunked = false;
    const char* line = (const char*)std::memchr(p, '\n', hdr_end);
    while (line && line + 1 < he) {
        ++line;
        const char* eol = (const char*)std::memchr(line, '\n', (size_t)(he - line));
        if (!eol) break;
        if (ieq_prefix(line, eol, "content-length:")) {
            const char* v = line + 15;
            while (v < eol && (*v == ' ' || *v == '\t')) ++v;
            if (v >= eol || !is_digit((unsigned char)*v)) return MI355X_SCRAPE_ERR_HTTP;
            content_length = 0;
            while (v < eol && is_digit((unsigned char)*v)) {
                content_length = content_length * 10 + (*v++ - '0');
                if (content_length > (long long)kMaxBodyBytes)
                    return MI355X_SCRAPE_ERR_TOO_LARGE;
            }
        } else if (ieq_prefix(line, eol, "connection:")) {
            if (icontains(line + 11, eol, "close")) close_after = true;
        } else if (ieq_prefix(line, eol, "transfer-encoding:")) {
            if (icontains(line + 18, eol, "chunked")) chunked = true;
        }
        line = eol;
    }
    if (chunked) return MI355X_SCRAPE_ERR_UNSUPPORTED;
    if (h->http_status != 200) return MI355X_SCRAPE_ERR_HTTP;

    if (content_length >= 0) {
        size_t total = hdr_end + (size_t)content_length;
        while (h->rx.size() < total) {
            bool dead = false;
            long n = recv_some(h, &dead);
            if (n <= 0) return n < 0 ? (int)n : MI355X_SCRAPE_ERR_IO;
        }
        // bytes past the body would desynchronise the next exchange
        if (h->rx.size() > total) close_after = true;
        *body_len = (size_t)content_length;
    } else {
        for (;;) {
            bool dead = false;
            long n = recv_some(h, &dead);
            if (n == 0) break;
            if (n < 0) return (int)n;
            if (h->rx.size() - hdr_end > kMaxBodyBytes) return MI355X_SCRAPE_ERR_TOO_LARGE;
        }
        close_after = true;
        *body_len = h->rx.size() - hdr_end;
    }
    *body = h->rx.data() + hdr_end;
    if (close_after) h->close_fd();
    return MI355X_SCRAPE_OK;
}

void fill(const Handle* h, const char* body, size_t body_len, mi355x_scrape_result* out)
{
    const Parsed& r = h->parsed;
    out->n_samples = (int32_t)r.values.size();
    out->n_strings = r.n_strings;
    out->arena_len = (int32_t)r.arena.size();
    out->body_len = (int32_t)body_len;
    out->http_status = h->http_status;
    out->connects = h->connects;
    out->values = r.values.data();
    out->label_counts = r.label_counts.data();
    out->arena = r.arena.data();
    out->body = body;
}

} // namespace

extern "C" {

void* mi355x_scrape_open(const char* host, int port, const char* path,
                         const char* host_header, double timeout_s)
{
    if (!host || !*host || port <= 0 || port > 65535) return nullptr;
    Handle* h = new Handle;
    h->host = host;
    h->port = port;
    h->path = (path && *path) ? path : "/";
    h->host_header = (host_header && *host_header) ? host_header : host;
    double ms = timeout_s * 1e3;
    h->timeout_ms = ms < 1.0 ? 1 : ms > 3.6e6 ? 3600000 : (int)ms;
    h->request = "GET " + h->path + " HTTP/1.1\r\nHost: " + h->host_header +
                 "\r\nAccept: text/plain\r\nConnection: keep-alive\r\n\r\n";
    return h;
}

void mi355x_scrape_close(void* handle)
{
    Handle* h = (Handle*)handle;
    if (!h) return;
    h->close_fd();
    delete h;
}

int mi355x_scrape_fetch(void* handle, mi355x_scrape_result* out)
{
    Handle* h = (Handle*)handle;
    std::memset(out, 0, sizeof(*out));
    h->parsed.clear();
    const char* body = nullptr;
    size_t body_len = 0;
    int rc = MI355X_SCRAPE_ERR_IO;
    for (int attempt = 0; attempt < 2; ++attempt) {
        bool reused = h->fd >= 0;
        if (!reused) {
            rc = do_connect(h);
            if (rc != MI355X_SCRAPE_OK) break;
        }
        bool stale = false;
        rc = round_trip(h, &stale, &body, &body_len);
        if (rc == MI355X_SCRAPE_OK) break;
        h->close_fd();
        // a kept connection the server has meanwhile closed (idle timeout,
        // restart): one retry on a fresh one
        if (!(reused && stale)) break;
    }
    if (rc != MI355X_SCRAPE_OK) {
        out->http_status = h->http_status;
        out->connects = h->connects;
        return rc;
    }
    rc = parse_text(body, body_len, &h->parsed);
    fill(h, body, body_len, out);
    return rc;
}

int mi355x_scrape_parse(void* handle, const char* buf, int len,
                        mi355x_scrape_result* out)
{
    Handle* h = (Handle*)handle;
    std::memset(out, 0, sizeof(*out));
    h->http_status = 0;
    // keep a copy so `body` obeys the same lifetime rule as after a fetch
    h->rx.assign(buf ? buf : "", buf && len > 0 ? (size_t)len : 0);
    int rc = parse_text(h->rx.data(), h->rx.size(), &h->parsed);
    fill(h, h->rx.data(), h->rx.size(), out);
    return rc;
}

} // extern "C"
