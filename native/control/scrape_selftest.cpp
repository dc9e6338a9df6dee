// scrape_selftest.cpp — stand-alone check of scrape_client.cpp, meant to be
// built with -fsanitize=address,undefined (make scrape-selftest). Parser
// inputs are heap buffers of their exact size so an overread is caught; the
// client runs against a loopback listener inside this program. Exits
// non-zero on the first mismatch; prints nothing on success.
//
//   scrape-selftest [BODY_FILE]
//
// BODY_FILE, a /metrics body saved from an exporter, is parsed at every
// truncation as well; without it a built-in body in the same format is.

#include "scrape_client.h"

#include <arpa/inet.h>
#include <netinet/in.h>
#include <poll.h>
#include <sys/socket.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

static int g_fail = 0;

#define EXPECT(cond)                                                         \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "%s:%d: EXPECT(%s) failed\n", __FILE__,     \
                         __LINE__, #cond);                                   \
            ++g_fail;                                                        \
        }                                                                    \
    } while (0)

struct S {
    std::string name;
    std::vector<std::pair<std::string, std::string>> labels;
    double value;
};

// Copy a result out, checking the layout's own invariants on the way.
static std::vector<S> unpack(const mi355x_scrape_result& r)
{
    std::vector<S> out;
    int si = 0;
    EXPECT(r.n_samples >= 0 && r.n_strings >= r.n_samples);
    // the arena is n_strings strings, each ended by '\n'
    std::vector<std::string> strs;
    const char* p = r.arena;
    const char* end = r.arena + r.arena_len;
    while (p < end) {
        const char* nl = (const char*)std::memchr(p, '\n', (size_t)(end - p));
        EXPECT(nl != nullptr);
        if (!nl) break;
        strs.emplace_back(p, nl);
        p = nl + 1;
    }
    EXPECT((int)strs.size() == r.n_strings);
    auto str = [&](int i) {
        EXPECT(i < (int)strs.size());
        return i < (int)strs.size() ? strs[i] : std::string();
    };
    for (int s = 0; s < r.n_samples; ++s) {
        S x;
        x.name = str(si++);
        for (int l = 0; l < r.label_counts[s]; ++l) {
            std::string k = str(si++);
            std::string v = str(si++);
            x.labels.emplace_back(k, v);
        }
        x.value = r.values[s];
        out.push_back(std::move(x));
    }
    EXPECT(si == r.n_strings);
    return out;
}

static std::vector<S> parse(void* h, const std::string& text, int want_rc = MI355X_SCRAPE_OK)
{
    // exact-size heap copy: one byte past the end is a red zone
    std::vector<char> exact(text.begin(), text.end());
    mi355x_scrape_result r;
    int rc = mi355x_scrape_parse(h, exact.data(), (int)exact.size(), &r);
    EXPECT(rc == want_rc);
    EXPECT(r.body_len == (int)text.size());
    if (rc != MI355X_SCRAPE_OK) return {};
    return unpack(r);
}

static void test_parser(void* h)
{
    auto one = [&](const std::string& line) {
        auto v = parse(h, line);
        EXPECT(v.size() == 1);
        return v.empty() ? S{} : v[0];
    };
    {   // escaped quote and backslash; \n stays two characters
        S s = one("m{a=\"x\\\"y\",b=\"c\\\\d\",c=\"e\\nf\"} 1\n");
        EXPECT(s.name == "m" && s.labels.size() == 3);
        if (s.labels.size() == 3) {
            EXPECT(s.labels[0].second == "x\"y");
            EXPECT(s.labels[1].second == "c\\d");
            EXPECT(s.labels[2].second == "e\\nf");
        }
    }
    {   // the two replace passes run one after the other: \\" -> \"
        S s = one("m{a=\"\\\\\\\"\"} 1");
        EXPECT(s.labels.size() == 1 && s.labels[0].second == "\\\"");
    }
    EXPECT(one("m{} 2").labels.empty());
    EXPECT(one("m 2").labels.empty());
    EXPECT(one("m 2 1700000000000").value == 2.0);
    EXPECT(one("m 2 -5").value == 2.0);
    EXPECT(std::isinf(one("m +Inf").value) && one("m +Inf").value > 0);
    EXPECT(std::isinf(one("m Inf").value));
    EXPECT(std::isinf(one("m -Inf").value) && one("m -Inf").value < 0);
    EXPECT(std::isnan(one("m NaN").value));
    EXPECT(one("m 1.5e3").value == 1500.0);
    EXPECT(one("m -2E-2").value == -0.02);
    EXPECT(one("m +7.").value == 7.0);
    EXPECT(std::isinf(one("m 1e999").value));
    EXPECT(one("m 1e-999").value == 0.0);
    EXPECT(one("  m\t3  \r\n").value == 3.0);
    EXPECT(parse(h, "a 1\r\nb 2\r\n").size() == 2);
    // a '}' inside a quoted value ends the label block early: rejected
    EXPECT(parse(h, "m{a=\"}\"} 1\n").empty());
    // rejected lines
    EXPECT(parse(h, "m\n").empty());
    EXPECT(parse(h, "m{a=\"b\"}\n").empty());
    EXPECT(parse(h, "m{a=\"b\" 1\n").empty());
    EXPECT(parse(h, "m 1e\n").empty());
    EXPECT(parse(h, "m .5\n").empty());
    EXPECT(parse(h, "m 1 2 3\n").empty());
    EXPECT(parse(h, "m 1 x\n").empty());
    EXPECT(parse(h, "9m 1\n").empty());
    EXPECT(parse(h, "# HELP m x\n# TYPE m gauge\n\n").empty());
    EXPECT(parse(h, "").empty());
    {   // truncated last line
        auto v = parse(h, "a{x=\"1\"} 1\nb{x=\"2");
        EXPECT(v.size() == 1);
    }
    {   // an escaped quote does not end the value
        S s = one("m{a=\"x\\\",b=\"y\"} 1");
        EXPECT(s.labels.size() == 1);
        if (s.labels.size() == 1)
            EXPECT(s.labels[0].first == "a" && s.labels[0].second == "x\",b=");
    }
    {   // non-ASCII passes through in comments and label values
        auto v = parse(h, "# HELP m caf\xc3\xa9\nm{a=\"\xc3\xa9\"} 1\n");
        EXPECT(v.size() == 1 && v[0].labels.size() == 1);
        if (v.size() == 1 && v[0].labels.size() == 1)
            EXPECT(v[0].labels[0].second == "\xc3\xa9");
    }
    // elsewhere it is the caller's to parse: Unicode spaces, digits, line ends
    parse(h, "m 1\xc2\xa0\n", MI355X_SCRAPE_DEFER);
    parse(h, "\xc2\xa0# c\n", MI355X_SCRAPE_DEFER);
    parse(h, "m\xc2\xa0" "1\n", MI355X_SCRAPE_DEFER);
    parse(h, "m \xd9\xa1\n", MI355X_SCRAPE_DEFER);
    parse(h, "m{a=\"x\xe2\x80\xa8y\"} 1\n", MI355X_SCRAPE_DEFER);
    parse(h, "# a\xc2\x85m 1\n", MI355X_SCRAPE_DEFER);
}

// The exporter's format: HELP/TYPE comments (with a non-ASCII dash, as the
// renderer's own HELP texts have), labelled series, one without labels.
static const char kBody[] =
    "# HELP dcgm_gpu_utilization GPU utilization (%) \xe2\x80\x94 busy share.\n"
    "# TYPE dcgm_gpu_utilization gauge\n"
    "dcgm_gpu_utilization{gpu=\"0\",UUID=\"GPU-mock-0000\",device=\"card0\","
    "modelName=\"AMD Instinct MI355X\",Hostname=\"node \\\"a\\\\b\\\"\"} 80.5\n"
    "dcgm_gpu_utilization{gpu=\"1\",UUID=\"GPU-mock-0001\",device=\"card1\","
    "modelName=\"AMD Instinct MI355X\",Hostname=\"n\"} 0\n"
    "# HELP dcgm_gpu_temp GPU temperature (C).\n"
    "# TYPE dcgm_gpu_temp gauge\n"
    "dcgm_gpu_temp{gpu=\"0\",UUID=\"GPU-mock-0000\"} 41.25 1700000000000\n"
    "amd_xgmi_total_bytes_per_second{gpu=\"0\"} 1.5e+09\r\n"
    "amd_exporter_samples_total 12\n"
    "amd_exporter_last_error_age_seconds +Inf\n";

static void test_truncations(void* h, const std::string& body, size_t min_samples)
{
    std::vector<S> full = parse(h, body);
    EXPECT(full.size() >= min_samples);
    for (size_t cut = 0; cut < body.size(); ++cut) {
        std::vector<S> part = parse(h, body.substr(0, cut));
        EXPECT(part.size() <= full.size());
        // every sample but the (possibly cut) last one is the full parse's
        for (size_t i = 0; i + 1 < part.size() && i < full.size(); ++i) {
            EXPECT(part[i].name == full[i].name);
            EXPECT(part[i].labels == full[i].labels);
        }
        if (g_fail) return;
    }
}

// ------------------------------------------------------------ loopback server

enum Mode { KEEPALIVE, SAY_CLOSE, EOF_BODY, SILENT_CLOSE, STALL, NOT_FOUND, CHUNKED };

struct Server {
    int lfd = -1;
    int port = 0;
    Mode mode;
    std::atomic<int> accepted{0};
    std::atomic<bool> stop{false};
    std::thread th;

    explicit Server(Mode m) : mode(m)
    {
        lfd = ::socket(AF_INET, SOCK_STREAM, 0);
        sockaddr_in a;
        std::memset(&a, 0, sizeof(a));
        a.sin_family = AF_INET;
        a.sin_addr.s_addr = htonl(INADDR_LOOPBACK);
        ::bind(lfd, (sockaddr*)&a, sizeof(a));
        socklen_t len = sizeof(a);
        getsockname(lfd, (sockaddr*)&a, &len);
        port = ntohs(a.sin_port);
        ::listen(lfd, 8);
        th = std::thread([this] { run(); });
    }
    ~Server()
    {
        stop = true;
        th.join();
        ::close(lfd);
    }
    static bool wait_readable(int fd, std::atomic<bool>& stop)
    {
        while (!stop) {
            pollfd p{fd, POLLIN, 0};
            if (::poll(&p, 1, 20) > 0) return true;
        }
        return false;
    }
    void run()
    {
        while (wait_readable(lfd, stop)) {
            int fd = ::accept(lfd, nullptr, nullptr);
            if (fd < 0) continue;
            ++accepted;
            serve(fd);
            ::close(fd);
        }
    }
    void serve(int fd)
    {
        const std::string body = "up{job=\"x\"} 1\n";
        std::string in;
        while (wait_readable(fd, stop)) {
            char b[1024];
            ssize_t n = ::recv(fd, b, sizeof(b), 0);
            if (n <= 0) return;
            in.append(b, (size_t)n);
            size_t e = in.find("\r\n\r\n");
            if (e == std::string::npos) continue;
            in.erase(0, e + 4);
            std::string r;
            std::string len = std::to_string(body.size());
            switch (mode) {
            case KEEPALIVE:
            case SILENT_CLOSE:
                r = "HTTP/1.1 200 OK\r\nContent-Length: " + len + "\r\n\r\n" + body;
                break;
            case SAY_CLOSE:
                r = "HTTP/1.1 200 OK\r\ncontent-length: " + len +
                    "\r\nConnection: close\r\n\r\n" + body;
                break;
            case EOF_BODY:
                r = "HTTP/1.0 200 OK\r\n\r\n" + body;
                break;
            case STALL:
                r = "HTTP/1.1 200 OK\r\nContent-Length: 100\r\n\r\n" + body;
                break;
            case NOT_FOUND:
                r = "HTTP/1.1 404 Not Found\r\nContent-Length: 0\r\n\r\n";
                break;
            case CHUNKED:
                r = "HTTP/1.1 200 OK\r\nTransfer-Encoding: chunked\r\n\r\n0\r\n\r\n";
                break;
            }
            ::send(fd, r.data(), r.size(), MSG_NOSIGNAL);
            if (mode == STALL) {
                wait_readable(fd, stop);   // until the client gives up
                return;
            }
            if (mode != KEEPALIVE) return;
        }
    }
};

static int fetch(void* h, mi355x_scrape_result* r)
{
    int rc = mi355x_scrape_fetch(h, r);
    if (rc == MI355X_SCRAPE_OK) {
        auto v = unpack(*r);
        EXPECT(v.size() == 1 && v[0].name == "up" && v[0].value == 1.0);
        EXPECT(r->http_status == 200);
    }
    return rc;
}

static void test_client()
{
    mi355x_scrape_result r;
    {
        Server s(KEEPALIVE);
        void* h = mi355x_scrape_open("127.0.0.1", s.port, "/metrics", "", 2.0);
        EXPECT(fetch(h, &r) == MI355X_SCRAPE_OK);
        EXPECT(fetch(h, &r) == MI355X_SCRAPE_OK);
        EXPECT(r.connects == 1 && s.accepted == 1);
        mi355x_scrape_close(h);
    }
    for (Mode m : {SAY_CLOSE, EOF_BODY, SILENT_CLOSE}) {
        Server s(m);
        void* h = mi355x_scrape_open("localhost", s.port, "/metrics", "", 2.0);
        EXPECT(fetch(h, &r) == MI355X_SCRAPE_OK);
        if (m == SILENT_CLOSE)   // let the close reach this side
            std::this_thread::sleep_for(std::chrono::milliseconds(50));
        EXPECT(fetch(h, &r) == MI355X_SCRAPE_OK);
        EXPECT(r.connects == 2 && s.accepted == 2);
        mi355x_scrape_close(h);
    }
    {
        Server s(STALL);
        void* h = mi355x_scrape_open("127.0.0.1", s.port, "/metrics", "", 0.2);
        auto t0 = std::chrono::steady_clock::now();
        EXPECT(fetch(h, &r) == MI355X_SCRAPE_ERR_TIMEOUT);
        double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        EXPECT(dt > 0.15 && dt < 1.5);
        mi355x_scrape_close(h);
    }
    {
        Server s(NOT_FOUND);
        void* h = mi355x_scrape_open("127.0.0.1", s.port, "/nope", "", 2.0);
        EXPECT(fetch(h, &r) == MI355X_SCRAPE_ERR_HTTP);
        EXPECT(r.http_status == 404);
        mi355x_scrape_close(h);
    }
    {
        Server s(CHUNKED);
        void* h = mi355x_scrape_open("127.0.0.1", s.port, "/metrics", "", 2.0);
        EXPECT(fetch(h, &r) == MI355X_SCRAPE_ERR_UNSUPPORTED);
        mi355x_scrape_close(h);
    }
    {   // a port nobody listens on
        int port;
        {
            Server s(KEEPALIVE);
            port = s.port;
        }
        void* h = mi355x_scrape_open("127.0.0.1", port, "/metrics", "", 0.5);
        EXPECT(fetch(h, &r) == MI355X_SCRAPE_ERR_CONNECT);
        mi355x_scrape_close(h);
    }
    EXPECT(mi355x_scrape_open("", 80, "/", "", 1.0) == nullptr);
    EXPECT(mi355x_scrape_open("h", 0, "/", "", 1.0) == nullptr);
}

int main(int argc, char** argv)
{
    void* h = mi355x_scrape_open("127.0.0.1", 1, "/", "", 1.0);
    test_parser(h);
    test_truncations(h, std::string(kBody, sizeof(kBody) - 1), 6);
    if (argc > 1) {
        std::ifstream f(argv[1], std::ios::binary);
        std::stringstream ss;
        ss << f.rdbuf();
        EXPECT(f.good() && !ss.str().empty());
        test_truncations(h, ss.str(), 1);
    }
    mi355x_scrape_close(h);
    test_client();
    return g_fail ? 1 : 0;
}
