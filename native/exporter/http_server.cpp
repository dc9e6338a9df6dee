#include "http_server.h"

#include <arpa/inet.h>
#include <fcntl.h>
#include <netinet/in.h>
#include <netinet/tcp.h>
#include <poll.h>
#include <sys/socket.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cstring>
#include <vector>

namespace mi355x {

HttpServer::HttpServer(std::string bind_addr, int port, Handler metrics, ReadyFn ready)
    : bind_addr_(std::move(bind_addr)), port_(port), metrics_(std::move(metrics)),
      ready_(std::move(ready))
{
}

HttpServer::~HttpServer() { stop(); }

bool HttpServer::start(std::string* err)
{
    int fd = ::socket(AF_INET, SOCK_STREAM, 0);
    listen_fd_ = fd;
    if (fd < 0) {
        if (err) *err = "socket() failed";
        return false;
    }
    int one = 1;
    setsockopt(fd, SOL_SOCKET, SO_REUSEADDR, &one, sizeof(one));
    sockaddr_in addr;
    std::memset(&addr, 0, sizeof(addr));
    addr.sin_family = AF_INET;
    addr.sin_port = htons((uint16_t)port_);
    if (bind_addr_.empty() || bind_addr_ == "0.0.0.0")
        addr.sin_addr.s_addr = INADDR_ANY;
    else if (inet_pton(AF_INET, bind_addr_.c_str(), &addr.sin_addr) != 1) {
        if (err) *err = "bad bind address " + bind_addr_;
        ::close(fd);
        listen_fd_ = -1;
        return false;
    }
    if (::bind(fd, (sockaddr*)&addr, sizeof(addr)) != 0) {
        if (err) *err = "bind failed on port " + std::to_string(port_);
        ::close(fd);
        listen_fd_ = -1;
        return false;
    }
    if (port_ == 0) {
        socklen_t len = sizeof(addr);
        getsockname(fd, (sockaddr*)&addr, &len);
        port_ = ntohs(addr.sin_port);
    }
    if (::listen(fd, 64) != 0) {
        if (err) *err = "listen failed";
        ::close(fd);
        listen_fd_ = -1;
        return false;
    }
    // the loop drains accept() until EAGAIN
    fcntl(fd, F_SETFL, fcntl(fd, F_GETFL, 0) | O_NONBLOCK);
    stop_ = false;
    thread_ = std::thread([this] { serve_loop(); });
    return true;
}

void HttpServer::stop()
{
    stop_ = true;
    int fd = listen_fd_.exchange(-1);
    if (fd >= 0) {
        ::shutdown(fd, SHUT_RDWR);
        // close AFTER joining the serve loop so its poll/accept never
        // touches a recycled fd number. The loop closes the connections
        // it owns itself, on its way out.
        if (thread_.joinable()) thread_.join();
        ::close(fd);
        return;
    }
    if (thread_.joinable()) thread_.join();
}

namespace {

using Clock = std::chrono::steady_clock;

// A request must fit in this much; one that reaches it without a
// terminator is answered from its first line and the connection closed.
constexpr size_t kMaxRequestBytes = 4095;
// Pipelined requests are not answered faster than the client reads: past
// this much unsent output the rest of the read buffer waits.
constexpr size_t kMaxPendingOut = 256 * 1024;
constexpr int kPollMs = 250;

bool ieq_at(const std::string& s, size_t pos, const char* lit)
{
    for (; *lit; ++lit, ++pos) {
        if (pos >= s.size()) return false;
        char c = s[pos];
        if (c >= 'A' && c <= 'Z') c = (char)(c - 'A' + 'a');
        if (c != *lit) return false;
    }
    return true;
}

// HTTP/1.1 persistence: keep the connection unless the request line is not
// HTTP/1.1 (1.0, 0.9, garbage) or a Connection header says close.
bool wants_close(const std::string& req, const std::string& line)
{
    if (line.size() < 8 || line.compare(line.size() - 8, 8, "HTTP/1.1") != 0)
        return true;
    size_t pos = 0;
    while ((pos = req.find("\r\n", pos)) != std::string::npos) {
        pos += 2;
        if (!ieq_at(req, pos, "connection:")) continue;
        size_t eol = req.find("\r\n", pos);
        if (eol == std::string::npos) eol = req.size();
        for (size_t i = pos + 11; i + 5 <= eol; ++i)
            if (ieq_at(req, i, "close")) return true;
    }
    return false;
}

} // namespace

struct HttpServer::Conn {
    int fd;
    std::string in;          // bytes received, not yet answered
    std::string out;         // responses not yet sent
    size_t out_off = 0;
    bool close_after = false; // close once `out` is flushed
    bool peer_eof = false;
    Clock::time_point last_active;
};

void HttpServer::serve_loop()
{
    std::vector<Conn> conns;
    std::vector<pollfd> pfds;
    while (!stop_) {
        int lfd = listen_fd_.load();
        if (lfd < 0) break;
        pfds.clear();
        pfds.push_back(pollfd{lfd, POLLIN, 0});
        for (const Conn& c : conns) {
            // a connection with unsent output is not read further until
            // the client has taken it
            short ev = c.out_off < c.out.size() ? POLLOUT : POLLIN;
            pfds.push_back(pollfd{c.fd, ev, 0});
        }
        int rc = ::poll(pfds.data(), pfds.size(), kPollMs);
        if (stop_) break;
        auto now = Clock::now();
        if (rc > 0) {
            // conns[i] pairs with pfds[i + 1]; connections accepted below
            // are appended and have no pollfd yet
            size_t n = conns.size();
            for (size_t i = 0; i < n; ++i) {
                if (!pfds[i + 1].revents) continue;
                conns[i].last_active = now;
                if (!service(conns[i], pfds[i + 1].revents)) {
                    // take what the client still had in flight (the rest
                    // of an oversize request), so that the close does not
                    // turn into a reset that overtakes the response
                    char sink[4096];
                    for (int k = 0; k < 16 && ::recv(conns[i].fd, sink, sizeof(sink), 0) > 0; ++k) {
                    }
                    ::close(conns[i].fd);
                    conns[i].fd = -1;
                }
            }
            if (pfds[0].revents & POLLIN) {
                for (;;) {
                    int fd = ::accept4(lfd, nullptr, nullptr, SOCK_NONBLOCK | SOCK_CLOEXEC);
                    if (fd < 0) break;
                    int one = 1;
                    setsockopt(fd, IPPROTO_TCP, TCP_NODELAY, &one, sizeof(one));
                    Conn c;
                    c.fd = fd;
                    c.last_active = now;
                    conns.push_back(std::move(c));
                }
            }
        }
        // idle timeout, then the cap: the longest-idle connections go first
        for (Conn& c : conns) {
            if (c.fd >= 0 && now - c.last_active > std::chrono::seconds(kIdleTimeoutS)) {
                ::close(c.fd);
                c.fd = -1;
            }
        }
        conns.erase(std::remove_if(conns.begin(), conns.end(),
                                   [](const Conn& c) { return c.fd < 0; }),
                    conns.end());
        while (conns.size() > (size_t)kMaxConnections) {
            auto oldest = std::min_element(conns.begin(), conns.end(),
                                           [](const Conn& a, const Conn& b) {
                                               return a.last_active < b.last_active;
                                           });
            ::close(oldest->fd);
            conns.erase(oldest);
        }
    }
    for (Conn& c : conns) ::close(c.fd);
}

// Returns false when the connection is finished and must be closed.
bool HttpServer::service(Conn& c, short revents)
{
    if ((revents & POLLIN) && c.in.size() < kMaxRequestBytes) {
        char buf[kMaxRequestBytes];
        size_t room = kMaxRequestBytes - c.in.size();
        ssize_t n = ::recv(c.fd, buf, room, 0);
        if (n > 0)
            c.in.append(buf, (size_t)n);
        else if (n == 0)
            c.peer_eof = true;
        else if (errno != EAGAIN && errno != EWOULDBLOCK && errno != EINTR)
            return false;
    } else if (revents & (POLLERR | POLLHUP | POLLNVAL)) {
        if (!(revents & POLLOUT)) return false;
    }
    for (;;) {
        answer_buffered(c);
        if (!flush(c)) return false;
        if (c.out_off < c.out.size()) return true;   // wait for POLLOUT
        if (c.close_after) return false;
        // everything sent: go on if the buffer holds more to answer
        if (!answerable(c)) break;
    }
    return !c.peer_eof;
}

// A complete request, or an unterminated one that gets its answer anyway:
// an oversize one, or what a peer sent before it finished sending.
bool HttpServer::answerable(const Conn& c)
{
    return c.in.find("\r\n\r\n") != std::string::npos ||
           c.in.size() >= kMaxRequestBytes || (c.peer_eof && !c.in.empty());
}

// Answer the complete requests in the read buffer, in order.
void HttpServer::answer_buffered(Conn& c)
{
    while (!c.close_after && c.out.size() - c.out_off < kMaxPendingOut) {
        size_t end = c.in.find("\r\n\r\n");
        if (end != std::string::npos) {
            std::string req = c.in.substr(0, end + 2);
            c.in.erase(0, end + 4);
            respond(c, req);
            continue;
        }
        // no terminator: answered from its first line, then closed
        if (answerable(c)) {
            std::string req;
            req.swap(c.in);
            c.close_after = true;
            respond(c, req);
        }
        break;
    }
}

bool HttpServer::flush(Conn& c)
{
    while (c.out_off < c.out.size()) {
        ssize_t n = ::send(c.fd, c.out.data() + c.out_off, c.out.size() - c.out_off,
                           MSG_NOSIGNAL);
        if (n > 0) {
            c.out_off += (size_t)n;
            continue;
        }
        if (n < 0 && errno == EINTR) continue;
        if (n < 0 && (errno == EAGAIN || errno == EWOULDBLOCK)) return true;
        return false;
    }
    c.out.clear();
    c.out_off = 0;
    return true;
}

void HttpServer::respond(Conn& c, const std::string& req)
{
    auto line_end = req.find("\r\n");
    std::string line = line_end == std::string::npos ? req : req.substr(0, line_end);

    const char* status = "200 OK";
    const char* ctype = "text/plain; charset=utf-8";
    std::string body;
    if (line.rfind("GET /metrics", 0) == 0) {
        body = metrics_();
        ctype = "text/plain; version=0.0.4; charset=utf-8";
    } else if (line.rfind("GET /healthz", 0) == 0) {
        body = "ok\n";
    } else if (line.rfind("GET /readyz", 0) == 0) {
        if (ready_ && ready_()) {
            body = "ready\n";
        } else {
            status = "503 Service Unavailable";
            body = "no successful GPU sample yet\n";
        }
    } else if (line.rfind("GET /", 0) == 0) {
        status = "404 Not Found";
        body = "see /metrics\n";
    } else {
        status = "405 Method Not Allowed";
        body = "GET only\n";
    }
    if (wants_close(req, line)) c.close_after = true;

    // headers and body leave in one send
    std::string& o = c.out;
    o.reserve(o.size() + body.size() + 160);
    o += "HTTP/1.1 ";
    o += status;
    o += "\r\nContent-Type: ";
    o += ctype;
    o += "\r\nContent-Length: ";
    o += std::to_string(body.size());
    o += c.close_after ? "\r\nConnection: close\r\n\r\n" : "\r\nConnection: keep-alive\r\n\r\n";
    o += body;
}

} // namespace mi355x
