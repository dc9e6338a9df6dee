// http_server.h — minimal HTTP/1.1 server for the exporter endpoints.
//
// Serves what the reference exporter serves on :9400 (dcgm-exporter.yaml:
// 31-32,39-41) plus the liveness/readiness endpoints the reference lacks
// (SURVEY.md §5.3 flags the missing probes):
//   GET /metrics  -> Prometheus text format (render callback)
//   GET /healthz  -> 200 once the process is up (liveness)
//   GET /readyz   -> 200 after the first successful counter sample
//                    (readiness), 503 before
// One thread runs one poll() loop over the listen socket and the open
// connections. Connections are persistent (HTTP/1.1 keep-alive), the way
// Prometheus scrapes: at 1 s (kube-prometheus-stack-values.yaml:5) a scrape
// costs no connect/accept/close. Sockets are non-blocking, so a silent or
// slow client never delays another connection: a partial send waits for
// POLLOUT as pending output.

#pragma once

#include <atomic>
#include <functional>
#include <string>
#include <thread>

namespace mi355x {

class HttpServer {
  public:
    using Handler = std::function<std::string()>;   // returns /metrics body
    using ReadyFn = std::function<bool()>;

    HttpServer(std::string bind_addr, int port, Handler metrics, ReadyFn ready);
    ~HttpServer();

    // returns false + err on bind failure. port 0 picks an ephemeral port
    // (tests); bound_port() reports it.
    bool start(std::string* err);
    void stop();
    int bound_port() const { return port_; }

    // At most this many connections stay open; when one more is accepted,
    // the longest-idle one is closed.
    static constexpr int kMaxConnections = 64;
    // A connection with no traffic for this long is closed. Longer than
    // the 1 s to 15 s scrape intervals in use, so a Prometheus keeps its
    // connection from one scrape to the next.
    static constexpr int kIdleTimeoutS = 60;

  private:
    struct Conn;
    void serve_loop();
    bool service(Conn& c, short revents);
    static bool answerable(const Conn& c);
    void answer_buffered(Conn& c);
    bool flush(Conn& c);
    void respond(Conn& c, const std::string& req);

    std::string bind_addr_;
    int port_;
    Handler metrics_;
    ReadyFn ready_;
    std::atomic<int> listen_fd_{-1};
    std::atomic<bool> stop_{false};
    std::thread thread_;
};

} // namespace mi355x
