// scrape_client.h — C ABI of libmi355x_scrape.so: a keep-alive HTTP/1.1
// scrape client plus a Prometheus text-exposition parser (ctypes surface
// for mi355x_gpu_hpa/control/scraper.py, and for scrape_selftest.cpp).
//
// One handle per target holds one persistent connection and the buffers of
// the last result. A fetch or a parse fills a flat result the caller turns
// into Sample(name, labels, value) objects without re-scanning text:
//
//   strings, in order:  name, k1, v1, k2, v2, ...   per sample
//   arena               the n_strings strings, each followed by '\n'
//                       (label values unescaped). No string holds a '\n':
//                       it ends a line, and unescaping creates none, so
//                       one split of the arena at '\n' yields them all.
//   label_counts[s]     number of (key, value) pairs of sample s
//   values[s]           the sample value
//
// The parser's specification is parse_prometheus_text() in scraper.py.
// Non-ASCII bytes are taken as they are in comments and inside a label
// block. Anywhere else Python's splitlines,
// strip, \s and \d have Unicode rules of their own; a body with a
// non-ASCII byte outside those two places, or with U+0085/U+2028/U+2029
// anywhere, is not parsed here: the call returns MI355X_SCRAPE_DEFER and
// the caller parses `body` itself.
//
// All pointers in the result stay valid until the next call on the handle.

#pragma once

#include <cstdint>

extern "C" {

enum {
    MI355X_SCRAPE_OK = 0,
    MI355X_SCRAPE_DEFER = 1,        // parse `body` in Python (see above)
    MI355X_SCRAPE_ERR_CONNECT = -1, // resolve/connect failed or timed out
    MI355X_SCRAPE_ERR_IO = -2,      // send/recv failed, or peer closed early
    MI355X_SCRAPE_ERR_TIMEOUT = -3, // send/recv exceeded the timeout
    MI355X_SCRAPE_ERR_HTTP = -4,    // malformed response or status != 200
    MI355X_SCRAPE_ERR_UNSUPPORTED = -5, // e.g. Transfer-Encoding: chunked
    MI355X_SCRAPE_ERR_TOO_LARGE = -6,   // response beyond kMaxBodyBytes
};

struct mi355x_scrape_result {
    int32_t n_samples;
    int32_t n_strings;
    int32_t arena_len;
    int32_t body_len;
    int32_t http_status;   // 0 for a parse of a caller-supplied buffer
    int32_t connects;      // connections this handle has opened so far
    const double* values;
    const int32_t* label_counts;
    const char* arena;
    const char* body;      // the raw response body (or the parsed buffer)
};

// host is a name or a literal address; host_header is what goes after
// "Host: ". timeout_s bounds connect, every send and every receive.
void* mi355x_scrape_open(const char* host, int port, const char* path,
                         const char* host_header, double timeout_s);
void mi355x_scrape_close(void* handle);

// GET the target over the kept connection (reconnecting once if the kept
// connection turns out dead) and parse the body.
int mi355x_scrape_fetch(void* handle, mi355x_scrape_result* out);

// Parse a caller-supplied buffer into the handle's result (no network).
int mi355x_scrape_parse(void* handle, const char* buf, int len,
                        mi355x_scrape_result* out);

} // extern "C"
