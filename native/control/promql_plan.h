// promql_plan.h — tokenizer, parser and flat plan for the PromQL subset of
// mi355x_gpu_hpa/control/promql.py (pure C++, no Python headers).
//
// The parser accepts a strict subset of what promql.parse() accepts and
// never reports an error: for anything it is not sure to evaluate exactly
// like the Python evaluator it answers "defer" (compile() returns false),
// and the caller runs the Python parser, which owns every error text.
// Deferred on purpose: =~ and !~ matchers, a matcher on __name__, any
// backslash, group_right, name or matcher lists not written `a, b, c`, an
// aggregation-function name used as a metric name, bytes outside ASCII
// other than inside a string literal, nesting deeper than kMaxDepth, more
// than kMaxNodes nodes, and
// every input promql.parse() would reject.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace promql {

constexpr int kMaxDepth = 64;
constexpr int kMaxNodes = 512;

enum class NodeKind : uint8_t { Scalar, Selector, Agg, BinOp };
enum class AggFunc : uint8_t { Sum, Avg, Max, Min, Count };
enum class MatchKind : uint8_t { Full, On, Ignoring };

struct Matcher {
  int32_t label;   // index into Plan::strings
  int32_t value;   // index into Plan::strings
  bool negate;     // != instead of =
};

// Half-open range into one of the plan's flat arrays.
struct Range {
  int32_t begin = 0;
  int32_t end = 0;
  int32_t size() const { return end - begin; }
};

struct Node {
  NodeKind kind = NodeKind::Scalar;
  // Scalar
  double value = 0.0;
  // Selector: strings[name], matchers[matchers.begin..end)
  int32_t name = -1;
  Range matchers;
  // Agg: func over nodes[child]; has_by distinguishes `by ()` from none
  AggFunc func = AggFunc::Sum;
  bool has_by = false;
  Range by;        // into Plan::names
  int32_t child = -1;
  // BinOp: nodes[lhs] op nodes[rhs]
  char op = 0;     // one of * / + -
  MatchKind match = MatchKind::Full;
  Range match_names;   // on(...) or ignoring(...) list, into Plan::names
  bool has_group_left = false;
  Range group_left;    // into Plan::names
  int32_t lhs = -1;
  int32_t rhs = -1;
};

// Children precede their parents in `nodes`; `root` is the last node.
struct Plan {
  std::vector<Node> nodes;
  std::vector<Matcher> matchers;
  std::vector<int32_t> names;        // label-name lists: indices into strings
  std::vector<std::string> strings;  // deduplicated
  int32_t root = -1;
};

// Parse `text[0..len)` into `out`. Returns true when the expression is
// inside the native subset; false means "defer to promql.parse()".
bool compile(const char* text, size_t len, Plan* out);

}  // namespace promql
