// promql_selftest.cpp — stand-alone self-test of the PromQL parser and plan
// (promql_plan.h), meant to be built with ASan+UBSan (`make
// promql-selftest`). Exit 0 and silence mean: every corpus expression was
// accepted or deferred as expected with a well-formed plan, and no
// truncation of one and no random byte string made the parser touch memory
// it should not.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "promql_plan.h"

namespace {

int g_failures = 0;

void fail(const char* what, const std::string& expr) {
  std::fprintf(stderr, "FAIL %s: %s\n", what, expr.c_str());
  ++g_failures;
}

bool in_range(int32_t i, size_t n) {
  return i >= 0 && static_cast<size_t>(i) < n;
}
bool range_ok(promql::Range r, size_t n) {
  return r.begin >= 0 && r.begin <= r.end && static_cast<size_t>(r.end) <= n;
}

// Every index of an accepted plan points inside the plan, and children
// come before their parents.
bool well_formed(const promql::Plan& p) {
  if (p.nodes.empty() || p.root != static_cast<int32_t>(p.nodes.size()) - 1)
    return false;
  if (p.nodes.size() > static_cast<size_t>(promql::kMaxNodes)) return false;
  for (int32_t s : p.names)
    if (!in_range(s, p.strings.size())) return false;
  for (const promql::Matcher& m : p.matchers)
    if (!in_range(m.label, p.strings.size()) ||
        !in_range(m.value, p.strings.size()))
      return false;
  for (size_t i = 0; i < p.nodes.size(); ++i) {
    const promql::Node& n = p.nodes[i];
    switch (n.kind) {
      case promql::NodeKind::Scalar:
        break;
      case promql::NodeKind::Selector:
        if (!in_range(n.name, p.strings.size()) ||
            !range_ok(n.matchers, p.matchers.size()))
          return false;
        break;
      case promql::NodeKind::Agg:
        if (!in_range(n.child, i) || !range_ok(n.by, p.names.size()))
          return false;
        break;
      case promql::NodeKind::BinOp:
        if (!in_range(n.lhs, i) || !in_range(n.rhs, i) ||
            !range_ok(n.match_names, p.names.size()) ||
            !range_ok(n.group_left, p.names.size()))
          return false;
        if (n.op != '*' && n.op != '/' && n.op != '+' && n.op != '-')
          return false;
        break;
    }
  }
  return true;
}

struct Case {
  const char* expr;
  bool accepted;
};

const Case kCorpus[] = {
    // the reference rule and the multi-metric rules
    {"avg(max by(node, pod, namespace) (dcgm_gpu_utilization) "
     "* on(pod) group_left(label_app) "
     "max by(pod, label_app) (kube_pod_labels{label_app=\"cuda-test\"}))",
     true},
    {"avg(max by(node, pod, namespace) (amd_hbm_bandwidth_utilization) * "
     "on(pod) group_left(label_app) max by(pod, label_app) "
     "(kube_pod_labels{label_app=\"cuda-test\"}))",
     true},
    {"avg(max by(node, pod, namespace) (amd_xgmi_link_utilization) * on(pod) "
     "group_left(label_app) max by(pod, label_app) "
     "(kube_pod_labels{label_app=\"cuda-test\"}))",
     true},
    // the adapter's query shape
    {"sum(cuda_test_gpu_avg{namespace=\"default\",deployment=\"cuda-test\"}) "
     "by (deployment)",
     true},
    {"sum by(g) (m)", true},
    {"sum(m) by (g)", true},
    {"count by () (m)", true},
    {"l * ignoring(gpu) r", true},
    {"l * ignoring(gpu) group_left() r", true},
    {"l * on(pod) group_left r", true},
    {"l / group_left(x, y) r", true},
    {"2 + 3 * 4", true},
    {"m * 100", true},
    {"100 / m", true},
    {"a + b * c", true},
    {"(a + b) * c", true},
    {"a - b / c", true},
    {"m / 0", true},
    {"m{a=\"x\", b!='y'}", true},
    {"m{}", true},
    {"1.5e3 * m:rate_5m", true},
    {"min(max(a) + count(b))", true},
    {"by + group_left_total", true},
    // deferred on purpose
    {"m{a=~\"x|y\"}", false},
    {"m{a!~\"x\"}", false},
    {"m{__name__=\"m\"}", false},
    {"m{a=\"x\\\"y\"}", false},
    {"l * on(pod) group_right(x) r", false},
    {"sum by(a b) (m)", false},
    {"sum by(a,) (m)", false},
    {"m{a=\"1\" b=\"2\"}", false},
    {"m{a=\"1\",}", false},
    {"sum", false},
    {"sum + 1", false},
    {"m{a=\"\xc3\xa9\"} * \xc2\xa0 2", false},
    // what promql.parse() rejects
    {"", false},
    {"avg(", false},
    {"m{a=}", false},
    {"m n", false},
    {"-1", false},
    {"1.", false},
    {"m{a=\"x}", false},
    {"a * on b", false},
    {"by + on", false},
    {"sum by(a) (m) by (b)", false},
    {"a ! b", false},
    {"a $ b", false},
};

void check(const std::string& expr, bool want) {
  promql::Plan plan;
  const bool got = promql::compile(expr.data(), expr.size(), &plan);
  if (got != want) fail(want ? "not accepted" : "not deferred", expr);
  if (got && !well_formed(plan)) fail("malformed plan", expr);
  if (!got && (!plan.nodes.empty() || plan.root != -1))
    fail("defer left a plan behind", expr);
}

// Any input: the parser answers, and what it accepts is well formed. The
// bytes are copied into an exactly-sized heap block so that ASan sees a
// read past either end.
void probe(const std::string& expr) {
  std::vector<char> exact(expr.begin(), expr.end());
  promql::Plan plan;
  if (promql::compile(exact.data(), exact.size(), &plan) && !well_formed(plan))
    fail("malformed plan", expr);
}

uint64_t g_rng = 0x9e3779b97f4a7c15ull;
uint32_t next_u32() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return static_cast<uint32_t>(g_rng >> 16);
}

}  // namespace

int main() {
  for (const Case& c : kCorpus) check(c.expr, c.accepted);

  for (const Case& c : kCorpus) {
    const std::string full(c.expr);
    for (size_t cut = 0; cut <= full.size(); ++cut) probe(full.substr(0, cut));
  }

  // random bytes, and random strings over the grammar's own alphabet
  // (which reach much deeper into the parser)
  const std::string alphabet = "ab_:09.eE+-*/(){},=!~\"' \t\nsumbyon\\";
  for (int i = 0; i < 20000; ++i) {
    std::string s;
    const size_t len = next_u32() % 48;
    const bool raw = (i & 1) != 0;
    for (size_t k = 0; k < len; ++k)
      s.push_back(raw ? static_cast<char>(next_u32() & 0xff)
                      : alphabet[next_u32() % alphabet.size()]);
    probe(s);
  }

  // nesting and chains beyond the limits defer instead of overflowing
  std::string deep(static_cast<size_t>(promql::kMaxDepth) + 8, '(');
  deep += "m";
  deep.append(static_cast<size_t>(promql::kMaxDepth) + 8, ')');
  check(deep, false);
  std::string huge(100000, '(');
  check(huge, false);
  std::string chain = "m";
  for (int i = 0; i < promql::kMaxNodes; ++i) chain += " + m";
  check(chain, false);
  check("((((m))))", true);

  if (g_failures) {
    std::fprintf(stderr, "%d failure(s)\n", g_failures);
    return 1;
  }
  return 0;
}
