// promql_plan.cpp — see promql_plan.h. The grammar mirrors _Parser in
// mi355x_gpu_hpa/control/promql.py production by production; wherever the
// Python parser is laxer than the list syntax `a, b, c`, or would raise,
// this one defers.
#include "promql_plan.h"

#include <charconv>
#include <string_view>
#include <system_error>

namespace promql {
namespace {

enum class Tok : uint8_t { Num, Id, Str, Op };

struct Token {
  Tok kind;
  std::string_view text;   // Str: without the quotes
};

bool is_space(unsigned char c) {
  return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\f' ||
         c == '\v';
}
bool is_digit(unsigned char c) { return c >= '0' && c <= '9'; }
bool is_id_start(unsigned char c) {
  return (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || c == '_' ||
         c == ':';
}
bool is_id_char(unsigned char c) { return is_id_start(c) || is_digit(c); }

// _TOKEN_RE of promql.py over ASCII. false = defer.
bool tokenize(std::string_view s, std::vector<Token>* out) {
  size_t i = 0;
  const size_t n = s.size();
  while (true) {
    while (i < n && is_space(static_cast<unsigned char>(s[i]))) ++i;
    if (i >= n) return true;
    const unsigned char c = static_cast<unsigned char>(s[i]);
    const size_t start = i;
    if (is_digit(c)) {
      // \d+(?:\.\d+)?(?:[eE][+-]?\d+)?
      while (i < n && is_digit(static_cast<unsigned char>(s[i]))) ++i;
      if (i + 1 < n && s[i] == '.' &&
          is_digit(static_cast<unsigned char>(s[i + 1]))) {
        ++i;
        while (i < n && is_digit(static_cast<unsigned char>(s[i]))) ++i;
      }
      if (i < n && (s[i] == 'e' || s[i] == 'E')) {
        size_t j = i + 1;
        if (j < n && (s[j] == '+' || s[j] == '-')) ++j;
        if (j < n && is_digit(static_cast<unsigned char>(s[j]))) {
          while (j < n && is_digit(static_cast<unsigned char>(s[j]))) ++j;
          i = j;
        }
      }
      out->push_back({Tok::Num, s.substr(start, i - start)});
    } else if (is_id_start(c)) {
      while (i < n && is_id_char(static_cast<unsigned char>(s[i]))) ++i;
      out->push_back({Tok::Id, s.substr(start, i - start)});
    } else if (c == '"' || c == '\'') {
      ++i;
      while (i < n && s[i] != static_cast<char>(c)) {
        if (s[i] == '\\') return false;   // escapes: Python's business
        ++i;
      }
      if (i >= n) return false;           // unterminated
      out->push_back({Tok::Str, s.substr(start + 1, i - start - 1)});
      ++i;
    } else {
      size_t len = 0;
      switch (c) {
        case '=':
          len = (i + 1 < n && s[i + 1] == '~') ? 2 : 1;
          break;
        case '!':
          if (i + 1 < n && (s[i + 1] == '~' || s[i + 1] == '=')) len = 2;
          break;
        case '{': case '}': case '(': case ')': case ',':
        case '*': case '/': case '+': case '-':
          len = 1;
          break;
        default:
          break;
      }
      if (len == 0) return false;   // not a token (or not ASCII): defer
      out->push_back({Tok::Op, s.substr(start, len)});
      i += len;
    }
  }
}

bool agg_func(std::string_view name, AggFunc* f) {
  if (name == "sum") { *f = AggFunc::Sum; return true; }
  if (name == "avg") { *f = AggFunc::Avg; return true; }
  if (name == "max") { *f = AggFunc::Max; return true; }
  if (name == "min") { *f = AggFunc::Min; return true; }
  if (name == "count") { *f = AggFunc::Count; return true; }
  return false;
}

class Parser {
 public:
  Parser(const std::vector<Token>& toks, Plan* plan)
      : toks_(toks), plan_(plan) {}

  bool parse() {
    int32_t root = -1;
    if (!additive(0, &root)) return false;
    if (i_ != toks_.size()) return false;   // trailing input
    // the evaluator recurses once per level of a left-deep chain
    if (plan_->nodes.size() > static_cast<size_t>(kMaxNodes)) return false;
    plan_->root = root;
    return true;
  }

 private:
  const Token* peek(size_t ahead = 0) const {
    return i_ + ahead < toks_.size() ? &toks_[i_ + ahead] : nullptr;
  }
  bool peek_is(Tok kind, std::string_view text) const {
    const Token* t = peek();
    return t && t->kind == kind && t->text == text;
  }
  bool accept_op(std::string_view text) {
    if (!peek_is(Tok::Op, text)) return false;
    ++i_;
    return true;
  }

  int32_t intern(std::string_view s) {
    for (size_t k = 0; k < plan_->strings.size(); ++k)
      if (plan_->strings[k] == s) return static_cast<int32_t>(k);
    plan_->strings.emplace_back(s);
    return static_cast<int32_t>(plan_->strings.size() - 1);
  }

  int32_t push(const Node& n) {
    plan_->nodes.push_back(n);
    return static_cast<int32_t>(plan_->nodes.size() - 1);
  }

  // `(` [id (`,` id)*] `)` — the Python parser also takes `(a b)` and
  // `(a,)`; those defer.
  bool name_list(Range* out) {
    if (!accept_op("(")) return false;
    std::vector<int32_t> local;
    if (!accept_op(")")) {
      while (true) {
        const Token* t = peek();
        if (!t || t->kind != Tok::Id) return false;
        local.push_back(intern(t->text));
        ++i_;
        if (accept_op(")")) break;
        if (!accept_op(",")) return false;
      }
    }
    out->begin = static_cast<int32_t>(plan_->names.size());
    plan_->names.insert(plan_->names.end(), local.begin(), local.end());
    out->end = static_cast<int32_t>(plan_->names.size());
    return true;
  }

  bool match_modifiers(Node* n) {
    const Token* t = peek();
    if (t && t->kind == Tok::Id && (t->text == "on" || t->text == "ignoring")) {
      n->match = t->text == "on" ? MatchKind::On : MatchKind::Ignoring;
      ++i_;
      if (!name_list(&n->match_names)) return false;
    }
    t = peek();
    if (t && t->kind == Tok::Id &&
        (t->text == "group_left" || t->text == "group_right")) {
      if (t->text == "group_right") return false;
      ++i_;
      n->has_group_left = true;
      if (peek_is(Tok::Op, "(") && !name_list(&n->group_left)) return false;
    }
    return true;
  }

  bool binary_level(int depth, bool additive_level, int32_t* out) {
    int32_t lhs = -1;
    if (!(additive_level ? multiplicative(depth, &lhs) : primary(depth, &lhs)))
      return false;
    while (true) {
      const Token* t = peek();
      if (!t || t->kind != Tok::Op || t->text.size() != 1) break;
      const char op = t->text[0];
      if (additive_level ? (op != '+' && op != '-') : (op != '*' && op != '/'))
        break;
      ++i_;
      Node n;
      n.kind = NodeKind::BinOp;
      n.op = op;
      if (!match_modifiers(&n)) return false;
      int32_t rhs = -1;
      if (!(additive_level ? multiplicative(depth, &rhs) : primary(depth, &rhs)))
        return false;
      n.lhs = lhs;
      n.rhs = rhs;
      lhs = push(n);
    }
    *out = lhs;
    return true;
  }

  bool additive(int depth, int32_t* out) {
    if (depth > kMaxDepth) return false;
    return binary_level(depth, true, out);
  }
  bool multiplicative(int depth, int32_t* out) {
    return binary_level(depth, false, out);
  }

  bool primary(int depth, int32_t* out) {
    const Token* t = peek();
    if (!t) return false;
    if (t->kind == Tok::Op && t->text == "(") {
      ++i_;
      if (!additive(depth + 1, out)) return false;
      return accept_op(")");
    }
    if (t->kind == Tok::Num) {
      Node n;
      n.kind = NodeKind::Scalar;
      const char* b = t->text.data();
      const char* e = b + t->text.size();
      auto r = std::from_chars(b, e, n.value);
      if (r.ec != std::errc() || r.ptr != e) return false;
      ++i_;
      *out = push(n);
      return true;
    }
    if (t->kind != Tok::Id) return false;
    AggFunc f;
    if (agg_func(t->text, &f)) {
      const Token* nxt = peek(1);
      const bool call = nxt && ((nxt->kind == Tok::Op && nxt->text == "(") ||
                                (nxt->kind == Tok::Id && nxt->text == "by"));
      if (!call) return false;   // a metric named like a function: defer
      ++i_;
      Node n;
      n.kind = NodeKind::Agg;
      n.func = f;
      if (peek_is(Tok::Id, "by")) {
        ++i_;
        n.has_by = true;
        if (!name_list(&n.by)) return false;
      }
      if (!accept_op("(")) return false;
      if (!additive(depth + 1, &n.child)) return false;
      if (!accept_op(")")) return false;
      if (!n.has_by && peek_is(Tok::Id, "by")) {
        ++i_;
        n.has_by = true;
        if (!name_list(&n.by)) return false;
      }
      *out = push(n);
      return true;
    }
    Node n;
    n.kind = NodeKind::Selector;
    n.name = intern(t->text);
    ++i_;
    if (accept_op("{")) {
      std::vector<Matcher> local;
      if (!accept_op("}")) {
        while (true) {
          const Token* name = peek();
          const Token* op = peek(1);
          const Token* val = peek(2);
          if (!name || !op || !val) return false;
          if (name->kind != Tok::Id || name->text == "__name__") return false;
          if (op->kind != Tok::Op || (op->text != "=" && op->text != "!="))
            return false;   // regex matchers and anything else
          if (val->kind != Tok::Str) return false;
          local.push_back({intern(name->text), intern(val->text),
                           op->text == "!="});
          i_ += 3;
          if (accept_op("}")) break;
          if (!accept_op(",")) return false;
        }
      }
      n.matchers.begin = static_cast<int32_t>(plan_->matchers.size());
      plan_->matchers.insert(plan_->matchers.end(), local.begin(), local.end());
      n.matchers.end = static_cast<int32_t>(plan_->matchers.size());
    }
    *out = push(n);
    return true;
  }

  const std::vector<Token>& toks_;
  Plan* plan_;
  size_t i_ = 0;
};

}  // namespace

bool compile(const char* text, size_t len, Plan* out) {
  *out = Plan();
  std::vector<Token> toks;
  if (!tokenize(std::string_view(text, len), &toks)) return false;
  Parser p(toks, out);
  if (!p.parse()) {
    *out = Plan();
    return false;
  }
  return true;
}

}  // namespace promql
