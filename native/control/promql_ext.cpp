// promql_ext.cpp — CPython extension `_mi355x_promql`: evaluates PromQL
// instant queries from cached plans (promql_plan.h) over a list of Sample
// objects, exactly like promql._eval() in mi355x_gpu_hpa/control/promql.py,
// or answers DEFER so that the caller runs the Python evaluator, which
// stays the specification and owns every error.
//
//   bind(Sample)              once, before the first evaluate()
//   evaluate(expr, samples)   -> list of Sample, or the DEFER object
//   counters()                -> dict: handled, deferred_parse,
//                                deferred_eval, compiles, cache_size
//   reset()                   drop the plan cache, zero the counters
//   CACHE_CAPACITY            bound of the plan cache (oldest plan leaves)
//
// evaluate() never raises an error of its own, never releases the GIL and
// never changes its inputs. It defers when the expression is outside the
// native subset (remembered in the cache, so such an expression is parsed
// natively once) and when an input is not exactly what the fast path
// assumes: list of exact Sample, labels an exact dict of exact str to exact
// str, value an exact float, name an exact str; or when the Python
// evaluator would raise (aggregation over a scalar, duplicate match keys).
#define PY_SSIZE_T_CLEAN
#include <Python.h>

#include <algorithm>
#include <cmath>
#include <deque>
#include <limits>
#include <memory>
#include <string>
#include <string_view>
#include <unordered_map>
#include <utility>
#include <vector>

#include "promql_plan.h"

namespace {

constexpr size_t kCacheCapacity = 128;

// --- plan cache -------------------------------------------------------------

struct Entry {
  std::string key;
  bool defer = true;
  promql::Plan plan;
  std::vector<PyObject*> strs;   // plan.strings as str objects (owned)

  ~Entry() {
    for (PyObject* s : strs) Py_XDECREF(s);
  }
};

std::unordered_map<std::string_view, std::shared_ptr<Entry>> g_cache;
std::deque<std::shared_ptr<Entry>> g_fifo;

struct Counters {
  unsigned long long handled = 0;
  unsigned long long deferred_parse = 0;
  unsigned long long deferred_eval = 0;
  unsigned long long compiles = 0;
} g_counters;

PyObject* g_sample_type = nullptr;
PyObject* g_defer = nullptr;
PyObject* g_empty_str = nullptr;
PyObject* g_dunder_name = nullptr;
PyObject* g_attr_name = nullptr;
PyObject* g_attr_labels = nullptr;
PyObject* g_attr_value = nullptr;
#if PY_VERSION_HEX >= 0x030C0000
PyObject* g_builtin_sum = nullptr;
#endif

std::shared_ptr<Entry> lookup_or_compile(const char* text, size_t len) {
  auto it = g_cache.find(std::string_view(text, len));
  if (it != g_cache.end()) return it->second;

  auto e = std::make_shared<Entry>();
  e->key.assign(text, len);
  ++g_counters.compiles;
  e->defer = !promql::compile(text, len, &e->plan);
  if (!e->defer) {
    e->strs.reserve(e->plan.strings.size());
    for (const std::string& s : e->plan.strings) {
      PyObject* o = PyUnicode_DecodeUTF8(s.data(),
                                         static_cast<Py_ssize_t>(s.size()),
                                         nullptr);
      if (!o) {
        PyErr_Clear();
        e->defer = true;
        break;
      }
      e->strs.push_back(o);
    }
  }
  while (g_fifo.size() >= kCacheCapacity) {
    g_cache.erase(std::string_view(g_fifo.front()->key));
    g_fifo.pop_front();
  }
  g_cache.emplace(std::string_view(e->key), e);
  g_fifo.push_back(e);
  return e;
}

// --- evaluation -------------------------------------------------------------

struct Defer {};   // thrown to leave an evaluation; any Python error is cleared

// Owned references that live until the call returns.
struct Arena {
  std::vector<PyObject*> refs;
  ~Arena() {
    for (PyObject* o : refs) Py_DECREF(o);
  }
  PyObject* keep(PyObject* o) {
    if (!o) throw Defer();
    refs.push_back(o);
    return o;
  }
};

// One series of an instant vector; every pointer is borrowed from the
// arena or from the caller's list.
struct Elem {
  PyObject* name;
  PyObject* labels;
  double value;
  PyObject* orig;   // the caller's Sample when a selector passed it through
};

struct Value {
  bool is_scalar = false;
  double scalar = 0.0;
  std::vector<Elem> vec;
};

inline bool str_ready(PyObject* s) {
#if PY_VERSION_HEX < 0x030C0000
  return PyUnicode_READY(s) == 0;
#else
  (void)s;
  return true;
#endif
}

inline bool str_eq(PyObject* a, PyObject* b) {
  if (a == b) return true;
  if (PyUnicode_GET_LENGTH(a) != PyUnicode_GET_LENGTH(b)) return false;
  return PyUnicode_Compare(a, b) == 0;
}

// labels.get(key, "") — borrowed
inline PyObject* label_get(PyObject* labels, PyObject* key) {
  PyObject* v = PyDict_GetItemWithError(labels, key);
  if (!v) {
    if (PyErr_Occurred()) throw Defer();
    return g_empty_str;
  }
  return v;
}

class Evaluator {
 public:
  Evaluator(const Entry& e, const std::vector<Elem>& input, Arena* arena)
      : e_(e), plan_(e.plan), input_(input), arena_(arena) {}

  Value eval(int32_t idx) {
    const promql::Node& n = plan_.nodes[static_cast<size_t>(idx)];
    switch (n.kind) {
      case promql::NodeKind::Scalar: {
        Value v;
        v.is_scalar = true;
        v.scalar = n.value;
        return v;
      }
      case promql::NodeKind::Selector:
        return selector(n);
      case promql::NodeKind::Agg:
        return agg(n);
      case promql::NodeKind::BinOp:
        return binop(n);
    }
    throw Defer();
  }

 private:
  PyObject* str(int32_t i) const { return e_.strs[static_cast<size_t>(i)]; }
  PyObject* name_at(int32_t i) const {
    return str(plan_.names[static_cast<size_t>(i)]);
  }

  Value selector(const promql::Node& n) {
    Value out;
    PyObject* want = str(n.name);
    for (const Elem& s : input_) {
      if (!str_eq(s.name, want)) continue;
      bool ok = true;
      for (int32_t m = n.matchers.begin; m < n.matchers.end && ok; ++m) {
        const promql::Matcher& mt = plan_.matchers[static_cast<size_t>(m)];
        const bool same = str_eq(label_get(s.labels, str(mt.label)),
                                 str(mt.value));
        ok = mt.negate ? !same : same;
      }
      if (ok) out.vec.push_back(s);
    }
    return out;
  }

  // tuple(labels.get(n, "") for n in names) — identifies the same groups
  // as Sample.label_key(names), whose tuples repeat the fixed names
  PyObject* key_of_names(PyObject* labels, promql::Range names) {
    PyObject* t = arena_->keep(PyTuple_New(names.size()));
    for (int32_t i = names.begin; i < names.end; ++i) {
      PyObject* v = label_get(labels, name_at(i));
      Py_INCREF(v);
      PyTuple_SET_ITEM(t, i - names.begin, v);
    }
    return t;
  }

  // mklabels(): all labels but __name__ (and but `drop`), in one canonical
  // order, flattened to (k1, v1, k2, v2, ...)
  PyObject* key_of_all(PyObject* labels, const promql::Range* drop) {
    std::vector<std::pair<PyObject*, PyObject*>> kv;
    kv.reserve(static_cast<size_t>(PyDict_GET_SIZE(labels)));
    Py_ssize_t pos = 0;
    PyObject *k, *v;
    while (PyDict_Next(labels, &pos, &k, &v)) {
      if (str_eq(k, g_dunder_name)) continue;
      bool dropped = false;
      if (drop)
        for (int32_t i = drop->begin; i < drop->end && !dropped; ++i)
          dropped = str_eq(k, name_at(i));
      if (!dropped) kv.emplace_back(k, v);
    }
    std::sort(kv.begin(), kv.end(),
              [](const std::pair<PyObject*, PyObject*>& a,
                 const std::pair<PyObject*, PyObject*>& b) {
                return PyUnicode_Compare(a.first, b.first) < 0;
              });
    PyObject* t = arena_->keep(
        PyTuple_New(static_cast<Py_ssize_t>(2 * kv.size())));
    for (size_t i = 0; i < kv.size(); ++i) {
      Py_INCREF(kv[i].first);
      Py_INCREF(kv[i].second);
      PyTuple_SET_ITEM(t, static_cast<Py_ssize_t>(2 * i), kv[i].first);
      PyTuple_SET_ITEM(t, static_cast<Py_ssize_t>(2 * i + 1), kv[i].second);
    }
    return t;
  }

  // Index stored under `key` in `index`, or -1.
  static Py_ssize_t index_get(PyObject* index, PyObject* key) {
    PyObject* v = PyDict_GetItemWithError(index, key);
    if (!v) {
      if (PyErr_Occurred()) throw Defer();
      return -1;
    }
    return PyLong_AsSsize_t(v);
  }
  static void index_set(PyObject* index, PyObject* key, Py_ssize_t i) {
    PyObject* v = PyLong_FromSsize_t(i);
    if (!v) throw Defer();
    const int rc = PyDict_SetItem(index, key, v);
    Py_DECREF(v);
    if (rc < 0) throw Defer();
  }

  double sum_of(const std::vector<double>& vals) {
#if PY_VERSION_HEX >= 0x030C0000
    // sum() is compensated from 3.12 on: let the interpreter's own add up
    PyObject* lst = arena_->keep(
        PyList_New(static_cast<Py_ssize_t>(vals.size())));
    for (size_t i = 0; i < vals.size(); ++i) {
      PyObject* f = PyFloat_FromDouble(vals[i]);
      if (!f) throw Defer();
      PyList_SET_ITEM(lst, static_cast<Py_ssize_t>(i), f);
    }
    PyObject* r = arena_->keep(PyObject_CallOneArg(g_builtin_sum, lst));
    if (!PyFloat_CheckExact(r)) throw Defer();
    return PyFloat_AS_DOUBLE(r);
#else
    // sum(): int 0 plus the first float, then left to right
    double acc = 0.0;
    for (double v : vals) acc += v;
    return acc;
#endif
  }

  double aggregate(promql::AggFunc f, const std::vector<double>& vals) {
    switch (f) {
      case promql::AggFunc::Sum:
        return sum_of(vals);
      case promql::AggFunc::Avg:
        return sum_of(vals) / static_cast<double>(vals.size());
      case promql::AggFunc::Max: {
        // max(): a later item replaces the current one only if it is
        // greater, so a NaN stays where it came first
        double m = vals[0];
        for (size_t i = 1; i < vals.size(); ++i)
          if (vals[i] > m) m = vals[i];
        return m;
      }
      case promql::AggFunc::Min: {
        double m = vals[0];
        for (size_t i = 1; i < vals.size(); ++i)
          if (vals[i] < m) m = vals[i];
        return m;
      }
      case promql::AggFunc::Count:
        return static_cast<double>(vals.size());
    }
    throw Defer();
  }

  Value agg(const promql::Node& n) {
    Value in = eval(n.child);
    if (in.is_scalar) throw Defer();   // "aggregation over scalar"
    Value out;
    if (in.vec.empty()) return out;

    struct Group {
      PyObject* labels;   // of the group's first series
      std::vector<double> vals;
    };
    std::vector<Group> groups;
    if (!n.has_by || n.by.size() == 0) {
      groups.push_back({in.vec[0].labels, {}});
      groups[0].vals.reserve(in.vec.size());
      for (const Elem& s : in.vec) groups[0].vals.push_back(s.value);
    } else {
      PyObject* index = arena_->keep(PyDict_New());
      for (const Elem& s : in.vec) {
        PyObject* key = key_of_names(s.labels, n.by);
        Py_ssize_t g = index_get(index, key);
        if (g < 0) {
          g = static_cast<Py_ssize_t>(groups.size());
          index_set(index, key, g);
          groups.push_back({s.labels, {}});
        }
        groups[static_cast<size_t>(g)].vals.push_back(s.value);
      }
    }
    out.vec.reserve(groups.size());
    for (const Group& g : groups) {
      PyObject* labels = arena_->keep(PyDict_New());
      if (n.has_by) {
        for (int32_t i = n.by.begin; i < n.by.end; ++i) {
          PyObject* v = label_get(g.labels, name_at(i));
          if (PyUnicode_GET_LENGTH(v) == 0) continue;
          if (PyDict_SetItem(labels, name_at(i), v) < 0) throw Defer();
        }
      }
      out.vec.push_back({g_empty_str, labels, aggregate(n.func, g.vals),
                         nullptr});
    }
    return out;
  }

  static double apply(char op, double a, double b) {
    switch (op) {
      case '*': return a * b;
      case '/': return b != 0 ? a / b : std::numeric_limits<double>::quiet_NaN();
      case '+': return a + b;
      default:  return a - b;
    }
  }

  PyObject* match_key(const promql::Node& n, PyObject* labels) {
    switch (n.match) {
      case promql::MatchKind::On:
        return key_of_names(labels, n.match_names);
      case promql::MatchKind::Ignoring:
        return key_of_all(labels, &n.match_names);
      case promql::MatchKind::Full:
        break;
    }
    return key_of_all(labels, nullptr);
  }

  Value binop(const promql::Node& n) {
    Value lhs = eval(n.lhs);
    Value rhs = eval(n.rhs);
    Value out;
    if (lhs.is_scalar && rhs.is_scalar) {
      out.is_scalar = true;
      out.scalar = apply(n.op, lhs.scalar, rhs.scalar);
      return out;
    }
    if (rhs.is_scalar) {
      out.vec.reserve(lhs.vec.size());
      for (const Elem& s : lhs.vec)
        out.vec.push_back({s.name, s.labels, apply(n.op, s.value, rhs.scalar),
                           nullptr});
      return out;
    }
    if (lhs.is_scalar) {
      out.vec.reserve(rhs.vec.size());
      for (const Elem& s : rhs.vec)
        out.vec.push_back({s.name, s.labels, apply(n.op, lhs.scalar, s.value),
                           nullptr});
      return out;
    }

    PyObject* right_index = arena_->keep(PyDict_New());
    for (size_t i = 0; i < rhs.vec.size(); ++i) {
      PyObject* key = match_key(n, rhs.vec[i].labels);
      if (index_get(right_index, key) >= 0) throw Defer();   // many-to-many
      index_set(right_index, key, static_cast<Py_ssize_t>(i));
    }
    PyObject* seen_left =
        n.has_group_left ? nullptr : arena_->keep(PyDict_New());
    for (const Elem& s : lhs.vec) {
      PyObject* key = match_key(n, s.labels);
      const Py_ssize_t ri = index_get(right_index, key);
      if (ri < 0) continue;
      const Elem& r = rhs.vec[static_cast<size_t>(ri)];
      if (seen_left) {
        if (index_get(seen_left, key) >= 0) throw Defer();   // many-to-one
        index_set(seen_left, key, 1);
      }
      PyObject* labels = arena_->keep(PyDict_Copy(s.labels));
      for (int32_t i = n.group_left.begin; i < n.group_left.end; ++i) {
        PyObject* v = PyDict_GetItemWithError(r.labels, name_at(i));
        if (!v) {
          if (PyErr_Occurred()) throw Defer();
          continue;
        }
        if (PyDict_SetItem(labels, name_at(i), v) < 0) throw Defer();
      }
      out.vec.push_back({g_empty_str, labels, apply(n.op, s.value, r.value),
                         nullptr});
    }
    return out;
  }

  const Entry& e_;
  const promql::Plan& plan_;
  const std::vector<Elem>& input_;
  Arena* arena_;
};

// The caller's list as Elems, or Defer if any element is not exactly what
// the Python evaluator's fast case looks like.
void extract(PyObject* samples, Arena* arena, std::vector<Elem>* out) {
  const Py_ssize_t n = PyList_GET_SIZE(samples);
  out->reserve(static_cast<size_t>(n));
  for (Py_ssize_t i = 0; i < n; ++i) {
    PyObject* s = PyList_GET_ITEM(samples, i);
    if (reinterpret_cast<PyObject*>(Py_TYPE(s)) != g_sample_type) throw Defer();
    PyObject* name = arena->keep(PyObject_GetAttr(s, g_attr_name));
    PyObject* labels = arena->keep(PyObject_GetAttr(s, g_attr_labels));
    PyObject* value = arena->keep(PyObject_GetAttr(s, g_attr_value));
    if (!PyUnicode_CheckExact(name) || !PyDict_CheckExact(labels) ||
        !PyFloat_CheckExact(value))
      throw Defer();
    if (!str_ready(name)) throw Defer();
    Py_ssize_t pos = 0;
    PyObject *k, *v;
    while (PyDict_Next(labels, &pos, &k, &v)) {
      if (!PyUnicode_CheckExact(k) || !PyUnicode_CheckExact(v)) throw Defer();
      if (!str_ready(k) || !str_ready(v)) throw Defer();
    }
    out->push_back({name, labels, PyFloat_AS_DOUBLE(value), s});
  }
}

PyObject* make_sample(PyObject* name, PyObject* labels, double value) {
  PyObject* f = PyFloat_FromDouble(value);
  if (!f) return nullptr;
  PyObject* s = PyObject_CallFunctionObjArgs(g_sample_type, name, labels, f,
                                             nullptr);
  Py_DECREF(f);
  return s;
}

// New list of Samples for `v` (promql.evaluate() wraps a scalar).
PyObject* materialize(const Value& v) {
  if (v.is_scalar) {
    PyObject* labels = PyDict_New();
    if (!labels) return nullptr;
    PyObject* s = make_sample(g_empty_str, labels, v.scalar);
    Py_DECREF(labels);
    if (!s) return nullptr;
    PyObject* lst = PyList_New(1);
    if (!lst) {
      Py_DECREF(s);
      return nullptr;
    }
    PyList_SET_ITEM(lst, 0, s);
    return lst;
  }
  PyObject* lst = PyList_New(static_cast<Py_ssize_t>(v.vec.size()));
  if (!lst) return nullptr;
  for (size_t i = 0; i < v.vec.size(); ++i) {
    const Elem& e = v.vec[i];
    PyObject* s;
    if (e.orig) {
      s = e.orig;
      Py_INCREF(s);
    } else {
      s = make_sample(e.name, e.labels, e.value);
      if (!s) {
        Py_DECREF(lst);
        return nullptr;
      }
    }
    PyList_SET_ITEM(lst, static_cast<Py_ssize_t>(i), s);
  }
  return lst;
}

PyObject* defer_result(unsigned long long* counter) {
  PyErr_Clear();
  ++*counter;
  Py_INCREF(g_defer);
  return g_defer;
}

PyObject* py_evaluate(PyObject*, PyObject* const* args, Py_ssize_t nargs) {
  if (nargs != 2) {
    PyErr_SetString(PyExc_TypeError, "evaluate(expr, samples)");
    return nullptr;
  }
  PyObject* expr = args[0];
  PyObject* samples = args[1];
  if (!g_sample_type || !PyUnicode_CheckExact(expr) ||
      !PyList_CheckExact(samples))
    return defer_result(&g_counters.deferred_eval);
  Py_ssize_t len = 0;
  const char* text = PyUnicode_AsUTF8AndSize(expr, &len);
  if (!text) return defer_result(&g_counters.deferred_parse);

  try {
    std::shared_ptr<Entry> entry =
        lookup_or_compile(text, static_cast<size_t>(len));
    if (entry->defer) return defer_result(&g_counters.deferred_parse);

    PyObject* result = nullptr;
    {
      Arena arena;
      try {
        std::vector<Elem> input;
        extract(samples, &arena, &input);
        Evaluator ev(*entry, input, &arena);
        result = materialize(ev.eval(entry->plan.root));
      } catch (const Defer&) {
        result = nullptr;
      }
    }
    if (!result) return defer_result(&g_counters.deferred_eval);
    ++g_counters.handled;
    return result;
  } catch (const std::exception&) {   // bad_alloc and the like
    return defer_result(&g_counters.deferred_eval);
  }
}

PyObject* py_bind(PyObject*, PyObject* arg) {
  if (!PyType_Check(arg)) {
    PyErr_SetString(PyExc_TypeError, "bind() takes the Sample class");
    return nullptr;
  }
  Py_INCREF(arg);
  Py_XSETREF(g_sample_type, arg);
  Py_RETURN_NONE;
}

PyObject* py_counters(PyObject*, PyObject*) {
  return Py_BuildValue(
      "{s:K,s:K,s:K,s:K,s:n}", "handled", g_counters.handled,
      "deferred_parse", g_counters.deferred_parse, "deferred_eval",
      g_counters.deferred_eval, "compiles", g_counters.compiles, "cache_size",
      static_cast<Py_ssize_t>(g_cache.size()));
}

PyObject* py_reset(PyObject*, PyObject*) {
  g_cache.clear();
  g_fifo.clear();
  g_counters = Counters();
  Py_RETURN_NONE;
}

PyMethodDef kMethods[] = {
    {"evaluate", reinterpret_cast<PyCFunction>(
                     reinterpret_cast<void (*)()>(py_evaluate)),
     METH_FASTCALL,
     "evaluate(expr, samples) -> list of Sample, or DEFER"},
    {"bind", py_bind, METH_O, "bind(Sample): the class results are built of"},
    {"counters", py_counters, METH_NOARGS,
     "handled / deferred_parse / deferred_eval / compiles / cache_size"},
    {"reset", py_reset, METH_NOARGS, "drop cached plans, zero the counters"},
    {nullptr, nullptr, 0, nullptr},
};

PyModuleDef kModule = {
    PyModuleDef_HEAD_INIT, "_mi355x_promql",
    "Native PromQL evaluator with a plan cache (see promql.py).", -1, kMethods,
    nullptr, nullptr, nullptr, nullptr,
};

}  // namespace

PyMODINIT_FUNC PyInit__mi355x_promql(void) {
  PyObject* m = PyModule_Create(&kModule);
  if (!m) return nullptr;
  g_defer = PyObject_CallNoArgs(reinterpret_cast<PyObject*>(&PyBaseObject_Type));
  g_empty_str = PyUnicode_FromString("");
  g_dunder_name = PyUnicode_InternFromString("__name__");
  g_attr_name = PyUnicode_InternFromString("name");
  g_attr_labels = PyUnicode_InternFromString("labels");
  g_attr_value = PyUnicode_InternFromString("value");
  bool ok = g_defer && g_empty_str && g_dunder_name && g_attr_name &&
            g_attr_labels && g_attr_value;
#if PY_VERSION_HEX >= 0x030C0000
  if (ok) {
    PyObject* builtins = PyEval_GetBuiltins();   // borrowed
    g_builtin_sum = builtins ? PyDict_GetItemString(builtins, "sum") : nullptr;
    Py_XINCREF(g_builtin_sum);
    ok = g_builtin_sum != nullptr;
  }
#endif
  if (ok) {
    Py_INCREF(g_defer);
    ok = PyModule_AddObject(m, "DEFER", g_defer) == 0 &&
         PyModule_AddIntConstant(m, "CACHE_CAPACITY",
                                 static_cast<long>(kCacheCapacity)) == 0;
  }
  if (!ok) {
    Py_DECREF(m);
    return nullptr;
  }
  return m;
}
