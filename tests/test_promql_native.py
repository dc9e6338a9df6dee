"""The native PromQL evaluator (native/control/promql_ext.cpp, behind
promql.evaluate) against its specification: promql._eval(promql.parse(expr),
samples). Every comparison takes the Python evaluator as the reference,
never the native path itself; "equal" means same length and order, equal
names and label dicts, and bit-identical values."""

import math
import random
import shutil
import struct
import subprocess
import sys
import sysconfig
from pathlib import Path

import pytest
import yaml

from mi355x_gpu_hpa.control import promql
from mi355x_gpu_hpa.control.loop import (
    REFERENCE_RULE_EXPR,
    ControlLoop,
    synth_pod_labels,
)
from mi355x_gpu_hpa.control.hpa import HpaSpec
from mi355x_gpu_hpa.control.promql import PromQLError, Sample

REPO = Path(__file__).resolve().parent.parent
NATIVE = REPO / "native"
NAN, INF = math.nan, math.inf


@pytest.fixture(scope="module", autouse=True)
def ext():
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    if not (Path(sysconfig.get_paths()["include"]) / "Python.h").is_file():
        pytest.skip("Python.h not available: promql-ext cannot be built")
    subprocess.run(["make", "-C", str(NATIVE), "promql-ext",
                    f"PYTHON={sys.executable}"],
                   check=True, capture_output=True)
    assert promql.native_available()
    assert promql.use_native(True)
    yield promql._load_ext()
    promql.use_native(None)


def test_make_target_skips_without_python_headers():
    """An interpreter make cannot ask for its headers: the target says that
    it skipped and succeeds."""
    p = subprocess.run(["make", "-C", str(NATIVE), "promql-ext",
                        "PYTHON=/nonexistent/python3"],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert "promql-ext: skipped" in p.stdout


# --- comparison -------------------------------------------------------------

def bits(v):
    assert type(v) is float
    return struct.pack("<d", v)


def key(vec):
    assert type(vec) is list
    return [(s.name, s.labels, bits(s.value)) for s in vec]


def reference(expr, samples):
    """What promql.evaluate computed before there was a native path."""
    res = promql._eval(promql.parse(expr), samples)
    if isinstance(res, float):
        return [Sample("", {}, res)]
    return res


def outcome(fn, *args):
    """("ok", comparable result) or ("raise", type, message)."""
    try:
        res = fn(*args)
    except Exception as e:  # noqa: BLE001 — the comparison is the point
        return ("raise", type(e), str(e))
    return ("ok", [(s.name, s.labels,
                    bits(s.value) if type(s.value) is float else s.value)
                   for s in res])


def assert_native_equals_reference(ext, expr, samples):
    want = reference(expr, samples)
    before = ext.counters()
    got = promql.evaluate(expr, samples)
    after = ext.counters()
    assert key(got) == key(want), expr
    assert after["handled"] == before["handled"] + 1, f"not native: {expr}"
    return want


# --- fixed corpus -----------------------------------------------------------

def device_samples(n):
    """The sample set of one control cycle at n devices (the bench's four
    families plus the kube_pod_labels join series)."""
    out = []
    for i in range(n):
        labels = {"gpu": str(i), "node": "node0", "pod": f"cuda-test-{i}",
                  "namespace": "default"}
        for fam, v in (("dcgm_gpu_utilization", 80.0 + 1.5 * i),
                       ("dcgm_gpu_temp", 55.0 + i),
                       ("amd_xgmi_total_bytes_per_second", 1e9 * i),
                       ("amd_exporter_samples_total", 100.0 + i),
                       ("amd_hbm_bandwidth_utilization", 33.3 * (i + 1)),
                       ("amd_xgmi_link_utilization", 7.0 / (i + 1))):
            out.append(Sample(fam, dict(labels), v))
    return out + synth_pod_labels([f"cuda-test-{i}" for i in range(n)])


def odd_samples():
    """Missing labels, empty label values, NaN, Inf, -0.0, cancellation."""
    return [
        Sample("m", {"g": "a", "pod": "p0"}, 1.0),
        Sample("m", {"g": "a", "pod": "p1"}, NAN),
        Sample("m", {"g": "", "pod": "p2"}, -0.0),
        Sample("m", {"pod": "p3"}, INF),
        Sample("m", {"g": "b", "pod": "p4", "__name__": "m"}, -INF),
        Sample("m", {"g": "b", "pod": "p5"}, 0.0),
        Sample("n", {"g": "a", "pod": "p0"}, NAN),
        Sample("n", {"g": "a", "pod": "p1"}, 2.0),
        Sample("n", {"g": "b", "pod": "p5", "extra": "café"}, 0.0),
        Sample("big", {"i": "0"}, 1e16),
        Sample("big", {"i": "1"}, 1.0),
        Sample("big", {"i": "2"}, -1e16),
        Sample("z", {"pod": "p0"}, -0.0),
        Sample("z", {"pod": "p1"}, 0.0),
        Sample("a", {}, 2.0), Sample("b", {}, 3.0), Sample("c", {}, 4.0),
        Sample("nanfirst", {"i": "0"}, NAN),
        Sample("nanfirst", {"i": "1"}, 5.0),
        Sample("nanlast", {"i": "0"}, 5.0),
        Sample("nanlast", {"i": "1"}, NAN),
    ]


def multi_metric_rules():
    doc = yaml.safe_load(
        (REPO / "deploy" / "multi-metric" /
         "gpu-metrics-prometheusrule.yaml").read_text())
    return [r["expr"] for g in doc["spec"]["groups"] for r in g["rules"]]


ADAPTER_QUERY = ('sum(cuda_test_gpu_avg{namespace="default",'
                 'deployment="cuda-test"}) by (deployment)')

ODD_CORPUS = [
    "m", "nothing", 'm{g="a"}', 'm{g!="a"}', 'm{g=""}', 'm{g!=""}',
    "m{missing=''}", 'm{missing!=""}', 'm{g="a", pod!="p1"}',
    "sum by(g) (m)", "sum(m) by (g)", "count by (g, missing) (m)",
    "max by(g) (m)", "min by(g) (m)", "avg by(g) (n)", "count(m)",
    "sum by () (m)", "sum(nothing)", "avg(nothing) by (g)",
    "avg(big)", "sum(big)", "avg by(i) (big)", "sum(big) / count(big)",
    "max(nanfirst)", "min(nanfirst)", "max(nanlast)", "min(nanlast)",
    "sum(z)", "avg(z)", "max(z)", "min(z)", "sum(m)", "avg(m)",
    "m * ignoring(g) n", "m * ignoring(g, extra) n",
    "m + ignoring(g, extra) group_left n",
    "m - on(pod) group_left() n", "m / on(pod) group_left(extra, g) n",
    "m * on(pod) n", "m * on(pod, g) n", "m * n", "a + b", "z * on(pod) z",
    "2 + 3 * 4", "1 / 0", "0 / 0", "1e3 - 0.5", "m * 100", "100 * m",
    "m / 0", "0 / m", "2 - z", "z - 2", "a + b * c", "(a + b) * c",
    "a - b / c", "a * 100 - b", "a / (b - b)", "sum(m) * 2",
    "sum by(g) (m) * on(g) sum by(g) (n)",
    "count(m) + count(n) * 2",
    'avg(max by(pod) (m) * on(pod) group_left(g) max by(pod, g) (n{g="a"}))',
]


def test_corpus_control_cycle(ext):
    rules = [REFERENCE_RULE_EXPR] + multi_metric_rules()
    assert len(rules) == 3
    for n in (1, 8):
        samples = device_samples(n)
        for expr in rules:
            want = assert_native_equals_reference(ext, expr, samples)
            assert len(want) == 1 and want[0].value > 0
        recorded = [Sample("cuda_test_gpu_avg",
                           {"namespace": "default", "deployment": "cuda-test"},
                           81.25)]
        want = assert_native_equals_reference(ext, ADAPTER_QUERY, recorded)
        assert key(want) == key([Sample("", {"deployment": "cuda-test"}, 81.25)])


@pytest.mark.parametrize("expr", ODD_CORPUS)
def test_corpus_odd_samples(ext, expr):
    assert_native_equals_reference(ext, expr, odd_samples())


def test_corpus_is_not_vacuous():
    s = odd_samples()
    assert reference("nothing", s) == [] and reference("sum(nothing)", s) == []
    assert reference("avg(big)", s)[0].value == sum([1e16, 1.0, -1e16]) / 3
    assert math.isnan(reference("max(nanfirst)", s)[0].value)
    assert reference("max(nanlast)", s)[0].value == 5.0
    assert math.isnan(reference("1 / 0", s)[0].value)
    assert bits(reference("sum(z)", s)[0].value) == bits(sum([-0.0, 0.0]))
    assert len(reference("m * ignoring(g, extra) n", s)) == 3
    assert reference("a + b * c", s)[0].value == 14.0
    assert len(reference("sum by(g) (m)", s)) == 3


def test_selector_passes_the_callers_objects_through(ext):
    s = odd_samples()
    got = promql.evaluate('n{g="a"}', s)
    want = reference('n{g="a"}', s)
    assert [id(x) for x in got] == [id(x) for x in want] == [id(s[6]), id(s[7])]
    # vector op scalar keeps the name and the very same labels dict
    got = promql.evaluate("a * 2", s)
    assert got[0].name == "a" and got[0].labels is s[14].labels


# --- defer set: same result or same error, native on and off -----------------

class SubSample(Sample):
    pass


class StrSub(str):
    pass


def plain():
    return [Sample("l", {"pod": "a", "gpu": "0"}, 2.0),
            Sample("l", {"pod": "a", "gpu": "1"}, 3.0),
            Sample("r", {"pod": "a"}, 10.0),
            Sample("r2", {"pod": "a", "k": "1"}, 10.0),
            Sample("r2", {"pod": "a", "k": "2"}, 20.0),
            Sample("m", {"a": "x", "q": 'x"y'}, 1.0),
            Sample("m", {"a": "y"}, 2.0),
            Sample("sum", {}, 7.0)]


DEFER_CASES = {
    "regex_match": ('m{a=~"x|y"}', plain),
    "regex_not_match": ('m{a!~"x"}', plain),
    "backslash_string": ('m{q="x\\"y"}', plain),
    "name_matcher": ('m{__name__="m"}', plain),
    "group_right": ("l * on(pod) group_right(k) r", plain),
    "lax_name_list": ("sum by(a q) (m)", plain),
    "trailing_comma_list": ("sum by(a,) (m)", plain),
    "lax_matcher_list": ('m{a="x" q!="z"}', plain),
    "function_name_as_metric": ("sum + 1", plain),
    "unicode_space": ("m * 2", plain),
    "malformed_open": ("avg(", plain),
    "malformed_matcher": ("m{a=}", plain),
    "malformed_trailing": ("m n", plain),
    "malformed_token": ("m $ 2", plain),
    "malformed_negative": ("-1", plain),
    "malformed_unterminated": ('m{a="x}', plain),
    "malformed_empty": ("", plain),
    "many_to_many": ("l * on(pod) r2", plain),
    "many_to_one_without_group_left": ("l * on(pod) r", plain),
    "aggregation_over_scalar": ("sum(1 + 2)", plain),
    "int_valued_sample": ("sum(m) * 2", lambda: plain() + [Sample("m", {}, 3)]),
    "int_valued_sample_elsewhere": (
        "max(l)", lambda: plain() + [Sample("other", {}, 3)]),
    "sample_subclass": (
        "sum by(a) (m)", lambda: plain() + [SubSample("m", {"a": "x"}, 4.0)]),
    "labels_not_a_dict": (
        "l + 1", lambda: plain() + [Sample("m", [("a", "x")], 4.0)]),
    "labels_dict_of_non_str": (
        "sum by(a) (m)", lambda: plain() + [Sample("m", {"a": 5}, 4.0)]),
    "str_subclass_label": (
        "sum by(a) (m)", lambda: plain() + [Sample("m", {"a": StrSub("x")}, 4.0)]),
    "name_not_a_str": ("m", lambda: plain() + [Sample(None, {}, 4.0)]),
    "not_a_sample": ("m", lambda: plain() + [object()]),
    "samples_as_tuple": ("max(l) + 1", lambda: tuple(plain())),
}


@pytest.mark.parametrize("name", sorted(DEFER_CASES))
def test_defer_set(ext, name):
    expr, make = DEFER_CASES[name]
    want = outcome(reference, expr, make())
    before = ext.counters()
    assert promql.use_native(True)
    on = outcome(promql.evaluate, expr, make())
    after = ext.counters()
    assert not promql.use_native(False)
    try:
        off = outcome(promql.evaluate, expr, make())
    finally:
        assert promql.use_native(True)
    assert on == off == want
    assert after["handled"] == before["handled"]
    assert (after["deferred_parse"] + after["deferred_eval"]
            == before["deferred_parse"] + before["deferred_eval"] + 1)


def test_defer_set_is_not_vacuous():
    kinds = {n: outcome(reference, e, m())[0]
             for n, (e, m) in DEFER_CASES.items()}
    assert kinds["regex_match"] == kinds["backslash_string"] == "ok"
    assert kinds["int_valued_sample"] == kinds["sample_subclass"] == "ok"
    assert kinds["many_to_many"] == kinds["group_right"] == "raise"
    assert kinds["aggregation_over_scalar"] == kinds["malformed_open"] == "raise"
    assert outcome(reference, *[DEFER_CASES["many_to_many"][0], plain()])[1] \
        is PromQLError


def test_environment_switch(ext, monkeypatch):
    for v in ("0", "false", "off", "no", " OFF "):
        monkeypatch.setenv(promql.NATIVE_ENV, v)
        assert not promql.use_native(None) and not promql.native_active()
        before = ext.counters()
        assert promql.evaluate("2 + 3", [])[0].value == 5.0
        assert ext.counters() == before
    monkeypatch.setenv(promql.NATIVE_ENV, "1")
    assert promql.use_native(None) and promql.native_active()
    monkeypatch.delenv(promql.NATIVE_ENV)
    assert promql.use_native(None)


# --- seeded random differential ---------------------------------------------

METRICS = ["m0", "m1", "m2"]
LABELS = ["a", "b", "pod", "__name__"]
LABEL_VALUES = ["", "x", "y", "z"]
VALUES = [0.0, -0.0, 1.0, 2.5, -3.0, 1e16, -1e16, 1.0, NAN, INF, -INF, 1e-300,
          1e300]
FUNCS = ["sum", "avg", "max", "min", "count"]
NUMBERS = ["0", "1", "2", "0.5", "100", "1e3", "2.5e-1", "3E+2", "007", "1e16"]


class Gen:
    """Expression trees from the native subset, and sample sets."""

    def __init__(self, seed):
        self.r = random.Random(seed)

    def names(self):
        r = self.r
        ns = [r.choice(LABELS) for _ in range(r.choice([0, 1, 1, 2, 3]))]
        sep = r.choice([",", ", ", " , "])
        return "(" + sep.join(ns) + ")"

    def selector(self):
        r = self.r
        s = r.choice(METRICS + ["nothing"])
        if r.random() < 0.4:
            q = r.choice(['"', "'"])
            ms = [f"{r.choice(LABELS[:3] + ['missing'])}{r.choice(['=', '!='])}"
                  f"{q}{r.choice(LABEL_VALUES)}{q}"
                  for _ in range(r.choice([0, 1, 1, 2]))]
            s += "{" + r.choice([",", ", "]).join(ms) + "}"
        return s

    def vector(self, depth):
        r = self.r
        k = r.random()
        if depth <= 0 or k < 0.25:
            return self.selector()
        if k < 0.55:
            f = r.choice(FUNCS)
            inner = self.vector(depth - 1)
            where = r.choice(["none", "prefix", "suffix"])
            if where == "prefix":
                return f"{f} by{self.names()} ({inner})"
            if where == "suffix":
                return f"{f}({inner}) by {self.names()}"
            return f"{f}({inner})"
        if k < 0.7:
            return f"({self.vector(depth - 1)})"
        return self.binary(depth)

    def binary(self, depth):
        r = self.r
        op = r.choice("*/+-")
        shape = r.random()
        if shape < 0.2:
            return f"{self.vector(depth - 1)} {op} {self.scalar(depth - 1)}"
        if shape < 0.35:
            return f"{self.scalar(depth - 1)} {op} {self.vector(depth - 1)}"
        mod = ""
        k = r.random()
        if k < 0.4:
            mod += f" on{self.names()}"
        elif k < 0.6:
            mod += f" ignoring{self.names()}"
        k = r.random()
        if k < 0.3:
            mod += " group_left"
        elif k < 0.5:
            mod += f" group_left{self.names()}"
        return f"{self.vector(depth - 1)} {op}{mod} {self.vector(depth - 1)}"

    def scalar(self, depth):
        r = self.r
        if depth <= 0 or r.random() < 0.7:
            return r.choice(NUMBERS)
        return (f"({self.scalar(depth - 1)} {r.choice('*/+-')} "
                f"{self.scalar(depth - 1)})")

    def expr(self):
        if self.r.random() < 0.08:
            return self.scalar(2)
        return self.vector(self.r.choice([1, 2, 2, 3]))

    def samples(self):
        r = self.r
        out = []
        for _ in range(r.choice([0, 1, 2, 3, 4, 6, 9])):
            labels = {}
            for name in r.sample(LABELS, r.choice([0, 1, 2, 2, 3])):
                labels[name] = r.choice(LABEL_VALUES)
            v = r.choice(VALUES) if r.random() < 0.7 else r.uniform(-1e3, 1e3)
            out.append(Sample(r.choice(METRICS), labels, v))
        return out


def test_random_differential(ext):
    """The first 1000 generated cases on which the reference returns: equal
    results, all handled natively. The reference alone decides membership."""
    gen = Gen(20241021)
    kept = tried = nonempty = 0
    ext.reset()
    while kept < 1000:
        tried += 1
        assert tried < 20000
        expr, samples = gen.expr(), gen.samples()
        try:
            want = reference(expr, samples)
        except PromQLError:
            continue
        kept += 1
        nonempty += bool(want)
        got = promql.evaluate(expr, samples)
        assert key(got) == key(want), (expr, samples)
    c = ext.counters()
    assert c["handled"] == 1000
    assert c["deferred_parse"] == 0 and c["deferred_eval"] == 0
    assert nonempty > 300      # the set is not mostly empty vectors


# --- cache ------------------------------------------------------------------

def test_repeated_expression_compiles_once(ext):
    ext.reset()
    samples = device_samples(1)
    for _ in range(50):
        promql.evaluate(REFERENCE_RULE_EXPR, samples)
        # a new str object with the same content every time, as the adapter
        # builds its query
        promql.evaluate("".join(["sum(dcgm_gpu_temp)", " by (gpu)"]), samples)
    c = ext.counters()
    assert c["compiles"] == 2 and c["cache_size"] == 2 and c["handled"] == 100


def test_cache_stays_within_capacity(ext):
    ext.reset()
    cap = ext.CACHE_CAPACITY
    assert 0 < cap <= 4096
    samples = odd_samples()
    for i in range(10 * cap):
        expr = f"sum by(g) (m) * {i} + {i % 7}"
        assert key(promql.evaluate(expr, samples)) == key(reference(expr, samples))
        assert ext.counters()["cache_size"] <= cap
    c = ext.counters()
    assert c["cache_size"] == cap and c["compiles"] == 10 * cap
    assert c["handled"] == 10 * cap
    # an evicted expression is compiled again and still right
    assert_native_equals_reference(ext, "sum by(g) (m) * 0 + 0", samples)
    assert ext.counters()["compiles"] == 10 * cap + 1


def test_deferring_expression_is_parsed_natively_once(ext):
    ext.reset()
    samples = plain()
    for expr in ('m{a=~"x|y"}', "m $ 2"):
        first = outcome(promql.evaluate, expr, samples)
        n = ext.counters()["compiles"]
        assert outcome(promql.evaluate, expr, samples) == first
        assert ext.counters()["compiles"] == n
    c = ext.counters()
    assert c["compiles"] == 2 and c["deferred_parse"] == 4 and c["handled"] == 0


def test_extension_never_raises_for_odd_arguments(ext):
    for args in ((1, []), ("m", None), (b"m", []), ("m\ud800", [])):
        assert ext.evaluate(*args) is ext.DEFER


# --- reference counts ---------------------------------------------------------

def test_reference_counts_are_unchanged(ext):
    samples = device_samples(2)
    s = samples[0]
    label_value = s.labels["pod"]
    exprs = [REFERENCE_RULE_EXPR, "dcgm_gpu_utilization",
             "dcgm_gpu_utilization * 2", "sum by(pod) (dcgm_gpu_temp)",
             "dcgm_gpu_temp * ignoring(x) dcgm_gpu_temp",
             "sum(1 + 2)", "dcgm_gpu_temp * on(node) dcgm_gpu_temp"]
    promql.use_native(False)
    want = [outcome(promql.evaluate, e, samples) for e in exprs]
    promql.use_native(True)
    assert [outcome(promql.evaluate, e, samples) for e in exprs] == want
    before = (sys.getrefcount(s), sys.getrefcount(s.labels),
              sys.getrefcount(label_value), sys.getrefcount(samples))
    handled = ext.counters()["handled"]
    for _ in range(2000):
        for e in exprs:
            try:
                promql.evaluate(e, samples)
            except PromQLError:
                pass
    after = (sys.getrefcount(s), sys.getrefcount(s.labels),
             sys.getrefcount(label_value), sys.getrefcount(samples))
    assert after == before
    assert ext.counters()["handled"] == handled + 2000 * 5


# --- loop level ---------------------------------------------------------------

class FixedScraper:
    def __init__(self, samples):
        self.samples = samples

    def scrape_once(self):
        return [Sample(s.name, dict(s.labels), s.value) for s in self.samples]


def run_loop(n, native):
    assert promql.use_native(native) == native
    try:
        pods = [f"cuda-test-{i}" for i in range(n)]
        base = [s for s in device_samples(n) if s.name != "kube_pod_labels"]
        loop = ControlLoop(
            FixedScraper(base),
            hpa_spec=HpaSpec(min_replicas=1, max_replicas=8, target_value=5.0),
            extra_samples=lambda: synth_pod_labels(pods),
            use_adapter=True)
        out = []
        for step in range(3):
            r = loop.step(now_s=1000.0 + 15.0 * step)
            out.append((r.recorded, key(loop.recorded_series),
                        r.metric_value, r.replicas))
        return out
    finally:
        promql.use_native(True)


@pytest.mark.parametrize("n", [1, 8])
def test_control_loop_same_with_native_on_and_off(ext, n):
    before = ext.counters()["handled"]
    on = run_loop(n, True)
    assert ext.counters()["handled"] == before + 6    # rule + adapter, 3 steps
    off = run_loop(n, False)
    assert ext.counters()["handled"] == before + 6
    assert on == off
    assert on[-1][3] == 8 and on[-1][2] == on[-1][0]["cuda_test_gpu_avg"] >= 80


# --- sanitizer self-test of the parser ---------------------------------------

def test_selftest_binary():
    """The ASan+UBSan program over the pure-C++ parser and plan: exit 0,
    nothing on stderr."""
    subprocess.run(["make", "-C", str(NATIVE), "promql-selftest"],
                   check=True, capture_output=True)
    p = subprocess.run([str(NATIVE / "build" / "promql-selftest")],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert p.stderr == ""
