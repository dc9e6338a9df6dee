"""bench.py --full on a real GPU: the secondary measurements that a plain
run skips (test_bench_cpu.py) are taken and land in the record."""

import pytest

from test_bench_cpu import _last_json_line, _run, check_contract

pytestmark = pytest.mark.gpu


def test_bench_full_fills_secondary_measurements(gpu):
    import sys

    p = _run([sys.executable, "bench.py", "--gpus", "1", "--steps", "10",
              "--warmup", "5", "--full"], timeout=120)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    r = _last_json_line(p.stdout)
    check_contract(r, 1)
    cfg = r["config"]
    # util error vs rocm-smi: a percentage-point difference of two busy%
    # readings, one entry per exported GPU
    assert cfg["gpus_exported"] >= 1
    assert 0 <= cfg["util_err_vs_rocm_smi_pct"] <= 100
    assert "0" in cfg["util_err_per_gpu_pct"]
    # load-step detection ran inside its 15 s budget
    assert 0 < cfg["load_step_detection_s"] <= 15.0
