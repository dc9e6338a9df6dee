"""GPU tests for the KV-cache decode attention kernel.

Inputs are rounded to bf16 before the call, so the kernel and the float64
reference (loadgen.attn_decode_ref) multiply the same numbers. In every
numerics test all positions >= seq_lens[b] of k and v are NaN: an output
that is not finite means a masked slot leaked. The one-hot and uniform
cases (tests/attn_cases.py) have closed forms, so a mismatch there is a
routing or masking bug, never rounding.
"""

import ctypes
import threading
import time

import numpy as np
import pytest

from attn_cases import D, HKV, nan_tail, onehot_case, uniform_case

pytestmark = pytest.mark.gpu


def _loadgen():
    from mi355x_gpu_hpa import loadgen

    assert loadgen.available(), (
        "libmi355x_loadgen.so missing on a GPU box — native path must load"
    )
    return loadgen


def _bf16(x):
    import torch

    return torch.from_numpy(x).bfloat16().float().numpy()


@pytest.mark.parametrize("group,seq_lens,lmax", [(8, [1, 37, 300], 320),
                                                 (1, [16, 17], 48),
                                                 (4, [33, 257], 257),
                                                 (16, [64], 64)])
def test_attn_onehot_routing(gpu, group, seq_lens, lmax):
    """Each head's probability mass sits on one position (every other
    weight is at most e^-45), so o is that position's V row: any wrong
    batch, head, position or d index shows in the V code."""
    lg = _loadgen()
    q, k, v, t = (onehot_case(group, seq_lens, lmax))
    q, k, v = _bf16(q), _bf16(k), _bf16(v)
    bi, hi = np.indices(t.shape)
    want = v[bi, hi // group, t]
    assert np.isfinite(want).all()
    for kv_splits in ([0, 2] if lmax >= 64 else [0]):
        o, lse = lg.attn_decode(q, k, v, seq_lens, kv_splits=kv_splits)
        print(f"kv_splits {kv_splits}: max |o - v[t]| "
              f"{np.abs(o - want).max():.3g}, max |lse - 1024/sqrt(128)| "
              f"{np.abs(lse - 1024 / np.sqrt(D)).max():.3g}")
        np.testing.assert_allclose(o, want, rtol=0, atol=1e-6)
        np.testing.assert_allclose(lse, 1024 / np.sqrt(D), rtol=0, atol=1e-4)


@pytest.fixture(scope="module")
def uniform():
    lg = _loadgen()
    seq_lens = [1, 37, 300]
    q, k, v = uniform_case(8, seq_lens, 320)
    q, k, v = _bf16(q), _bf16(k), _bf16(v)
    return seq_lens, q, k, v, lg.attn_decode_ref(q, k, v, seq_lens)


# 10 = ceil(320/32): one 32-position block per split. With 3 or 10 splits
# the sequences of length 1 and 37 leave splits empty (l = 0, m = -inf).
@pytest.mark.parametrize("kv_splits", [0, 1, 3, 10])
def test_attn_uniform_counts_every_position(gpu, uniform, kv_splits):
    """q = 0: every p is exactly 1 and the V sums are exact in f32
    (125 * 4096 < 2^24), so o is the mean of the first len rows up to a few
    f32 roundings. One dropped or double-counted position of the 300 moves
    every component by at least 5.7e-4."""
    lg = _loadgen()
    seq_lens, q, k, v, (o_ref, lse_ref) = uniform
    o, lse = lg.attn_decode(q, k, v, seq_lens, kv_splits=kv_splits)
    print(f"kv_splits {kv_splits}: max |o - ref| "
          f"{np.abs(o - o_ref).max():.3g}, max |lse - ref| "
          f"{np.abs(lse - lse_ref).max():.3g}")
    np.testing.assert_allclose(o, o_ref, rtol=4e-6, atol=1e-5)
    want_lse = np.repeat(np.log(seq_lens)[:, None], 8 * HKV, axis=1)
    np.testing.assert_allclose(lse, want_lse, rtol=0, atol=1e-5)


@pytest.fixture(scope="module")
def random_case():
    lg = _loadgen()
    seq_lens, lmax = [600, 257, 17], 600
    rng = np.random.default_rng(97)
    q = _bf16(4 * rng.standard_normal((3, 8 * HKV, D), dtype=np.float32))
    k = rng.standard_normal((3, HKV, lmax, D), dtype=np.float32)
    v = rng.uniform(-1, 1, (3, HKV, lmax, D)).astype(np.float32)
    k = nan_tail(_bf16(k), seq_lens)
    v = nan_tail(_bf16(v), seq_lens)
    return seq_lens, q, k, v, lg.attn_decode_ref(q, k, v, seq_lens)


@pytest.mark.parametrize("kv_splits", [0, 4])
def test_attn_random(gpu, random_case, kv_splits):
    """Peaked random softmax (q = 4 N(0,1), |o| averages about 0.26). P
    enters the second MFMA as bf16, relative error at most 2^-9 each, which
    bounds |do| by 2^-9 max|v|, twice that if l is summed from the rounded
    values too; the tolerance is four times the single bound. lse: the same
    derivation, ln(1 + 2^-9) with a factor 2. A second call returns the same
    bits (no atomics, fixed merge order)."""
    lg = _loadgen()
    seq_lens, q, k, v, (o_ref, lse_ref) = random_case
    o, lse = lg.attn_decode(q, k, v, seq_lens, kv_splits=kv_splits)
    print(f"kv_splits {kv_splits}: max |o - ref| "
          f"{np.abs(o - o_ref).max():.3g}, max |lse - ref| "
          f"{np.abs(lse - lse_ref).max():.3g}, mean |o| "
          f"{np.abs(o_ref).mean():.3g}")
    atol = 2.0 ** -7 * np.nanmax(np.abs(v))
    np.testing.assert_allclose(o, o_ref, rtol=0, atol=atol)
    np.testing.assert_allclose(lse, lse_ref, rtol=0, atol=2.0 ** -8)
    o2, lse2 = lg.attn_decode(q, k, v, seq_lens, kv_splits=kv_splits)
    np.testing.assert_array_equal(o2.view(np.uint32), o.view(np.uint32))
    np.testing.assert_array_equal(lse2.view(np.uint32), lse.view(np.uint32))


# lmax 40: ceil(40/32) = 2 splits at most
@pytest.mark.parametrize("hq,d,kv_splits,lens", [(8, 64, 0, [40, 40]),
                                                 (64, 128, 0, [40, 40]),
                                                 (8, 128, 3, [40, 40]),
                                                 (8, 128, 0, [40, 41]),
                                                 (8, 128, 0, [0, 40])],
                         ids=["d64", "g32", "splits_over", "len_over", "len0"])
def test_attn_dimension_errors(gpu, hq, d, kv_splits, lens):
    """The library entry itself rejects what the Python wrapper would have
    caught: -1 and a message, before any device call."""
    lg = _loadgen()
    lib = lg._load()
    batch, lmax = 2, 40
    q = np.ones((batch, hq, d), np.float32)
    k = np.ones((batch, HKV, lmax, d), np.float32)
    o = np.full((batch, hq, d), -7.0, np.float32)
    lse = np.full((batch, hq), -7.0, np.float32)
    rc = lib.lg_attn_decode_verify(0, q, k, k.copy(),
                                   np.array(lens, np.int32), o, lse, batch,
                                   hq, HKV, lmax, d, kv_splits, 0.0)
    assert rc == -1
    assert "attn decode" in lib.lg_last_error().decode()
    assert (o == -7.0).all() and (lse == -7.0).all()


# Measured on the MI355X, five triad/attention pairs in one process each:
# profiles/attn_decode.md. bar = min(0.5, 0.8 * lowest measured ratio).
STREAM_BAR = 0.5


def test_attn_streams_kv(gpu):
    """Fallback detector, not a perf test: the default 1 GiB cache must
    stream at no less than STREAM_BAR times the rate the project's own
    triad reaches in this process. A path that lost its memory-level
    parallelism or its vector loads lands near a tenth. A low reading is
    re-measured once after a settle."""
    lg = _loadgen()
    triad = lg.bw_burn(100.0, 1.0, gb=1.5)
    assert triad > 0
    ms, gbps = lg.attn_decode_bench()
    if gbps < STREAM_BAR * triad:
        time.sleep(2.0)
        ms, gbps = lg.attn_decode_bench()
    print(f"attention KV stream {gbps:.0f} GB/s ({ms:.3f} ms/step), "
          f"triad {triad:.0f} GB/s")
    assert ms > 0
    assert gbps >= STREAM_BAR * triad, (
        f"attention streams {gbps:.0f} GB/s against a {triad:.0f} GB/s triad")


def test_attn_burn(gpu):
    """The burn entry runs on the shared duty engine: 100 % for 2 s takes
    2..4 s, a stop flag raised after 0.5 s ends a 30 s burn within 2 s, and
    the reported KV rate is positive."""
    lg = _loadgen()
    assert lg.device_count() >= 1
    lib = lg._load()
    shape = dict(batch=8, hq=32, hkv=4, ctx=2048)

    def burn(seconds, stop):
        gbps = ctypes.c_double(0.0)
        rc = lib.lg_attn_decode_burn(
            0, ctypes.c_double(100.0), ctypes.c_double(seconds),
            shape["batch"], shape["hq"], shape["hkv"], shape["ctx"], D,
            ctypes.c_double(100.0), stop, ctypes.byref(gbps))
        return rc, gbps.value

    t0 = time.monotonic()
    gbps = lg.attn_burn(100.0, 2.0, **shape)
    wall = time.monotonic() - t0
    assert 2.0 <= wall <= 4.0, wall
    assert gbps > 0

    stop = ctypes.c_int(0)
    timer = threading.Timer(0.5, lambda: setattr(stop, "value", 1))
    t0 = time.monotonic()
    timer.start()
    try:
        rc, gbps = burn(30.0, ctypes.byref(stop))
    finally:
        timer.cancel()
    assert rc == 0
    assert time.monotonic() - t0 <= 2.0
    assert gbps > 0
