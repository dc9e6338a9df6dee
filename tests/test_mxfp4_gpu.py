"""GPU tests for the MXFP4 (E2M1 + E8M0 block scale) MFMA GEMM.

The reference is always a numpy float64 matmul over the DEQUANTIZED
operands the library returns (aq @ btq.T) — what the matrix core must have
multiplied. The exact-data tests use inputs the quantizer represents
without error and whose partial sums are exact in f32 in any order, so a
mismatch there is an operand-layout or scale-routing bug, never rounding.
"""

import ctypes
import threading
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

E2M1 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], np.float32)


def _loadgen():
    from mi355x_gpu_hpa import loadgen

    assert loadgen.available(), (
        "libmi355x_loadgen.so missing on a GPU box — native path must load"
    )
    return loadgen


def _exact_operand(rng, rows, k):
    """Random E2M1 values times 2^s, s in {-1, 0, 1} per (row, 32-block);
    the first element of each block is +-6 * 2^s so the quantizer must pick
    e = s and represents every element exactly."""
    nb = k // 32
    val = E2M1[rng.integers(0, 8, (rows, nb, 32))]
    val *= rng.choice(np.float32([-1, 1]), (rows, nb, 32))
    val[:, :, 0] = 6 * rng.choice(np.float32([-1, 1]), (rows, nb))
    s = rng.integers(-1, 2, (rows, nb, 1))
    return (val * np.exp2(s)).astype(np.float32).reshape(rows, k)


def _ref(aq, btq):
    return aq.astype(np.float64) @ btq.astype(np.float64).T


def _check_exact(m, n, k, seed, max_ctas=0):
    lg = _loadgen()
    rng = np.random.default_rng(seed)
    a = _exact_operand(rng, m, k)
    bt = _exact_operand(rng, n, k)
    c, aq, btq = lg.gemm_mxfp4(a, bt, max_ctas=max_ctas)
    np.testing.assert_array_equal(aq, a)
    np.testing.assert_array_equal(btq, bt)
    # products are multiples of 2^-4 and the absolute row sums stay far
    # below 2^20, so every f32 summation order is exact
    assert (np.abs(a).astype(np.float64) @ np.abs(bt).astype(np.float64).T
            ).max() < 2 ** 20
    np.testing.assert_array_equal(c.astype(np.float64), _ref(aq, btq))


# (256,256,256): one K-tile, the tail-clamp path; (256,256,512): both LDS
# buffers; (512,256,768): odd K-tile count and M != N tile counts (a tm/tn
# swap shows); (1024,1024,1024): 16 tiles, the 4x4 super-tile raster.
@pytest.mark.parametrize("m,n,k", [(256, 256, 256), (256, 256, 512),
                                   (512, 256, 768), (1024, 1024, 1024)])
def test_gemm_mxfp4_exact(gpu, m, n, k):
    _check_exact(m, n, k, seed=41)


def test_gemm_mxfp4_scale_routing(gpu):
    """Every element of a block equals 2^s(row, block): all element codes
    are identical, so only the scale bytes steer the result, which is
    sum_b 32 * 2^(sa[i,b] + sb[j,b]) exactly. Separates a scale
    permutation from an element permutation."""
    lg = _loadgen()
    m, n, k = 256, 256, 512
    rng = np.random.default_rng(42)
    sa = rng.integers(-2, 3, (m, k // 32))
    sb = rng.integers(-2, 3, (n, k // 32))
    a = np.repeat(np.exp2(sa), 32, axis=1).astype(np.float32)
    bt = np.repeat(np.exp2(sb), 32, axis=1).astype(np.float32)
    c, aq, btq = lg.gemm_mxfp4(a, bt)
    np.testing.assert_array_equal(aq, a)
    np.testing.assert_array_equal(btq, bt)
    want = 32.0 * (np.exp2(sa) @ np.exp2(sb).T)
    np.testing.assert_array_equal(want, _ref(aq, btq))
    np.testing.assert_array_equal(c.astype(np.float64), want)


@pytest.mark.parametrize("m,n,k", [(256, 256, 256), (512, 512, 1024)])
def test_gemm_mxfp4_random(gpu, m, n, k):
    """Random data with per-block magnitudes 2^-3..2^3 and asymmetric
    column-0 ramps. Products are exact in f32; only the K-long f32
    accumulation rounds, so the band is the fp8 test's, scaled by the
    operand magnitude. A one-element K rotation of B gives errors a
    thousand times the atol, so the band cannot hide a layout fault."""
    lg = _loadgen()
    rng = np.random.default_rng(88)
    a = rng.uniform(-1, 1, (m, k)).astype(np.float32)
    bt = rng.uniform(-1, 1, (n, k)).astype(np.float32)
    a *= np.repeat(np.exp2(rng.integers(-3, 4, (m, k // 32))), 32, axis=1)
    bt *= np.repeat(np.exp2(rng.integers(-3, 4, (n, k // 32))), 32, axis=1)
    a[:, 0] += np.arange(m) * 0.01
    bt[:, 0] -= np.arange(n) * 0.01
    a = a.astype(np.float32)
    bt = bt.astype(np.float32)
    c, aq, btq = lg.gemm_mxfp4(a, bt)
    # the GPU path quantizes exactly like the public host quantizer
    np.testing.assert_array_equal(aq, lg.mxfp4_quantize(a)[2])
    np.testing.assert_array_equal(btq, lg.mxfp4_quantize(bt)[2])
    atol = 2e-3 * np.sqrt(k) * np.abs(aq).max() * np.abs(btq).max()
    np.testing.assert_allclose(c, _ref(aq, btq), rtol=2e-3, atol=atol)


@pytest.mark.parametrize("max_ctas", [3, 16])
def test_gemm_mxfp4_multi_tile_ctas(gpu, max_ctas):
    """16 tiles over 3 CTAs (6 per CTA, uneven remainder and early exit)
    and over 16 CTAs, bit-equal to the reference."""
    _check_exact(1024, 1024, 512, seed=43, max_ctas=max_ctas)


@pytest.mark.parametrize("m,n,k", [(256, 256, 128), (128, 256, 256)])
def test_gemm_mxfp4_dimension_errors(gpu, m, n, k):
    lg = _loadgen()
    with pytest.raises(lg.LoadgenError):
        lg.gemm_mxfp4(np.ones((m, k), np.float32), np.ones((n, k), np.float32))


def _floor_check(bench_fn, floor_tf, what):
    """Fallback detector, not a perf test: an implausibly low reading is
    re-measured once after a settle."""
    ms, tf = bench_fn()
    if tf <= floor_tf:
        time.sleep(2.0)
        ms, tf = bench_fn()
    assert ms > 0
    assert tf > floor_tf, f"{what} at {tf:.0f} TF/s — MFMA path not engaged?"


def test_gemm_mxfp4_bench_sane(gpu):
    """The project's fp8 floor: a non-MFMA path cannot reach 200 TF/s."""
    lg = _loadgen()
    _floor_check(lambda: lg.gemm_mxfp4_bench(m=2048, n=2048, k=2048, warmup=2,
                                             iters=10), 200, "mxfp4 GEMM")


def test_gemm_mxfp4_burn(gpu):
    """The burn entry runs on the shared duty engine: 100 % for 2 s takes
    2..4 s, and a stop flag raised after 0.5 s ends it within 2 s."""
    lg = _loadgen()
    assert lg.device_count() >= 1
    lib = lg._load()

    def burn(seconds, stop):
        return lib.lg_gemm_mxfp4_burn(
            0, ctypes.c_double(100.0), ctypes.c_double(seconds),
            2048, 2048, 2048, ctypes.c_double(100.0), stop)

    t0 = time.monotonic()
    assert burn(2.0, None) == 0
    wall = time.monotonic() - t0
    assert 2.0 <= wall <= 4.0, wall

    stop = ctypes.c_int(0)
    timer = threading.Timer(0.5, lambda: setattr(stop, "value", 1))
    t0 = time.monotonic()
    timer.start()
    try:
        assert burn(30.0, ctypes.byref(stop)) == 0
    finally:
        timer.cancel()
    assert time.monotonic() - t0 <= 2.0
