"""GPU tests for the decode-phase MXFP4 weight-streaming GEMM.

c[layer] = dq(x)[m, k] @ dq(w[layer])[n, k].T with 1 <= m <= 64 over a ring
of weight matrices. The reference is always a numpy float64 matmul over the
DEQUANTIZED operands the library returns. The exact-data tests use inputs
the quantizer represents without error and whose partial sums are exact in
f32 in any order, so every wave split, K slice combine and layer stride is
checked bit for bit; a mismatch there is a layout or routing bug, never
rounding.
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


def _ref(xq, wq):
    """float64 reference; wq [n, k] or [layers, n, k]."""
    return xq.astype(np.float64) @ np.swapaxes(wq.astype(np.float64), -1, -2)


def _check_exact(m, n, k, seed, k_splits=0, layers=None):
    lg = _loadgen()
    rng = np.random.default_rng(seed)
    x = _exact_operand(rng, m, k)
    if layers is None:
        w = _exact_operand(rng, n, k)
    else:
        w = np.stack([_exact_operand(rng, n, k) for _ in range(layers)])
    c, xq, wq = lg.decode_mxfp4(x, w, k_splits=k_splits)
    assert c.shape == w.shape[:-2] + (m, n)
    np.testing.assert_array_equal(xq, x)
    np.testing.assert_array_equal(wq, w)
    # |value| <= 12, so a product is at most 144 and a multiple of 2^-4;
    # the absolute row sums stay below 144 * 1024 < 2^20, so every f32
    # summation order and every split combine is exact
    assert k <= 1024
    bound = _ref(np.abs(x), np.abs(w)).max()
    assert bound <= 144 * 1024 < 2 ** 20
    np.testing.assert_array_equal(c.astype(np.float64), _ref(xq, wq))


# (1,64,128): one valid row of a padded fragment, a single k-step (three of
# the four waves idle); (16,64,256); (17,128,384): padding across a fragment
# boundary, an odd k-step count, two 64-row N groups; (64,256,1024): every M
# fragment, M != N (an M/N swap shows).
@pytest.mark.parametrize("m,n,k", [(1, 64, 128), (16, 64, 256),
                                   (17, 128, 384), (64, 256, 1024)])
def test_decode_mxfp4_exact(gpu, m, n, k):
    _check_exact(m, n, k, seed=51)


def test_decode_mxfp4_scale_routing(gpu):
    """Every element of a block equals 2^s(row, block): all element codes
    are identical, so only the scale bytes steer the result, which is
    32 * (2^sx @ 2^sw.T) exactly. Separates a scale permutation from an
    element permutation, for X and W independently (their exponents are
    drawn independently)."""
    lg = _loadgen()
    m, n, k = 16, 64, 512
    rng = np.random.default_rng(52)
    sx = rng.integers(-2, 3, (m, k // 32))
    sw = rng.integers(-2, 3, (n, k // 32))
    x = np.repeat(np.exp2(sx), 32, axis=1).astype(np.float32)
    w = np.repeat(np.exp2(sw), 32, axis=1).astype(np.float32)
    c, xq, wq = lg.decode_mxfp4(x, w)
    np.testing.assert_array_equal(xq, x)
    np.testing.assert_array_equal(wq, w)
    want = 32.0 * (np.exp2(sx) @ np.exp2(sw).T)
    np.testing.assert_array_equal(want, _ref(xq, wq))
    np.testing.assert_array_equal(c.astype(np.float64), want)


# k_splits > 1 goes through the partial-C workspace and the ordered slice
# sum; 8 slices of 8 k-steps leave one step per slice (three waves idle);
# 3 slices of 6 steps leave two steps for four waves.
@pytest.mark.parametrize("m,n,k,k_splits", [(16, 64, 1024, 1),
                                            (16, 64, 1024, 2),
                                            (16, 64, 1024, 8),
                                            (3, 128, 768, 3),
                                            (16, 64, 1024, 0),
                                            (3, 128, 768, 0)])
def test_decode_mxfp4_forced_splits(gpu, m, n, k, k_splits):
    _check_exact(m, n, k, seed=53, k_splits=k_splits)


def test_decode_mxfp4_layer_ring(gpu):
    """Three different layers: each output layer is bit-equal to its own
    reference (an element or scale stride error between layers shows)."""
    _check_exact(5, 128, 256, seed=54, layers=3)


@pytest.mark.parametrize("m,n,k", [(16, 256, 1024), (48, 128, 512)])
def test_decode_mxfp4_random(gpu, m, n, k):
    """Random data with per-block magnitudes 2^-3..2^3 and asymmetric
    column-0 ramps, within the project's MXFP4 band; a second call returns
    the same bits (no atomics, fixed combine order)."""
    lg = _loadgen()
    rng = np.random.default_rng(89)
    x = rng.uniform(-1, 1, (m, k)).astype(np.float32)
    w = rng.uniform(-1, 1, (n, k)).astype(np.float32)
    x *= np.repeat(np.exp2(rng.integers(-3, 4, (m, k // 32))), 32, axis=1)
    w *= np.repeat(np.exp2(rng.integers(-3, 4, (n, k // 32))), 32, axis=1)
    x[:, 0] += np.arange(m) * 0.01
    w[:, 0] -= np.arange(n) * 0.01
    x = x.astype(np.float32)
    w = w.astype(np.float32)
    c, xq, wq = lg.decode_mxfp4(x, w)
    np.testing.assert_array_equal(xq, lg.mxfp4_quantize(x)[2])
    np.testing.assert_array_equal(wq, lg.mxfp4_quantize(w)[2])
    atol = 2e-3 * np.sqrt(k) * np.abs(xq).max() * np.abs(wq).max()
    np.testing.assert_allclose(c, _ref(xq, wq), rtol=2e-3, atol=atol)
    c2, _, _ = lg.decode_mxfp4(x, w)
    np.testing.assert_array_equal(c2, c)


@pytest.mark.parametrize("m,n,k,k_splits", [(0, 64, 128, 0), (65, 64, 128, 0),
                                            (16, 32, 128, 0), (16, 64, 64, 0),
                                            (16, 64, 384, 2)])
def test_decode_mxfp4_dimension_errors(gpu, m, n, k, k_splits):
    lg = _loadgen()
    with pytest.raises(lg.LoadgenError):
        lg.decode_mxfp4(np.ones((m, k), np.float32),
                        np.ones((n, k), np.float32), k_splits=k_splits)


def test_decode_mxfp4_streams_weights(gpu):
    """Fallback detector, not a perf test: the default 544 MiB ring must
    stream at no less than half the rate the project's own triad reaches
    in this process. The decode step also pays MFMA issue, the combine and
    a kernel boundary per step; a path that lost its memory-level
    parallelism or its vector loads lands near a tenth. A low reading is
    re-measured once after a settle."""
    lg = _loadgen()
    triad = lg.bw_burn(100.0, 1.0, gb=1.5)
    assert triad > 0

    def bench():
        return lg.decode_mxfp4_bench(m=16, n=8192, k=8192, layers=16,
                                     warmup=2, iters=10)

    ms, gbps = bench()
    if gbps < 0.5 * triad:
        time.sleep(2.0)
        ms, gbps = bench()
    print(f"decode weight stream {gbps:.0f} GB/s ({ms:.3f} ms/step), "
          f"triad {triad:.0f} GB/s")
    assert ms > 0
    assert gbps >= 0.5 * triad, (
        f"decode streams {gbps:.0f} GB/s against a {triad:.0f} GB/s triad")


def test_decode_mxfp4_burn(gpu):
    """The burn entry runs on the shared duty engine: 100 % for 2 s takes
    2..4 s, a stop flag raised after 0.5 s ends a 30 s burn within 2 s, and
    the reported weight rate is positive."""
    lg = _loadgen()
    assert lg.device_count() >= 1
    lib = lg._load()

    def burn(seconds, stop):
        gbps = ctypes.c_double(0.0)
        rc = lib.lg_decode_mxfp4_burn(
            0, ctypes.c_double(100.0), ctypes.c_double(seconds),
            16, 4096, 4096, 4, ctypes.c_double(100.0), stop,
            ctypes.byref(gbps))
        return rc, gbps.value

    t0 = time.monotonic()
    gbps = lg.decode_burn(100.0, 2.0, batch=16, n=4096, k=4096, layers=4)
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
