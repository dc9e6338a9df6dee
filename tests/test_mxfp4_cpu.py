"""CPU tests for the MXFP4 (E2M1 + E8M0 block scale) host quantizer.

The quantizer lives in native/loadgen/mxfp4_host.h and is reached from
Python through the host-only libmi355x_mxfp4.so (no HIP, no GPU). It is
checked bit-for-bit against an independent numpy implementation of the
OCP MX v1.0 rule written here: e = floor(log2(amax)) - 2 clamped to
[-127, 127], elements rounded to the nearest E2M1 value with ties to the
even code, saturating at +-6.
"""

import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent
NATIVE = REPO / "native"

MAGS = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
TIES = np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0])


@pytest.fixture(scope="module")
def lg():
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    subprocess.run(
        ["make", "-C", str(NATIVE), "mxfp4-host", "mxfp4-selftest"],
        check=True, capture_output=True,
    )
    from mi355x_gpu_hpa import loadgen

    return loadgen


def ref_quantize(x):
    """Independent numpy MXFP4 quantizer: (packed, scales, deq)."""
    r, k = x.shape
    xb = x.astype(np.float64).reshape(r, k // 32, 32)
    amax = np.abs(xb).max(axis=2)
    _, ex = np.frexp(amax)  # amax = m * 2^ex, m in [0.5, 1)
    e = np.clip(ex - 1 - 2, -127, 127)
    e = np.where(amax == 0, 0, e).astype(np.int64)
    v = np.ldexp(xb, -e[:, :, None])  # exact in float64
    # nearest magnitude; on a tie the even code
    dist = np.abs(np.abs(v)[..., None] - MAGS)
    best = dist.min(axis=-1, keepdims=True)
    cand = dist == best
    even = cand & (np.arange(8) % 2 == 0)
    code = np.where(even.any(axis=-1), even.argmax(axis=-1),
                    cand.argmax(axis=-1))
    neg = (v < 0) & (code != 0)
    deq = np.ldexp(np.where(neg, -MAGS[code], MAGS[code]), e[:, :, None])
    code = (code | (neg << 3)).astype(np.uint8).reshape(r, k)
    packed = code[:, 0::2] | (code[:, 1::2] << 4)
    scales = (e + 127).astype(np.uint8)
    return packed, scales, deq.reshape(r, k).astype(np.float32)


def _edge_data():
    """Random blocks across the whole f32 range, zero blocks, and every tie
    point times a power-of-two scale, both signs. 2^-140 reaches the lower
    scale clamp; the upper one (e = 127) cannot be reached from finite f32
    (amax < 2^128 gives e <= 125), so the top of the range is the largest
    finite values."""
    rng = np.random.default_rng(4)
    rows, k = 24, 32 * 9  # 288 columns: a multiple of 32 only
    exps = rng.integers(-140, 129, size=(rows, k // 32))
    x = rng.uniform(-1, 1, (rows, k // 32, 32)) * np.exp2(exps)[:, :, None]
    x = np.clip(x, -np.finfo(np.float32).max, np.finfo(np.float32).max)
    x[3, 2] = 0.0
    x[7] = 0.0
    x[8, 0, :] = np.where(np.arange(32) % 2, -0.0, 0.0)
    x[9, 4, 0] = np.finfo(np.float32).max
    x[10, 1, :] = 2.0 ** -149
    for i, s in enumerate([-126, -20, -1, 0, 3, 60, 120]):
        blk = np.zeros(32)
        blk[0] = 6.0  # pins the block exponent to s
        blk[1:8] = TIES
        blk[8:15] = -TIES
        blk[15:22] = np.nextafter(TIES, 10.0)
        blk[22:29] = -np.nextafter(TIES, 0.0)
        blk[29:32] = [7.9, -6.5, 5.5]  # the saturating band (6, 8)
        x[11 + i, i] = blk * 2.0 ** s
    return x.reshape(rows, k).astype(np.float32)


def test_quantizer_matches_numpy_bitwise(lg):
    x = _edge_data()
    assert np.isfinite(x).all()
    packed, scales, deq = lg.mxfp4_quantize(x)
    rp, rs, rd = ref_quantize(x)
    assert scales.min() == 0 and scales.max() == 252  # low clamp, f32 top
    np.testing.assert_array_equal(scales, rs)
    np.testing.assert_array_equal(packed, rp)
    np.testing.assert_array_equal(deq.view(np.uint32), rd.view(np.uint32))
    assert not (scales == 255).any()


def test_ties_round_to_even_code(lg):
    x = np.zeros((1, 32), np.float32)
    x[0, 0] = 6.0
    x[0, 1:8] = TIES
    x[0, 8:15] = -TIES
    packed, scales, deq = lg.mxfp4_quantize(x)
    assert scales[0, 0] == 127
    want = [6.0, 0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0]
    np.testing.assert_array_equal(deq[0, :8], want)
    np.testing.assert_array_equal(deq[0, 8:15], [-w for w in want[1:]])


def test_error_bound(lg):
    """|deq - x| <= amax_block / 4: the worst case is saturation, values in
    (6, 8) * 2^e land on 6 * 2^e while amax < 8 * 2^e.

    The relative bound is a property of blocks whose exponent is not
    clamped. For amax < 2^-125 the E8M0 floor pins e at -127, the smallest
    non-zero magnitude any MXFP4 encoding can express is 2^-128, and no
    quantizer can meet amax/4 (x = 2^-149 alone must become 0). There the
    scaled values are below 4, where E2M1 steps are at most 1, so the
    absolute error is at most half a step: 2^-128."""
    x = _edge_data()
    _, scales, deq = lg.mxfp4_quantize(x)
    xb = x.astype(np.float64).reshape(x.shape[0], -1, 32)
    err = np.abs(deq.astype(np.float64).reshape(xb.shape) - xb)
    amax = np.abs(xb).max(axis=2, keepdims=True)
    clamped = (amax > 0) & (amax < 2.0 ** -125)
    assert clamped.any() and (~clamped).sum() > 150
    assert (scales[clamped[:, :, 0]] == 0).all()
    assert (err <= amax / 4)[np.broadcast_to(~clamped, err.shape)].all()
    assert (err <= 2.0 ** -128)[np.broadcast_to(clamped, err.shape)].all()


def test_layout(lg):
    """Element 2i is the low nibble of byte i; scale byte b covers elements
    32b..32b+31."""
    x = np.zeros((2, 96), np.float32)
    x[0, 0] = 6.0     # code 7, block 0, low nibble of byte 0
    x[0, 1] = -1.0    # code 10, high nibble of byte 0
    x[0, 33] = 0.5    # alone in block 1: e = -3, 0.5/2^-3 = 4 -> code 6
    x[1, 64] = 48.0   # block 2 of row 1: e = 3, code 7
    x[1, 95] = -8.0   # -8/8 = -1 -> code 10, high nibble of the last byte
    packed, scales, deq = lg.mxfp4_quantize(x)
    assert packed.shape == (2, 48) and scales.shape == (2, 3)
    assert packed[0, 0] & 0xF == 7 and packed[0, 0] >> 4 == 10
    assert packed[0, 16] == 6 << 4
    assert packed[1, 32] == 7 and packed[1, 47] == 10 << 4
    np.testing.assert_array_equal(scales, [[127, 124, 127], [127, 127, 130]])
    np.testing.assert_array_equal(deq, x)
    # decode by hand from the public format
    code = np.empty((2, 96), np.uint8)
    code[:, 0::2] = packed & 0xF
    code[:, 1::2] = packed >> 4
    val = np.where(code & 8, -MAGS[code & 7], MAGS[code & 7])
    val = val * np.exp2(np.repeat(scales.astype(np.int64), 32, axis=1) - 127)
    np.testing.assert_array_equal(val, x)


@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan])
def test_non_finite_input_raises(lg, bad):
    x = np.ones((2, 64), np.float32)
    x[1, 37] = bad
    with pytest.raises(lg.LoadgenError, match="non-finite"):
        lg.mxfp4_quantize(x)


def test_bad_k_raises(lg):
    with pytest.raises(lg.LoadgenError):
        lg.mxfp4_quantize(np.ones((2, 48), np.float32))


def test_selftest_binary(lg):
    """The ASan+UBSan self-test program: exit 0, nothing on stderr."""
    p = subprocess.run([str(NATIVE / "build" / "mxfp4-selftest")],
                       capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr
    assert p.stderr == ""


def test_burn_rejects_fp8_and_fp4_together(lg):
    with pytest.raises(ValueError):
        lg.gemm_burn(50.0, 1.0, fp8=True, fp4=True)
