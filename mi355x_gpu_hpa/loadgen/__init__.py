"""ctypes bindings for the CDNA4 HIP load-generator library.

Native side: native/loadgen/{vector_add,gemm_bf16,gemm_fp8_256,
gemm_mxfp4_256,gemm_mxfp4_decode,attn_decode}.hip + loadgen_lib.cpp, built by ``make -C native loadgen``
into native/build/libmi355x_loadgen.so. The MXFP4 quantizer is also built
on its own, without HIP, into native/build/libmi355x_mxfp4.so.

These are the MI355X-native replacements for the reference's CUDA workload
(`k8s.gcr.io/cuda-vector-add:v0.1`, cuda-test-deployment.yaml:18-19).

On a GPU box the HIP library MUST load and the kernels MUST run — there is
no CPU fallback here by design (a silent eager fallback would fake the GPU
tests); calls raise LoadgenError with the native error string on failure.
"""

from __future__ import annotations

import ctypes
import os

import numpy as np

from .. import NATIVE_BUILD

_LIB_PATH = os.environ.get(
    "MI355X_LOADGEN_LIB", str(NATIVE_BUILD / "libmi355x_loadgen.so")
)
_MXFP4_LIB_PATH = os.environ.get(
    "MI355X_MXFP4_LIB", str(NATIVE_BUILD / "libmi355x_mxfp4.so")
)


class LoadgenError(RuntimeError):
    pass


_lib = None


def _load():
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise LoadgenError(
                f"libmi355x_loadgen.so not found at {_LIB_PATH}; "
                "run `make -C native loadgen`"
            )
        lib = ctypes.CDLL(_LIB_PATH)
        lib.lg_last_error.restype = ctypes.c_char_p
        lib.lg_device_count.restype = ctypes.c_int
        lib.lg_vector_add_loop.argtypes = [
            ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_double)
        ]
        lib.lg_vector_add_verify.argtypes = [
            ctypes.c_int,
            np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS"),
            np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS"),
            np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS"),
            ctypes.c_int,
        ]
        lib.lg_gemm_bf16_bench.argtypes = [
            ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
            ctypes.c_int, ctypes.c_int,
            ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
        ]
        lib.lg_gemm_bf16_verify.argtypes = [
            ctypes.c_int,
            np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS"),
            np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS"),
            np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS"),
            ctypes.c_int, ctypes.c_int, ctypes.c_int,
        ]
        lib.lg_gemm_bf16_verify_variant.argtypes = (
            lib.lg_gemm_bf16_verify.argtypes + [ctypes.c_int]
        )
        lib.lg_gemm_bf16_bench_variant.argtypes = [
            ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
            ctypes.c_int, ctypes.c_int, ctypes.c_int,
            ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
        ]
        lib.lg_gemm_burn.argtypes = [
            ctypes.c_int, ctypes.c_double, ctypes.c_double,
            ctypes.c_int, ctypes.c_int, ctypes.c_int,
            ctypes.c_double, ctypes.c_void_p,
        ]
        lib.lg_gemm_fp8_burn.argtypes = lib.lg_gemm_burn.argtypes
        lib.lg_gemm_fp8_bench.argtypes = [
            ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
            ctypes.c_int, ctypes.c_int, ctypes.c_int,
            ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
        ]
        lib.lg_gemm_fp8_verify_variant.argtypes = [
            ctypes.c_int,
            np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS"),
            np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS"),
            np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS"),
            np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS"),
            np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS"),
            ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
        ]
        lib.lg_gemm_fp8_verify.argtypes = [
            ctypes.c_int,
            np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS"),
            np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS"),
            np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS"),
            np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS"),
            np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS"),
            ctypes.c_int, ctypes.c_int, ctypes.c_int,
        ]
        lib.lg_gemm_mxfp4_burn.argtypes = lib.lg_gemm_burn.argtypes
        lib.lg_gemm_mxfp4_bench.argtypes = lib.lg_gemm_bf16_bench.argtypes
        lib.lg_gemm_mxfp4_verify.argtypes = (
            lib.lg_gemm_fp8_verify.argtypes + [ctypes.c_int]
        )
        lib.lg_decode_mxfp4_verify.argtypes = (
            lib.lg_gemm_fp8_verify.argtypes + [ctypes.c_int, ctypes.c_int]
        )
        lib.lg_decode_mxfp4_bench.argtypes = [
            ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
            ctypes.c_int, ctypes.c_int, ctypes.c_int,
            ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
        ]
        lib.lg_decode_mxfp4_burn.argtypes = [
            ctypes.c_int, ctypes.c_double, ctypes.c_double,
            ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
            ctypes.c_double, ctypes.c_void_p, ctypes.POINTER(ctypes.c_double),
        ]
        lib.lg_attn_decode_verify.argtypes = [
            ctypes.c_int,
            np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS"),
            np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS"),
            np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS"),
            np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS"),
            np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS"),
            np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS"),
            ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
            ctypes.c_int, ctypes.c_int, ctypes.c_double,
        ]
        lib.lg_attn_decode_bench.argtypes = [
            ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
            ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
            ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
        ]
        lib.lg_attn_decode_bench_splits.argtypes = [
            ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
            ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
            ctypes.c_int,
            ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
        ]
        lib.lg_attn_decode_burn.argtypes = [
            ctypes.c_int, ctypes.c_double, ctypes.c_double,
            ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
            ctypes.c_int, ctypes.c_double, ctypes.c_void_p,
            ctypes.POINTER(ctypes.c_double),
        ]
        lib.lg_bw_burn.argtypes = [
            ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double,
            ctypes.c_double, ctypes.c_void_p, ctypes.POINTER(ctypes.c_double),
        ]
        _lib = lib
    return _lib


_mxfp4_lib = None


def _load_mxfp4():
    """The host-only MXFP4 quantizer library (no HIP dependency)."""
    global _mxfp4_lib
    if _mxfp4_lib is None:
        if not os.path.exists(_MXFP4_LIB_PATH):
            raise LoadgenError(
                f"libmi355x_mxfp4.so not found at {_MXFP4_LIB_PATH}; "
                "run `make -C native mxfp4-host`"
            )
        lib = ctypes.CDLL(_MXFP4_LIB_PATH)
        lib.lg_mxfp4_last_error.restype = ctypes.c_char_p
        lib.lg_mxfp4_quantize.argtypes = [
            np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS"),
            ctypes.c_int, ctypes.c_int,
            np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS"),
            np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS"),
            np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS"),
        ]
        _mxfp4_lib = lib
    return _mxfp4_lib


def _check(rc: int):
    if rc != 0:
        raise LoadgenError(_load().lg_last_error().decode())


def available() -> bool:
    return os.path.exists(_LIB_PATH)


def device_count() -> int:
    return _load().lg_device_count()


def vector_add_loop(device: int = 0, n: int = 50_000, iters: int = 100) -> float:
    """Run the reference load shape (launch loop); returns total wall ms."""
    ms = ctypes.c_double()
    _check(_load().lg_vector_add_loop(device, n, iters, ctypes.byref(ms)))
    return ms.value


def vector_add(a: np.ndarray, b: np.ndarray, device: int = 0) -> np.ndarray:
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape and a.ndim == 1
    out = np.empty_like(a)
    _check(_load().lg_vector_add_verify(device, a, b, out, a.size))
    return out


def gemm_bf16(a: np.ndarray, bt: np.ndarray, device: int = 0,
              variant: int = 1) -> np.ndarray:
    """C f32 [m,n] = bf16(a) [m,k] @ bf16(bt).T [k,n] on the GPU.

    variant: 1 = 128^2 swizzled tile (default), 0 = 128^2 linear LDS,
    2 = 256^2 8-phase schedule (m,n must be multiples of 256)."""
    a = np.ascontiguousarray(a, np.float32)
    bt = np.ascontiguousarray(bt, np.float32)
    m, k = a.shape
    n, k2 = bt.shape
    assert k == k2
    out = np.empty((m, n), np.float32)
    _check(_load().lg_gemm_bf16_verify_variant(device, a, bt, out, m, n, k,
                                               variant))
    return out


def gemm_bench(m=4096, n=4096, k=4096, warmup=5, iters=50, device=0,
               variant=1):
    """Returns (ms_per_gemm, tflops)."""
    ms = ctypes.c_double()
    tf = ctypes.c_double()
    _check(_load().lg_gemm_bf16_bench_variant(device, m, n, k, warmup, iters,
                                              variant,
                                              ctypes.byref(ms), ctypes.byref(tf)))
    return ms.value, tf.value


def gemm_fp8(a: np.ndarray, bt: np.ndarray, device: int = 0,
             raster: int = 1):
    """FP8 (E4M3) MFMA GEMM numerics entry: quantizes the f32 inputs to
    E4M3, computes C = Aq @ Btq^T on the GPU, and returns
    (c, aq, btq) where aq/btq are the dequantized (f32) operands the GPU
    actually multiplied — the caller computes the exact reference from
    them. M,N %% 256 == 0, K %% 128 == 0."""
    m, k = a.shape
    n, k2 = bt.shape
    assert k == k2
    a = np.ascontiguousarray(a, np.float32)
    bt = np.ascontiguousarray(bt, np.float32)
    c = np.empty((m, n), np.float32)
    aq = np.empty_like(a)
    btq = np.empty_like(bt)
    _check(_load().lg_gemm_fp8_verify_variant(device, a, bt, c, aq, btq,
                                              m, n, k, raster))
    return c, aq, btq


def gemm_fp8_bench(m=8192, n=8192, k=8192, warmup=2, iters=10, raster=1,
                   device=0):
    """Returns (ms_per_gemm, tflops) for the fp8 kernel."""
    ms = ctypes.c_double()
    tf = ctypes.c_double()
    _check(_load().lg_gemm_fp8_bench(device, m, n, k, warmup, iters, raster,
                                     ctypes.byref(ms), ctypes.byref(tf)))
    return ms.value, tf.value


def mxfp4_quantize(x: np.ndarray):
    """OCP MX FP4 quantizer (host only, no GPU needed): x f32 [r, k] with
    k % 32 == 0 -> (packed u8 [r, k/2], scales u8 [r, k/32], deq f32 [r, k]).

    packed[r, i] holds element 2i in bits 3:0 and 2i+1 in bits 7:4 (E2M1
    codes); scales[r, b] is the E8M0 byte (value 2^(byte-127)) of elements
    32b..32b+31; deq is what those bytes decode to. Non-finite input
    raises LoadgenError."""
    x = np.ascontiguousarray(x, np.float32)
    if x.ndim != 2:
        raise LoadgenError("mxfp4_quantize expects a 2-D array")
    r, k = x.shape
    packed = np.empty((r, k // 2), np.uint8)
    scales = np.empty((r, k // 32), np.uint8)
    deq = np.empty((r, k), np.float32)
    lib = _load_mxfp4()
    if lib.lg_mxfp4_quantize(x, r, k, packed, scales, deq) != 0:
        raise LoadgenError(lib.lg_mxfp4_last_error().decode())
    return packed, scales, deq


def gemm_mxfp4(a: np.ndarray, bt: np.ndarray, device: int = 0,
               max_ctas: int = 0):
    """MXFP4 (E2M1 + E8M0 block scale) MFMA GEMM numerics entry: quantizes
    the f32 inputs like mxfp4_quantize(), computes C = Aq @ Btq^T on the
    GPU, and returns (c, aq, btq) where aq/btq are the dequantized (f32)
    operands the GPU actually multiplied. M,N,K % 256 == 0. max_ctas > 0
    caps the grid so each CTA loops over several tiles."""
    m, k = a.shape
    n, k2 = bt.shape
    assert k == k2
    a = np.ascontiguousarray(a, np.float32)
    bt = np.ascontiguousarray(bt, np.float32)
    c = np.empty((m, n), np.float32)
    aq = np.empty_like(a)
    btq = np.empty_like(bt)
    _check(_load().lg_gemm_mxfp4_verify(device, a, bt, c, aq, btq, m, n, k,
                                        max_ctas))
    return c, aq, btq


def gemm_mxfp4_bench(m=8192, n=8192, k=8192, warmup=2, iters=10, device=0):
    """Returns (ms_per_gemm, tflops) for the MXFP4 kernel (2*M*N*K FLOPs)."""
    ms = ctypes.c_double()
    tf = ctypes.c_double()
    _check(_load().lg_gemm_mxfp4_bench(device, m, n, k, warmup, iters,
                                       ctypes.byref(ms), ctypes.byref(tf)))
    return ms.value, tf.value


def gemm_burn(target_util_pct: float, seconds: float, device: int = 0,
              m: int = 4096, n: int = 4096, k: int = 4096,
              period_ms: float = 100.0, fp8: bool = False,
              fp4: bool = False):
    """Duty-cycled GEMM load at a target GPU-busy percentage (closed-loop
    on measured GPU-active time); fp8=True burns with the E4M3 kernel,
    fp4=True with the MXFP4 kernel (not both)."""
    if fp8 and fp4:
        raise ValueError("gemm_burn: fp8 and fp4 are mutually exclusive")
    lib = _load()
    fn = (lib.lg_gemm_mxfp4_burn if fp4
          else lib.lg_gemm_fp8_burn if fp8 else lib.lg_gemm_burn)
    _check(fn(device, target_util_pct, seconds, m, n, k, period_ms, None))


def decode_mxfp4(x: np.ndarray, w: np.ndarray, device: int = 0,
                 k_splits: int = 0):
    """Decode-phase MXFP4 weight-streaming GEMM numerics entry: x f32
    [m, k] with 1 <= m <= 64, w f32 [n, k] (one layer) or [layers, n, k];
    n % 64 == 0, k % 128 == 0. Both are quantized like mxfp4_quantize();
    returns (c, xq, wq) with c[..., m, n] = xq @ wq[layer].T per layer and
    xq/wq the dequantized (f32) operands the GPU actually multiplied.
    k_splits: 0 = the library's heuristic, > 0 forces that many K slices
    across CTAs (must divide k/128)."""
    x = np.ascontiguousarray(x, np.float32)
    w = np.ascontiguousarray(w, np.float32)
    if x.ndim != 2 or w.ndim not in (2, 3) or x.shape[1] != w.shape[-1]:
        raise LoadgenError("decode_mxfp4 expects x [m, k] and w [n, k] or "
                           "[layers, n, k]")
    m, k = x.shape
    w3 = w.reshape((-1,) + w.shape[-2:])
    layers, n, _ = w3.shape
    c = np.empty((layers, m, n), np.float32)
    xq = np.empty_like(x)
    wq = np.empty_like(w3)
    _check(_load().lg_decode_mxfp4_verify(device, x, w3, c, xq, wq, m, n, k,
                                          layers, k_splits))
    if w.ndim == 2:
        return c[0], xq, wq[0]
    return c, xq, wq


def decode_mxfp4_bench(m=16, n=8192, k=8192, layers=16, warmup=2, iters=10,
                       device=0):
    """Returns (ms_per_step, weight_gbps): one step is a pass over the ring
    of `layers` weight matrices; weight_gbps counts the weight elements and
    scales streamed per step."""
    ms = ctypes.c_double()
    gbps = ctypes.c_double()
    _check(_load().lg_decode_mxfp4_bench(device, m, n, k, layers, warmup,
                                         iters, ctypes.byref(ms),
                                         ctypes.byref(gbps)))
    return ms.value, gbps.value


def decode_burn(target_util_pct: float, seconds: float, device: int = 0,
                batch: int = 16, n: int = 8192, k: int = 8192,
                layers: int = 16, period_ms: float = 100.0) -> float:
    """Duty-cycled decode load at a target GPU-busy percentage (the shared
    closed-loop duty engine over decode steps): the busy-but-bandwidth-bound
    shape of a small-batch MXFP4 serving pod. Returns the weight GB/s
    streamed during the busy bursts."""
    gbps = ctypes.c_double()
    _check(_load().lg_decode_mxfp4_burn(device, target_util_pct, seconds,
                                        batch, n, k, layers, period_ms, None,
                                        ctypes.byref(gbps)))
    return gbps.value


ATTN_HEAD_DIM = 128


def _attn_args(q, k, v, seq_lens):
    """Shape checks shared by attn_decode and attn_decode_ref; returns
    (batch, hq, hkv, lmax, seq_lens as int32)."""
    if q.ndim != 3 or k.ndim != 4 or v.ndim != 4:
        raise LoadgenError("attn_decode expects q [B, Hq, D] and k, v "
                           "[B, Hkv, Lmax, D]")
    if k.shape != v.shape:
        raise LoadgenError(f"attn_decode: k {k.shape} and v {v.shape} differ")
    if q.shape[-1] != ATTN_HEAD_DIM or k.shape[-1] != ATTN_HEAD_DIM:
        raise LoadgenError("attn_decode: head dimension must be 128")
    batch, hq, _ = q.shape
    hkv, lmax = k.shape[1], k.shape[2]
    if k.shape[0] != batch:
        raise LoadgenError("attn_decode: q and k batch dimensions differ")
    if batch < 1 or hkv < 1 or lmax < 1:
        raise LoadgenError("attn_decode: empty batch, heads or context")
    if hq % hkv or hq // hkv > 16:
        raise LoadgenError(f"attn_decode: {hq} q heads over {hkv} kv heads; "
                           "need a multiple, at most 16 per kv head")
    lens = np.asarray(seq_lens)
    if lens.shape != (batch,) or lens.dtype.kind not in "iu":
        raise LoadgenError(f"attn_decode: seq_lens must be {batch} integers")
    if lens.min() < 1 or lens.max() > lmax:
        raise LoadgenError(f"attn_decode: seq_lens outside 1..{lmax}")
    return batch, hq, hkv, lmax, np.ascontiguousarray(lens, np.int32)


def attn_decode(q: np.ndarray, k: np.ndarray, v: np.ndarray, seq_lens,
                device: int = 0, kv_splits: int = 0, scale=None):
    """Single-token decode attention on the GPU: q f32 [B, Hq, 128], k and
    v f32 [B, Hkv, Lmax, 128] (converted to bf16), seq_lens [B] in 1..Lmax;
    query head h reads kv head h // (Hq // Hkv), Hq // Hkv <= 16. Positions
    >= seq_lens[b] are never read into the result. Returns (o f32
    [B, Hq, 128], lse f32 [B, Hq]) with lse the natural-log sum of
    exp(scale * q.k_i). kv_splits: 0 = the library's heuristic, > 0 forces
    that many splits of the context across CTAs (<= ceil(Lmax/32)).
    scale: None = 1/sqrt(128)."""
    q = np.ascontiguousarray(q, np.float32)
    k = np.ascontiguousarray(k, np.float32)
    v = np.ascontiguousarray(v, np.float32)
    batch, hq, hkv, lmax, lens = _attn_args(q, k, v, seq_lens)
    o = np.empty((batch, hq, ATTN_HEAD_DIM), np.float32)
    lse = np.empty((batch, hq), np.float32)
    _check(_load().lg_attn_decode_verify(
        device, q, k, v, lens, o, lse, batch, hq, hkv, lmax, ATTN_HEAD_DIM,
        kv_splits, 0.0 if scale is None else float(scale)))
    return o, lse


def attn_decode_ref(q: np.ndarray, k: np.ndarray, v: np.ndarray, seq_lens,
                    scale=None):
    """float64 numpy reference of attn_decode over the arrays as given (no
    bf16 rounding, no GPU). Slices every slab to seq_lens[b] first, so a
    position >= seq_lens[b] is never indexed."""
    q = np.asarray(q, np.float64)
    k = np.asarray(k)
    v = np.asarray(v)
    batch, hq, hkv, _, lens = _attn_args(q, k, v, seq_lens)
    group = hq // hkv
    if scale is None:
        scale = 1.0 / np.sqrt(ATTN_HEAD_DIM)
    o = np.empty((batch, hq, ATTN_HEAD_DIM), np.float64)
    lse = np.empty((batch, hq), np.float64)
    for b in range(batch):
        for h in range(hkv):
            kk = k[b, h, :lens[b]].astype(np.float64)
            vv = v[b, h, :lens[b]].astype(np.float64)
            heads = slice(h * group, (h + 1) * group)
            s = scale * (q[b, heads] @ kk.T)
            m = s.max(axis=1, keepdims=True)
            p = np.exp(s - m)
            tot = p.sum(axis=1, keepdims=True)
            o[b, heads] = (p @ vv) / tot
            lse[b, heads] = (m + np.log(tot))[:, 0]
    return o, lse


def attn_decode_bench(batch=32, hq=64, hkv=8, ctx=8192, warmup=2, iters=10,
                      device=0, kv_splits=0):
    """Returns (ms_per_step, kv_gbps): one step is decode attention for
    `batch` sequences of `ctx` cached positions each; kv_gbps counts the K
    and V bytes read per step, batch * hkv * ctx * 2 * 128 * 2. kv_splits
    as for attn_decode."""
    ms = ctypes.c_double()
    gbps = ctypes.c_double()
    _check(_load().lg_attn_decode_bench_splits(
        device, batch, hq, hkv, ctx, ATTN_HEAD_DIM, kv_splits, warmup, iters,
        ctypes.byref(ms), ctypes.byref(gbps)))
    return ms.value, gbps.value


def attn_burn(target_util_pct: float, seconds: float, device: int = 0,
              batch: int = 32, hq: int = 64, hkv: int = 8, ctx: int = 8192,
              period_ms: float = 100.0) -> float:
    """Duty-cycled decode-attention load at a target GPU-busy percentage
    (the shared closed-loop duty engine over attention steps): the KV-cache
    side of a decode pod. Returns the KV GB/s read during the busy bursts."""
    gbps = ctypes.c_double()
    _check(_load().lg_attn_decode_burn(device, target_util_pct, seconds,
                                       batch, hq, hkv, ctx, ATTN_HEAD_DIM,
                                       period_ms, None, ctypes.byref(gbps)))
    return gbps.value


def bw_burn(target_util_pct: float, seconds: float, device: int = 0,
            gb: float = 6.0, period_ms: float = 100.0) -> float:
    """Duty-cycled streaming-triad HBM load (the bandwidth axis of the
    multi-metric HPA). Returns achieved GB/s during the busy bursts."""
    gbps = ctypes.c_double()
    _check(_load().lg_bw_burn(device, target_util_pct, seconds, gb,
                              period_ms, None, ctypes.byref(gbps)))
    return gbps.value
