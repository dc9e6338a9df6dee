"""CPU-side checks of the decode-attention bindings: bad arguments are
rejected before the HIP library is touched, the float64 reference meets its
closed forms, and the documented default cache is 1 GiB."""

import inspect

import numpy as np
import pytest

from attn_cases import D, HKV, onehot_case, uniform_case
from mi355x_gpu_hpa import loadgen


def _args(qs, ks, vs, lens):
    return (np.ones(qs, np.float32), np.ones(ks, np.float32),
            np.ones(vs, np.float32), np.array(lens))


@pytest.mark.parametrize("qs,ks,vs,lens", [
    ((2, 128), (2, 2, 40, 128), (2, 2, 40, 128), [40, 40]),           # 2-D q
    ((2, 8, 128), (2, 2, 40, 128), (2, 2, 41, 128), [40, 40]),        # k != v
    ((2, 8, 64), (2, 2, 40, 64), (2, 2, 40, 64), [40, 40]),           # D = 64
    ((2, 6, 128), (2, 4, 40, 128), (2, 4, 40, 128), [40, 40]),        # 6 / 4
    ((2, 64, 128), (2, 2, 40, 128), (2, 2, 40, 128), [40, 40]),       # G = 32
    ((2, 8, 128), (2, 2, 40, 128), (2, 2, 40, 128), [40, 0]),         # len 0
    ((2, 8, 128), (2, 2, 40, 128), (2, 2, 40, 128), [41, 40]),        # Lmax+1
    ((2, 8, 128), (2, 2, 40, 128), (2, 2, 40, 128), [40, 40, 40]),    # length
], ids=["q2d", "kv_mismatch", "d64", "hq6_hkv4", "g32", "len0", "len_over",
        "lens_shape"])
def test_attn_decode_rejects_bad_arguments(monkeypatch, qs, ks, vs, lens):
    def no_load():
        raise AssertionError("the HIP library was loaded")

    monkeypatch.setattr(loadgen, "_load", no_load)
    with pytest.raises(loadgen.LoadgenError):
        loadgen.attn_decode(*_args(qs, ks, vs, lens))


def test_attn_ref_onehot_selects_the_target_row():
    seq_lens, lmax, group = [1, 37, 300], 320, 8
    q, k, v, t = onehot_case(group, seq_lens, lmax)
    o, lse = loadgen.attn_decode_ref(q, k, v, seq_lens)
    assert np.isfinite(o).all() and np.isfinite(lse).all()
    for b in range(len(seq_lens)):
        for h in range(group * HKV):
            want = v[b, h // group, t[b, h]].astype(np.float64)
            err = np.abs(o[b, h] - want).max()
            assert err <= 1e-12, (b, h, err)
    np.testing.assert_allclose(lse, 1024 / np.sqrt(D), rtol=0, atol=1e-12)


def test_attn_ref_uniform_is_the_mean():
    seq_lens, lmax, group = [1, 37, 300], 320, 8
    q, k, v = uniform_case(group, seq_lens, lmax)
    o, lse = loadgen.attn_decode_ref(q, k, v, seq_lens)
    for b, n in enumerate(seq_lens):
        for h in range(group * HKV):
            want = v[b, h // group, :n].astype(np.float64).mean(axis=0)
            np.testing.assert_allclose(o[b, h], want, rtol=0, atol=1e-12)
        np.testing.assert_allclose(lse[b], np.log(n), rtol=0, atol=1e-12)


def test_attn_defaults_describe_a_1gib_cache():
    """The documented default cache (batch 32, 8 kv heads, 8192 positions,
    K and V, 128 bf16 each) is exactly 1 GiB, four times the 256 MiB
    Infinity Cache; bench and burn agree on it."""
    p = inspect.signature(loadgen.attn_decode_bench).parameters
    shape = {x: p[x].default for x in ("batch", "hq", "hkv", "ctx")}
    assert shape["batch"] * shape["hkv"] * shape["ctx"] * 2 * 128 * 2 == 1 << 30
    b = inspect.signature(loadgen.attn_burn).parameters
    assert {x: b[x].default for x in shape} == shape
    assert loadgen.ATTN_HEAD_DIM == D == 128
