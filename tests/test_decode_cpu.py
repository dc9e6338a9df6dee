"""CPU-side checks of the decode bindings: argument shapes are rejected
before the HIP library is touched."""

import numpy as np
import pytest

from mi355x_gpu_hpa import loadgen


@pytest.mark.parametrize("xs,ws", [((16,), (64, 128)),
                                   ((16, 128), (128,)),
                                   ((16, 128), (2, 2, 64, 128)),
                                   ((16, 128), (64, 256))])
def test_decode_mxfp4_rejects_bad_shapes(xs, ws):
    with pytest.raises(loadgen.LoadgenError):
        loadgen.decode_mxfp4(np.ones(xs, np.float32), np.ones(ws, np.float32))


def test_decode_defaults_describe_an_hbm_sized_ring():
    """The documented default ring (16 x 8192 x 8192 MXFP4 with scales) is
    544 MiB, more than twice the 256 MiB Infinity Cache."""
    import inspect

    p = inspect.signature(loadgen.decode_mxfp4_bench).parameters
    n, k, layers = (p[x].default for x in ("n", "k", "layers"))
    ring = layers * (n * k // 2 + n * k // 32)
    assert ring == 544 << 20
    b = inspect.signature(loadgen.decode_burn).parameters
    assert (b["n"].default, b["k"].default, b["layers"].default,
            b["batch"].default) == (n, k, layers, 16)
