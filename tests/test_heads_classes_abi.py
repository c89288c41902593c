"""Sizes the C ABI reports for 1 to 9 semantic classes (no GPU, no compute calls).

The fused bf16 heads take up to 8 classes (two groups of four, csrc/trunk.h kHeadsMaxC): up to
there the bf16 packed layout carries their fragment-ordered weight streams, above it the streams are
left out and the layer-by-layer heads run.  spnerf_param_info, spnerf_packed_bytes and
spnerf_mlp_workspace_bytes must agree with each other and grow with the class count."""
import ctypes

import numpy as np
import pytest

from spnerf_amd import _lib
from oracle.weights import ModelDims, param_specs
from test_abi import cfg_of

MAX_C = 8
CLASSES = list(range(1, MAX_C + 2))
# the fused heads' weight streams (bf16 elements, W = 512, H = 256): semantic hidden, feat, Q, the
# solar pass's Q, sun_v 2 / 3, the narrow heads' hi / lo rows, and the dX launch's four transposes
W, H = 512, 256
STREAMS = H * W + W * W + 2 * H * W + H * W + 2 * H * H + 32 * (W + 2 * H) + 2 * H * H + W * 2 * H + W * (W + H)


def _cfg(C, dtype):
    c = cfg_of(ModelDims(width=W, sem=True, num_sem_classes=C))
    c.dtype = dtype
    return c


def _params(c):
    L = _lib.lib()
    out, buf = {}, ctypes.create_string_buffer(128)
    for i in range(L.spnerf_param_count(ctypes.byref(c))):
        r, k = ctypes.c_int64(), ctypes.c_int64()
        assert L.spnerf_param_info(ctypes.byref(c), i, buf, 128, ctypes.byref(r), ctypes.byref(k)) == 0
        out[buf.value.decode()] = (r.value, k.value) if k.value else (r.value,)
    return out


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("C", CLASSES)
def test_parameter_shapes_and_sizes_are_consistent(C, dtype):
    L = _lib.lib()
    c = _cfg(C, dtype)
    shapes = _params(c)
    specs = param_specs(ModelDims(width=W, sem=True, num_sem_classes=C))
    assert shapes == {name: tuple(shape) for name, shape, _ in specs}
    assert shapes["logit_from_label.2.weight"] == (C, H) and shapes["logit_from_label.2.bias"] == (C,)
    n = sum(int(np.prod(s)) for s in shapes.values())
    packed = L.spnerf_packed_bytes(ctypes.byref(c))
    assert packed % 256 == 0 and packed > 4 * n      # every parameter once in fp32, 256-B blocks
    if dtype == 1 and C <= MAX_C:
        # ... and the fused heads' streams on top of the same class count's fp32 layout
        assert packed >= L.spnerf_packed_bytes(ctypes.byref(_cfg(C, 0))) + 2 * STREAMS
    for flags in (0, _lib.SPNERF_MLP_SAVE):
        for rays, S in ((1, 16), (97, 40), (300, 64)):
            ws = L.spnerf_mlp_workspace_bytes(ctypes.byref(c), rays, S, flags)
            assert ws > 0 and ws % 4 == 0, (rays, S, flags, ws)


@pytest.mark.parametrize("dtype", [0, 1])
def test_sizes_grow_with_the_class_count(dtype):
    """Monotone in C: the workspace everywhere, the packed layout everywhere in fp32 and up to the
    fused heads' bound in bf16 (one class above it the streams are not packed: the size drops by
    them, as it did between 4 and 5 classes before the kernels took a second class group)."""
    L = _lib.lib()
    packed = [L.spnerf_packed_bytes(ctypes.byref(_cfg(C, dtype))) for C in CLASSES]
    upto = MAX_C if dtype == 1 else MAX_C + 1
    assert all(b >= a for a, b in zip(packed[:upto], packed[1:upto])), packed
    assert packed[upto - 1] > packed[0], packed
    if dtype == 1:
        assert packed[MAX_C] < packed[MAX_C - 1] and packed[MAX_C - 1] - packed[MAX_C] <= 2 * STREAMS + 65536, packed
    for flags in (0, _lib.SPNERF_MLP_SAVE):
        ws = [L.spnerf_mlp_workspace_bytes(ctypes.byref(_cfg(C, dtype)), 300, 64, flags) for C in CLASSES]
        assert all(b >= a for a, b in zip(ws, ws[1:])), (flags, ws)     # (the output rows are the caller's)
