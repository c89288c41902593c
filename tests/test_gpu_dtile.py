"""Tile-ordered D between the saving trunk and the dX chain (option fused_bwd 2) — needs an MI355X.

With fused_bwd 2 the saving 128-point trunk writes D = cos(z) of the layers the chain reads in the
MFMA accumulator order of 64-point blocks (csrc/trunk.h dtile_off) from one epilogue pass, and
k_trunk_bwd_bf16 loads its fragments straight into the epilogue's registers.  D holds the same bf16
values at other addresses and nothing else reads it, so every render key and every parameter
gradient must equal fused_bwd 1 (row-major D) bit for bit — and through tests/test_gpu_variants.py
and tests/test_gpu_trunk.py the layer-by-layer path.  The cases: two windows on block boundaries
with the solar pass and a half-full last forward tile; a partial last block (padded D buffers,
dropped rows); a second window off a block boundary (the whole pass falls back to row-major); one
partial block; K0p = 32 skip columns; a row-major D_0 beside tiled D_1.. (the per-layer mask); and
a layer-by-layer forward under fused_bwd 2 (row-major everywhere).
"""
import pytest
import torch

from spnerf_amd import _lib
from oracle.weights import ModelDims
from test_gpu_trunk import _assert_bitwise, _render

pytestmark = pytest.mark.gpu


def _pair(dims, n_rays, guided, sc, n_samples, options=None, fused=True):
    out = []
    for fb in (1, 2):
        out.append(_render(fused, dims, n_rays, guided, sc, n_samples=n_samples, options={"fused_bwd": fb, **(options or {})}))
    return out


@pytest.mark.parametrize("dims,n_rays,n_samples,guided,sc,options", [
    # windows of 257·64 points each start on 64-point boundaries; the solar pass; 257·64 is no
    # multiple of 128: the forward's last tile is half full
    (ModelDims(width=512, sem=True), 257, 64, True, 0.1, None),
    # 12 040 points: a partial last 64-point block
    (ModelDims(width=512), 301, 40, False, 0.0, None),
    # window 1 starts at point 12 040, off a block boundary: the pass stays row-major
    (ModelDims(width=512), 301, 40, True, 0.0, None),
    # one partial block, one tile
    (ModelDims(width=512), 1, 16, False, 0.0, None),
    # no PE: K0p = 32 skip columns
    (ModelDims(width=512, mapping=False), 130, 64, False, 0.1, None),
    # layer 0 as its own GEMM: D_0 row-major beside tiled D_1.. (the per-layer mask)
    (ModelDims(width=512, sem=True), 257, 64, True, 0.1, {"trunk_l0": 1}),
])
def test_tiled_d_bitwise_vs_row_major(dims, n_rays, n_samples, guided, sc, options):
    assert _lib.get_option("fused_trunk") == 1
    row_major, tiled = _pair(dims, n_rays, guided, sc, n_samples, options)
    _assert_bitwise(tiled, row_major)


def test_layerwise_forward_keeps_row_major_chain():
    """fused_trunk 0 writes every D row-major whatever fused_bwd says; the backward follows what
    the forward recorded, not the option."""
    row_major, tiled = _pair(ModelDims(width=512, sem=True), 257, True, 0.1, 64, fused=False)
    _assert_bitwise(tiled, row_major)
