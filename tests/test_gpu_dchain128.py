"""The dX chain on 128-point tiles over tile-ordered D (option fused_bwd 3) — needs an MI355X.

Under fused_bwd 3 the saving trunk writes what it writes under 2, and k_trunk_bwd_bf16 runs its
128-point instance when every layer the chain reads was recorded tile-ordered: a tile is two adjacent
64-point blocks of D, the k order, the x D product and the rounding are those of the 64-point chain,
and the column sums stay one per 64-row block.  D and dZ hold the same values, only the tiling
differs, so every render key and every parameter gradient must equal fused_bwd 2 bit for bit.  Where
the record is incomplete (a row-major pass, a row-major D_0, a layer-by-layer forward) 3 launches the
64-point instance; the library's read-back option trunk_bwd_tile (the tile sizes of the dX chain
launches since it was last zeroed, or-ed) shows which instance ran.
"""
import pytest
import torch

from spnerf_amd import _lib
from oracle.weights import ModelDims
from test_gpu_trunk import _assert_bitwise, _render

pytestmark = pytest.mark.gpu


def _pair(dims, n_rays, guided, sc, n_samples, options=None, fused=True):
    """(fused_bwd 2, fused_bwd 3) results and the chain tile sizes each one launched."""
    out, tiles = [], []
    for fb in (2, 3):
        _lib.set_option("trunk_bwd_tile", 0)
        out.append(_render(fused, dims, n_rays, guided, sc, n_samples=n_samples, options={"fused_bwd": fb, **(options or {})}))
        tiles.append(_lib.get_option("trunk_bwd_tile"))
    return out, tiles


CASES = [
    # 257 blocks per window: the window boundary falls mid-tile, the block count is odd, and the
    # column sums of layer 0 and the skip layer come from both block positions
    (ModelDims(width=512, sem=True), 257, 64, True, 0.1, None, 128),
    # 64.5 tiles: the last tile has one whole block and one absent block
    (ModelDims(width=512), 129, 64, False, 0.0, None, 128),
    # 12 040 points: the last tile has one partial block (8 rows) and nothing else
    (ModelDims(width=512), 301, 40, False, 0.0, None, 128),
    # window 1 starts off a block boundary: the pass is row-major, so 3 takes the 64-point path
    (ModelDims(width=512), 301, 40, True, 0.0, None, 64),
    # one partial block, one tile
    (ModelDims(width=512), 1, 16, False, 0.0, None, 128),
    # no PE: K0p = 32 skip columns
    (ModelDims(width=512, mapping=False), 130, 64, False, 0.1, None, 128),
    # layer 0 as its own GEMM: D_0 is row-major, the mask incomplete, so 3 falls back to the
    # 64-point DT instance
    (ModelDims(width=512, sem=True), 257, 64, True, 0.1, {"trunk_l0": 1}, 64),
]


@pytest.fixture(scope="module")
def runs():
    """Each case rendered once under fused_bwd 2 and 3, shared by the tests below."""
    cache = {}

    def get(i):
        if i not in cache:
            dims, n_rays, n_samples, guided, sc, options, _ = CASES[i]
            cache[i] = _pair(dims, n_rays, guided, sc, n_samples, options)
        return cache[i]
    return get


@pytest.mark.parametrize("case", range(len(CASES)))
def test_chain128_bitwise_vs_chain64(runs, case):
    assert _lib.get_option("fused_trunk") == 1
    (tiled64, tiled128), _ = runs(case)
    _assert_bitwise(tiled128, tiled64)


def test_layerwise_forward_keeps_row_major_chain():
    """fused_trunk 0 writes every D row-major whatever fused_bwd says; the backward follows what the
    forward recorded, not the option: the 64-point chain under 3 as under 2."""
    (a, b), tiles = _pair(ModelDims(width=512, sem=True), 257, True, 0.1, 64, fused=False)
    _assert_bitwise(b, a)
    assert tiles == [64, 64]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_instance_that_ran(runs, case):
    """fused_bwd 2 never launches the 128-point instance; 3 launches it (and nothing else) exactly
    where the recorded mask covers every layer the chain reads."""
    _, tiles = runs(case)
    assert tiles == [64, CASES[case][6]], tiles


def test_fused_bwd_3_round_trips_and_is_the_default():
    old = _lib.get_option("fused_bwd")
    assert old == 3
    try:
        for v in (0, 1, 2, 3):
            _lib.set_option("fused_bwd", v)
            assert _lib.get_option("fused_bwd") == v
    finally:
        _lib.set_option("fused_bwd", old)
