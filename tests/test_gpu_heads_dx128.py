"""The training heads' dX chain as one 128-point launch (option fused_heads_bwd) — needs an MI355X.

With fused_heads_bwd 1 (the default) the saving trunk writes D_{L-1} tile-ordered too (csrc/trunk.h
dtile_off) where the fused launch will consume it, and k_heads_dx128_bf16 computes dS2, dZQ's sun half,
dZG's feat half and dZ_{L-1} from one LDS image: the same MFMAs in the same K order and the same
epilogue arithmetic as the four layer-by-layer GEMMs (fused_heads_bwd 0), so every render key and every
parameter gradient must be equal bit for bit.  The read-back option heads_bwd_path (1 = the fused launch,
2 = the four GEMMs, or-ed since last zeroed) shows which path ran.
"""
import pytest
import torch

import spnerf_amd
from spnerf_amd import _lib
from oracle.weights import ModelDims
from test_gpu_trunk import DEV, _assert_bitwise, _render

pytestmark = pytest.mark.gpu

C3 = ModelDims(width=512, sem=True)   # guided, solar pass, semantic C = 3, W = 512
SHAPES = [
    (2, 64),      # one 128-point tile
    (97, 64),     # ragged last tile and block
    (301, 40),    # tiles straddling rays, P not a multiple of 64
    (1, 16),      # less than one block
    (1024, 64),   # many tiles per workgroup
]


def _run(dims, n_rays, n_samples, on, options=None):
    """(render, gradients) under the product's training heads (heads_epi 2) and the heads dX paths that ran."""
    _lib.set_option("heads_bwd_path", 0)
    out = _render(True, dims, n_rays, True, 0.1, n_samples=n_samples, options={"heads_epi": 2, "fused_heads_bwd": on, **(options or {})})
    return out, _lib.get_option("heads_bwd_path")


@pytest.fixture(scope="module")
def runs():
    cache = {}

    def get(i):
        if i not in cache:
            n_rays, n_samples = SHAPES[i]
            cache[i] = (_run(C3, n_rays, n_samples, 0), _run(C3, n_rays, n_samples, 1))
        return cache[i]
    return get


@pytest.mark.parametrize("case", range(len(SHAPES)))
def test_fused_heads_dx_bitwise_vs_four_gemms(runs, case):
    (gemms, _), (fused, _) = runs(case)
    _assert_bitwise(fused, gemms)


# The guided main pass is two windows of B x S points in one workspace; window 1 starts at point B x S.
# At 301 x 40 (12 040) and 1 x 16 that is off a 64-point block boundary, so the pass is saved row-major
# (as tests/test_gpu_dchain128.py shows for the dX chain) and takes the four GEMMs; the solar pass is one
# aligned window and takes the fused launch
FUSED_PATHS = [1, 1, 3, 3, 1]


@pytest.mark.parametrize("case", range(len(SHAPES)))
def test_path_that_ran(runs, case):
    """Both passes of the render (mode 0 and the solar pass, mode 2) take the fused launch, and nothing
    else, wherever the forward could save D_{L-1} tile-ordered; with the option off only the four GEMMs run."""
    (_, p0), (_, p1) = runs(case)
    assert (p0, p1) == (2, FUSED_PATHS[case]), (p0, p1)


def test_four_gemm_path_for_other_shapes():
    """A β model and W = 64 do not fit the fused launch: the four GEMMs run under the default."""
    from test_gpu_variants import _render_heads
    assert _lib.get_option("fused_heads_bwd") == 1
    _, path = _run(ModelDims(width=64, sem=True), 33, 64, 1)
    assert path == 2, path
    _lib.set_option("heads_bwd_path", 0)
    _render_heads({}, True, n=33)
    assert _lib.get_option("heads_bwd_path") == 2


def test_four_gemm_path_refuses_tiled_d():
    """The forward saved D_{L-1} tile-ordered for the fused launch; with the option switched off before
    the backward the xD head GEMM must refuse the buffer (an argument error), not read it."""
    from test_gpu_trunk import gu, gu_rays, make_model
    args = gu.args_of({"args": dict(n_samples=64, n_importance=0, model="sp-nerf", beta=False, guidedsample=False,
                                    sc_lambda=0.0, margin=1e-4, stdscale=1.0, chunk=5120, noise_std=0.0)})
    model = make_model(ModelDims(width=512), 2, "bf16")
    rays = torch.tensor(gu_rays(2, 9), device=DEV)
    res = spnerf_amd.render_rays({"coarse": model}, args, rays, None, mode="train")
    loss = sum((v.float() ** 2).mean() for k, v in sorted(res.items()) if v.requires_grad)
    _lib.set_option("fused_heads_bwd", 0)
    try:
        with pytest.raises(Exception) as e:
            loss.backward()
            torch.cuda.synchronize()
        assert "tile-ordered" in str(e.value), str(e.value)
    finally:
        _lib.set_option("fused_heads_bwd", 1)


def test_graph_replay_equals_eager():
    """Capture and replay of the step (render, loss, backward) equals eager bit for bit at 2 x 64."""
    import copy
    from spnerf_amd import random_source
    from test_gpu_graph import StaticRandom
    from test_gpu_trunk import gu, gu_rays, make_model
    args = gu.args_of({"args": dict(n_samples=64, n_importance=0, model="sp-nerf", beta=False, guidedsample=True,
                                    sc_lambda=0.1, margin=1e-4, stdscale=1.0, chunk=5120, noise_std=0.0)})
    n = 2
    rays = torch.tensor(gu_rays(n, 9), device=DEV)
    kw = dict(valid_depth=torch.tensor([1, 0], device=DEV),
              target_depths=torch.stack([rays[:, 7] * 0.5, torch.ones(n, device=DEV)], 1),
              target_std=torch.full((n,), 0.01, device=DEV))
    sem = torch.tensor([0, 2], device=DEV)
    m_e = make_model(C3, 2, "bf16")
    m_g = copy.deepcopy(m_e)
    src = StaticRandom()

    def fwd_bwd(model):
        src.reset()
        res = spnerf_amd.render_rays({"coarse": model}, args, rays, None, semantics=sem, mode="train", **kw)
        loss = sum((v.float() ** 2).mean() for k, v in sorted(res.items()) if v.requires_grad)
        loss.backward()
        return loss

    with random_source(src):
        fwd_bwd(m_e)                     # fills the static draws
        m_e.zero_grad(set_to_none=True)
        m_g.zero_grad(set_to_none=True)
        m_g.invalidate_packed()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            loss_g = fwd_bwd(m_g)
        _lib.set_option("heads_bwd_path", 0)
        loss_e = fwd_bwd(m_e)
        assert _lib.get_option("heads_bwd_path") == 1
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss_e, loss_g)
        for (name, pe), (_, pg) in zip(m_e.named_parameters(), m_g.named_parameters()):
            assert (pe.grad is None) == (pg.grad is None), name
            if pe.grad is not None:
                assert torch.equal(pe.grad, pg.grad), name
