"""4 to 8 semantic classes on the fused bf16 heads kernels (needs an MI355X).

The reference trainer's default class count is 5 (label maps exist for 3, 4 and 5).  The logits'
narrow part of the fused heads works in groups of four classes: one group for C <= 4, a second pass
over the semantic accumulators for C <= 8 (csrc/heads_tile.h, template parameter NG), above which
the library falls back to the layer-by-layer heads as before.  Checked here: which kernels run, that
the fused training heads (heads_epi 2) agree with the wave-per-point heads (heads_epi 0, general in
C) within the bounds test_gpu_variants.test_training_heads_kernel_agree uses for the same
arithmetic difference, that every class column is wired to its own weight row, that the inference
kernels agree with each other and with the layer-by-layer heads, that bf16 at C = 5 stays within
test_gpu_bf16's per-output bounds of the fp32 HIP render, and that a captured step replays bit for
bit.  Shapes: 300 rays x 64 guided samples (full tiles, several rays per tile, windows 0 and 1),
97 x 40 unguided (a ragged last tile), and 128 samples per ray (every tile within one ray: the
instance that stages the ray's Q rows in the output staging the logits share) — 150 rays where
gradients are compared, the 19 200 points of the guided shape, since the whole-gradient bound is a
bound on rounding noise averaged over the points; 37 rays (a ragged last tile) for the wiring."""
import copy
import functools

import numpy as np
import pytest
import torch

import golden_util as gu
import spnerf_amd
from spnerf_amd import _lib, random_source
from oracle.weights import ModelDims
from test_gpu_bf16 import out_tol
from test_gpu_c5 import FixedU
from test_gpu_graph import StaticRandom
from test_gpu_parity import DEV, gu_rays, make_model

pytestmark = pytest.mark.gpu

MAX_C = 8          # the built bound (csrc/trunk.h kHeadsMaxC); MAX_C + 1 must fall back
TRAIN_SHAPES = [(300, 64, True), (97, 40, False), (150, 128, False)]
M2W, M2B = "logit_from_label.2.weight", "logit_from_label.2.bias"


class _options:
    def __init__(self, opts):
        self.opts = opts

    def __enter__(self):
        self.old = {k: _lib.get_option(k) for k in self.opts}
        for k, v in self.opts.items():
            _lib.set_option(k, v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            _lib.set_option(k, v)


def _train_inputs(C, n, n_samples, guided):
    args = gu.args_of({"args": dict(n_samples=n_samples, n_importance=0, model="sp-nerf", beta=False,
                                    guidedsample=guided, sc_lambda=0.1, margin=1e-4, stdscale=1.0, chunk=5120,
                                    noise_std=0.0)})
    rays = torch.tensor(gu_rays(n, 31), device=DEV)
    g = torch.Generator(device="cpu").manual_seed(8)
    kw = {}
    if guided:
        kw = dict(valid_depth=(torch.rand(n, generator=g) < 0.7).long().to(DEV),
                  target_depths=torch.stack([rays[:, 7] * 0.5, torch.ones(n, device=DEV)], 1),
                  target_std=torch.full((n,), 0.01, device=DEV))
    pick = torch.tensor(list(range(C)) + [-100])
    labels = pick[torch.randint(0, C + 1, (n,), generator=g)].to(DEV)
    return args, rays, labels, kw


def _train(C, n, n_samples, guided, opts, precision="bf16", backward=True, edit=None):
    """A training render (solar pass on, C classes) and its gradients under the given options."""
    args, rays, labels, kw = _train_inputs(C, n, n_samples, guided)
    model = make_model(ModelDims(width=512, sem=True, num_sem_classes=C), 9, precision)
    if edit is not None:
        with torch.no_grad():
            edit(dict(model.named_parameters()))
        model.invalidate_packed()
    with _options(opts):
        torch.manual_seed(7)
        res = spnerf_amd.render_rays({"coarse": model}, args, rays, None, semantics=labels, mode="train", **kw)
        grads = {}
        if backward:
            loss = sum((v.float() ** 2).mean() for k, v in sorted(res.items()) if v.requires_grad)
            loss.backward()
            grads = {k: p.grad.detach().cpu() for k, p in model.named_parameters() if p.grad is not None}
        torch.cuda.synchronize()
    return {k: v.detach().cpu() for k, v in res.items()}, grads


@functools.lru_cache(maxsize=None)
def _train_cached(C, n, n_samples, guided, epi):
    return _train(C, n, n_samples, guided, {"heads_epi": epi})


def _profiled(fn):
    _lib.prof_reset()
    _lib.prof_enable(True)
    try:
        fn()
    finally:
        _lib.prof_enable(False)
    classes = set(_lib.prof_classes())
    return classes, {c: _lib.prof_read(c)["launches"] for c in classes}


def _infer(C, B, S, opts, precision="bf16", seed=9):
    g = torch.Generator(device="cpu").manual_seed(11)
    rays = torch.tensor(gu.synthetic_rays(B, 25), device=DEV)
    u = torch.rand(B, S, generator=g).to(DEV)
    labels = torch.randint(0, C, (B,), generator=g).to(DEV)
    args = gu.args_of({"args": dict(n_samples=S, n_importance=0, model="sp-nerf", beta=False, guidedsample=False,
                                    sc_lambda=0.0, margin=1e-4, stdscale=1.0, chunk=5120, noise_std=0.0)})
    model = make_model(ModelDims(width=512, sem=True, num_sem_classes=C), seed, precision)
    with _options(opts), torch.no_grad(), random_source(FixedU(u)):
        res = spnerf_amd.render_rays({"coarse": model}, args, rays, None, semantics=labels, mode="test")
    torch.cuda.synchronize()
    return res


# ---- 1. selection

@pytest.mark.parametrize("C", [4, 5, MAX_C])
def test_training_selects_the_fused_heads(C):
    """Default options: one heads launch per forward (the guided main pass's two windows and the
    solar pass, as test_training_heads_kernel_launches counts them at C = 3) and the fused heads dX
    launch in the backward, for every class count up to the bound."""
    assert _lib.get_option("heads_epi") == 2 and _lib.get_option("fused_heads_bwd") == 1
    _lib.set_option("heads_bwd_path", 0)
    classes, launches = _profiled(lambda: _train(C, 300, 64, True, {}))
    assert "heads_train" in classes, classes
    assert launches["heads_train"] == 3, launches
    assert "heads_fwd" not in classes, classes
    assert _lib.get_option("heads_bwd_path") == 1


def test_inference_selects_the_fused_kernel_at_five_classes():
    """The profiling classes of a 5-class inference render are those of the 3-class one (the trunk
    with the heads on its last LDS image), not the layer-by-layer heads'."""
    c3, _ = _profiled(lambda: _infer(3, 130, 128, {}))
    c5, _ = _profiled(lambda: _infer(5, 130, 128, {}))
    assert c3 and "heads_fwd" not in c3, c3
    assert c5 == c3, (c3, c5)
    # ... and with the heads as their own launch after the trunk
    h3, _ = _profiled(lambda: _infer(3, 130, 128, {"trunk_heads": 0}))
    h5, _ = _profiled(lambda: _infer(5, 130, 128, {"trunk_heads": 0}))
    assert h5 == h3 and h3 != c3, (h3, h5, c3)


def test_above_the_bound_falls_back_and_renders():
    """One class more than the fused kernels take: the layer-by-layer heads run, in a training
    render (fused path forced by its option) and in inference, and the render is finite.  (Forward
    only: the backward of a model with more than 8 semantic input columns stops at the 8-row limit
    of the per-ray reductions, whatever heads ran.)"""
    C = MAX_C + 1
    out = {}
    classes, _ = _profiled(lambda: out.update(r=_train(C, 97, 40, False, {"heads_epi": 2}, backward=False)))
    assert "heads_train" not in classes and "heads_fwd" in classes, classes
    res, _ = out["r"]
    assert res["sem_logits_coarse"].shape == (97, C)
    assert all(torch.isfinite(v).all() for v in res.values())
    c3, _ = _profiled(lambda: _infer(3, 130, 128, {}))
    classes, _ = _profiled(lambda: out.update(i=_infer(C, 130, 128, {})))
    assert "heads_fwd" in classes and classes != c3, (classes, c3)
    assert all(torch.isfinite(v).all() for v in out["i"].values())


# ---- 2. training agreement with the wave-per-point heads

@pytest.mark.parametrize("n,n_samples,guided", TRAIN_SHAPES)
@pytest.mark.parametrize("C", [4, 5, 8])
def test_training_heads_agree_with_wave_per_point_heads(C, n, n_samples, guided):
    """heads_epi 2 against heads_epi 0 (what a 5-class user ran before): the wide layers are the
    same arithmetic, the narrow heads sum in another fp32 order — the bounds of
    test_training_heads_kernel_agree: renders within 1e-5 of each tensor's largest entry + 1e-7,
    every gradient tensor within 5e-4 of its largest entry, the whole gradient within 1e-4."""
    r0, g0 = _train_cached(C, n, n_samples, guided, 0)
    r1, g1 = _train_cached(C, n, n_samples, guided, 2)
    assert sorted(r0) == sorted(r1) and sorted(g0) == sorted(g1)
    assert M2W in g0 and M2B in g0
    for k in r0:
        assert torch.isfinite(r1[k]).all(), k
        scale = r0[k].abs().max().item()
        err = (r0[k] - r1[k]).abs().max().item()
        print(k, f"{err:.2e} of {scale:.2e}")
        assert err <= 1e-5 * scale + 1e-7, k
    worst, num, den = {}, 0.0, 0.0
    for k in g0:
        assert torch.isfinite(g1[k]).all(), k
        scale = g0[k].abs().max().item()
        worst[k] = (g0[k] - g1[k]).abs().max().item() / (scale + 1e-30)
        num += float(((g0[k] - g1[k]).double() ** 2).sum())
        den += float((g0[k].double() ** 2).sum())
    print({k: f"{v:.1e}" for k, v in sorted(worst.items(), key=lambda x: -x[1])[:6]}, (num / den) ** 0.5)
    # every class row takes gradient (a dropped second group would leave rows 4.. at zero)
    assert g1[M2W].shape[0] == C and bool((g1[M2W].abs().amax(1) > 0).all()), g1[M2W].abs().amax(1)
    assert bool((g1[M2B].abs() > 0).all()), g1[M2B]
    assert max(worst.values()) <= 5e-4, worst
    assert (num / den) ** 0.5 <= 1e-4


# ---- 3. per-class wiring

@pytest.mark.parametrize("n,n_samples,guided", [(97, 40, False), (37, 128, False)])
@pytest.mark.parametrize("c", range(5))
def test_each_class_column_reads_its_own_weight_row(c, n, n_samples, guided):
    """C = 5, W_m2 zero except row c, bias[c'] = c' + 1: every other column is exactly c' + 1 (its
    eight partials are zeros), column c matches the wave-per-point heads — slot aliasing between the
    groups or with the Q rows staged in the output staging's columns 8..15 would show in either."""
    C = 5

    def edit(p):
        row = p[M2W][c].clone()
        p[M2W].zero_()
        p[M2W][c] = row
        p[M2B].copy_(torch.arange(1, C + 1, dtype=p[M2B].dtype))

    ref = _train(C, n, n_samples, guided, {"heads_epi": 0}, backward=False, edit=edit)[0]["sem_logits_coarse"]
    got = _train(C, n, n_samples, guided, {"heads_epi": 2}, backward=False, edit=edit)[0]["sem_logits_coarse"]
    assert got.shape == (n, C)
    for o in range(C):
        if o != c:
            assert torch.equal(got[:, o], torch.full((n,), float(o + 1))), (o, got[:4, o])
    scale = ref.abs().max().item()
    assert float((ref[:, c] - ref[:, c].mean()).abs().max()) > 0     # the live column is not a constant
    assert (got[:, c] - ref[:, c]).abs().max().item() <= 1e-5 * scale + 1e-7


# ---- 4. inference agreement

@pytest.mark.parametrize("B,S", [(1, 16), (130, 128), (300, 64)])
def test_trunk_with_fused_heads_bit_identical_at_five_classes(B, S):
    """trunk_heads 2 (the heads inside the trunk launch) against trunk_heads 0 (the heads kernel
    after it): the same H_L bits, the same heads code — bit-identical, as at C = 3."""
    a = _infer(5, B, S, {"trunk_heads": 2})
    b = _infer(5, B, S, {"trunk_heads": 0})
    for k in b:
        assert torch.isfinite(a[k]).all(), k
        assert torch.equal(a[k], b[k]), (k, float((a[k] - b[k]).abs().max()))


@pytest.mark.parametrize("C", [5, 8])
@pytest.mark.parametrize("B,S", [(1, 16), (130, 128)])
def test_fused_inference_heads_match_layer_by_layer_heads(C, B, S):
    """The fused inference heads against the G / Q / sun_v GEMMs + wave-per-point heads
    (fused_heads 0): the same bf16 rounding points, other fp32 summation orders — norm-relative
    2e-3 per key, the bound of test_gpu_c5's test of the same name."""
    a = _infer(C, B, S, {"fused_heads": 1}, seed=6)
    b = _infer(C, B, S, {"fused_heads": 0}, seed=6)
    assert a["sem_logits_coarse"].shape == (B, C)
    for k in b:
        x, y = a[k].cpu().numpy(), b[k].cpu().numpy()
        assert np.isfinite(x).all(), k
        e = gu.rel_err(x, y)
        print(k, f"{e:.2e}")
        assert e < 2e-3, (k, e)


# ---- 5. anchor to the fp32 path

def test_five_classes_bf16_close_to_fp32():
    """bf16 against the fp32 HIP render of the same 5-class model and draws (the fp32 path at 5
    classes is pinned to the reference's own outputs by test_gpu_parity), within test_gpu_bf16's
    per-output bounds, in training (fused training heads) and in inference (fused trunk + heads)."""
    lo = _train(5, 300, 64, True, {}, precision="fp32", backward=False)[0]
    hi = _train_cached(5, 300, 64, True, 2)[0]
    ilo, ihi = _infer(5, 130, 128, {}, precision="fp32"), _infer(5, 130, 128, {})
    for what, a, b in (("train", hi, lo), ("test", ihi, ilo)):
        assert sorted(a) == sorted(b)
        for k in b:
            e = gu.rel_err(a[k].cpu().numpy(), b[k].cpu().numpy())
            print(what, k, f"{e:.2e} (bound {out_tol(k):.1e})")
            assert e < out_tol(k), (what, k, e)


# ---- 6. graph

def test_graph_replay_equals_eager_at_five_classes():
    """One captured 5-class training step (render, loss, backward) replayed twice equals the eager
    step bit for bit — inputs, warm-up, capture and replay on one stream."""
    from spnerf_amd.losses import DepthLoss, SemanticLoss, SNerfLoss
    B, C = 256, 5
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        args = gu.args_of({"args": dict(n_samples=64, n_importance=0, model="sp-nerf", beta=False, guidedsample=True,
                                        sc_lambda=0.1, margin=1e-4, stdscale=1.0, chunk=5120, noise_std=0.0)})
        rays = torch.tensor(gu_rays(B, 3), device=DEV)
        g = torch.Generator().manual_seed(1)
        valid = (torch.rand(B, generator=g) < 0.68).long().to(DEV)
        depths = torch.stack([rays[:, 7] * 0.5, torch.rand(B, generator=g).to(DEV)], 1)
        tstd = torch.full((B,), 0.01, device=DEV)
        sems = torch.randint(0, C, (B,), generator=g).to(DEV)
        rgbs = torch.rand(B, 3, generator=g).to(DEV)
        m_e = make_model(ModelDims(width=512, sem=True, num_sem_classes=C), 9, "bf16")
        m_g = copy.deepcopy(m_e)
        src = StaticRandom()
        sl, dl, ce = SNerfLoss(lambda_sc=0.1), DepthLoss(1.0, usealldepth=False), SemanticLoss(1.0)

        def fwd_bwd(model):
            src.reset()
            res = spnerf_amd.render_rays({"coarse": model}, args, rays, None, semantics=sems, mode="train",
                                         valid_depth=valid, target_depths=depths, target_std=tstd)
            loss = sl(res, rgbs)[0] + dl(res, depths[:, 0], depths[:, 1], valid, tstd)[0] + ce(res, sems)[0]
            loss.backward()
            return loss

        with random_source(src):
            fwd_bwd(m_e)                     # fills the static draws
            m_e.zero_grad(set_to_none=True)
            m_g.zero_grad(set_to_none=True)
            m_g.invalidate_packed()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=s):
                loss_g = fwd_bwd(m_g)
            _lib.set_option("heads_bwd_path", 0)
            for it in range(2):
                m_e.zero_grad(set_to_none=True)
                loss_e = fwd_bwd(m_e)
                graph.replay()
                s.synchronize()
                assert torch.equal(loss_e, loss_g), (it, float(loss_e), float(loss_g))
                for (n, pe), (_, pg) in zip(m_e.named_parameters(), m_g.named_parameters()):
                    assert torch.equal(pe.grad, pg.grad), (it, n)
            assert _lib.get_option("heads_bwd_path") == 1
    torch.cuda.synchronize()
