"""LPIPS on the GPU (csrc/lpips.hip, spnerf_amd.perceptual) — needs an MI355X.

Everything is compared with the float64 restatement tests/lpips_torch.py on the same fp32 images and
the same seeded fp32 weights.  Bars: every post-ReLU tap element-wise within 1e-4 of that tap's
max-abs (the project's fp32 bar), the score and each per-tap term within 1e-5 relative (torch's own
fp32 is within about 1e-6 of the restatement on these inputs; 10x for another summation order over
K <= 3 456).  Measured on an MI355X, worst over the five shapes: taps 1.7e-6 of their max-abs, score
1.2e-7, per-tap term 8.5e-7 relative.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import lpips_torch as lt
import spnerf_amd
from spnerf_amd import _lib, _lpips_lib, perceptual

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TAP_TOL = 1e-4
SCORE_TOL = 1e-5
# 31 x 31: every stage at its minimum (taps 7, 3, 1, 1, 1; the last three see only padding around one
# position).  35 x 47: not square, taps 8 x 11, 3 x 5, 1 x 2, the first pool drops a row.  34 x 46:
# conv1's stride leaves a remainder of 3 in both axes, taps 7 x 10, 3 x 4, 1 x 1, both pools drop a
# column.  64 x 64 and 97 x 130: several GEMM tiles and a partial one in M (450 and 1 426 rows).
SHAPES = [(31, 31), (35, 47), (34, 46), (64, 64), (97, 130)]


@functools.lru_cache(maxsize=None)
def weights():
    return spnerf_amd.LpipsWeights.from_tensors(*lt.seeded_weights(), device=DEV)


@functools.lru_cache(maxsize=None)
def case(H, W):
    """(a, b, score, layers, taps of a, taps of b) of the restatement for one shape, computed once."""
    a, b = lt.pair(H, W)
    score, layers, fa, fb = lt.lpips(a, b, lt.seeded_weights())
    return a, b, score, tuple(layers), tuple(fa), tuple(fb)


def hwc(t):
    """The (H * W, 3) plane of a (3, H, W) image, on the device."""
    return t.permute(1, 2, 0).reshape(-1, 3).contiguous().to(DEV)


def rel(got, want):
    return abs(got - want) / abs(want)


@pytest.mark.parametrize("H,W", SHAPES)
def test_taps_and_score_match_restatement(H, W):
    a, b, score, layers, fa, fb = case(H, W)
    got, got_layers, feats = spnerf_amd.lpips(hwc(a), hwc(b), weights(), hw=(H, W), return_features=True)
    assert got.dtype == torch.float64 and got.dim() == 0 and got.is_cuda and tuple(got_layers.shape) == (5,)
    worst = 0.0
    for l in range(5):
        assert tuple(feats[l].shape) == (2,) + tuple(fa[l].shape[1:]) + (fa[l].shape[0],), l
        for img, ref in ((0, fa[l]), (1, fb[l])):
            ref = ref.permute(1, 2, 0)
            err = float((feats[l][img].cpu().double() - ref).abs().max()) / float(ref.abs().max())
            worst = max(worst, err)
            assert err <= TAP_TOL, (l, img, err)
    errs = [rel(float(got_layers[l]), layers[l]) for l in range(5)]
    print(f"{H}x{W}: lpips {float(got):.6e} (ref {score:.6e}) rel {rel(float(got), score):.1e}; "
          f"layers rel {max(errs):.1e}; taps {worst:.1e} of max-abs")
    assert all(d > 0 for d in layers)
    assert rel(float(got), score) <= SCORE_TOL
    assert max(errs) <= SCORE_TOL, errs
    assert float(got) == functools.reduce(lambda s, d: s + d, got_layers.tolist(), 0.0)   # the taps added in order
    alone = spnerf_amd.lpips(hwc(a), hwc(b), weights(), hw=(H, W))                  # features_out = NULL: the same bits
    assert float(alone) == float(got)


def test_row_bands_give_the_same_bits():
    H, W = 97, 130
    a, b, score, *_ = case(H, W)
    least = perceptual.workspace_bytes(H, W, 1)
    assert least < perceptual.workspace_bytes(H, W)
    n = perceptual.bands(H, W, least)
    assert n[0] >= 3 and n[1] >= 2 and perceptual.bands(H, W, perceptual.workspace_bytes(H, W)) == [1] * 5, n
    whole, wl, wf = spnerf_amd.lpips(hwc(a), hwc(b), weights(), hw=(H, W), return_features=True)
    split, sl, sf = spnerf_amd.lpips(hwc(a), hwc(b), weights(), hw=(H, W), return_features=True, max_workspace_bytes=least)
    assert float(whole) == float(split) and torch.equal(wl, sl)
    assert all(torch.equal(u, v) for u, v in zip(wf, sf))
    mid = spnerf_amd.lpips(hwc(a), hwc(b), weights(), hw=(H, W), max_workspace_bytes=(least + perceptual.workspace_bytes(H, W)) // 2)
    assert float(mid) == float(whole)
    assert rel(float(split), score) <= SCORE_TOL


@pytest.mark.parametrize("H,W", [(31, 31), (97, 130)])
def test_identity_symmetry_and_reproducibility(H, W):
    a, b, *_ = case(H, W)
    ta, tb = hwc(a), hwc(b)
    same, same_layers = spnerf_amd.lpips(ta, ta.clone(), weights(), hw=(H, W), return_layers=True)
    assert float(same) == 0.0 and bool((same_layers == 0).all())
    ab, ab_layers = spnerf_amd.lpips(ta, tb, weights(), hw=(H, W), return_layers=True)
    ba, ba_layers = spnerf_amd.lpips(tb, ta, weights(), hw=(H, W), return_layers=True)
    assert float(ab) == float(ba) and torch.equal(ab_layers, ba_layers)       # one launch serves both images: bit for bit
    again, again_layers = spnerf_amd.lpips(ta, tb, weights(), hw=(H, W), return_layers=True)
    assert float(again) == float(ab) and torch.equal(again_layers, ab_layers)


def test_layouts_and_normalize():
    H, W = 35, 47
    a, b, score, *_ = case(H, W)
    flat = float(spnerf_amd.lpips(hwc(a), hwc(b), weights(), hw=(H, W)))
    assert float(spnerf_amd.lpips(hwc(a).view(H, W, 3), hwc(b).view(H, W, 3), weights())) == flat
    assert float(spnerf_amd.lpips(a.to(DEV), b.to(DEV), weights(), layout="chw")) == flat
    assert float(spnerf_amd.lpips(a.to(DEV)[None], b.to(DEV)[None], weights(), layout="chw")) == flat
    # planar rows padded with NaN: a read outside the image would show
    bx, by = (torch.full((3, H, W + 5), float("nan"), device=DEV) for _ in range(2))
    vx, vy = bx[:, :, :W], by[:, :, :W]
    vx.copy_(a.to(DEV))
    vy.copy_(b.to(DEV))
    assert not vx.is_contiguous()
    assert float(spnerf_amd.lpips(vx, vy, weights(), layout="chw")) == flat
    pre = float(spnerf_amd.lpips(2 * hwc(a) - 1, 2 * hwc(b) - 1, weights(), hw=(H, W), normalize=False))
    assert rel(pre, flat) <= 1e-6 and rel(pre, score) <= SCORE_TOL
    with pytest.raises(ValueError, match="channels, not 3"):
        spnerf_amd.lpips(torch.zeros(H, W, 4, device=DEV), torch.zeros(H, W, 4, device=DEV), weights())
    with pytest.raises(ValueError, match="needs hw"):
        spnerf_amd.lpips(hwc(a), hwc(b), weights())


def test_nan_pixel_gives_nan():
    H, W = 35, 47
    a, b, *_ = case(H, W)
    bad = hwc(a).clone()
    bad[17 * W + 20, 1] = float("nan")
    s, layers = spnerf_amd.lpips(bad, hwc(b), weights(), hw=(H, W), return_layers=True)
    assert np.isnan(float(s)) and bool(torch.isnan(layers).all())
    assert np.isnan(float(spnerf_amd.lpips(hwc(b), bad, weights(), hw=(H, W))))
    assert np.isfinite(float(spnerf_amd.lpips(hwc(a), hwc(b), weights(), hw=(H, W))))     # and nothing is left behind


def test_argument_errors():
    w = weights()
    small = torch.rand(30 * 40, 3, device=DEV)
    with pytest.raises(_lib.SpnerfError, match="image 30 x 40 smaller than 31"):
        spnerf_amd.lpips(small, small, w, hw=(30, 40))
    L = _lpips_lib.lib()
    H, W = 35, 47
    x = torch.rand(H * W, 3, device=DEV)
    least = perceptual.workspace_bytes(H, W, 1)
    ws = torch.empty(least, dtype=torch.uint8, device=DEV)
    res = torch.full((11,), -7.0, dtype=torch.float64, device=DEV)
    rc = L.spnerf_lpips(_lib.ptr(x), _lib.ptr(x), H, W, 1, 3 * W, 3, 1, _lib.ptr(w.packed), _lib.ptr(ws), least - 16, None,
                        _lib.ptr(res), _lib.stream_of(x))
    assert rc == -1 and b"too small" in L.spnerf_last_error()
    torch.cuda.synchronize()
    assert bool((res == -7).all())                       # refused before any launch
    with pytest.raises(ValueError, match="weights on"):
        perceptual.launch_lpips(x, x, H, W, (1, 3 * W, 3), True, perceptual.LpipsWeights(w.packed.cpu()), res.data_ptr())
    with pytest.raises(TypeError, match="LpipsWeights"):
        spnerf_amd.lpips(x, x, None, hw=(H, W))


def test_result_struct_and_state_dict_weights():
    H, W = 35, 47
    a, b, score, layers, *_ = case(H, W)
    w2 = spnerf_amd.LpipsWeights.from_state_dict(lt.package_state_dict(lt.seeded_weights()), DEV)
    tv, lin = lt.split_state_dicts(lt.seeded_weights())
    w3 = spnerf_amd.LpipsWeights.from_state_dict(tv, DEV, lin_sd=lin)
    assert torch.equal(w2.packed, weights().packed) and torch.equal(w3.packed, weights().packed)
    x, y = hwc(a), hwc(b)
    res = torch.zeros(11, dtype=torch.float64, device=DEV)
    perceptual.launch_lpips(x, y, H, W, (1, 3 * W, 3), True, w2, res.data_ptr())
    host = _lpips_lib.LpipsResult.from_buffer_copy(res.cpu().numpy().tobytes())
    assert ctypes.sizeof(host) == res.numel() * 8
    assert list(zip(host.h, host.w)) == perceptual.tap_sizes(H, W) == [(8, 11), (3, 5), (1, 2), (1, 2), (1, 2)]
    assert rel(host.lpips, score) <= SCORE_TOL and all(rel(host.layer[l], layers[l]) <= SCORE_TOL for l in range(5))


def test_view_metrics_scores_lpips_in_the_same_copy():
    H, W = 35, 47
    a, b, score, layers, *_ = case(H, W)
    rgb, tgt = hwc(a), hwc(b)
    old = spnerf_amd.view_metrics(rgb, tgt, hw=(H, W))
    assert "lpips" not in old and "lpips_layers" not in old
    got = spnerf_amd.view_metrics({"rgb": rgb}, tgt, hw=(H, W), lpips=weights())
    assert sorted(got) == sorted(list(old) + ["lpips", "lpips_layers"])
    for k, v in old.items():
        assert np.array_equal(got[k], v), k
    direct, direct_layers = spnerf_amd.lpips(rgb, tgt, weights(), hw=(H, W), return_layers=True)
    assert got["lpips"] == float(direct) and got["lpips_layers"] == direct_layers.tolist()
    assert rel(got["lpips"], score) <= SCORE_TOL
    chw = spnerf_amd.view_metrics(rgb, tgt, hw=(H, W), ssim_layout="chw", lpips=weights())
    assert chw["lpips"] == float(spnerf_amd.lpips(rgb.view(3, H, W), tgt.view(3, H, W), weights(), layout="chw"))
    with pytest.raises(ValueError, match="needs hw"):
        spnerf_amd.view_metrics(rgb, tgt, lpips=weights())
