"""SSIM on the GPU (csrc/ssim.hip, spnerf_amd.image) — needs an MI355X.

Everything is compared with the float64 restatement tests/ssim_numpy.py on the same fp32 inputs,
map and mean within 1e-9 absolute: the kernel evaluates the same formula in fp64 in another
order, the worst-case fp64 rounding of a 121-tap moment is about 1.3e-14, and divided by
C2 = 9e-4 that is about 1.5e-11 — the bound leaves about 60x, and is the one the fp64 NCC tables of
the DSM registration are held to.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import spnerf_amd
import ssim_numpy as sn
from spnerf_amd import _image_lib, image

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = 1e-9
# (H, W, ws): the two smallest legal shapes (every tap mirrors), one tile row of many tile columns,
# a partial last tile in either axis and in both, the view fixture's 12 x 10, and 17 x 17 tiles:
# more tile sums per channel than the finish has threads
SHAPES = [(2, 2, 3), (6, 6, 11), (3, 200, 3), (31, 33, 5), (33, 31, 7), (65, 70, 11), (12, 10, 3), (272, 530, 9)]


@functools.lru_cache(maxsize=None)
def case(C, H, W, ws):
    """(x, y, map of the restatement) for one shape: fp32 (C, H, W) images, computed once."""
    g = np.random.default_rng(1000 * H + 10 * W + ws + C)
    yy, xx = np.mgrid[0:H, 0:W]
    x = np.stack([0.5 + 0.4 * np.sin(0.3 * xx + 0.2 * yy + c) * np.cos(0.11 * yy - c) for c in range(C)])
    x = np.clip(x + 0.05 * g.standard_normal(x.shape), 0, 1).astype(np.float32)
    y = np.clip(x + 0.1 * g.standard_normal(x.shape) * (xx > W // 3), 0, 1).astype(np.float32)   # a third of it identical
    ref = sn.ssim_map(x, y, ws)
    for a in (x, y, ref):
        a.setflags(write=False)
    return x, y, ref


def device_images(x, y, layout):
    """The images as the caller of that layout holds them, and the keywords that say so."""
    C, H, W = x.shape
    if layout == "chw":
        return torch.tensor(x, device=DEV)[None], torch.tensor(y, device=DEV)[None], {}
    flat = lambda a: torch.tensor(np.ascontiguousarray(a.transpose(1, 2, 0)).reshape(H * W, C), device=DEV)   # noqa: E731
    return flat(x), flat(y), dict(layout="hwc", hw=(H, W))


@pytest.mark.parametrize("layout", ["chw", "hwc"])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("H,W,ws", SHAPES)
def test_ssim_matches_restatement(H, W, ws, C, layout):
    x, y, ref = case(C, H, W, ws)
    tx, ty, kw = device_images(x, y, layout)
    score, smap = spnerf_amd.ssim(tx, ty, window_size=ws, return_map=True, **kw)
    assert score.dtype == torch.float64 and score.dim() == 0 and score.is_cuda
    assert smap.dtype == torch.float64 and tuple(smap.shape) == (C, H, W)
    err_map = float(np.abs(smap.cpu().numpy() - ref).max())
    err = abs(float(score) - float(ref.mean()))
    print(f"({C},{H},{W}) ws {ws} {layout}: map {err_map:.2e} mean {err:.2e} (ssim {float(score):.6f})")
    assert err_map <= TOL and err <= TOL
    alone = spnerf_amd.ssim(tx, ty, window_size=ws, **kw)           # map = NULL: the same bits
    assert float(alone) == float(score)
    again = spnerf_amd.ssim(tx, ty, window_size=ws, **kw)           # two calls bit-equal
    assert float(again) == float(alone)


@pytest.mark.parametrize("layout", ["chw", "hwc"])
@pytest.mark.parametrize("H,W,ws", [(6, 6, 11), (33, 31, 7), (65, 70, 11)])
def test_padded_rows_are_not_read(H, W, ws, layout):
    """A row stride larger than the row, the gaps NaN: a read outside the image would show."""
    C = 3
    x, y, ref = case(C, H, W, ws)
    pad = 5
    if layout == "chw":
        bx, by = (torch.full((C, H, W + pad), float("nan"), device=DEV) for _ in range(2))
        vx, vy = bx[:, :, :W], by[:, :, :W]
        vx.copy_(torch.tensor(x, device=DEV))
        vy.copy_(torch.tensor(y, device=DEV))
        kw = {}
    else:
        bx, by = (torch.full((H, W + pad, C), float("nan"), device=DEV) for _ in range(2))
        vx, vy = bx[:, :W], by[:, :W]
        vx.copy_(torch.tensor(x, device=DEV).permute(1, 2, 0))
        vy.copy_(torch.tensor(y, device=DEV).permute(1, 2, 0))
        kw = dict(layout="hwc")
    assert not vx.is_contiguous() and bool(torch.isnan(bx).any())
    score, smap = spnerf_amd.ssim(vx, vy, window_size=ws, return_map=True, **kw)
    tx, ty, kw2 = device_images(x, y, layout)
    dense, dmap = spnerf_amd.ssim(tx, ty, window_size=ws, return_map=True, **kw2)
    assert np.isfinite(float(score)) and bool(torch.isfinite(smap).all())
    assert float(score) == float(dense) and torch.equal(smap, dmap)
    assert abs(float(score) - float(ref.mean())) <= TOL


@pytest.mark.parametrize("H,W,ws", [(2, 2, 3), (33, 31, 7), (65, 70, 11)])
def test_map_stays_inside_its_buffer(H, W, ws):
    C = 3
    x, y, ref = case(C, H, W, ws)
    tx, ty = torch.tensor(x, device=DEV), torch.tensor(y, device=DEV)
    n, guard = C * H * W, 64
    buf = torch.full((n + 2 * guard,), -7.0, dtype=torch.float64, device=DEV)
    res = torch.zeros(6, dtype=torch.float64, device=DEV)
    image.launch_ssim(tx, ty, C, H, W, tx.stride(), ws, 1.0, res.data_ptr(), buf[guard:guard + n])
    assert bool((buf[:guard] == -7).all()) and bool((buf[guard + n:] == -7).all())
    got = buf[guard:guard + n].view(C, H, W).cpu().numpy()
    assert float(np.abs(got - ref).max()) <= TOL
    host = _image_lib.SsimResult.from_buffer_copy(res.cpu().numpy().tobytes())
    assert host.n == n and abs(host.ssim - float(ref.mean())) <= TOL
    for c in range(4):
        want = float(ref[c].mean()) if c < C else 0.0
        assert abs(host.channel_mean[c] - want) <= TOL, c
    assert ctypes.sizeof(host) == res.numel() * 8


def test_nan_pixel_gives_nan_and_max_val_scales():
    x, y, ref = case(3, 31, 33, 5)
    tx, ty = torch.tensor(x, device=DEV)[None], torch.tensor(y, device=DEV)[None]
    bad = tx.clone()
    bad[0, 1, 17, 20] = float("nan")
    assert np.isnan(float(spnerf_amd.ssim(bad, ty, window_size=5)))
    assert np.isnan(float(spnerf_amd.ssim(ty, bad, window_size=5)))
    # the same images on a 255 scale with max_val 255: the formula is homogeneous but for its eps
    s255 = float(spnerf_amd.ssim(tx * 255, ty * 255, window_size=5, max_val=255.0))
    ref255 = sn.ssim(x.astype(np.float32) * np.float32(255), y.astype(np.float32) * np.float32(255), 5, 255.0)
    assert abs(s255 - ref255) <= TOL
    with pytest.raises(ValueError, match="one image at a time"):
        spnerf_amd.ssim(torch.cat([tx, tx]), torch.cat([ty, ty]))
    with pytest.raises(spnerf_amd._lib.SpnerfError, match="window size 4"):
        spnerf_amd.ssim(tx, ty, window_size=4)


# ---- view integration -----------------------------------------------------------------------------

@pytest.mark.parametrize("case_name", ["a", "b", "c"])
def test_view_metrics_scores_ssim_in_the_same_copy(case_name):
    from test_gpu_view import render_case
    d, planes, m = render_case(case_name)
    C = d["meta"]["dims"]["num_sem_classes"]
    rgb = torch.tensor(planes["rgb"], device=DEV)
    tgt = torch.tensor(d["target"], device=DEV)
    sem, lab = torch.tensor(planes["sem_class"], device=DEV), torch.tensor(d["labels"], device=DEV)
    old = spnerf_amd.view_metrics(rgb, tgt, sem, lab, C)                 # without hw: what it returned before
    assert sorted(old) == sorted(m) == ["confusion", "correct", "miou", "mse", "n", "oa", "psnr"]
    hw = (12, 10)
    flat_tgt = d["target"].reshape(-1, 3)
    for layout in ("hwc", "chw"):
        got = spnerf_amd.view_metrics(rgb, tgt, sem, lab, C, hw=hw, ssim_layout=layout)
        assert sorted(got) == sorted(list(old) + ["ssim", "ssim_channels"])
        for k, v in old.items():
            assert np.array_equal(got[k], v) and np.array_equal(m[k], v), k
        ref = sn.ssim_map(sn.chw_of(planes["rgb"], hw, layout), sn.chw_of(flat_tgt, hw, layout), 3)
        print(case_name, layout, got["ssim"], float(ref.mean()))
        assert abs(got["ssim"] - float(ref.mean())) <= TOL
        assert len(got["ssim_channels"]) == 3
        assert all(abs(got["ssim_channels"][c] - float(ref[c].mean())) <= TOL for c in range(3))
    # the training loop's call, main.py:261: the (H * W, 3) render viewed as (1, 3, H, W)
    direct = spnerf_amd.ssim(rgb.view(1, 3, *hw), tgt.reshape(-1, 3).view(1, 3, *hw))
    assert float(direct) == got["ssim"]
    # and eval.py:393's: the permuted image, through strides or as the flat plane
    hwc = spnerf_amd.view_metrics(rgb, tgt, hw=hw)["ssim"]
    assert float(spnerf_amd.ssim(rgb.view(*hw, 3).permute(2, 0, 1), tgt.view(*hw, 3).permute(2, 0, 1))) == hwc
    assert float(spnerf_amd.ssim(rgb, tgt.reshape(-1, 3), layout="hwc", hw=hw)) == hwc
    with pytest.raises(ValueError, match="is not the view's 120 rays"):
        spnerf_amd.view_metrics(rgb, tgt, hw=(10, 10))
