"""Image scores on the GPU: ``ssim``, the drop-in for the reference's ``metrics.ssim``
(modules/metrics.py:210-215, eval.py:120-125: ``kornia.losses.ssim(img1, img2, 3)`` of kornia
0.5.3, the mean of the SSIM map), evaluated in fp64 on the fp32 images by csrc/ssim.hip
(include/spnerf_amd_image.h).  Both memory layouts of the reference's two callers are the same
kernel through element strides: eval.py:393's permuted (3, H, W) image and main.py:261's
``.view(1, 3, H, W)`` of the (H·W, 3) render.
"""
from __future__ import annotations

import ctypes

import torch

from . import _image_lib, _lib

RESULT_BYTES = ctypes.sizeof(_image_lib.SsimResult)


def launch_ssim(x, y, C, H, W, strides, window_size, max_val, result_ptr, ssim_map=None) -> None:
    """``spnerf_image_ssim`` on the current stream of ``x``'s device: images ``x`` and ``y`` (fp32
    device tensors sharing the element strides ``(channel, row, pixel)``) into the
    ``spnerf_image_ssim_result`` at device address ``result_ptr``."""
    L = _image_lib.lib()
    nbytes = L.spnerf_image_ssim_workspace_bytes(C, H, W, int(window_size))
    if nbytes < 0:
        _lib.check(int(nbytes), "image_ssim_workspace_bytes")
    ws = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=x.device)
    _lib.check(L.spnerf_image_ssim(_lib.ptr(x), _lib.ptr(y), C, H, W, int(strides[0]), int(strides[1]), int(strides[2]),
                                   int(window_size), float(max_val), _lib.ptr(ws), _lib.ptr(ssim_map),
                                   ctypes.c_void_p(result_ptr), _lib.stream_of(x)), "image_ssim")


def _as_chw(t, layout, hw):
    """The (C, H, W) strided view of an image given as ``layout`` says (no copy)."""
    if layout == "chw":
        if t.dim() == 4:
            if t.shape[0] != 1:
                raise ValueError(f"ssim scores one image at a time, got a batch of {t.shape[0]}")
            t = t[0]
        if t.dim() != 3:
            raise ValueError(f"layout 'chw' takes a (1, C, H, W) or (C, H, W) image, got {tuple(t.shape)}")
        if hw is not None and tuple(hw) != tuple(t.shape[1:]):
            raise ValueError(f"hw {tuple(hw)} is not the image's {tuple(t.shape[1:])}")
        return t
    if layout == "hwc":
        if t.dim() == 2:
            if hw is None or int(hw[0]) * int(hw[1]) != t.shape[0]:
                raise ValueError(f"layout 'hwc' on {tuple(t.shape)} needs hw=(H, W) with H * W = {t.shape[0]}")
            t = t.as_strided((int(hw[0]), int(hw[1]), t.shape[1]), (int(hw[1]) * t.stride(0), t.stride(0), t.stride(1)),
                             t.storage_offset())
        if t.dim() != 3:
            raise ValueError(f"layout 'hwc' takes an (H * W, C) or (H, W, C) image, got {tuple(t.shape)}")
        if hw is not None and tuple(hw) != tuple(t.shape[:2]):
            raise ValueError(f"hw {tuple(hw)} is not the image's {tuple(t.shape[:2])}")
        return t.permute(2, 0, 1)
    raise ValueError(f"layout {layout!r} is neither 'chw' nor 'hwc'")


def ssim(pred, gt, window_size=3, max_val=1.0, layout="chw", hw=None, return_map=False):
    """``metrics.ssim(pred, gt)``: the mean over all C·H·W values of the SSIM map of kornia 0.5.3
    (Gaussian window of ``window_size`` with σ 1.5, reflect border, C1 = (0.01·max_val)², C2 =
    (0.03·max_val)², eps 1e-12), as a 0-dim float64 device tensor, without a host synchronisation.

    ``layout="chw"``: (1, C, H, W) or (C, H, W) images — the drop-in.  ``layout="hwc"``: (H, W, C)
    images, or with ``hw=(H, W)`` the (H·W, C) planes ``render_image`` returns, read in place
    through strides.  Strided views are read in place when both images share their strides;
    otherwise both are made contiguous first.  With ``return_map=True`` the result is
    ``(score, map)``, the map a (C, H, W) float64 device tensor."""
    _lib.require_device(pred, gt)
    if tuple(pred.shape) != tuple(gt.shape):
        raise ValueError(f"ssim: images of different shapes {tuple(pred.shape)} and {tuple(gt.shape)}")
    x = _as_chw(pred.float(), layout, hw)
    y = _as_chw(gt.to(pred.device).float(), layout, hw)
    if x.stride() != y.stride():
        x, y = x.contiguous(), y.contiguous()
    C, H, W = x.shape
    res = torch.empty(RESULT_BYTES // 8, dtype=torch.float64, device=x.device)
    ssim_map = torch.empty((C, H, W), dtype=torch.float64, device=x.device) if return_map else None
    launch_ssim(x, y, C, H, W, x.stride(), window_size, max_val, res.data_ptr(), ssim_map)
    return (res[0], ssim_map) if return_map else res[0]
