"""What the ground-grid modules share (ortho, shadow, rectify, sweep, sgm, occlusion, surface, dsm_view):
the argument checks, which are all decided on the host before any device is touched, and the tables the
kernels read in device memory.  The messages are part of each public function's contract
(tests/test_*_abi.py pin them); ``GroundGrid`` lives in ``ortho`` and ``Camera`` in ``rectify``, which
both import this module, so the two are looked up when a check runs."""
from __future__ import annotations

import math
import numbers

import numpy as np
import torch

from . import _lib, _rectify_lib
from ._ortho_lib import OrthoGrid

MAX_VIEWS = _rectify_lib.RECTIFY_MAX_VIEWS
MAX_CHANNELS = _rectify_lib.RECTIFY_MAX_CHANNELS


# ---- argument checks ------------------------------------------------------------------------------

def _what(t):
    return f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__


def _check_int(name, value, lo, hi):
    if not isinstance(value, numbers.Integral) or isinstance(value, bool) or not lo <= value <= hi:
        raise ValueError(f"{name} {value!r} must be an integer in {lo}..{hi}")
    return int(value)


def _check_real(name, value, what, ok):
    if not isinstance(value, numbers.Real) or isinstance(value, bool) or not math.isfinite(value) or not ok(value):
        raise ValueError(f"{name} {value!r} must be {what}")
    return float(value)


def _check_grid(grid):
    from .ortho import GroundGrid
    if not isinstance(grid, GroundGrid):
        raise ValueError(f"grid must be a GroundGrid, got {type(grid).__name__}")
    return grid


def _check_cameras(cameras):
    from .rectify import Camera
    cams = [cameras] if isinstance(cameras, Camera) else list(cameras)
    if not cams or len(cams) > MAX_VIEWS:
        raise ValueError(f"{len(cams)} cameras in one call (1 to {MAX_VIEWS})")
    for v, c in enumerate(cams):
        if not isinstance(c, Camera):
            raise ValueError(f"cameras[{v}] must be a rectify.Camera, got {type(c).__name__}")
    return cams


def _check_images(images, n_views=None, cameras=None):
    imgs = list(images) if isinstance(images, (list, tuple, torch.Tensor)) else None
    if not imgs or len(imgs) > MAX_VIEWS:
        raise ValueError(f"images must be 1 to {MAX_VIEWS} (h, w, C) tensors, got {type(images).__name__ if imgs is None else len(imgs)}")
    for v, im in enumerate(imgs):
        if (not isinstance(im, torch.Tensor) or im.dim() != 3 or im.numel() == 0 or im.dtype != torch.float32
                or im.shape[2] > MAX_CHANNELS):
            raise ValueError(f"images[{v}] must be a non-empty (h, w, C) float32 tensor with C <= {MAX_CHANNELS}, got {_what(im)}")
        if im.shape[2] != imgs[0].shape[2]:
            raise ValueError(f"images[{v}] has {im.shape[2]} channels, images[0] has {imgs[0].shape[2]}")
    if n_views is not None and len(imgs) != n_views:
        raise ValueError(f"{len(imgs)} images for {n_views} views")
    if cameras is not None:
        for v, (im, cam) in enumerate(zip(imgs, cameras)):
            if cam.shape is not None and tuple(im.shape[:2]) != cam.shape:
                raise ValueError(f"images[{v}] is {tuple(im.shape[:2])}, its camera's image is {cam.shape}")
    return imgs


def _check_alts(alt_lo, alt_hi):
    alt_lo, alt_hi = float(alt_lo), float(alt_hi)
    if not (math.isfinite(alt_lo) and math.isfinite(alt_hi) and alt_hi > alt_lo):
        raise ValueError(f"alt_hi {alt_hi} must be above alt_lo {alt_lo}")
    return alt_lo, alt_hi


_NO_GRID = object()   # "no grid to hold the DSM against"; None is a caller's bad grid and is refused as one


def _check_dsm(name, dsm, grid=_NO_GRID):
    """A DSM as the fp64 kernels take it, float64 or float32 (widened); with ``grid``, which must then be a
    GroundGrid, of its shape."""
    if not isinstance(dsm, torch.Tensor) or dsm.dim() != 2 or dsm.numel() == 0 or dsm.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{name} must be a non-empty (H, W) float64 or float32 tensor, got {_what(dsm)}")
    if grid is not _NO_GRID and tuple(dsm.shape) != _check_grid(grid).shape:
        raise ValueError(f"{name} {tuple(dsm.shape)} is not the grid's {grid.shape}")


def _check_raster(name, t, shape=None):
    """A float32 raster as the fp32 kernels take it; with ``shape``, of that shape."""
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.numel() == 0 or t.dtype != torch.float32:
        raise ValueError(f"{name} must be a non-empty (H, W) float32 tensor, got {_what(t)}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} {tuple(t.shape)} is not the grid's {tuple(shape)}")


def _resolution(resolution_or_grid, shape):
    from .ortho import GroundGrid
    if isinstance(resolution_or_grid, GroundGrid):
        if tuple(shape) != resolution_or_grid.shape:
            raise ValueError(f"dsm {tuple(shape)} is not the grid's {resolution_or_grid.shape}")
        return resolution_or_grid.resolution
    if not isinstance(resolution_or_grid, numbers.Real) or isinstance(resolution_or_grid, bool):
        raise ValueError(f"resolution_or_grid must be a GroundGrid or the cell size in metres, got {resolution_or_grid!r}")
    res = float(resolution_or_grid)
    if not (math.isfinite(res) and res > 0):
        raise ValueError(f"resolution {res} must be positive")
    return res


# ---- devices: the two rules differ in what a caller sees, and each keeps its callers -----------------

def _require_cuda(device):
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.SpnerfError(f"spnerf_amd runs the render path on the MI355X (HIP) only; got device {dev}.")
    return dev


def _require_one_device(*tensors):
    """rectify's rule: the GPU is required first, mixed devices are then a SpnerfError."""
    _lib.require_device(*tensors)
    if len({t.device for t in tensors}) != 1:
        raise _lib.SpnerfError(f"the tensors of one call must be on one device, got {sorted({str(t.device) for t in tensors})}")
    return tensors[0].device


def _one_device(*tensors):
    """The sweeps' rule: mixed devices are a ValueError, an argument error like the others; then the GPU is required."""
    devices = sorted({str(t.device) for t in tensors})
    if len(devices) != 1:
        raise ValueError(f"the tensors of one call must be on one device, got {devices}")
    _lib.require_device(*tensors)
    return tensors[0].device


# ---- the tables the kernels read, in device memory, and the planes they write ---------------------------

def _grid_struct(grid):
    return OrthoGrid(grid.xoff, grid.ytop, grid.resolution, grid.xsize, grid.ysize, grid.zone, 1 if grid.south else 0, 1)


def _camera_table(cams, device):
    return torch.from_numpy(np.stack([c.packed() for c in cams])).to(device)


def _image_table(imgs, device):
    """(table, images): the device table of spnerf_rectify_image and the contiguous images it points to."""
    imgs = [im.contiguous() for im in imgs]
    rows = (_rectify_lib.RectifyImage * len(imgs))(*[_rectify_lib.RectifyImage(im.data_ptr(), im.shape[0], im.shape[1]) for im in imgs])
    table = torch.frombuffer(bytearray(bytes(rows)), dtype=torch.uint8).to(device)
    return table, imgs


def _pick_planes(H, W, device, volume_planes=None):
    """The (H, W) planes a pick writes — altitude, score, index, views — and, for K = ``volume_planes``, the
    (K, H, W) score volume next to them."""
    out = {"altitude": torch.empty((H, W), dtype=torch.float32, device=device), "score": torch.empty((H, W), dtype=torch.float32, device=device),
           "index": torch.empty((H, W), dtype=torch.int32, device=device), "views": torch.empty((H, W), dtype=torch.uint8, device=device)}
    if volume_planes is not None:
        out["volume"] = torch.empty((volume_planes, H, W), dtype=torch.float32, device=device)
    return out
