"""Camera images on the ground grid (csrc/rectify.hip, include/spnerf_amd_rectify.h).

``render_ortho`` puts what the model learnt on the lidar ROI grid and ``cast_shadows`` casts that
DSM geometrically; ``orthorectify`` puts the data there: every cell centre, at its DSM altitude,
goes through the inverse transverse Mercator projection and a camera's RPC projection to a pixel
position, and the image is read there bilinearly.  With it an ortho product can be held against the
pixels it was trained on, a DSM checked for photo-consistency across views (``mosaic``'s "spread"),
and the true orthophoto of the source imagery made: the occlusion mask is ``cast_shadows`` with
the camera's line of sight (``view_directions``) in place of the sun's.

Conventions: a camera is an ``RPCModel`` plus an image downscale, rescaled as ``image_rays``
rescales it; pixel (col, row) with whole coordinates is the sample position of that pixel, as in
``get_rays(cols, rows, ...)``; an image is a device tensor (h, w, C) float32 with C <= 4, and the
images of one call may differ in size; the DSM lies in the ``GroundGrid`` layout (row 0 the
northernmost).  Geometry is fp64 throughout.
"""
from __future__ import annotations

import ctypes
import dataclasses
import math
import numbers

import numpy as np
import torch

from . import _lib, _rectify_lib
from ._ground import (_camera_table, _check_alts, _check_cameras, _check_dsm, _check_grid, _check_images, _grid_struct, _image_table,
                      _require_cuda, _require_one_device, _what)
from .ortho import GroundGrid
from .satellite import RPCModel, rescale_rpc

MAX_VIEWS = _rectify_lib.RECTIFY_MAX_VIEWS
MAX_CHANNELS = _rectify_lib.RECTIFY_MAX_CHANNELS
MODES = {"mean": _rectify_lib.RECTIFY_MEAN, "median": _rectify_lib.RECTIFY_MEDIAN}
HIDDEN, VISIBLE, NODATA = 0, 1, 255   # the values of "visible"


@dataclasses.dataclass(frozen=True)
class Camera:
    """An RPC camera and the downscale of its image: the model is rescaled as ``image_rays`` rescales
    it, ``rescale_rpc(rpc, 1 / downscale)``.  ``shape`` is the (h, w) its image must have, where known."""
    rpc: RPCModel
    downscale: float = 1.0
    shape: tuple | None = None

    def __post_init__(self):
        if not isinstance(self.rpc, RPCModel):
            raise ValueError(f"Camera: rpc must be an RPCModel, got {type(self.rpc).__name__}")
        ds = self.downscale
        if not isinstance(ds, numbers.Real) or isinstance(ds, bool) or not (math.isfinite(ds) and ds > 0):
            raise ValueError(f"Camera: downscale {ds!r} must be positive")
        object.__setattr__(self, "downscale", float(ds))
        if self.shape is not None:
            object.__setattr__(self, "shape", (int(self.shape[0]), int(self.shape[1])))

    @classmethod
    def from_meta(cls, meta: dict, img_downscale: float = 1.0):
        """The camera of one image's metadata (its "rpc", "height" and "width"), sized as ``image_rays``
        sizes the image: (height // img_downscale, width // img_downscale)."""
        return cls(RPCModel(meta["rpc"]), img_downscale,
                   (int(meta["height"] // img_downscale), int(meta["width"] // img_downscale)))

    def packed(self) -> np.ndarray:
        """The 90 doubles of the rescaled model, in the C ABI's order."""
        return np.array(list(rescale_rpc(self.rpc, 1.0 / self.downscale).packed()), np.float64)


# ---- argument checks: everything below is decided on the host, before any device is touched ------

def _check_mode(mode):
    if mode not in MODES:
        raise ValueError(f"mosaic mode {mode!r} is neither 'mean' nor 'median'")
    return MODES[mode]


# ---- the steps ----------------------------------------------------------------------------------------

def project_cells(dsm: torch.Tensor, grid: GroundGrid, cameras) -> torch.Tensor:
    """``pix`` (V, H, W, 2) float64 on the device: [col, row] of every cell centre of ``grid`` at its
    altitude ``dsm`` (H, W) in each of ``cameras``; NaN where the DSM is NaN.  The inverse projection of
    a cell is computed once for all views."""
    cams = _check_cameras(cameras)
    _check_dsm("dsm", dsm, grid)
    dev = _require_one_device(dsm)
    L = _rectify_lib.lib()
    dsm = dsm.double().contiguous()
    table = _camera_table(cams, dev)
    pix = torch.empty((len(cams),) + grid.shape + (2,), dtype=torch.float64, device=dev)
    _lib.check(L.spnerf_rectify_project(_lib.ptr(dsm), ctypes.byref(_grid_struct(grid)), _lib.ptr(table), len(cams), _lib.ptr(pix),
                                        _lib.stream_of(dsm)), "rectify_project")
    return pix


def sample_images(images, pix: torch.Tensor):
    """Read image v at ``pix[v]``: ``images`` are V device tensors (h, w, C) float32, ``pix`` is
    (V, H, W, 2) float64 [col, row].  Returns ``rgb`` (V, H, W, C) float32 and ``valid`` (V, H, W) uint8.
    A cell is valid when its position is finite and inside the image, 0 <= col <= w − 1 and
    0 <= row <= h − 1; its value is the bilinear read in fp64 (include/spnerf_amd_rectify.h states the
    order), cast once.  An invalid cell is NaN in every channel."""
    imgs = _check_images(images)
    if not isinstance(pix, torch.Tensor) or pix.dim() != 4 or pix.shape[3] != 2 or pix.numel() == 0 or pix.dtype != torch.float64:
        raise ValueError(f"pix must be a non-empty (V, H, W, 2) float64 tensor, got {_what(pix)}")
    if pix.shape[0] != len(imgs):
        raise ValueError(f"{len(imgs)} images for {pix.shape[0]} views")
    dev = _require_one_device(pix, *imgs)
    L = _rectify_lib.lib()
    V, H, W, C = len(imgs), pix.shape[1], pix.shape[2], imgs[0].shape[2]
    pix = pix.contiguous()
    table, imgs = _image_table(imgs, dev)
    rgb = torch.empty((V, H, W, C), dtype=torch.float32, device=dev)
    valid = torch.empty((V, H, W), dtype=torch.uint8, device=dev)
    _lib.check(L.spnerf_rectify_sample(_lib.ptr(table), V, C, _lib.ptr(pix), H * W, _lib.ptr(rgb), _lib.ptr(valid),
                                       _lib.stream_of(pix)), "rectify_sample")
    return rgb, valid


def view_directions(grid: GroundGrid, cameras, alt_lo, alt_hi, device="cuda"):
    """One line of sight per camera over ``grid``, in the form ``cast_shadows`` takes: ``dirs`` (V, 3)
    float32 (east, north, up) from the ground towards the camera, up > 0, and ``spread`` (V,) float32,
    both on ``device``.  At the grid's centre the point at ``alt_lo`` is projected into the camera, that
    pixel localised at ``alt_hi`` and brought back to UTM; the difference, normalised, is the direction.
    ``spread`` is the largest component difference between the same vector at any of the four grid
    corners and the centre's: times the scene's altitude range it bounds, in metres, what one direction
    per view displaces."""
    cams = _check_cameras(cameras)
    _check_grid(grid)
    alt_lo, alt_hi = _check_alts(alt_lo, alt_hi)
    dev = _require_cuda(device)
    L = _rectify_lib.lib()
    table = _camera_table(cams, dev)
    dirs = torch.empty((len(cams), 3), dtype=torch.float32, device=dev)
    spread = torch.empty(len(cams), dtype=torch.float32, device=dev)
    _lib.check(L.spnerf_rectify_view_dirs(ctypes.byref(_grid_struct(grid)), _lib.ptr(table), len(cams), alt_lo, alt_hi, _lib.ptr(dirs),
                                          _lib.ptr(spread), _lib.stream_of(dirs)), "rectify_view_dirs")
    return dirs, spread


def mosaic(rgb: torch.Tensor, usable: torch.Tensor, mode: str = "median"):
    """Combine the views of every cell: ``rgb`` (V, H, W, C) float32, ``usable`` (V, H, W) uint8 (1
    counts).  Returns ``mosaic_rgb`` (H, W, C) float32 — per channel the ``"mean"`` or the
    ``"median"`` (an even count: the mean of the two middle values) of the usable views, accumulated in
    fp64 in view order and cast once — ``count`` (H, W) int32, and ``spread`` (H, W) float32: the RMS
    deviation from the per-channel mean over the usable views and the channels, 0 for a count of 1.
    A cell no view can use is NaN in both float planes."""
    if (not isinstance(rgb, torch.Tensor) or rgb.dim() != 4 or rgb.numel() == 0 or rgb.dtype != torch.float32
            or rgb.shape[0] > MAX_VIEWS or rgb.shape[3] > MAX_CHANNELS):
        raise ValueError(f"rgb must be a non-empty (V, H, W, C) float32 tensor with V <= {MAX_VIEWS} and C <= {MAX_CHANNELS}, got {_what(rgb)}")
    if not isinstance(usable, torch.Tensor) or usable.dtype != torch.uint8 or tuple(usable.shape) != tuple(rgb.shape[:3]):
        raise ValueError(f"usable must be a {tuple(rgb.shape[:3])} uint8 tensor, got {_what(usable)}")
    code = _check_mode(mode)
    dev = _require_one_device(rgb, usable)
    L = _rectify_lib.lib()
    rgb, usable = rgb.contiguous(), usable.contiguous()
    V, H, W, C = rgb.shape
    out = torch.empty((H, W, C), dtype=torch.float32, device=dev)
    count = torch.empty((H, W), dtype=torch.int32, device=dev)
    spread = torch.empty((H, W), dtype=torch.float32, device=dev)
    _lib.check(L.spnerf_rectify_mosaic(_lib.ptr(rgb), _lib.ptr(usable), V, H * W, C, code, _lib.ptr(out), _lib.ptr(count),
                                       _lib.ptr(spread), _lib.stream_of(rgb)), "rectify_mosaic")
    return out, count, spread


_mosaic_views = mosaic   # orthorectify's keyword has the function's name


def orthorectify(images, cameras, dsm: torch.Tensor, grid: GroundGrid, alt_lo, alt_hi, *, occlusion=True, mosaic=None,
                 pix=False) -> dict:
    """Put the V camera images ``images`` on ``grid`` over the (H, W) device DSM ``dsm`` — float64, or
    float32 widened as ``cast_shadows`` widens it.  One launch projects every cell into every camera
    and reads the images; the result has the bytes of ``sample_images(images, project_cells(...))``.

    Returns a dict of device tensors: ``rgb`` (V, H, W, C) float32 and ``valid`` (V, H, W) uint8 always.
    With ``occlusion``: ``visible`` (V, H, W) uint8 read off ``cast_shadows(dsm, grid, dirs)`` — 1
    visible, 0 hidden behind higher terrain, 255 where the DSM is NaN — with ``dirs`` (V, 3) and
    ``dir_spread`` (V,) of ``view_directions(grid, cameras, alt_lo, alt_hi)``: one line of sight per
    view, whose cost ``dir_spread`` bounds.  With ``mosaic="mean"`` or ``"median"``: ``mosaic_rgb``,
    ``count`` and ``spread`` of ``rectify.mosaic`` over the views with ``valid & (visible == 1)``, or
    ``valid`` alone without ``occlusion``.  With ``pix=True``: ``pix`` (V, H, W, 2) float64.

    No plane is copied to the host.  With ``occlusion`` the call synchronises with the host once: the V
    directions are copied there, because ``cast_shadows`` takes and checks them there — after the fused
    launch has been enqueued, so a camera whose line of sight comes out non-finite or with up <= 0 (a model
    that does not see the grid) raises ``cast_shadows``' ``ValueError`` only then."""
    cams = _check_cameras(cameras)
    imgs = _check_images(images, len(cams), cams)
    _check_dsm("dsm", dsm, grid)
    alt_lo, alt_hi = _check_alts(alt_lo, alt_hi)
    code = None if mosaic is None else _check_mode(mosaic)
    dev = _require_one_device(dsm, *imgs)
    L = _rectify_lib.lib()
    dsm = dsm.double().contiguous()
    V, (H, W), C = len(cams), grid.shape, imgs[0].shape[2]
    cam_table = _camera_table(cams, dev)
    img_table, imgs = _image_table(imgs, dev)
    out = {"rgb": torch.empty((V, H, W, C), dtype=torch.float32, device=dev),
           "valid": torch.empty((V, H, W), dtype=torch.uint8, device=dev)}
    if pix:
        out["pix"] = torch.empty((V, H, W, 2), dtype=torch.float64, device=dev)
    _lib.check(L.spnerf_rectify(_lib.ptr(dsm), ctypes.byref(_grid_struct(grid)), _lib.ptr(cam_table), _lib.ptr(img_table), V, C,
                                _lib.ptr(out["rgb"]), _lib.ptr(out["valid"]), _lib.ptr(out.get("pix")), _lib.stream_of(dsm)),
               "rectify")
    usable = out["valid"]
    if occlusion:
        from .shadow import cast_shadows
        out["dirs"], out["dir_spread"] = view_directions(grid, cams, alt_lo, alt_hi, device=dev)
        hidden = cast_shadows(dsm, grid, out["dirs"])
        out["visible"] = torch.where(hidden > 1, hidden, 1 - hidden)
        usable = usable & (out["visible"] == VISIBLE)
    if code is not None:
        out["mosaic_rgb"], out["count"], out["spread"] = _mosaic_views(out["rgb"], usable, mosaic)
    return out
