"""A photo-consistency DSM on the ground grid from the camera images alone (csrc/sweep.hip,
include/spnerf_amd_sweep.h).

``render_ortho``, ``cast_shadows`` and ``orthorectify`` all take a DSM; ``plane_sweep`` makes one
without a trained network: for K horizontal planes every view is put on the grid at that altitude,
the views are scored against each other around each cell — the mean pairwise zero-normalised
cross-correlation of their grey windows — and the best plane per cell is kept, refined by a parabola
through its two neighbours.  The header states every operation and its order; ``plane_grey``,
``window_score`` and ``pick_plane`` are the three steps on their own, and the fused call has their
bytes.  Occlusion is not modelled, as in any plane sweep; ``occlusion.visible_sweep`` is this sweep with the
views gated by a visibility floor from a prior DSM.

Conventions are ``rectify``'s: cameras are ``rectify.Camera``s, an image is a device tensor
(h, w, C) float32 with C <= 4, the planes lie in the ``GroundGrid`` layout (row 0 the northernmost).
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib, _sweep_lib
from ._ground import (_camera_table, _check_cameras, _check_grid, _check_images, _check_int, _check_real, _grid_struct, _image_table,
                      _one_device, _pick_planes, _what)

MIN_VIEWS = _sweep_lib.SWEEP_MIN_VIEWS
MAX_VIEWS = _sweep_lib.SWEEP_MAX_VIEWS
MAX_PLANES = _sweep_lib.SWEEP_MAX_PLANES
MAX_RADIUS = _sweep_lib.SWEEP_MAX_RADIUS


# ---- argument checks: everything below is decided on the host, before any device is touched ------

def _check_view_count(n):
    if not MIN_VIEWS <= n <= MAX_VIEWS:
        raise ValueError(f"{n} views in one sweep ({MIN_VIEWS} to {MAX_VIEWS})")


def _check_planes(alt_lo, step, planes):
    return (_check_real("alt_lo", alt_lo, "finite", lambda x: True), _check_real("step", step, "finite and > 0", lambda x: x > 0),
            _check_int("planes", planes, 1, MAX_PLANES))


def _check_window(n_views, radius, min_views, min_std):
    return (_check_int("radius", radius, 1, MAX_RADIUS), _check_int("min_views", min_views, 2, n_views),
            _check_real("min_std", min_std, "finite and >= 0", lambda x: x >= 0))


def _check_scene(images, cameras, grid):
    cams = _check_cameras(cameras)
    _check_view_count(len(cams))
    imgs = _check_images(images, len(cams), cams)
    return cams, imgs, _check_grid(grid)


# ---- the steps ----------------------------------------------------------------------------------------

def plane_grey(images, cameras, grid, alt):
    """``grey`` (V, H, W) float32 and ``valid`` (V, H, W) uint8: every view on ``grid`` at the altitude
    ``alt``, its channels averaged (in fp64, cast once).  ``valid`` is 1 where the bilinear read lies
    inside the image and the grey is finite; ``grey`` is NaN where the read does not."""
    cams, imgs, grid = _check_scene(images, cameras, grid)
    alt = _check_real("alt", alt, "finite", lambda x: True)
    dev = _one_device(*imgs)
    L = _sweep_lib.lib()
    V, (H, W), C = len(cams), grid.shape, imgs[0].shape[2]
    cam_table = _camera_table(cams, dev)
    img_table, imgs = _image_table(imgs, dev)
    grey = torch.empty((V, H, W), dtype=torch.float32, device=dev)
    valid = torch.empty((V, H, W), dtype=torch.uint8, device=dev)
    _lib.check(L.spnerf_sweep_grey(ctypes.byref(_grid_struct(grid)), _lib.ptr(cam_table), _lib.ptr(img_table), V, C, alt, _lib.ptr(grey),
                                   _lib.ptr(valid), _lib.stream_of(grey)), "sweep_grey")
    return grey, valid


def window_score(grey: torch.Tensor, valid: torch.Tensor, *, radius=2, min_views=2, min_std=0.0):
    """``score`` (H, W) float32 and ``views`` (H, W) uint8 of one plane from its ``grey`` (V, H, W)
    float32 and ``valid`` (V, H, W) uint8 (1 counts).  A view is usable at a cell when it is valid
    at every in-grid cell of the (2·radius + 1)² window, the window holds at least 2 cells, and its
    window greys have a sum of squared deviations above cells·min_std²; ``views`` counts them, and with
    fewer than ``min_views`` the score is NaN, else the mean pairwise ZNCC of the usable views."""
    if not isinstance(grey, torch.Tensor) or grey.dim() != 3 or grey.numel() == 0 or grey.dtype != torch.float32:
        raise ValueError(f"grey must be a non-empty (V, H, W) float32 tensor, got {_what(grey)}")
    _check_view_count(grey.shape[0])
    if not isinstance(valid, torch.Tensor) or valid.dtype != torch.uint8 or tuple(valid.shape) != tuple(grey.shape):
        raise ValueError(f"valid must be a {tuple(grey.shape)} uint8 tensor, got {_what(valid)}")
    radius, min_views, min_std = _check_window(grey.shape[0], radius, min_views, min_std)
    dev = _one_device(grey, valid)
    L = _sweep_lib.lib()
    grey, valid = grey.contiguous(), valid.contiguous()
    V, H, W = grey.shape
    score = torch.empty((H, W), dtype=torch.float32, device=dev)
    views = torch.empty((H, W), dtype=torch.uint8, device=dev)
    _lib.check(L.spnerf_sweep_score(_lib.ptr(grey), _lib.ptr(valid), V, H, W, radius, min_views, min_std, _lib.ptr(score),
                                    _lib.ptr(views), _lib.stream_of(grey)), "sweep_score")
    return score, views


def pick_plane(volume: torch.Tensor, views: torch.Tensor, alt_lo, step) -> dict:
    """The best plane per cell of a score ``volume`` (K, H, W) float32 with its usable-view counts
    ``views`` (K, H, W) uint8, plane k at ``alt_lo + k·step``: ``index`` (H, W) int32, the lowest plane
    with the largest non-NaN score, −1 where there is none; ``altitude`` (H, W) float32, that plane's
    moved by up to half a step to the vertex of the parabola through its two neighbours; ``score`` and
    ``views`` at ``index`` (NaN and 0 at −1)."""
    if not isinstance(volume, torch.Tensor) or volume.dim() != 3 or volume.numel() == 0 or volume.dtype != torch.float32:
        raise ValueError(f"volume must be a non-empty (K, H, W) float32 tensor, got {_what(volume)}")
    if not isinstance(views, torch.Tensor) or views.dtype != torch.uint8 or tuple(views.shape) != tuple(volume.shape):
        raise ValueError(f"views must be a {tuple(volume.shape)} uint8 tensor, got {_what(views)}")
    alt_lo, step, K = _check_planes(alt_lo, step, volume.shape[0])
    dev = _one_device(volume, views)
    L = _sweep_lib.lib()
    volume, views = volume.contiguous(), views.contiguous()
    _, H, W = volume.shape
    out = _pick_planes(H, W, dev)
    _lib.check(L.spnerf_sweep_pick(_lib.ptr(volume), _lib.ptr(views), K, H * W, alt_lo, step, _lib.ptr(out["altitude"]),
                                   _lib.ptr(out["score"]), _lib.ptr(out["index"]), _lib.ptr(out["views"]), _lib.stream_of(volume)),
               "sweep_pick")
    return out


def plane_sweep(images, cameras, grid, alt_lo, step, planes, *, radius=2, min_views=2, min_std=0.0, volume=False) -> dict:
    """Sweep ``planes`` horizontal planes, ``alt_lo + k·step``, over ``grid`` and keep the most
    photo-consistent one per cell: one launch, with the bytes of ``plane_grey``, ``window_score`` per
    plane and ``pick_plane``, but no cost volume in memory.

    Returns a dict of (H, W) device tensors: ``altitude`` float32 (NaN where no plane could be scored),
    ``score`` float32 (the mean pairwise ZNCC at the chosen plane), ``index`` int32 (−1 where none) and
    ``views`` uint8 (the views that took part); with ``volume=True`` also ``volume`` (K, H, W) float32,
    every plane's score.  ``orthorectify(images, cameras, out["altitude"].double(), grid, ...)`` gives the
    true orthophoto of the swept DSM, ``cast_shadows`` its shadows."""
    cams, imgs, grid = _check_scene(images, cameras, grid)
    alt_lo, step, K = _check_planes(alt_lo, step, planes)
    radius, min_views, min_std = _check_window(len(cams), radius, min_views, min_std)
    dev = _one_device(*imgs)
    L = _sweep_lib.lib()
    V, (H, W), C = len(cams), grid.shape, imgs[0].shape[2]
    cam_table = _camera_table(cams, dev)
    img_table, imgs = _image_table(imgs, dev)
    out = _pick_planes(H, W, dev, K if volume else None)
    _lib.check(L.spnerf_sweep(ctypes.byref(_grid_struct(grid)), _lib.ptr(cam_table), _lib.ptr(img_table), V, C, alt_lo, step, K, radius,
                              min_views, min_std, _lib.ptr(out["altitude"]), _lib.ptr(out["score"]), _lib.ptr(out["index"]),
                              _lib.ptr(out["views"]), _lib.ptr(out.get("volume")), _lib.stream_of(out["altitude"])), "sweep")
    return out
