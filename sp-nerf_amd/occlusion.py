"""The plane sweep with its views gated by a visibility floor from a prior DSM (csrc/occlusion.hip,
include/spnerf_amd_occlusion.h).

``plane_sweep`` lets every view take part in every cell's score, also a view that sees the cell's plane
position behind a building: next to a 16 m roof the four shipped cameras lose strips of ground 1.5 to
5.7 m wide, each on another side.  With a prior DSM — a first sweep's, the lidar's, ``render_ortho``'s,
any registered raster — ``visibility_floor`` marches it along every camera's line of sight (the march of
``cast_shadows``) and gives, per view and cell, the lowest altitude from which the camera is still seen;
``gate_plane`` takes the views below their floor out of one plane's stored greys, ``visible_sweep`` is
``plane_sweep`` with that gate at every plane in the same single launch, and ``refine_sweep`` is the
two-pass chain: ``smooth_sweep`` → ``view_directions`` → ``visibility_floor`` → ``visible_sweep`` →
``sgm.aggregate`` → ``sgm.pick``.  The header states every operation and its order; the fused call has
the bytes of ``plane_grey`` → ``gate_plane`` → ``window_score`` per plane → ``pick_plane``.

Not there: the aggregation stays occlusion-unaware (its penalties do not know the gate), the floor comes
from one line of sight per camera (``view_directions``' ``spread`` bounds what that displaces), and the
two passes are not iterated.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib, _occlusion_lib, sgm
from . import sweep as _sweep
from ._ground import _camera_table, _check_dsm, _check_int, _check_real, _grid_struct, _image_table, _one_device, _pick_planes, _resolution, _what
from .rectify import view_directions

MAX_VIEWS = _occlusion_lib.OCCLUSION_MAX_VIEWS


# ---- argument checks: everything below is decided on the host, before any device is touched ------

def _check_slack(slack):
    return _check_real("slack", slack, "finite and >= 0", lambda x: x >= 0)


def _check_floor(floor, shape):
    if not isinstance(floor, torch.Tensor) or floor.dtype != torch.float32 or tuple(floor.shape) != tuple(shape):
        raise ValueError(f"floor must be a {tuple(shape)} float32 tensor, got {_what(floor)}")


def view_lines(dirs) -> np.ndarray:
    """(V, 3) lines of sight (east, north, up) from the ground towards the camera, as ``view_directions``
    returns them -> (V, 3) float32 on the host, checked: 1 to 16 of them, finite, up > 0."""
    if isinstance(dirs, torch.Tensor):
        dirs = dirs.detach().cpu().numpy()
    dirs = np.asarray(dirs)
    if dirs.ndim != 2 or dirs.shape[1] != 3 or dirs.dtype.kind not in "fiu":
        raise ValueError(f"dirs must be (V, 3) vectors (east, north, up), got {dirs.dtype} {tuple(dirs.shape)}")
    if not 1 <= dirs.shape[0] <= MAX_VIEWS:
        raise ValueError(f"{dirs.shape[0]} directions in one call (1 to {MAX_VIEWS})")
    dirs = np.ascontiguousarray(dirs, np.float32)
    if not np.isfinite(dirs).all():
        raise ValueError("dirs holds a non-finite direction")
    low = np.nonzero(~(dirs[:, 2] > 0))[0]
    if low.size:
        raise ValueError(f"dirs[{int(low[0])}] has up = {float(dirs[low[0], 2])}: a line of sight points from the ground up to its camera")
    return dirs


# ---- the steps ----------------------------------------------------------------------------------------

def visibility_floor(dsm: torch.Tensor, grid, dirs) -> torch.Tensor:
    """``floor`` (V, H, W) float32 of the (H, W) device DSM ``dsm`` — float64, or float32 (widened), row 0
    the northernmost, as ``cast_shadows`` takes it — on ``grid`` (a ``GroundGrid`` or the cell size in
    metres) under the V lines of sight ``dirs`` (``view_directions``' first result): per view and cell the
    lowest altitude from which the camera is still seen over the DSM, −inf where nothing stands towards
    the camera.  The march is ``cast_shadows``'; the cell's own height is not read, so a NaN cell still
    gets a floor, and NaN heights on the way are skipped."""
    _check_dsm("dsm", dsm)
    res = _resolution(grid, dsm.shape)
    host = view_lines(dirs)
    V, (H, W) = host.shape[0], dsm.shape
    _lib.require_device(dsm)
    L = _occlusion_lib.lib()
    dsm = dsm.double().contiguous()
    nbytes = L.spnerf_occlusion_workspace_bytes(H, W)
    if nbytes < 0:
        _lib.check(int(nbytes), "occlusion_workspace_bytes")
    ws = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dsm.device)
    floor = torch.empty((V, H, W), dtype=torch.float32, device=dsm.device)
    _lib.check(L.spnerf_occlusion_floor(_lib.ptr(dsm), H, W, res, host.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), V, _lib.ptr(ws),
                                        _lib.ptr(floor), _lib.stream_of(dsm)), "occlusion_floor")
    return floor


def gate_plane(grey: torch.Tensor, valid: torch.Tensor, floor: torch.Tensor, alt, *, slack=0.0):
    """A new ``grey`` / ``valid`` pair of the plane at altitude ``alt`` (``plane_grey``'s, (V, H, W) float32
    and uint8) with the views below their ``floor`` (V, H, W) float32 taken out: where
    ``alt + slack < floor`` the grey is NaN and the valid byte 0, everything else is copied.  The
    comparison is strict and in fp64; a NaN floor gates nothing."""
    if not isinstance(grey, torch.Tensor) or grey.dim() != 3 or grey.numel() == 0 or grey.dtype != torch.float32:
        raise ValueError(f"grey must be a non-empty (V, H, W) float32 tensor, got {_what(grey)}")
    if not 1 <= grey.shape[0] <= MAX_VIEWS:
        raise ValueError(f"{grey.shape[0]} views in one call (1 to {MAX_VIEWS})")
    if not isinstance(valid, torch.Tensor) or valid.dtype != torch.uint8 or tuple(valid.shape) != tuple(grey.shape):
        raise ValueError(f"valid must be a {tuple(grey.shape)} uint8 tensor, got {_what(valid)}")
    _check_floor(floor, grey.shape)
    alt = _check_real("alt", alt, "finite", lambda x: True)
    slack = _check_slack(slack)
    _one_device(grey, valid, floor)
    L = _occlusion_lib.lib()
    grey, valid, floor = grey.clone(memory_format=torch.contiguous_format), valid.clone(memory_format=torch.contiguous_format), floor.contiguous()
    V, H, W = grey.shape
    _lib.check(L.spnerf_occlusion_gate(_lib.ptr(grey), _lib.ptr(valid), _lib.ptr(floor), V, H * W, alt, slack, _lib.stream_of(grey)),
               "occlusion_gate")
    return grey, valid


def visible_sweep(images, cameras, grid, alt_lo, step, planes, floor, *, slack, radius=2, min_views=2, min_std=0.0, volume=False) -> dict:
    """``plane_sweep`` with view v left out of cell w at plane k where ``alt_lo + k·step + slack <
    floor[v, w]`` (``floor`` (V, H, W) float32, ``visibility_floor``'s): one launch, the floors of a tile
    and its halo read once, a gated view neither projected nor read.  Returns ``plane_sweep``'s dict; with
    every floor −inf or NaN those are ``plane_sweep``'s bytes."""
    cams, imgs, grid = _sweep._check_scene(images, cameras, grid)
    alt_lo, step, K = _sweep._check_planes(alt_lo, step, planes)
    radius, min_views, min_std = _sweep._check_window(len(cams), radius, min_views, min_std)
    _check_floor(floor, (len(cams),) + grid.shape)
    slack = _check_slack(slack)
    dev = _one_device(*imgs, floor)
    L = _occlusion_lib.lib()
    V, (H, W), C = len(cams), grid.shape, imgs[0].shape[2]
    cam_table = _camera_table(cams, dev)
    img_table, imgs = _image_table(imgs, dev)
    floor = floor.contiguous()
    out = _pick_planes(H, W, dev, K if volume else None)
    _lib.check(L.spnerf_occlusion_sweep(ctypes.byref(_grid_struct(grid)), _lib.ptr(cam_table), _lib.ptr(img_table), V, C, alt_lo, step, K,
                                        radius, min_views, min_std, _lib.ptr(floor), slack, _lib.ptr(out["altitude"]),
                                        _lib.ptr(out["score"]), _lib.ptr(out["index"]), _lib.ptr(out["views"]), _lib.ptr(out.get("volume")),
                                        _lib.stream_of(out["altitude"])), "occlusion_sweep")
    return out


def refine_sweep(images, cameras, grid, alt_lo, step, planes, *, prior=None, slack=None, radius=2, min_views=2, min_std=0.0, p1=sgm.P1,
                 p2=sgm.P2, unscored=1.0, paths=8, volume=False) -> dict:
    """The two-pass sweep: a ``prior`` DSM (H, W) — ``smooth_sweep``'s altitude unless one is given: the
    lidar's, ``render_ortho``'s, any registered raster — gives the ``visibility_floor`` under the cameras'
    lines of sight (``view_directions`` over the swept range), ``visible_sweep(volume=True)`` scores the
    planes with the hidden views left out, and ``sgm.aggregate`` → ``sgm.pick`` choose the planes jointly.
    ``slack`` defaults to one ``step``: a view is gated only where the prior stands more than a plane above
    the swept altitude.  Returns ``sgm.pick``'s dict plus ``floor`` (V, H, W) and ``prior`` (H, W, the DSM the
    floor was made from), and with ``volume=True`` also ``volume`` and ``aggregated``.  The aggregation
    itself does not know the gate.  The floor is a maximum along the line of sight, so the result is as good
    as the prior: on the JAX_269 ROI the lidar as the prior improves on ``smooth_sweep``, the sweep's own noisy
    first pass makes it worse.  Without a lidar use ``clean.bootstrap_sweep``, which takes the
    speckles out of the first pass before the floor is made from it: that brings the error back to
    ``smooth_sweep``'s, not below it."""
    cams, imgs, grid = _sweep._check_scene(images, cameras, grid)
    alt_lo, step, K = _sweep._check_planes(alt_lo, step, planes)
    _check_int("planes", K, 2, sgm.MAX_PLANES)
    _sweep._check_window(len(cams), radius, min_views, min_std)
    sgm._check_penalties(p1, p2, unscored, paths)
    slack = step if slack is None else _check_slack(slack)
    if not isinstance(volume, bool):
        raise ValueError(f"volume {volume!r} must be a bool")
    if prior is not None:
        _check_dsm("prior", prior, grid)
        _one_device(*imgs, prior)
    kw = dict(radius=radius, min_views=min_views, min_std=min_std)
    if prior is None:
        prior = sgm.smooth_sweep(images, cameras, grid, alt_lo, step, K, p1=p1, p2=p2, unscored=unscored, paths=paths, **kw)["altitude"]
    dirs, _ = view_directions(grid, cams, alt_lo, alt_lo + (K - 1) * step, imgs[0].device)
    floor = visibility_floor(prior, grid, dirs)
    raw = visible_sweep(images, cameras, grid, alt_lo, step, K, floor, slack=slack, volume=True, **kw)["volume"]
    agg = sgm.aggregate(raw, p1=p1, p2=p2, unscored=unscored, paths=paths)
    out = sgm.pick(agg, raw, alt_lo, step)
    out["floor"], out["prior"] = floor, prior
    if volume:
        out["volume"], out["aggregated"] = raw, agg
    return out
