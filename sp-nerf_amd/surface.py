"""The plane sweep around a base surface, and the coarse-to-fine chain it makes possible
(csrc/surface.hip, include/spnerf_amd_surface.h).

``plane_sweep`` and its siblings take K horizontal planes ``alt_lo + k·step`` shared by all cells.
``surface_sweep`` takes a ``base`` raster on the grid instead and scores the K surfaces
``base + (off_lo + k·step)``: a few offsets around a coarser sweep's altitude, around a trained network's
``render_ortho`` DSM, around a lidar.  ``surface_grey`` is ``plane_grey`` with that per-cell altitude,
``surface_lift`` turns the pick's relative altitude into an altitude, and the fused call has the bytes of
``surface_grey`` → ``window_score`` per surface → ``pick_plane(off_lo)`` → ``surface_lift``.
``coarsen`` and ``upsample_dsm`` move between a grid and the same ground at f times the cell size, and
``pyramid_sweep`` is the chain: ``smooth_sweep`` on the coarsest grid, then per finer level
``upsample_dsm`` → ``surface_sweep(volume=True)`` → ``sgm.aggregate`` → ``sgm.pick`` → ``surface_lift``.
The header states every operation and its order.

Not there: an image pyramid (a 2 m grid still reads the 1.3 m pixels bilinearly, unfiltered), a surface
sweep gated by a visibility floor, filling of the cells without an altitude (a NaN base stays NaN), and a
reach that varies from cell to cell.
"""
from __future__ import annotations

import ctypes
import math
import numbers

import torch

from . import _lib, _surface_lib, sgm
from . import sweep as _sweep
from .ortho import GroundGrid
from ._ground import (_camera_table, _check_grid, _check_int, _check_raster, _check_real, _grid_struct, _image_table, _one_device,
                      _pick_planes)

MAX_FACTOR = _surface_lib.SURFACE_MAX_FACTOR


# ---- argument checks: everything below is decided on the host, before any device is touched ------

def _check_shape(shape):
    try:
        H, W = shape
        ok = all(isinstance(n, numbers.Integral) and not isinstance(n, bool) and n > 0 for n in (H, W))
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"shape {shape!r} must be (H, W), two positive integers")
    if H * W > 2 ** 32:
        raise ValueError(f"a grid of {W} x {H} cells is too large for one call")
    return int(H), int(W)


def _coarse_shape(shape, factor):
    return (-(-shape[0] // factor), -(-shape[1] // factor))


def _check_factors(factors):
    try:
        fs = tuple(factors)
    except TypeError:
        fs = None
    if not fs or not all(isinstance(f, numbers.Integral) and not isinstance(f, bool) and 2 <= f <= MAX_FACTOR for f in fs):
        raise ValueError(f"factors {factors!r} must be a non-empty tuple of integers in 2..{MAX_FACTOR}")
    fs = tuple(int(f) for f in fs)
    if any(b >= a for a, b in zip(fs, fs[1:])):
        raise ValueError(f"factors {factors!r} must be strictly descending")
    for a, b in zip(fs, fs[1:] + (1,)):
        if a % b:
            raise ValueError(f"factors {factors!r}: {a} is not an integer multiple of {b}")
    return fs


def level_plan(factors, planes, reach):
    """The levels of ``pyramid_sweep``: a list of (factor, step multiple, surfaces) from the coarsest level
    to the implied last one of factor 1.  Level l has the step ``step·min(f_l, 2)``; the first one
    ceil(planes / min(f_0, 2)) planes, i.e. ceil(planes·step / s_0); a later one
    2·ceil(reach·s_(l-1) / s_l) + 1 offsets centred on 0."""
    fs = _check_factors(factors) + (1,)
    mult = [min(f, 2) for f in fs]
    plan = [(fs[0], mult[0], -(-planes // mult[0]))]
    for l in range(1, len(fs)):
        plan.append((fs[l], mult[l], 2 * math.ceil(reach * (mult[l - 1] // mult[l])) + 1))
    return plan


def coarsen(grid: GroundGrid, factor) -> GroundGrid:
    """``grid`` at ``factor`` times the cell size: the same ``xoff``, ``ytop`` and zone, ceil(H / factor) x
    ceil(W / factor) cells, so the last row and column may reach past the fine grid.  ``factor`` 1..8."""
    grid = _check_grid(grid)
    f = _check_int("factor", factor, 1, MAX_FACTOR)
    H, W = _coarse_shape(grid.shape, f)
    return GroundGrid(grid.xoff, grid.ytop, W, H, grid.resolution * f, grid.zone, grid.south)


# ---- the steps ----------------------------------------------------------------------------------------

def surface_grey(images, cameras, grid, base: torch.Tensor, offset):
    """``plane_grey`` on the surface ``base + offset``: ``base`` an (H, W) float32 device raster, the
    altitude of a cell ``(double)base + offset``.  Where ``base`` is not finite every view is invalid
    (``valid`` 0, ``grey`` NaN), as for a read outside the image."""
    cams, imgs, grid = _sweep._check_scene(images, cameras, grid)
    _check_raster("base", base, grid.shape)
    offset = _check_real("offset", offset, "finite", lambda x: True)
    dev = _one_device(*imgs, base)
    L = _surface_lib.lib()
    V, (H, W), C = len(cams), grid.shape, imgs[0].shape[2]
    cam_table = _camera_table(cams, dev)
    img_table, imgs = _image_table(imgs, dev)
    base = base.contiguous()
    grey = torch.empty((V, H, W), dtype=torch.float32, device=dev)
    valid = torch.empty((V, H, W), dtype=torch.uint8, device=dev)
    _lib.check(L.spnerf_surface_grey(ctypes.byref(_grid_struct(grid)), _lib.ptr(cam_table), _lib.ptr(img_table), V, C, _lib.ptr(base),
                                     offset, _lib.ptr(grey), _lib.ptr(valid), _lib.stream_of(grey)), "surface_grey")
    return grey, valid


def surface_lift(base: torch.Tensor, rel: torch.Tensor) -> torch.Tensor:
    """``(float)((double)base + (double)rel)`` elementwise, two (H, W) float32 device rasters: the altitude
    of a relative altitude ``rel`` — what ``pick_plane`` / ``sgm.pick`` return for ``alt_lo = off_lo`` —
    over its ``base``.  NaN propagates."""
    _check_raster("base", base)
    _check_raster("rel", rel, base.shape)
    dev = _one_device(base, rel)
    L = _surface_lib.lib()
    base, rel = base.contiguous(), rel.contiguous()
    out = torch.empty(tuple(base.shape), dtype=torch.float32, device=dev)
    _lib.check(L.spnerf_surface_lift(_lib.ptr(base), _lib.ptr(rel), base.numel(), _lib.ptr(out), _lib.stream_of(out)), "surface_lift")
    return out


def upsample_dsm(coarse: torch.Tensor, factor, shape) -> torch.Tensor:
    """The (ceil(H / factor), ceil(W / factor)) float32 raster ``coarse`` of ``coarsen(grid, factor)``
    resampled bilinearly to the ``shape`` = (H, W) of ``grid``: cell centres against cell centres, the
    coarse indices clamped at the border, non-finite entries left out and the other weights renormalised,
    NaN where no finite entry has a weight.  ``factor`` 1 copies the finite values."""
    f = _check_int("factor", factor, 1, MAX_FACTOR)
    H, W = _check_shape(shape)
    _check_raster("coarse", coarse)
    if tuple(coarse.shape) != _coarse_shape((H, W), f):
        raise ValueError(f"coarse {tuple(coarse.shape)} is not {_coarse_shape((H, W), f)}, a {(H, W)} grid coarsened by {f}")
    dev = _one_device(coarse)
    L = _surface_lib.lib()
    coarse = coarse.contiguous()
    out = torch.empty((H, W), dtype=torch.float32, device=dev)
    _lib.check(L.spnerf_surface_upsample(_lib.ptr(coarse), f, H, W, _lib.ptr(out), _lib.stream_of(out)), "surface_upsample")
    return out


def surface_sweep(images, cameras, grid, base: torch.Tensor, off_lo, step, planes, *, radius=2, min_views=2, min_std=0.0,
                  volume=False) -> dict:
    """``plane_sweep`` over the ``planes`` surfaces ``base + (off_lo + k·step)``, ``base`` an (H, W) float32
    tensor on the images' device: one launch, the bases of a tile and its halo read once, a cell without a
    finite base neither projected nor read.  Returns ``plane_sweep``'s dict: ``index``, ``score`` and
    ``views`` are the pick over the K offsets, ``altitude`` is ``surface_lift(base, ·)`` of the pick's
    altitude for ``alt_lo = off_lo`` (NaN where no surface could be scored or the base is not finite), and
    with ``volume=True`` ``volume[k]`` is the score of offset k.  With a constant base c whose sums with the
    offsets are exact, ``index``, ``score``, ``views`` and ``volume`` are ``plane_sweep``'s bytes at
    ``alt_lo = c + off_lo`` (``altitude`` too over a zero base; otherwise it is rounded once more)."""
    cams, imgs, grid = _sweep._check_scene(images, cameras, grid)
    _check_real("off_lo", off_lo, "finite", lambda x: True)
    off_lo, step, K = _sweep._check_planes(off_lo, step, planes)
    radius, min_views, min_std = _sweep._check_window(len(cams), radius, min_views, min_std)
    _check_raster("base", base, grid.shape)
    dev = _one_device(*imgs, base)
    L = _surface_lib.lib()
    V, (H, W), C = len(cams), grid.shape, imgs[0].shape[2]
    cam_table = _camera_table(cams, dev)
    img_table, imgs = _image_table(imgs, dev)
    base = base.contiguous()
    out = _pick_planes(H, W, dev, K if volume else None)
    _lib.check(L.spnerf_surface_sweep(ctypes.byref(_grid_struct(grid)), _lib.ptr(cam_table), _lib.ptr(img_table), V, C, _lib.ptr(base),
                                      off_lo, step, K, radius, min_views, min_std, _lib.ptr(out["altitude"]), _lib.ptr(out["score"]),
                                      _lib.ptr(out["index"]), _lib.ptr(out["views"]), _lib.ptr(out.get("volume")),
                                      _lib.stream_of(out["altitude"])), "surface_sweep")
    return out


def pyramid_sweep(images, cameras, grid, alt_lo, step, planes, *, factors=(4,), reach=3, radius=2, min_views=2, min_std=0.0, p1=sgm.P1,
                  p2=sgm.P2, unscored=1.0, paths=8) -> dict:
    """The coarse-to-fine sweep of the altitudes ``alt_lo .. alt_lo + planes·step``.  ``factors`` is a
    strictly descending tuple of integers in 2..8, each a multiple of the next; a last level of factor 1 is
    implied.  Level l works on ``coarsen(grid, f_l)`` with the step s_l = ``step``·min(f_l, 2).  The first
    level is ``smooth_sweep`` with ceil(planes·step / s_0) planes from ``alt_lo``; every later level
    resamples the previous altitude to its own grid (``upsample_dsm``), scores 2·ceil(reach·s_(l-1) / s_l) + 1
    offsets centred on 0 around it (``surface_sweep(volume=True)`` — 13 at the defaults), and picks them
    jointly: ``sgm.aggregate`` → ``sgm.pick`` → ``surface_lift``.  Returns the last level's ``altitude``,
    ``score``, ``index`` and ``photo`` plus ``base``, the resampled altitude it was swept around.  A cell
    whose base is NaN stays NaN: holes are not filled.  On the JAX_269 ROI the last level does not improve
    on its base: the data term of a 2.5 m window on 1.3 m pixels is as weak as it was."""
    cams, imgs, grid = _sweep._check_scene(images, cameras, grid)
    alt_lo, step, planes = _sweep._check_planes(alt_lo, step, planes)
    _sweep._check_window(len(cams), radius, min_views, min_std)
    sgm._check_penalties(p1, p2, unscored, paths)
    reach = _check_real("reach", reach, "finite and > 0", lambda x: x > 0)
    plan = level_plan(factors, planes, reach)
    for f, _, K in plan:
        _check_int(f"planes of the level of factor {f}:", K, 1, sgm.MAX_PLANES)
    _one_device(*imgs)
    kw = dict(radius=radius, min_views=min_views, min_std=min_std)
    pen = dict(p1=p1, p2=p2, unscored=unscored, paths=paths)
    f0, m0, K0 = plan[0]
    out = sgm.smooth_sweep(images, cameras, coarsen(grid, f0), alt_lo, step * m0, K0, **kw, **pen)
    f_prev = f0
    for f, m, K in plan[1:]:
        level = coarsen(grid, f)
        base = upsample_dsm(out["altitude"], f_prev // f, level.shape)
        s, off_lo = step * m, -(K // 2) * (step * m)
        raw = surface_sweep(images, cameras, level, base, off_lo, s, K, volume=True, **kw)["volume"]
        out = sgm.pick(sgm.aggregate(raw, **pen), raw, off_lo, s)
        out["altitude"] = surface_lift(base, out["altitude"])
        out["base"] = base
        f_prev = f
    return out
