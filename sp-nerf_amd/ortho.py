"""A DSM and true-ortho products on a UTM ground grid (csrc/ortho.hip, include/spnerf_amd_ortho.h):
the route of S-NeRF / EO-NeRF beside the reference's per-view one (``dsm.get_dsm_from_nerf_prediction``).

One vertical ray is cast per cell of the grid — or s x s sub-rays, box-filtered afterwards — from
``max_alt`` down to ``min_alt`` on the ellipsoid normal, and ``render_image`` / ``relight_image``
render those rays like any others.  The altitude, albedo, class and shadow of a cell are read
straight off the grid the lidar ROI and the ground-truth rasters live on: no point cloud, no
forward projection, no rasteriser, and no cell without a value.

The rays are built in fp64 up to one cast: the fp32 rounding of ECEF that the camera rays
reproduce (``get_rays`` casts before ``normalize_rays`` centres: half a metre at 6.4e6 m) would
be a whole cell here and is not made.
"""
from __future__ import annotations

import ctypes
import dataclasses
import math
import numbers
import os

import numpy as np
import torch

from . import _lib, _ortho_lib
from ._ground import _require_cuda
from .relight import PRODUCTS as RELIGHT_PRODUCTS, SUN_PLANES, _directions, relight_image
from .satellite import sun_direction
from .view import PRODUCTS as VIEW_PRODUCTS, render_image

MAX_SUPERSAMPLE = _ortho_lib.ORTHO_MAX_SUPERSAMPLE


@dataclasses.dataclass(frozen=True)
class GroundGrid:
    """A north-up grid of square cells in WGS-84 UTM metres: cell (j, i) covers eastings
    [xoff + i·res, xoff + (i + 1)·res) and northings (ytop − (j + 1)·res, ytop − j·res]."""
    xoff: float
    ytop: float
    xsize: int
    ysize: int
    resolution: float
    zone: int
    south: bool = False

    def __post_init__(self):
        for name in ("xsize", "ysize", "zone"):
            v = getattr(self, name)
            if not isinstance(v, numbers.Integral) or isinstance(v, bool):
                raise ValueError(f"GroundGrid: {name} must be an integer, got {v!r}")
            object.__setattr__(self, name, int(v))
        for name in ("xoff", "ytop", "resolution"):
            v = float(getattr(self, name))
            if not math.isfinite(v):
                raise ValueError(f"GroundGrid: {name} {v} is not finite")
            object.__setattr__(self, name, v)
        object.__setattr__(self, "south", bool(self.south))
        if self.xsize <= 0 or self.ysize <= 0:
            raise ValueError(f"GroundGrid: {self.xsize} x {self.ysize} cells")
        if not self.resolution > 0:
            raise ValueError(f"GroundGrid: resolution {self.resolution} must be positive")
        if not 1 <= self.zone <= 60:
            raise ValueError(f"GroundGrid: UTM zone {self.zone} outside 1..60")

    @classmethod
    def from_roi(cls, roi, zone, south=False):
        """The grid of a lidar ROI file — (xoff, yoff, size, resolution), ``yoff`` the bottom edge —
        given as its path or its four numbers: the reading of
        ``get_dsm_from_nerf_prediction(roi_txt=)`` (satellite_scene.py:524-531)."""
        meta = np.loadtxt(roi) if isinstance(roi, (str, os.PathLike)) else np.asarray(roi, np.float64)
        meta = np.asarray(meta, np.float64).reshape(-1)
        if meta.shape[0] != 4:
            raise ValueError(f"a ROI is (xoff, yoff, size, resolution), got {meta.shape[0]} numbers")
        size, res = int(meta[2]), float(meta[3])
        return cls(float(meta[0]), float(meta[1]) + size * res, size, size, res, zone, south)

    @classmethod
    def from_bounds(cls, e_min, e_max, n_min, n_max, resolution, zone, south=False):
        """The grid that holds the box [e_min, e_max] x [n_min, n_max], snapped to multiples of
        ``resolution`` as ``get_dsm_from_nerf_prediction`` snaps a cloud's bounds
        (satellite_scene.py:533-538)."""
        res = float(resolution)
        if not res > 0:
            raise ValueError(f"GroundGrid: resolution {res} must be positive")
        if not (e_max >= e_min and n_max >= n_min):
            raise ValueError("GroundGrid.from_bounds: empty box")
        xoff = math.floor(e_min / res) * res
        xsize = int(1 + math.floor((e_max - xoff) / res))
        ytop = math.ceil(n_max / res) * res
        ysize = int(1 - math.floor((n_min - ytop) / res))
        return cls(xoff, ytop, xsize, ysize, res, zone, south)

    @property
    def shape(self):
        return (self.ysize, self.xsize)

    def cell_centres(self):
        """(easting, northing) of the cell centres, two (ysize, xsize) float64 host arrays."""
        e = self.xoff + (np.arange(self.xsize, dtype=np.float64) + 0.5) * self.resolution
        n = self.ytop - (np.arange(self.ysize, dtype=np.float64) + 0.5) * self.resolution
        return np.broadcast_to(e[None, :], self.shape).copy(), np.broadcast_to(n[:, None], self.shape).copy()


# ---- argument checks: everything below is decided on the host, before any device is touched ------

def _check_grid(grid, supersample, rows):
    if not isinstance(grid, GroundGrid):
        raise ValueError(f"grid must be a GroundGrid, got {type(grid).__name__}")
    if not isinstance(supersample, numbers.Integral) or isinstance(supersample, bool) or not 1 <= supersample <= MAX_SUPERSAMPLE:
        raise ValueError(f"supersample {supersample!r} outside 1..{MAX_SUPERSAMPLE}")
    if rows is None:
        return int(supersample), 0, grid.ysize
    try:
        j0, j1 = rows
        ok = all(isinstance(j, numbers.Integral) and not isinstance(j, bool) for j in (j0, j1))
    except (TypeError, ValueError):
        ok = False
    if not ok or not 0 <= j0 < j1 <= grid.ysize:
        raise ValueError(f"rows {rows!r} must be (j0, j1) with 0 <= j0 < j1 <= ysize = {grid.ysize}")
    return int(supersample), int(j0), int(j1)


def _check_scene(min_alt, max_alt, center, rng):
    min_alt, max_alt = float(min_alt), float(max_alt)
    if not (math.isfinite(min_alt) and math.isfinite(max_alt) and max_alt > min_alt):
        raise ValueError(f"max_alt {max_alt} must be above min_alt {min_alt}")
    cen = np.asarray(center, np.float64).reshape(-1)
    if cen.shape[0] != 3 or not np.isfinite(cen).all():
        raise ValueError(f"center must be 3 finite numbers, got {center!r}")
    # the scene holds its normalisation as float32 (scene.loc); spnerf_dsm_points takes these values
    cen = np.asarray(cen, np.float32).astype(np.float64)
    rng = float(np.float32(rng))
    if not (math.isfinite(rng) and rng > 0):
        raise ValueError(f"rng {rng} must be positive")
    return min_alt, max_alt, cen, rng


def _sun_vector(sun):
    """An (elevation°, azimuth°) pair or a 3-vector -> 3 float32."""
    v = np.asarray(sun.detach().cpu() if isinstance(sun, torch.Tensor) else sun, np.float64).reshape(-1)
    if v.shape[0] == 2:
        v = sun_direction(float(v[0]), float(v[1]))
    elif v.shape[0] != 3:
        raise ValueError(f"sun must be an (elevation, azimuth) pair in degrees or a 3-vector, got {v.shape[0]} numbers")
    if not np.isfinite(v).all():
        raise ValueError("sun holds a non-finite number")
    return v.astype(np.float32)


def _check_semantics(semantics, grid):
    if semantics is None:
        return None
    shape = tuple(semantics.shape) if hasattr(semantics, "shape") else None
    if shape != grid.shape:
        raise ValueError(f"semantics must hold one label per cell, {grid.shape}, got {shape}")
    return semantics


def _launch_rays(grid, s, j0, j1, min_alt, max_alt, cen, rng, sun, dev):
    n = (j1 - j0) * grid.xsize * s * s
    stride = 8 if sun is None else 11
    rays = torch.empty(n, stride, dtype=torch.float32, device=dev)
    g = _ortho_lib.OrthoGrid(grid.xoff, grid.ytop, grid.resolution, grid.xsize, grid.ysize, grid.zone, 1 if grid.south else 0, s)
    c = (ctypes.c_double * 3)(*cen)
    sn = None if sun is None else (ctypes.c_float * 3)(*[float(v) for v in sun])
    _lib.check(_ortho_lib.lib().spnerf_ortho_rays(ctypes.byref(g), j0, j1 - j0, min_alt, max_alt, c, rng, sn, _lib.ptr(rays),
                                                 stride, _lib.stream_of(rays)), "ortho_rays")
    return rays


def ortho_rays(grid, min_alt, max_alt, center, rng, sun=None, supersample=1, rows=None, device="cuda") -> torch.Tensor:
    """The vertical rays of ``grid`` in the normalised scene (``center`` / ``rng``:
    SatelliteSceneDataset.center / .range), (n, 11) float32 on ``device`` — (n, 8) without ``sun`` —
    in the layout of the camera rays: o, d, near = 0, far, sun direction.  Ray
    ((j·xsize + i)·s + a)·s + b is sub-ray (a, b) of cell (j, i) with s = ``supersample``: it starts
    at ``max_alt`` above (E, N) = (xoff + (i + (b + ½)/s)·res, ytop − (j + (a + ½)/s)·res) and ends
    at ``min_alt``, so depth·rng is metres below ``max_alt``.  ``sun`` is an (elevation°, azimuth°)
    pair or a 3-vector; ``rows=(j0, j1)`` is a band of a large grid."""
    s, j0, j1 = _check_grid(grid, supersample, rows)
    min_alt, max_alt, cen, rng = _check_scene(min_alt, max_alt, center, rng)
    sun = None if sun is None else _sun_vector(sun)
    return _launch_rays(grid, s, j0, j1, min_alt, max_alt, cen, rng, sun, _require_cuda(device))


def reduce_subrays(x: torch.Tensor, supersample: int, ray_dim: int = 0) -> torch.Tensor:
    """Box filter of the s² contiguous sub-rays of every cell along dimension ``ray_dim`` of a
    float32 or float64 device tensor: (…, cells·s², …) -> (…, cells, …), summed in fp64 in sub-ray
    order, one division, one cast.  With s = 1 ``x`` itself comes back."""
    s = int(supersample)
    if not 1 <= s <= MAX_SUPERSAMPLE:
        raise ValueError(f"supersample {supersample!r} outside 1..{MAX_SUPERSAMPLE}")
    if x.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"reduce_subrays takes float32 or float64 planes, got {x.dtype}")
    if not 0 <= ray_dim < x.dim() or x.shape[ray_dim] % (s * s):
        raise ValueError(f"dimension {ray_dim} of {tuple(x.shape)} does not hold whole cells of {s * s} sub-rays")
    _lib.require_device(x)
    if s == 1:
        return x
    x = x.contiguous()
    lead, cells, trail = tuple(x.shape[:ray_dim]), x.shape[ray_dim] // (s * s), tuple(x.shape[ray_dim + 1:])
    out = torch.empty(lead + (cells,) + trail, dtype=x.dtype, device=x.device)
    _lib.check(_ortho_lib.lib().spnerf_ortho_reduce(_lib.ptr(x), _lib.ptr(out), math.prod(lead), cells, math.prod(trail), s,
                                                   1 if x.dtype == torch.float64 else 0, _lib.stream_of(x)), "ortho_reduce")
    return out


def classes(logits: torch.Tensor) -> torch.Tensor:
    """(cells, C) float32 mean logits -> (cells,) int32 labels by the rule of the ``sem_class``
    plane: the first index of the maximum, a NaN counting as the maximum."""
    _lib.require_device(logits)
    if logits.dim() != 2 or logits.shape[1] == 0 or logits.dtype != torch.float32:
        raise ValueError(f"logits must be (cells, C) float32, got {logits.dtype} {tuple(logits.shape)}")
    logits = logits.contiguous()
    out = torch.empty(logits.shape[0], dtype=torch.int32, device=logits.device)
    _lib.check(_ortho_lib.lib().spnerf_ortho_classes(_lib.ptr(logits), logits.shape[0], logits.shape[1], _lib.ptr(out),
                                                    _lib.stream_of(logits)), "ortho_classes")
    return out


def _plan(models, args, grid, min_alt, max_alt, center, rng, ts, semantics, supersample, products, rows, allowed, what):
    """The checks ``render_ortho`` and ``relight_ortho`` share, in ``relight_image``'s order."""
    if args.model != "sp-nerf":
        raise ValueError(f'model {args.model} is not valid')
    if "sc" in products:
        raise ValueError(f"the sc product is not an image product: the solar march's per-ray terms belong to a camera "
                         f"view's loss ({what} renders ground cells)")
    unknown = [p for p in products if p not in allowed]
    if unknown:
        raise ValueError(f"unknown products {unknown}; the products are {tuple(p for p in allowed if p != 'sc')}")
    s, j0, j1 = _check_grid(grid, supersample, rows)
    scene = _check_scene(min_alt, max_alt, center, rng)
    if not isinstance(ts, numbers.Integral) or isinstance(ts, bool):
        raise ValueError(f"ts must be one int for all rays, got {ts!r}")
    _check_semantics(semantics, grid)
    return s, j0, j1, scene


def _grid_inputs(models, args, grid, s, j0, j1, scene, sun, ts, semantics):
    """(rays, ts, semantics, ray_offset, clamp) of a band: what ``render_image`` takes for it such
    that the bands of a grid reassemble to the whole — the draws keyed by the ray's index in the
    whole grid, guided sampling clamped to the whole grid's first ray."""
    model = models["fine" if args.n_importance > 0 else "coarse"]
    dev = next(model.parameters()).device
    _lib.require_device(next(model.parameters()), semantics if isinstance(semantics, torch.Tensor) else None)
    rays = _launch_rays(grid, s, j0, j1, *scene, sun, dev)
    clamp = None
    if args.guidedsample:
        clamp = rays[0, 6:8] if j0 == 0 else _launch_rays(grid, s, 0, 1, *scene, sun, dev)[0, 6:8]
    n = rays.shape[0]
    ts_rays = torch.full((n,), int(ts), dtype=torch.long, device=dev) if args.beta else None
    sem_rays = None
    if semantics is not None:
        sem_rays = torch.as_tensor(semantics)[j0:j1].to(dev).reshape(-1).repeat_interleave(s * s)
    return rays, ts_rays, sem_rays, j0 * grid.xsize * s * s, clamp


def _to_grid(planes, s, j1_j0, xsize, sun_planes=()):
    """Reduce every plane over its cells' sub-rays and shape it (rows, xsize, ·); the class plane
    is the argmax of the reduced logits."""
    out = {}
    for name, t in planes.items():
        if name == "sem_class":
            continue
        k = 1 if name in sun_planes else 0
        r = reduce_subrays(t, s, k)
        out[name] = r.reshape(tuple(r.shape[:k]) + (j1_j0, xsize) + tuple(r.shape[k + 1:]))
    if "sem_class" in planes:
        cls = planes["sem_class"] if s == 1 else classes(out["sem_logits"].reshape(j1_j0 * xsize, -1))
        out["sem_class"] = cls.reshape(j1_j0, xsize)
    return out


def render_ortho(models, args, grid, min_alt, max_alt, center, rng, sun, *, ts=0, semantics=None, supersample=1,
                 products=("rgb", "depth", "sun", "albedo", "sky", "sem"), chunk=None, rows=None) -> dict:
    """Render the cells of ``grid`` (or its rows ``rows=(j0, j1)``) under the sun direction ``sun``:
    ``ortho_rays`` → ``render_image(..., center=, rng=)`` → the box filter over each cell's
    ``supersample``² sub-rays.  Every plane of ``render_image`` comes back shaped (rows, xsize[, ·])
    on the device, and besides them "dsm" (rows, xsize) float64: the altitude of every cell (the
    reduced "alt"), with a value in every cell.  ``sem_class`` is the argmax of the reduced
    ``sem_logits``.

    ``semantics``: optional (ysize, xsize) labels on the grid, repeated over each cell's sub-rays;
    ``ts``: one int for all rays (the reference's ``predefined_val_ts`` is 0).  ``products`` are
    ``render_image``'s except "sc": the solar march's per-ray terms are not an image product.  With
    an on-device random source the result depends neither on ``chunk`` nor on the banding."""
    s, j0, j1, scene = _plan(models, args, grid, min_alt, max_alt, center, rng, ts, semantics, supersample, products, rows,
                             VIEW_PRODUCTS, "render_ortho")
    sun = _sun_vector(sun)
    if "rgb_coarse" in products and not args.n_importance > 0:
        raise ValueError("the rgb_coarse product is the coarse image beside a fine model's: it needs n_importance > 0")
    rays, ts_rays, sem_rays, offset, clamp = _grid_inputs(models, args, grid, s, j0, j1, scene, sun, ts, semantics)
    img = render_image(models, args, rays, ts_rays, sem_rays, chunk=chunk, products=products, ray_offset=offset,
                       center=scene[2], rng=scene[3], clamp_near_far=clamp)
    out = _to_grid(img, s, j1 - j0, grid.xsize)
    out["dsm"] = out["alt"]
    return out


def relight_ortho(models, args, grid, min_alt, max_alt, center, rng, sun_dirs, *, ts=0, semantics=None, supersample=1,
                  products=("rgb", "sun", "sky"), chunk=None, rows=None, cast=False) -> dict:
    """``render_ortho`` over ``relight_image``: the cells of ``grid`` under the K sun directions
    ``sun_dirs`` (K, 3) from one pass over their geometry.  The sun-dependent planes come back as
    "rgb" (K, rows, xsize, 3), "sun" (K, rows, xsize) and "sky" (K, rows, xsize, 3); the others once,
    as ``render_ortho`` shapes them.  With "depth" among the products "dsm" comes back too.

    ``cast=True`` adds "shadow_geo" (K, ysize, xsize) uint8: the geometric shadows of that "dsm" under
    ``sun_dirs`` (``shadow.cast_shadows``), to hold the learnt "sun" against
    (``shadow.shadow_agreement``).  It needs "depth" among the products and the whole grid
    (``rows=None``): a band lacks the occluders outside it.  The other planes do not change."""
    s, j0, j1, scene = _plan(models, args, grid, min_alt, max_alt, center, rng, ts, semantics, supersample, products, rows,
                             RELIGHT_PRODUCTS, "relight_ortho")
    dirs = _directions(sun_dirs)
    if cast:
        from . import shadow
        if "depth" not in products:
            raise ValueError('cast=True casts the shadows of the call\'s own DSM: it needs "depth" among the products')
        if rows is not None:
            raise ValueError("cast=True needs the whole grid (rows=None): a band lacks the occluders outside it")
        shadow.sun_directions(dirs)
    if "rgb_coarse" in products and not args.n_importance > 0:
        raise ValueError("the rgb_coarse product is the coarse image beside a fine model's: it needs n_importance > 0")
    rays, ts_rays, sem_rays, offset, clamp = _grid_inputs(models, args, grid, s, j0, j1, scene, dirs[0].numpy(), ts, semantics)
    img = relight_image(models, args, rays, dirs, ts_rays, sem_rays, chunk=chunk, products=products, ray_offset=offset,
                        clamp_near_far=clamp)
    if "depth" in img:
        from .dsm import _points
        img["alt"] = _points(rays, img["depth"], scene[2], scene[3])[0][:, 2]
    out = _to_grid(img, s, j1 - j0, grid.xsize, SUN_PLANES)
    if "alt" in out:
        out["dsm"] = out["alt"]
    if cast:
        out["shadow_geo"] = shadow.cast_shadows(out["dsm"], grid, dirs)
    return out
