"""A ground-grid DSM seen from a camera, and the depth priors that makes of it (csrc/dsm_view.hip,
include/spnerf_amd_dsmview.h).

``orthorectify``, the sweeps and ``cast_shadows`` map grid → image: a cell is projected into a camera and
the image read there.  ``view_dsm`` maps image → grid: the line of sight of every pixel of a lattice —
the straight segment between the pixel's localisations at ``alt_hi`` and ``alt_lo``, in (E, N, altitude) —
is walked down over the DSM to the first point at or below the surface, which gives an altitude and a
depth image of the camera, the ground point and the fractional grid cell of every pixel.  ``sample_at``
reads any raster on the grid at those cells (a sweep's ``score`` or ``views``), ``hit_ecef`` turns the
ground points into ECEF, and ``dsm_depth_priors`` puts the three together into what
``dataset.load_depth_data`` takes: ``pts2d``, ``pts3d`` and ``correl`` per image, a DSM with a per-cell
weight delivered to the trainer's depth supervision.  The header states every operation and its order.

Not there: a curved line of sight (the chord error of the straight segment is measured),
filling of the cells without an altitude (a NaN or ±inf cell is transparent), a segment shorter than one
cell along its major axis (it may cross no cell-centre line and then reads nothing: choose
``alt_hi − alt_lo`` so that the segment spans several cells), and priors at another image scale than 1
(``load_depth_data`` refuses them).
"""
from __future__ import annotations

import ctypes
import numbers

import numpy as np
import torch

from . import _dsmview_lib, _lib
from .ortho import GroundGrid
from ._ground import _camera_table, _check_alts, _check_grid, _check_int, _check_raster, _check_real, _grid_struct, _one_device, _what
from .rectify import Camera

MODES = {"nearest": _dsmview_lib.DSMVIEW_NEAREST, "bilinear": _dsmview_lib.DSMVIEW_BILINEAR}
INT32_MAX = 2 ** 31 - 1


# ---- argument checks: everything below is decided on the host, before any device is touched ------

def _check_camera(camera):
    if not isinstance(camera, Camera):
        raise ValueError(f"camera must be a rectify.Camera, got {type(camera).__name__}")
    return camera


def _check_altitudes(alt_lo, alt_hi):
    for name, v in (("alt_lo", alt_lo), ("alt_hi", alt_hi)):
        _check_real(name, v, "finite", lambda x: True)
    return _check_alts(alt_lo, alt_hi)


def _check_lattice(rect, stride):
    stride = _check_int("stride", stride, 1, INT32_MAX)
    try:
        col0, row0, n_cols, n_rows = rect
        ok = all(isinstance(v, numbers.Integral) and not isinstance(v, bool) for v in (col0, row0, n_cols, n_rows))
        ok = ok and n_cols >= 1 and n_rows >= 1 and abs(col0) <= INT32_MAX and abs(row0) <= INT32_MAX
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"rect {rect!r} must be (col0, row0, n_cols, n_rows): four integers, n_cols and n_rows positive")
    if col0 + (n_cols - 1) * stride > INT32_MAX or row0 + (n_rows - 1) * stride > INT32_MAX or n_cols * n_rows > 2 ** 32:
        raise ValueError(f"rect {tuple(rect)!r} with stride {stride} is too large for one call")
    return (int(col0), int(row0), int(n_cols), int(n_rows)), stride


def _check_mode(mode):
    if mode not in MODES:
        raise ValueError(f"mode {mode!r} is neither 'nearest' nor 'bilinear'")
    return MODES[mode]


# ---- the steps ----------------------------------------------------------------------------------------

def view_dsm(dsm: torch.Tensor, grid: GroundGrid, camera: Camera, *, alt_lo, alt_hi, rect, stride=1) -> dict:
    """Cast the lines of sight of a pixel lattice of ``camera`` onto ``dsm``, an (H, W) float32 device raster
    on ``grid``.  ``rect`` = (col0, row0, n_cols, n_rows) and ``stride`` give the lattice: entry (r, c) is
    image pixel (col0 + c·stride, row0 + r·stride), whole pixels of the camera's (rescaled) image.  The
    segment of a pixel runs from its localisation at ``alt_hi`` to the one at ``alt_lo``; the DSM must lie
    between the two where it is to be hit.  Returns (n_rows, n_cols[, 2]) device tensors: ``hit`` uint8,
    ``altitude`` float32, ``ground`` float64 (E, N), ``cell`` float32 (x, y) — the fractional grid
    coordinate of the crossing, cell centres at whole numbers, what ``sample_at`` reads — and ``depth``
    float32, metres from the ``alt_hi`` end of the segment.  A pixel whose segment meets no finite cell
    is a miss: ``hit`` 0 and NaN elsewhere.  Non-finite cells are transparent.  The walk stands on the
    cell-centre lines the segment crosses along its major axis, and one beyond its end: a segment that crosses
    none of them reads nothing, so ``alt_hi − alt_lo`` has to carry the line of sight across several cells."""
    grid = _check_grid(grid)
    _check_raster("dsm", dsm, grid.shape)
    camera = _check_camera(camera)
    alt_lo, alt_hi = _check_altitudes(alt_lo, alt_hi)
    (col0, row0, n_cols, n_rows), stride = _check_lattice(rect, stride)
    dev = _one_device(dsm)
    L = _dsmview_lib.lib()
    dsm = dsm.contiguous()
    cam = _camera_table([camera], dev)
    nbytes = L.spnerf_dsmview_workspace_bytes(grid.ysize, grid.xsize)
    if nbytes < 0:
        _lib.check(int(nbytes), "dsmview_workspace_bytes")
    ws = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dev)
    out = {"hit": torch.empty((n_rows, n_cols), dtype=torch.uint8, device=dev),
           "altitude": torch.empty((n_rows, n_cols), dtype=torch.float32, device=dev),
           "ground": torch.empty((n_rows, n_cols, 2), dtype=torch.float64, device=dev),
           "cell": torch.empty((n_rows, n_cols, 2), dtype=torch.float32, device=dev),
           "depth": torch.empty((n_rows, n_cols), dtype=torch.float32, device=dev)}
    _lib.check(L.spnerf_dsmview_cast(ctypes.byref(_grid_struct(grid)), _lib.ptr(dsm), _lib.ptr(cam), alt_lo, alt_hi, col0, row0, stride,
                                     n_cols, n_rows, _lib.ptr(ws), _lib.ptr(out["hit"]), _lib.ptr(out["altitude"]), _lib.ptr(out["ground"]),
                                     _lib.ptr(out["cell"]), _lib.ptr(out["depth"]), _lib.stream_of(dsm)), "dsmview_cast")
    return out


def sample_at(raster: torch.Tensor, cell: torch.Tensor, mode="nearest") -> torch.Tensor:
    """``raster``, an (H, W) float32 device tensor on the grid, read at ``cell`` (..., 2) float32 [x, y] as
    ``view_dsm`` returns it: ``"nearest"`` is the cell the crossing lies in, whatever it holds;
    ``"bilinear"`` the four surrounding centres with non-finite entries left out and the weights
    renormalised (``upsample_dsm``'s rule).  NaN at a miss.  Returns ``cell``'s shape without its last axis."""
    _check_raster("raster", raster)
    if not isinstance(cell, torch.Tensor) or cell.dim() < 1 or cell.shape[-1] != 2 or cell.numel() == 0 or cell.dtype != torch.float32:
        raise ValueError(f"cell must be a non-empty (..., 2) float32 tensor, got {_what(cell)}")
    mode = _check_mode(mode)
    dev = _one_device(raster, cell)
    L = _dsmview_lib.lib()
    raster, cell = raster.contiguous(), cell.contiguous()
    out = torch.empty(tuple(cell.shape[:-1]), dtype=torch.float32, device=dev)
    _lib.check(L.spnerf_dsmview_sample(_lib.ptr(raster), raster.shape[0], raster.shape[1], _lib.ptr(cell), out.numel(), mode, _lib.ptr(out),
                                       _lib.stream_of(out)), "dsmview_sample")
    return out


def hit_ecef(ground: torch.Tensor, altitude: torch.Tensor, grid: GroundGrid) -> torch.Tensor:
    """(..., 3) float64 ECEF of the points ``ground`` (..., 2) float64 (E, N) in ``grid``'s UTM zone at
    ``altitude`` (...) float32: the inverse transverse Mercator projection and the geodetic-to-ECEF formula
    in fp64 (a kernel: the two device functions the ray generator and ``ortho_rays`` use, where torch
    would restate both series).  NaN propagates."""
    grid = _check_grid(grid)
    if not isinstance(ground, torch.Tensor) or ground.dim() < 1 or ground.shape[-1] != 2 or ground.numel() == 0 or ground.dtype != torch.float64:
        raise ValueError(f"ground must be a non-empty (..., 2) float64 tensor, got {_what(ground)}")
    if not isinstance(altitude, torch.Tensor) or altitude.dtype != torch.float32 or tuple(altitude.shape) != tuple(ground.shape[:-1]):
        raise ValueError(f"altitude must be a float32 tensor of shape {tuple(ground.shape[:-1])}, got {_what(altitude)}")
    dev = _one_device(ground, altitude)
    L = _dsmview_lib.lib()
    ground, altitude = ground.contiguous(), altitude.contiguous()
    out = torch.empty(tuple(altitude.shape) + (3,), dtype=torch.float64, device=dev)
    _lib.check(L.spnerf_dsmview_ecef(_lib.ptr(ground), _lib.ptr(altitude), altitude.numel(), grid.zone, 1 if grid.south else 0, _lib.ptr(out),
                                     _lib.stream_of(out)), "dsmview_ecef")
    return out


def normalised_depth(depth: torch.Tensor, range) -> torch.Tensor:
    """``view_dsm``'s ``depth`` (metres from the ``alt_hi`` end of the segment) in the trainer's units:
    divided by ``range`` — ``satellite.scene_normalisation``'s second result — in fp32, as ``normalize_rays``
    scales near and far.  A distance does not move with the scene's centre, so only the range is taken.  The
    segment's end is the near point of ``get_rays`` at the same altitudes; its metric is (E, N, altitude),
    which differs from ECEF's by the projection's scale factor (4e-4 of the horizontal part at most)."""
    if not isinstance(depth, torch.Tensor) or depth.dtype != torch.float32:
        raise ValueError(f"depth must be a float32 tensor, got {_what(depth)}")
    if isinstance(range, np.floating):
        range = float(range)
    rng = _check_real("range", range, "finite and > 0", lambda x: x > 0)
    return depth / torch.tensor(np.float32(rng), device=depth.device)


META_KEYS = ("rpc", "height", "width", "min_alt", "max_alt")


def dsm_depth_priors(dsm: torch.Tensor, weight: torch.Tensor, grid: GroundGrid, metas, *, alt_lo, alt_hi, stride=1, min_weight=None,
                     rect=None) -> list:
    """Depth priors for ``dataset.load_depth_data`` from a DSM and a per-cell weight, both (H, W) float32
    device rasters on ``grid`` — a sweep's ``altitude`` and ``score``.  ``metas`` are the full-resolution
    camera metadata of the images (``rpc``, ``height``, ``width``, ``min_alt``, ``max_alt``).  Per image the
    pixels (col0 + c·stride, row0 + r·stride) of ``rect`` = (col0, row0, n_cols, n_rows) — the whole image
    when None — are cast with ``view_dsm``; a pixel is kept when it hits, its weight
    ``sample_at(weight, cell, "nearest")`` is finite and, with ``min_weight``, not below it.  Returns one
    dict per image: its metadata and ``pts2d`` (K, 2) int64 [col, row] in raster order (on the host),
    ``pts3d`` (K, 3) float64 ECEF of the crossings (``hit_ecef``) and ``correl`` (K,) float32, on the device.
    The list goes into ``load_depth_data`` as it is (which needs K >= 1 for every image and casts ``pts3d``
    to float32: a quantisation of the ECEF coordinates, measured in DESIGN.md §8.19)."""
    grid = _check_grid(grid)
    _check_raster("dsm", dsm, grid.shape)
    _check_raster("weight", weight, grid.shape)
    alt_lo, alt_hi = _check_altitudes(alt_lo, alt_hi)
    if min_weight is not None:
        min_weight = _check_real("min_weight", min_weight, "finite or None", lambda x: True)
    metas = list(metas) if isinstance(metas, (list, tuple)) else None
    if not metas:
        raise ValueError("metas must be a non-empty list of camera metadata")
    lattices = []
    for i, m in enumerate(metas):
        if not isinstance(m, dict) or any(k not in m for k in META_KEYS):
            raise ValueError(f"metas[{i}] must be a dict with {', '.join(META_KEYS)}")
        h, w = int(m["height"]), int(m["width"])
        _check_int("stride", stride, 1, INT32_MAX)
        r = rect if rect is not None else (0, 0, (w - 1) // stride + 1, (h - 1) // stride + 1)
        (col0, row0, n_cols, n_rows), s = _check_lattice(r, stride)
        if col0 < 0 or row0 < 0 or col0 + (n_cols - 1) * s >= w or row0 + (n_rows - 1) * s >= h:
            raise ValueError(f"rect {tuple(r)!r} with stride {s} leaves the {h} x {w} image of metas[{i}]")
        lattices.append((col0, row0, n_cols, n_rows))
    _one_device(dsm, weight)
    out = []
    for m, lattice in zip(metas, lattices):
        col0, row0, n_cols, _ = lattice
        view = view_dsm(dsm, grid, Camera.from_meta(m, 1), alt_lo=alt_lo, alt_hi=alt_hi, rect=lattice, stride=stride)
        w = sample_at(weight, view["cell"], "nearest")
        keep = (view["hit"] == 1) & torch.isfinite(w)
        if min_weight is not None:
            keep &= w >= min_weight
        at = torch.nonzero(keep.reshape(-1)).reshape(-1)      # raster order: strictly increasing in row·width + col
        pts2d = torch.stack([col0 + (at % n_cols) * stride, row0 + (at // n_cols) * stride], 1)
        ground, altitude = view["ground"].reshape(-1, 2)[at], view["altitude"].reshape(-1)[at]
        pts3d = hit_ecef(ground, altitude, grid) if at.numel() else torch.empty((0, 3), dtype=torch.float64, device=dsm.device)
        out.append({**m, "pts2d": pts2d.cpu(), "pts3d": pts3d, "correl": w.reshape(-1)[at]})
    return out
