"""A swept DSM cleaned between the steps of the ground-grid chain (csrc/clean.hip,
include/staged/spnerf_amd_clean.h): what the classical stereo chain (s2p, OpenCV's SGBM) does after the
aggregation.

``speckle_filter`` labels the connected components of the raster — two finite 4-neighbours are joined when
their heights differ by at most ``max_diff`` — and drops the components of at most ``max_size`` cells;
``median_dsm`` replaces a cell by the lower median of the finite values in its window; ``fill_holes`` gives a
hole the lowest or the nearest of the first finite values met in eight directions; ``clean_dsm`` chains the
three behind an optional weight threshold; ``bootstrap_sweep`` is ``refine_sweep`` with ``clean_dsm`` between
its two passes, so that an upward outlier of the first pass no longer hides the cells behind it.  Every
raster is an (H, W) float32 device tensor, row 0 the northernmost; a cell that is not finite is a hole; inputs
are never written.  The header states every operation: nothing rounds, and the results are the bytes of the
numpy statement (tests/clean_numpy.py).

Not there: occlusion-aware aggregation, and an edge-aware fill guided by the ortho mosaic.
"""
from __future__ import annotations

import ctypes

import torch

from . import _clean_abi, _lib, sgm
from . import sweep as _sweep
from ._ground import _check_int, _check_raster, _check_real, _one_device

TILE = _clean_abi.CLEAN_TILE
MAX_RADIUS = _clean_abi.CLEAN_MAX_RADIUS
MAX_REACH = _clean_abi.CLEAN_MAX_REACH
MODES = {"lowest": _clean_abi.CLEAN_LOWEST, "nearest": _clean_abi.CLEAN_NEAREST}
MAX_CELLS = 2 ** 31 - 1
REJECTED_WEIGHT, REJECTED_SPECKLE, REJECTED_MEDIAN = 1, 2, 4
# bootstrap_sweep's defaults, chosen on the 512 x 512 JAX_269 ROI, 64 planes half a metre apart (profiles/r26/clean.txt,
# DESIGN.md §8.20): the row of the lowest altitude MAE against the lidar among max_size 25 / 100 / 400 / 1600 cells,
# max_diff 1 / 2 steps, median radius 0 / 1 / 2, min_weight None / 0.25.  100 cells are 25 m² at 0.5 m.  The rows from
# max_size 100 upwards lie within 0.3 m of one another, so this is a shallow choice
SPECKLE_CELLS = 100
MAX_DIFF_STEPS = 2
MEDIAN_RADIUS = 0
MIN_WEIGHT = 0.25
# what bootstrap_sweep's prior may be gated on: the first pass's raw ZNCC at the pick, or a plane volume_confidence
# takes from the first pass's aggregated volume
WEIGHTS = ("photo", "margin", "peak_margin", "curvature", "mlm")


# ---- argument checks: everything below is decided on the host, before any device is touched ------

def _f32(x):
    return ctypes.c_float(x).value


def _check_cells(name, dsm):
    _check_raster(name, dsm)
    if dsm.shape[0] * dsm.shape[1] > MAX_CELLS:
        raise ValueError(f"a grid of {dsm.shape[1]} x {dsm.shape[0]} cells is too large for one call")


def _check_speckle(max_diff, max_size):
    max_diff = _check_real("max_diff", max_diff, "finite and >= 0", lambda x: x >= 0 and abs(_f32(x)) != float("inf"))
    return max_diff, _check_int("max_size", max_size, 0, MAX_CELLS)


def _check_median(radius, min_count, fill, lowest=1):
    radius = _check_int("radius", radius, lowest, MAX_RADIUS)
    min_count = _check_int("min_count", min_count, 1, max((2 * radius + 1) ** 2, 1))
    if not isinstance(fill, bool):
        raise ValueError(f"fill {fill!r} must be a bool")
    return radius, min_count, fill


def _check_fill(reach, mode, min_dirs):
    reach = _check_int("reach", reach, 1, MAX_REACH)
    if not isinstance(mode, str) or mode not in MODES:
        raise ValueError(f"mode {mode!r} is neither 'lowest' nor 'nearest'")
    return reach, MODES[mode], _check_int("min_dirs", min_dirs, 1, 8)


def _check_weight(weight, min_weight, shape=None):
    if (weight is None) != (min_weight is None):
        raise ValueError("weight and min_weight go together: give both or neither")
    if weight is None:
        return None
    if shape is not None:
        _check_raster("weight", weight, shape)
    return _check_real("min_weight", min_weight, "finite", lambda x: True)


def _check_chain(max_diff, max_size, radius, reach, mode, min_dirs):
    max_diff, max_size = _check_speckle(max_diff, max_size)
    radius = _check_int("radius", radius, 0, MAX_RADIUS)
    if reach is None:
        _check_fill(1, mode, min_dirs)
    else:
        _check_fill(reach, mode, min_dirs)
    return max_diff, max_size, radius


# ---- the steps ----------------------------------------------------------------------------------------

def workspace_bytes(height, width) -> int:
    """The bytes of device memory one ``speckle_filter`` call of this size works in (it allocates them itself):
    two int32 planes and the 16 bytes of the iteration bound's word."""
    n = ctypes.c_int64(0)
    _lib.check(_clean_abi.lib().spnerf_clean_workspace_bytes(height, width, ctypes.byref(n)), "clean_workspace_bytes")
    return n.value


def _speckle(dsm, max_diff, max_size):
    """``speckle_filter``'s dict and the workspace it ran in (whose last four int32 hold the bound's word)."""
    dev = _one_device(dsm)
    L = _clean_abi.lib()
    dsm = dsm.contiguous()
    H, W = dsm.shape
    out = {"dsm": torch.empty_like(dsm), "label": torch.empty((H, W), dtype=torch.int32, device=dev),
           "size": torch.empty((H, W), dtype=torch.int32, device=dev)}
    work = torch.empty(workspace_bytes(H, W) // 4, dtype=torch.int32, device=dev)
    _lib.check(L.spnerf_clean_speckle(_lib.ptr(dsm), H, W, max_diff, max_size, _lib.ptr(out["dsm"]), _lib.ptr(out["label"]), _lib.ptr(out["size"]),
                                      _lib.ptr(work), work.numel() * 4, _lib.stream_of(dsm)), "clean_speckle")
    return out, work


def speckle_filter(dsm: torch.Tensor, *, max_diff, max_size) -> dict:
    """The components of ``dsm`` under "finite 4-neighbours whose heights differ by at most ``max_diff``" and the
    raster without the small ones: ``label`` (H, W) int32, the smallest linear index ``y·W + x`` of the cell's
    component, −1 at a hole; ``size`` (H, W) int32, the component's cells, 0 at a hole; ``dsm``, NaN where
    ``1 <= size <= max_size`` and the input elsewhere (an inf stays an inf).  ``max_size`` 0 removes nothing.  The
    call waits for the device: it reads back whether a bounded loop of the labelling ran out, which is raised as a
    ``SpnerfError`` and never happens on a correct build."""
    _check_cells("dsm", dsm)
    max_diff, max_size = _check_speckle(max_diff, max_size)
    return _speckle(dsm, max_diff, max_size)[0]


def median_dsm(dsm: torch.Tensor, *, radius=1, min_count=1, fill=False) -> torch.Tensor:
    """The lower median of the finite values in the (2·``radius``+1)² window around every cell, clipped to the
    grid: always one of the inputs, a zero as +0; NaN where fewer than ``min_count`` values are finite.  A hole
    stays as it is unless ``fill``."""
    _check_cells("dsm", dsm)
    radius, min_count, fill = _check_median(radius, min_count, fill)
    _one_device(dsm)
    L = _clean_abi.lib()
    dsm = dsm.contiguous()
    out = torch.empty_like(dsm)
    _lib.check(L.spnerf_clean_median(_lib.ptr(dsm), dsm.shape[0], dsm.shape[1], radius, min_count, 1 if fill else 0, _lib.ptr(out),
                                     _lib.stream_of(dsm)), "clean_median")
    return out


def fill_holes(dsm: torch.Tensor, *, reach, mode="lowest", min_dirs=1) -> dict:
    """Every hole of ``dsm`` filled from the first finite cells met within ``reach`` steps in the eight directions
    E, NE, N, NW, W, SW, S, SE, when at least ``min_dirs`` of them found one: ``mode`` "lowest" writes the minimum
    (the background behind an occlusion), "nearest" the one at the smallest distance, the earlier direction on a
    tie.  Returns ``dsm`` and ``filled`` (H, W) uint8, 1 where a value was written."""
    _check_cells("dsm", dsm)
    reach, mode, min_dirs = _check_fill(reach, mode, min_dirs)
    dev = _one_device(dsm)
    L = _clean_abi.lib()
    dsm = dsm.contiguous()
    H, W = dsm.shape
    out = {"dsm": torch.empty_like(dsm), "filled": torch.empty((H, W), dtype=torch.uint8, device=dev)}
    _lib.check(L.spnerf_clean_fill(_lib.ptr(dsm), H, W, reach, mode, min_dirs, _lib.ptr(out["dsm"]), _lib.ptr(out["filled"]), _lib.stream_of(dsm)),
               "clean_fill")
    return out


def clean_dsm(dsm: torch.Tensor, *, weight=None, min_weight=None, max_diff, max_size, radius=1, reach=None, mode="lowest", min_dirs=1) -> dict:
    """The chain, in this order: cells whose ``weight`` (H, W) float32 is below ``min_weight`` or NaN become NaN
    (both or neither are given); ``speckle_filter(max_diff, max_size)``; ``median_dsm(radius, fill=False)`` unless
    ``radius`` is 0; ``fill_holes(reach, mode, min_dirs)`` unless ``reach`` is None.  Returns ``dsm``; ``rejected``
    (H, W) uint8, a bit mask over the cells that were finite when their step ran — 1: taken out by the weight,
    2: by the speckle filter, 4: value changed by the median; ``filled`` (zero without a fill); and the speckle
    filter's ``label`` and ``size``.  ``max_diff`` and ``max_size`` have no default: they depend on the cell size
    and the plane step."""
    _check_cells("dsm", dsm)
    min_weight = _check_weight(weight, min_weight, dsm.shape)
    max_diff, max_size, radius = _check_chain(max_diff, max_size, radius, reach, mode, min_dirs)
    _one_device(*([dsm] if weight is None else [dsm, weight]))
    rejected = torch.zeros(dsm.shape, dtype=torch.uint8, device=dsm.device)
    cur = dsm
    if weight is not None:
        low = torch.isfinite(cur) & ~(weight >= min_weight)
        rejected |= low.to(torch.uint8) * REJECTED_WEIGHT
        cur = torch.where(low, torch.full_like(cur, float("nan")), cur)
    speckle = speckle_filter(cur, max_diff=max_diff, max_size=max_size)
    rejected |= (torch.isfinite(cur) & ~torch.isfinite(speckle["dsm"])).to(torch.uint8) * REJECTED_SPECKLE
    cur = speckle["dsm"]
    if radius:
        smooth = median_dsm(cur, radius=radius)
        rejected |= (torch.isfinite(cur) & (smooth != cur)).to(torch.uint8) * REJECTED_MEDIAN
        cur = smooth
    if reach is not None:
        filled = fill_holes(cur, reach=reach, mode=mode, min_dirs=min_dirs)
        cur, mask = filled["dsm"], filled["filled"]
    else:
        mask = torch.zeros(dsm.shape, dtype=torch.uint8, device=dsm.device)
    return {"dsm": cur, "rejected": rejected, "filled": mask, "label": speckle["label"], "size": speckle["size"]}


def bootstrap_sweep(images, cameras, grid, alt_lo, step, planes, *, max_diff=None, max_size=None, radius=MEDIAN_RADIUS, min_weight=MIN_WEIGHT,
                    reach=None, mode="lowest", min_dirs=1, slack=None, sweep_radius=2, min_views=2, min_std=0.0, p1=sgm.P1, p2=sgm.P2, unscored=1.0,
                    paths=8, volume=False, weight="photo") -> dict:
    """``refine_sweep`` from its own first pass with the outliers taken out of the prior: ``smooth_sweep``, then
    ``clean_dsm`` of its ``altitude`` (with its ``photo``, the raw ZNCC at the pick, as the weight unless
    ``min_weight`` is None), then ``refine_sweep(prior=cleaned)``.  Returns ``refine_sweep``'s dict plus ``first``
    (the first pass's altitude) and ``cleaned`` (``clean_dsm``'s dict).  ``max_diff`` defaults to ``MAX_DIFF_STEPS``
    ``step``s, ``max_size`` to ``SPECKLE_CELLS``, ``slack`` to one ``step``; ``radius`` is the median's (0: none) and
    ``sweep_radius`` the ZNCC window's, ``refine_sweep``'s ``radius``.  With ``reach=None`` the cleaned prior keeps its
    holes: the floor's march skips NaN, so a removed outlier hides nothing.  ``weight`` names what ``min_weight`` gates:
    "photo", or one of "margin", "peak_margin", "curvature", "mlm" — that plane of ``volume_confidence`` over the first
    pass's aggregated volume at its defaults (a NaN there, no second peak or no neighbour, is rejected like any NaN
    weight); ``min_weight`` is then on that plane's scale and has no default worth keeping.  On the JAX_269 ROI this takes the two-pass
    sweep from 12.4 m back to ``smooth_sweep``'s 7.6 m of altitude MAE, not below it."""
    from . import occlusion
    cams, imgs, grid = _sweep._check_scene(images, cameras, grid)
    alt_lo, step, K = _sweep._check_planes(alt_lo, step, planes)
    _check_int("planes", K, 2, sgm.MAX_PLANES)
    _sweep._check_window(len(cams), sweep_radius, min_views, min_std)
    sgm._check_penalties(p1, p2, unscored, paths)
    if slack is not None:
        occlusion._check_slack(slack)
    if not isinstance(volume, bool):
        raise ValueError(f"volume {volume!r} must be a bool")
    max_diff = MAX_DIFF_STEPS * step if max_diff is None else max_diff
    max_size = SPECKLE_CELLS if max_size is None else max_size
    _check_chain(max_diff, max_size, radius, reach, mode, min_dirs)
    if grid.shape[0] * grid.shape[1] > MAX_CELLS:
        raise ValueError(f"a grid of {grid.shape[1]} x {grid.shape[0]} cells is too large for one call")
    if min_weight is not None:
        _check_real("min_weight", min_weight, "finite", lambda x: True)
    if not isinstance(weight, str) or weight not in WEIGHTS:
        raise ValueError(f"weight {weight!r} must be one of {', '.join(map(repr, WEIGHTS))}")
    _one_device(*imgs)
    kw = dict(radius=sweep_radius, min_views=min_views, min_std=min_std, p1=p1, p2=p2, unscored=unscored, paths=paths)
    if weight == "photo" or min_weight is None:
        first = sgm.smooth_sweep(images, cameras, grid, alt_lo, step, K, **kw)
        gate = first["photo"]
    else:
        from .confidence import volume_confidence
        first = sgm.smooth_sweep(images, cameras, grid, alt_lo, step, K, volume=True, **kw)
        gate = volume_confidence(first["aggregated"], alt_lo, step, planes=(weight,))[weight]
    cleaned = clean_dsm(first["altitude"], weight=None if min_weight is None else gate, min_weight=min_weight, max_diff=max_diff,
                        max_size=max_size, radius=radius, reach=reach, mode=mode, min_dirs=min_dirs)
    out = occlusion.refine_sweep(images, cameras, grid, alt_lo, step, K, prior=cleaned["dsm"], slack=slack, volume=volume, **kw)
    out["first"], out["cleaned"] = first["altitude"], cleaned
    return out
