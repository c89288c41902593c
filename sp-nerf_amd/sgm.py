"""The plane sweep's score volume regularised across cells by semi-global aggregation (csrc/sgm.hip,
include/spnerf_amd_sgm.h), after Hirschmüller (2008).

``plane_sweep`` picks each cell's plane on its own, so an ambiguous window — a repetitive roof, water,
a shadow that moved between acquisitions — takes whichever plane happens to score highest.
``aggregate`` turns the (K, H, W) scores into costs, accumulates them along 4 or 8 scanline directions
with a penalty ``p1`` for a change of one plane between neighbouring cells and ``p2`` for a jump, and
returns the average on the score scale; ``pick`` is the sweep's pick on that volume plus the raw score at
the chosen plane; ``smooth_sweep`` is ``plane_sweep(volume=True)`` → ``aggregate`` → ``pick``.  The header
states every operation and its order: everything is fp32 and the results are those bytes.

Not there: occlusion-aware aggregation, a ``p2`` that follows the image gradients, and filling of the
cells no plane could be scored at (they stay NaN / −1, though paths cross them at a flat cost).
"""
from __future__ import annotations

import ctypes
import numbers

import torch

from . import _lib, _sgm_lib
from . import sweep as _sweep
from ._ground import _check_int, _check_real, _one_device, _what

MAX_PLANES = _sgm_lib.SGM_MAX_PLANES
# the defaults, chosen on the 512 x 512 JAX_269 ROI, 64 planes half a metre apart, radius 2 (profiles/r22/sgm.txt,
# DESIGN.md §8.16): a jump costs the whole range of a ZNCC cost, a step of one plane an eighth of that
P1 = 0.25
P2 = 2.0


# ---- argument checks: everything below is decided on the host, before any device is touched ------

def _f32(x):
    return ctypes.c_float(x).value


def _check_penalties(p1, p2, unscored, paths):
    p1 = _check_real("p1", p1, "finite and >= 0", lambda x: x >= 0 and abs(_f32(x)) != float("inf"))
    p2 = _check_real("p2", p2, f"finite and >= p1 {p1!r}", lambda x: x >= p1 and abs(_f32(x)) != float("inf"))
    unscored = _check_real("unscored", unscored, "finite", lambda x: abs(_f32(x)) != float("inf"))
    if not isinstance(paths, numbers.Integral) or isinstance(paths, bool) or paths not in (4, 8):
        raise ValueError(f"paths {paths!r} must be 4 or 8")
    return p1, p2, unscored, int(paths)


def _check_volume(name, volume):
    if not isinstance(volume, torch.Tensor) or volume.dim() != 3 or volume.numel() == 0 or volume.dtype != torch.float32:
        raise ValueError(f"{name} must be a non-empty (K, H, W) float32 tensor, got {_what(volume)}")
    _check_int("planes", volume.shape[0], 1, MAX_PLANES)
    if volume.shape[1] * volume.shape[2] > 2 ** 32:
        raise ValueError(f"a grid of {volume.shape[2]} x {volume.shape[1]} cells is too large for one call")


# ---- the steps ----------------------------------------------------------------------------------------

def workspace_bytes(planes, height, width, paths=8) -> int:
    """The bytes of device memory one ``aggregate`` call of these sizes works in (it allocates them itself):
    (1 + paths) cell-major copies of the volume and a byte per cell."""
    n = ctypes.c_int64(0)
    L = _sgm_lib.lib()
    _lib.check(L.spnerf_sgm_workspace_bytes(planes, height, width, paths, ctypes.byref(n)), "sgm_workspace_bytes")
    return n.value


def aggregate(volume: torch.Tensor, *, p1=P1, p2=P2, unscored=1.0, paths=8) -> torch.Tensor:
    """The (K, H, W) float32 score ``volume`` (higher is better, NaN or ±inf unscored) aggregated along
    ``paths`` directions: the cost 1 − score (``unscored`` where there is none) accumulated along every
    scanline with ``p1`` added for a neighbouring cell one plane away and ``p2`` for one further away,
    averaged over the directions and returned as 1 − cost, a (K, H, W) float32 tensor ``pick`` and
    ``sweep.pick_plane`` take as it is.  NaN at every plane of a cell without any scored plane."""
    _check_volume("volume", volume)
    p1, p2, unscored, paths = _check_penalties(p1, p2, unscored, paths)
    dev = _one_device(volume)
    L = _sgm_lib.lib()
    volume = volume.contiguous()
    K, H, W = volume.shape
    out = torch.empty_like(volume)
    work = torch.empty(workspace_bytes(K, H, W, paths), dtype=torch.uint8, device=dev)
    _lib.check(L.spnerf_sgm_aggregate(_lib.ptr(volume), K, H, W, p1, p2, unscored, paths, _lib.ptr(out), _lib.ptr(work), work.numel(),
                                      _lib.stream_of(volume)), "sgm")
    return out


def pick(aggregated: torch.Tensor, volume: torch.Tensor, alt_lo, step) -> dict:
    """The sweep's pick over an ``aggregated`` (K, H, W) float32 volume, plane k at ``alt_lo + k·step``:
    ``index`` (H, W) int32, −1 where every plane is NaN; ``altitude`` (H, W) float32, refined by the
    parabola through the two neighbouring planes; ``score``, the aggregated value at ``index``; and
    ``photo``, the raw score of ``volume`` there (NaN at −1 or where that entry was unscored)."""
    _check_volume("aggregated", aggregated)
    if not isinstance(volume, torch.Tensor) or volume.dtype != torch.float32 or tuple(volume.shape) != tuple(aggregated.shape):
        raise ValueError(f"volume must be a {tuple(aggregated.shape)} float32 tensor, got {_what(volume)}")
    alt_lo = _check_real("alt_lo", alt_lo, "finite", lambda x: True)
    step = _check_real("step", step, "finite and > 0", lambda x: x > 0)
    dev = _one_device(aggregated, volume)
    L = _sgm_lib.lib()
    aggregated, volume = aggregated.contiguous(), volume.contiguous()
    K, H, W = aggregated.shape
    out = {"altitude": torch.empty((H, W), dtype=torch.float32, device=dev), "score": torch.empty((H, W), dtype=torch.float32, device=dev),
           "index": torch.empty((H, W), dtype=torch.int32, device=dev), "photo": torch.empty((H, W), dtype=torch.float32, device=dev)}
    _lib.check(L.spnerf_sgm_pick(_lib.ptr(aggregated), _lib.ptr(volume), K, H * W, alt_lo, step, _lib.ptr(out["altitude"]),
                                 _lib.ptr(out["score"]), _lib.ptr(out["index"]), _lib.ptr(out["photo"]), _lib.stream_of(aggregated)),
               "sgm_pick")
    return out


def smooth_sweep(images, cameras, grid, alt_lo, step, planes, *, radius=2, min_views=2, min_std=0.0, p1=P1, p2=P2, unscored=1.0,
                 paths=8, volume=False, confidence=False) -> dict:
    """``plane_sweep(volume=True)`` → ``aggregate`` → ``pick``: the swept DSM with its planes chosen
    jointly across cells.  Returns a dict of (H, W) device tensors — ``altitude``, ``score`` (the
    aggregated value), ``index`` and ``photo`` (the raw ZNCC at the chosen plane) — and with
    ``volume=True`` also ``volume`` and ``aggregated`` (K, H, W).  ``altitude`` feeds ``orthorectify`` and
    ``cast_shadows`` as the sweep's does.  With ``confidence=True`` also ``confidence``, the dict
    ``volume_confidence`` gives for the aggregated volume at its defaults, and ``confidence_raw``, the same
    for the raw one; every other plane is what it is without."""
    cams, _, _ = _sweep._check_scene(images, cameras, grid)
    _sweep._check_planes(alt_lo, step, planes)
    _check_int("planes", planes, 1, MAX_PLANES)
    _sweep._check_window(len(cams), radius, min_views, min_std)
    _check_penalties(p1, p2, unscored, paths)
    if not isinstance(volume, bool):
        raise ValueError(f"volume {volume!r} must be a bool")
    if not isinstance(confidence, bool):
        raise ValueError(f"confidence {confidence!r} must be a bool")
    raw = _sweep.plane_sweep(images, cameras, grid, alt_lo, step, planes, radius=radius, min_views=min_views, min_std=min_std,
                             volume=True)["volume"]
    agg = aggregate(raw, p1=p1, p2=p2, unscored=unscored, paths=paths)
    out = pick(agg, raw, alt_lo, step)
    if volume:
        out["volume"], out["aggregated"] = raw, agg
    if confidence:
        from .confidence import volume_confidence
        out["confidence"], out["confidence_raw"] = volume_confidence(agg, alt_lo, step), volume_confidence(raw, alt_lo, step)
    return out
