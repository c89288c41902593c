"""Geometric shadows over a ground-grid DSM (csrc/shadow.hip, include/spnerf_amd_shadow.h).

Every other shadow of the project is the network's ``sun_v``: a learnt scalar that can be trusted
near the sun directions seen in training.  The DSM is the other source of truth: a cell is shadowed
when the terrain between it and the sun rises above the sun ray.  ``cast_shadows`` casts a DSM —
``render_ortho``'s, the lidar truth, any registered raster — under K sun directions without touching
the MLP, and ``shadow_agreement`` scores a learnt sun plane (``relight_ortho``'s "sun") against the
result: EO-NeRF's consistency of the learnt shadows with the learnt geometry, as numbers.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib, _shadow_lib
from ._ground import _check_dsm, _resolution
from .relight import _directions
from .satellite import sun_direction

NODATA = 255   # the shadow of a cell whose height is NaN


def sun_directions(sun_dirs) -> torch.Tensor:
    """(K, 3) vectors (east, north, up) pointing from the ground towards the sun, as
    ``satellite.sun_direction`` returns them, or (K, 2) (elevation°, azimuth°) pairs -> (K, 3) float32
    on the host, checked: finite, and the sun above the horizon (up > 0)."""
    if not isinstance(sun_dirs, torch.Tensor):
        sun_dirs = np.asarray(sun_dirs)
    if sun_dirs.ndim == 2 and sun_dirs.shape[1] == 2 and sun_dirs.shape[0] > 0:
        pairs = np.asarray(sun_dirs.detach().cpu() if isinstance(sun_dirs, torch.Tensor) else sun_dirs, np.float64)
        if not np.isfinite(pairs).all():
            raise ValueError("sun_dirs holds a non-finite direction")
        sun_dirs = np.stack([sun_direction(float(el), float(az)) for el, az in pairs])
    elif sun_dirs.ndim != 2 or sun_dirs.shape[1] != 3:
        raise ValueError(f"sun_dirs must be (K, 3) vectors or (K, 2) (elevation, azimuth) pairs in degrees, got "
                         f"{tuple(sun_dirs.shape)}")
    dirs = _directions(sun_dirs)
    low = torch.nonzero(~(dirs[:, 2] > 0)).reshape(-1)
    if low.numel():
        k = int(low[0])
        raise ValueError(f"sun_dirs[{k}] has up = {float(dirs[k, 2])}: a shadow is cast by a sun above the horizon "
                         "(the vector points from the ground towards the sun)")
    return dirs


def cast_shadows(dsm: torch.Tensor, resolution_or_grid, sun_dirs, excess: bool = False):
    """Cast the (H, W) device DSM ``dsm`` — float64, or float32 (widened) — row 0 the northernmost (the
    ``GroundGrid`` layout; ``render_ortho``'s "dsm"), cells of ``resolution_or_grid`` metres, under the K
    sun directions ``sun_dirs``: (K, 3) vectors as ``satellite.sun_direction`` returns them or (K, 2)
    (elevation°, azimuth°) pairs.  Returns ``shadow`` (K, H, W) uint8 on the device — 1 where the
    terrain towards the sun rises above the sun ray, 0 where it does not, 255 where the cell's own
    height is NaN — and with ``excess=True`` also ``excess`` (K, H, W) float64: by how many metres the
    highest occluder stands above the sun ray (negative: the clearance; −inf: nothing between the
    cell and the grid's edge; NaN where the height is).  ``shadow`` is the same either way.

    The march of a cell follows the grid along the major axis of the sun's azimuth, one column (or
    row) per step, interpolating the heights linearly across the other axis; NaN heights on the way
    are skipped.  Arithmetic is fp64; the result is bit-reproducible (include/spnerf_amd_shadow.h)."""
    _check_dsm("dsm", dsm)
    res = _resolution(resolution_or_grid, dsm.shape)
    dirs = sun_directions(sun_dirs)
    K, (H, W) = dirs.shape[0], dsm.shape
    if K > _shadow_lib.SHADOW_MAX_DIRS:
        raise ValueError(f"{K} directions in one call (at most {_shadow_lib.SHADOW_MAX_DIRS})")
    _lib.require_device(dsm)
    L = _shadow_lib.lib()
    dsm = dsm.double().contiguous()
    nbytes = L.spnerf_shadow_workspace_bytes(H, W)
    if nbytes < 0:
        _lib.check(int(nbytes), "shadow_workspace_bytes")
    ws = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dsm.device)
    shadow = torch.empty((K, H, W), dtype=torch.uint8, device=dsm.device)
    exc = torch.empty((K, H, W), dtype=torch.float64, device=dsm.device) if excess else None
    host = np.ascontiguousarray(dirs.numpy(), np.float32)
    _lib.check(L.spnerf_shadow_cast(_lib.ptr(dsm), H, W, res, host.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), K, _lib.ptr(ws),
                                    _lib.ptr(shadow), _lib.ptr(exc), _lib.stream_of(dsm)), "shadow_cast")
    return (shadow, exc) if excess else shadow


def shadow_agreement(sun: torch.Tensor, shadow: torch.Tensor) -> dict:
    """Score a learnt sun plane ``sun`` (K, H, W) float32 (``relight_ortho``'s "sun": 1 lit, 0
    shadowed) against cast shadows ``shadow`` (K, H, W) uint8, in one pass on the device and one
    device-to-host copy.  A cell counts when its shadow is 0 or 1 and its sun is finite.  Per
    direction, as length-K numpy arrays: ``n`` the counted cells, ``mae`` the mean of
    |sun − (1 − shadow)|, ``mean_sun_lit`` / ``mean_sun_shadow`` the mean sun over the lit / the
    shadowed cells, and ``iou`` of the shadowed set with the learnt one (sun < 0.5):
    tp / (tp + fp + fn).  A ratio is NaN where its denominator is 0.  The counts behind them come
    back too: ``n_lit``, ``n_shadow``, ``tp``, ``fp``, ``fn``."""
    for name, t, dtype in (("sun", sun, torch.float32), ("shadow", shadow, torch.uint8)):
        if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.numel() == 0 or t.dtype != dtype:
            what = f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
            raise ValueError(f"{name} must be a non-empty (K, H, W) {dtype} tensor, got {what}")
    if sun.shape != shadow.shape:
        raise ValueError(f"sun {tuple(sun.shape)} and shadow {tuple(shadow.shape)} must have the same shape")
    K, cells = sun.shape[0], sun.shape[1] * sun.shape[2]
    if K > _shadow_lib.SHADOW_MAX_DIRS:
        raise ValueError(f"{K} directions in one call (at most {_shadow_lib.SHADOW_MAX_DIRS})")
    _lib.require_device(sun, shadow)
    L = _shadow_lib.lib()
    sun, shadow = sun.contiguous(), shadow.to(sun.device).contiguous()
    nbytes = L.spnerf_shadow_agreement_workspace_bytes(cells, K)
    if nbytes < 0:
        _lib.check(int(nbytes), "shadow_agreement_workspace_bytes")
    ws = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=sun.device)
    res = torch.empty(K * _shadow_lib.RESULT_BYTES, dtype=torch.uint8, device=sun.device)
    _lib.check(L.spnerf_shadow_agreement(_lib.ptr(sun), _lib.ptr(shadow), cells, K, _lib.ptr(ws), _lib.ptr(res),
                                         _lib.stream_of(sun)), "shadow_agreement")
    raw = res.cpu().numpy().tobytes()                          # the one copy
    host = (_shadow_lib.ShadowAgreementResult * K).from_buffer_copy(raw)
    return scores_from_sums({f: np.array([getattr(r, f) for r in host]) for f, _ in _shadow_lib.ShadowAgreementResult._fields_})


def scores_from_sums(sums: dict) -> dict:
    """The ratios of ``shadow_agreement`` from the per-direction sums and counts of
    ``spnerf_shadow_agreement_result``; NaN where a denominator is 0."""
    def ratio(a, b):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        return np.divide(a, b, out=np.full(a.shape, np.nan), where=b != 0)

    n_lit, n_shadow = np.asarray(sums["n_lit"], np.int64), np.asarray(sums["n_shadow"], np.int64)
    tp, fp, fn = (np.asarray(sums[k], np.int64) for k in ("tp", "fp", "fn"))
    n = n_lit + n_shadow
    return {"n": n, "mae": ratio(sums["sum_abs"], n), "mean_sun_lit": ratio(sums["sum_sun_lit"], n_lit),
            "mean_sun_shadow": ratio(sums["sum_sun_shadow"], n_shadow), "iou": ratio(tp, tp + fp + fn),
            "n_lit": n_lit, "n_shadow": n_shadow, "tp": tp, "fp": fp, "fn": fn}
