"""How unambiguous each cell's pick is, read from the sweep's (K, H, W) score volume (csrc/confidence.hip,
include/staged/spnerf_amd_confidence.h), after the measures Hu & Mordohai (2012) compare for stereo.

``score`` and ``photo`` of the picks are the height of the peak; ``volume_confidence`` says whether the peak
stands alone: ``margin`` (best minus the best plane outside the pick's own peak), ``peak_margin`` (best minus the
next local maximum), ``peaks`` and ``support`` (local maxima and planes within ``tau`` of the best), ``curvature``
(of the parabola at the pick), ``mlm`` (the maximum-likelihood measure, 1 for a lone winner) and ``spread`` (the
RMS distance in metres of that distribution from the pick), with ``scored`` and ``index``.  Each is an (H, W)
raster that ``clean_dsm(weight=)``, ``dsm_depth_priors(weight=)`` and ``mosaic`` take as a weight.  The header
states every plane; all but ``mlm`` and ``spread`` are exact.  ``sparsification`` is the instrument that says
whether such a number is any good: the error of the cells kept as the least confident are removed.

Not there: a confidence inside ``pyramid_sweep``'s levels or ``surface_sweep``, a cross-check between view
subsets, the per-direction winners of the aggregation, and learned confidences; ``spread`` is not yet fed to
``load_depth_data`` as a prior's ``std``.
"""
from __future__ import annotations

import ctypes

import torch

from . import _confidence_abi, _lib, sgm
from ._ground import _check_int, _check_real, _one_device, _what

MAX_PLANES = _confidence_abi.CONF_MAX_PLANES
PLANES = tuple(name for name, _ in _confidence_abi.CONF_OUTPUTS)
_DTYPES = {"int32": torch.int32, "float32": torch.float32}
# the defaults, on the score scale: the rows of the lowest sparsification area on the aggregated volume of the 512 x 512
# JAX_269 ROI, 64 planes half a metre apart, among tau 0.02 / 0.05 / 0.1 and temperature 0.02 / 0.05 / 0.1 / 0.2
# (profiles/r27/confidence.txt): "-support, tau 0.1" (1.0623; no row that takes a tau beats a flat
# curve) and "-spread, temperature 0.2" (0.5461; mlm is lowest there too, 0.7566).  Both are the largest value tried, so
# the lowest area may lie beyond the grid
TAU = 0.1
TEMPERATURE = 0.2


# ---- argument checks: everything below is decided on the host, before any device is touched ------

def _f32(x):
    return ctypes.c_float(x).value


def _check_planes(planes):
    if planes is None:
        return PLANES
    names = None if isinstance(planes, str) else list(planes) if isinstance(planes, (list, tuple, set, frozenset)) else None
    if not names or any(not isinstance(n, str) or n not in PLANES for n in names):
        raise ValueError(f"planes {planes!r} must be None or a non-empty list of names among {', '.join(PLANES)}")
    return tuple(n for n in PLANES if n in names)


def _check_measure(tau, temperature, exclude):
    tau = _check_real("tau", tau, "finite and >= 0", lambda x: x >= 0 and abs(_f32(x)) != float("inf"))
    temperature = _check_real("temperature", temperature, "finite and > 0", lambda x: 0 < _f32(x) < float("inf"))
    return tau, temperature, _check_int("exclude", exclude, 1, 2 ** 31 - 1)


# ---- the launch -------------------------------------------------------------------------------------------

def volume_confidence(volume: torch.Tensor, alt_lo, step, *, tau=TAU, temperature=TEMPERATURE, exclude=1, planes=None) -> dict:
    """The confidence planes of a (K, H, W) float32 score ``volume`` (higher is better, NaN or ±inf unscored), plane
    k at ``alt_lo + k·step`` — ``plane_sweep(volume=True)``'s ``volume`` or ``aggregate``'s result — in one launch.
    Returns a dict of (H, W) device tensors: ``scored``, ``index``, ``peaks``, ``support`` int32 and ``margin``,
    ``peak_margin``, ``curvature``, ``mlm``, ``spread`` float32, or only those named in ``planes`` (the kernel
    skips what the others alone would need).  ``tau`` and ``temperature`` are on the score scale; ``exclude`` is
    how many planes on either side of the pick ``margin`` counts to the pick's own peak.  Where no plane is scored
    ``index`` is −1, every float plane NaN and every other int plane 0.  The defaults are the rows of the lowest
    sparsification area on the ROI's aggregated volume, "-support, tau 0.1" and "-spread, temperature 0.2"
    (DESIGN.md §8.21), each the largest value of its grid."""
    sgm._check_volume("volume", volume)
    alt_lo = _check_real("alt_lo", alt_lo, "finite", lambda x: True)
    step = _check_real("step", step, "finite and > 0", lambda x: x > 0)
    tau, temperature, exclude = _check_measure(tau, temperature, exclude)
    names = _check_planes(planes)
    dev = _one_device(volume)
    L = _confidence_abi.lib()
    volume = volume.contiguous()
    K, H, W = volume.shape
    out = {name: torch.empty((H, W), dtype=_DTYPES[kind], device=dev) for name, kind in _confidence_abi.CONF_OUTPUTS if name in names}
    _lib.check(L.spnerf_conf_volume(_lib.ptr(volume), K, H * W, alt_lo, step, tau, temperature, exclude, *[_lib.ptr(out.get(name)) for name in PLANES],
                                    _lib.stream_of(volume)), "conf_volume")
    return out


# ---- the instrument ---------------------------------------------------------------------------------------

def sparsification(error: torch.Tensor, confidence: torch.Tensor, *, steps=100) -> dict:
    """The sparsification curve of ``confidence`` against ``error`` (tensors of one shape, any float dtype): the
    cells at which both are finite, n of them, are sorted by descending confidence, ties by cell index (a stable
    sort); for the removed shares i / ``steps``, i = 0 … ``steps`` − 1, the n − ⌊n·i / steps⌋ most confident cells
    are kept and ``curve[i]`` is their mean error (float64).  ``area`` is the curve's integral over the removed
    share by the trapezoid rule divided by ``curve[0]``: 1 − 1 / ``steps`` for a confidence that says nothing (a flat
    curve), lower is better, and the lowest any confidence can reach is that of ``confidence = -error`` (the
    oracle).  Returns ``curve`` (a (steps,) float64 tensor on the inputs' device), ``area`` (a float) and ``cells``
    (n).  Plain torch: a measuring instrument, not a hot path."""
    for name, t in (("error", error), ("confidence", confidence)):
        if not isinstance(t, torch.Tensor) or not t.is_floating_point() or t.numel() == 0:
            raise ValueError(f"{name} must be a non-empty floating-point tensor, got {_what(t)}")
    if tuple(error.shape) != tuple(confidence.shape):
        raise ValueError(f"confidence {tuple(confidence.shape)} is not error's {tuple(error.shape)}")
    steps = _check_int("steps", steps, 2, 2 ** 20)
    if error.device != confidence.device:
        raise ValueError(f"the tensors of one call must be on one device, got {sorted({str(error.device), str(confidence.device)})}")
    err, conf = error.reshape(-1).double(), confidence.reshape(-1).double()
    both = torch.isfinite(err) & torch.isfinite(conf)
    err, conf = err[both], conf[both]
    n = int(err.numel())
    if n == 0:
        return {"curve": torch.full((steps,), float("nan"), dtype=torch.float64, device=error.device), "area": float("nan"), "cells": 0}
    order = torch.sort(conf, descending=True, stable=True).indices
    total = torch.cumsum(err[order], 0)
    kept = n - (n * torch.arange(steps, dtype=torch.int64, device=err.device)) // steps
    curve = total[kept - 1] / kept.double()
    area = float(((curve[:-1] + curve[1:]) * (0.5 / steps)).sum() / curve[0])
    return {"curve": curve, "area": area, "cells": n}
