"""ctypes signatures of the whole-view exports (include/spnerf_amd_view.h), applied to the same
libspnerf_amd.so handle as ``_lib.SIGNATURES``; errors come back through ``_lib.check``."""
from __future__ import annotations

import ctypes
from ctypes import POINTER, c_double, c_float, c_int32, c_int64, c_void_p

from . import _lib

SPNERF_VIEW_ABI_VERSION = 1
VIEW_MAX_CLASSES = 32


class ViewPlanes(ctypes.Structure):
    """spnerf_view_planes: device pointers of the image planes, NULL = skipped (64 bytes)."""
    _fields_ = [("rgb", c_void_p), ("depth", c_void_p), ("sun", c_void_p), ("albedo", c_void_p), ("sky", c_void_p),
                ("beta", c_void_p), ("sem_logits", c_void_p), ("sem_class", c_void_p)]


class ViewMetricsResult(ctypes.Structure):
    """spnerf_view_metrics_result: what the metrics finish leaves on the device."""
    _fields_ = [("mse", c_double), ("psnr", c_double), ("n", c_int64), ("correct", c_int64),
                ("table", c_int64 * ((VIEW_MAX_CLASSES + 1) * VIEW_MAX_CLASSES))]


# name → (restype, argtypes); the exact export list of include/spnerf_amd_view.h
SIGNATURES = {
    "spnerf_view_abi_version": (c_int32, []),
    "spnerf_view_composite_products": (c_int32, [c_int64, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_float, c_int32,
                                                 c_int32, c_int32, c_int64, POINTER(ViewPlanes), POINTER(_lib.Rng),
                                                 c_void_p]),
    "spnerf_view_metrics_workspace_bytes": (c_int64, [c_int64, c_int32]),
    "spnerf_view_metrics": (c_int32, [c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p,
                                      c_void_p]),
}

lib = _lib.bind(SIGNATURES, "spnerf_view_abi_version", SPNERF_VIEW_ABI_VERSION, "view")
