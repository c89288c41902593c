"""ctypes signatures of the LPIPS exports (include/spnerf_amd_lpips.h), applied to the same
libspnerf_amd.so handle as ``_lib.SIGNATURES``; errors come back through ``_lib.check``."""
from __future__ import annotations

import ctypes
from ctypes import POINTER, c_double, c_int32, c_int64, c_void_p

from . import _lib

SPNERF_LPIPS_ABI_VERSION = 1
LPIPS_TAPS = 5
LPIPS_MIN_SIDE = 31
LPIPS_MAX_SIDE = 8192


class LpipsResult(ctypes.Structure):
    """spnerf_lpips_result: what the LPIPS finish leaves on the device (88 bytes)."""
    _fields_ = [("lpips", c_double), ("layer", c_double * LPIPS_TAPS), ("h", c_int32 * LPIPS_TAPS), ("w", c_int32 * LPIPS_TAPS)]


_PTRS = POINTER(c_void_p)   # a host array of device pointers

# name → (restype, argtypes); the exact export list of include/spnerf_amd_lpips.h
SIGNATURES = {
    "spnerf_lpips_abi_version": (c_int32, []),
    "spnerf_lpips_weights_floats": (c_int64, []),
    "spnerf_lpips_pack_weights": (c_int32, [_PTRS, _PTRS, _PTRS, c_void_p, c_void_p]),
    "spnerf_lpips_workspace_bytes": (c_int64, [c_int32, c_int32, c_int64]),
    "spnerf_lpips_bands": (c_int32, [c_int32, c_int32, c_int64, POINTER(c_int32)]),
    "spnerf_lpips_features_floats": (c_int64, [c_int32, c_int32]),
    "spnerf_lpips": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int64, c_int64, c_int64, c_int32, c_void_p, c_void_p,
                               c_int64, c_void_p, c_void_p, c_void_p]),
}

lib = _lib.bind(SIGNATURES, "spnerf_lpips_abi_version", SPNERF_LPIPS_ABI_VERSION, "LPIPS")
