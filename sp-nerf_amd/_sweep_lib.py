"""ctypes signatures of the plane-sweep exports (include/spnerf_amd_sweep.h), applied to the same
libspnerf_amd.so handle as ``_lib.SIGNATURES``; errors come back through ``_lib.check``."""
from __future__ import annotations

from ctypes import POINTER, c_double, c_int32, c_int64, c_void_p

from . import _lib
from ._ortho_lib import OrthoGrid

SPNERF_SWEEP_ABI_VERSION = 1
SWEEP_MIN_VIEWS = 2
SWEEP_MAX_VIEWS = 16
SWEEP_MAX_PLANES = 4096
SWEEP_MAX_RADIUS = 4
SWEEP_TILE = 16

# name → (restype, argtypes); the exact export list of include/spnerf_amd_sweep.h
SIGNATURES = {
    "spnerf_sweep_abi_version": (c_int32, []),
    "spnerf_sweep_grey": (c_int32, [POINTER(OrthoGrid), c_void_p, c_void_p, c_int32, c_int32, c_double, c_void_p, c_void_p, c_void_p]),
    "spnerf_sweep_score": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_double, c_void_p, c_void_p,
                                     c_void_p]),
    "spnerf_sweep_pick": (c_int32, [c_void_p, c_void_p, c_int32, c_int64, c_double, c_double, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_void_p]),
    "spnerf_sweep": (c_int32, [POINTER(OrthoGrid), c_void_p, c_void_p, c_int32, c_int32, c_double, c_double, c_int32, c_int32, c_int32,
                               c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
}

lib = _lib.bind(SIGNATURES, "spnerf_sweep_abi_version", SPNERF_SWEEP_ABI_VERSION, "plane-sweep")
