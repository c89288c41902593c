"""ctypes signatures of the surface-sweep exports (include/spnerf_amd_surface.h), applied to the same
libspnerf_amd.so handle as ``_lib.SIGNATURES``; errors come back through ``_lib.check``."""
from __future__ import annotations

from ctypes import POINTER, c_double, c_int32, c_int64, c_void_p

from . import _lib
from ._ortho_lib import OrthoGrid

SPNERF_SURFACE_ABI_VERSION = 1
SURFACE_MAX_FACTOR = 8

# name → (restype, argtypes); the exact export list of include/spnerf_amd_surface.h
SIGNATURES = {
    "spnerf_surface_abi_version": (c_int32, []),
    "spnerf_surface_grey": (c_int32, [POINTER(OrthoGrid), c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_double, c_void_p, c_void_p,
                                      c_void_p]),
    "spnerf_surface_lift": (c_int32, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "spnerf_surface_upsample": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "spnerf_surface_sweep": (c_int32, [POINTER(OrthoGrid), c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_double, c_double, c_int32,
                                       c_int32, c_int32, c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
}

lib = _lib.bind(SIGNATURES, "spnerf_surface_abi_version", SPNERF_SURFACE_ABI_VERSION, "surface-sweep")
