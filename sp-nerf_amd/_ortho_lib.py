"""ctypes signatures of the ground-grid exports (include/spnerf_amd_ortho.h), applied to the same
libspnerf_amd.so handle as ``_lib.SIGNATURES``; errors come back through ``_lib.check``."""
from __future__ import annotations

import ctypes
from ctypes import POINTER, c_double, c_float, c_int32, c_int64, c_void_p

from . import _lib

SPNERF_ORTHO_ABI_VERSION = 1
ORTHO_MAX_SUPERSAMPLE = 4


class OrthoGrid(ctypes.Structure):
    """spnerf_ortho_grid (include/spnerf_amd_ortho.h)."""
    _fields_ = [("xoff", c_double), ("ytop", c_double), ("resolution", c_double), ("xsize", c_int32), ("ysize", c_int32),
                ("zone", c_int32), ("south", c_int32), ("supersample", c_int32), ("reserved", c_int32 * 3)]


# name → (restype, argtypes); the exact export list of include/spnerf_amd_ortho.h
SIGNATURES = {
    "spnerf_ortho_abi_version": (c_int32, []),
    "spnerf_ortho_rays": (c_int32, [POINTER(OrthoGrid), c_int32, c_int32, c_double, c_double, POINTER(c_double), c_double,
                                    POINTER(c_float), c_void_p, c_int32, c_void_p]),
    "spnerf_ortho_reduce": (c_int32, [c_void_p, c_void_p, c_int64, c_int64, c_int32, c_int32, c_int32, c_void_p]),
    "spnerf_ortho_classes": (c_int32, [c_void_p, c_int64, c_int32, c_void_p, c_void_p]),
}

lib = _lib.bind(SIGNATURES, "spnerf_ortho_abi_version", SPNERF_ORTHO_ABI_VERSION, "ground-grid")
