"""ctypes signatures of the occlusion exports (include/spnerf_amd_occlusion.h), applied to the same
libspnerf_amd.so handle as ``_lib.SIGNATURES``; errors come back through ``_lib.check``."""
from __future__ import annotations

from ctypes import POINTER, c_double, c_float, c_int32, c_int64, c_void_p

from . import _lib
from ._ortho_lib import OrthoGrid

SPNERF_OCCLUSION_ABI_VERSION = 1
OCCLUSION_MAX_VIEWS = 16

# name → (restype, argtypes); the exact export list of include/spnerf_amd_occlusion.h
SIGNATURES = {
    "spnerf_occlusion_abi_version": (c_int32, []),
    "spnerf_occlusion_workspace_bytes": (c_int64, [c_int32, c_int32]),
    "spnerf_occlusion_floor": (c_int32, [c_void_p, c_int32, c_int32, c_double, POINTER(c_float), c_int32, c_void_p, c_void_p, c_void_p]),
    "spnerf_occlusion_gate": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int64, c_double, c_double, c_void_p]),
    "spnerf_occlusion_sweep": (c_int32, [POINTER(OrthoGrid), c_void_p, c_void_p, c_int32, c_int32, c_double, c_double, c_int32, c_int32,
                                         c_int32, c_double, c_void_p, c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_void_p]),
}

lib = _lib.bind(SIGNATURES, "spnerf_occlusion_abi_version", SPNERF_OCCLUSION_ABI_VERSION, "occlusion")
