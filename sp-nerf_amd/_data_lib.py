"""ctypes signatures of the training-set exports (include/spnerf_amd_data.h), applied to the same
libspnerf_amd.so handle as ``_lib.SIGNATURES``; errors come back through ``_lib.check``."""
from __future__ import annotations

from ctypes import POINTER, c_double, c_float, c_int32, c_int64, c_void_p

from . import _lib

SPNERF_DATA_ABI_VERSION = 1
DATA_WORKSPACE_BYTES = 4096
VOID_LABEL = -100

# name → (restype, argtypes); the exact export list of include/spnerf_amd_data.h
SIGNATURES = {
    "spnerf_data_abi_version": (c_int32, []),
    "spnerf_rpc_rays_f64": (c_int32, [POINTER(c_double), c_double, c_double, c_double, c_void_p, c_int64,
                                      POINTER(c_float), c_float, POINTER(c_float), c_void_p, c_int32, c_void_p]),
    "spnerf_depth_priors": (c_int32, [POINTER(c_double), c_double, c_double, c_int32, c_int32, POINTER(c_float), c_float,
                                      c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "spnerf_scene_bounds": (c_int32, [POINTER(c_double), c_double, c_double, c_double, c_int32, c_int32, c_void_p,
                                      c_void_p]),
    "spnerf_semantic_labels": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_int32, c_int32, c_int32,
                                         c_int32, c_void_p, c_void_p, c_void_p]),
}

lib = _lib.bind(SIGNATURES, "spnerf_data_abi_version", SPNERF_DATA_ABI_VERSION, "data")
