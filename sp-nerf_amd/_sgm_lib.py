"""ctypes signatures of the semi-global aggregation exports (include/spnerf_amd_sgm.h), applied to the
same libspnerf_amd.so handle as ``_lib.SIGNATURES``; errors come back through ``_lib.check``."""
from __future__ import annotations

from ctypes import POINTER, c_double, c_float, c_int32, c_int64, c_void_p

from . import _lib

SPNERF_SGM_ABI_VERSION = 1
SGM_MAX_PLANES = 512
SGM_TILE = 64

# name → (restype, argtypes); the exact export list of include/spnerf_amd_sgm.h
SIGNATURES = {
    "spnerf_sgm_abi_version": (c_int32, []),
    "spnerf_sgm_workspace_bytes": (c_int32, [c_int32, c_int32, c_int32, c_int32, POINTER(c_int64)]),
    "spnerf_sgm_aggregate": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_float, c_float, c_float, c_int32, c_void_p, c_void_p,
                                       c_int64, c_void_p]),
    "spnerf_sgm_pick": (c_int32, [c_void_p, c_void_p, c_int32, c_int64, c_double, c_double, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_void_p]),
}

lib = _lib.bind(SIGNATURES, "spnerf_sgm_abi_version", SPNERF_SGM_ABI_VERSION, "semi-global aggregation")
