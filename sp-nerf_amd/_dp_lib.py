"""ctypes signatures of the data-parallel training-step exports (include/spnerf_amd_dp.h), applied
to the same libspnerf_amd.so handle as ``_lib.SIGNATURES``; errors come back through ``_lib.check``."""
from __future__ import annotations

from ctypes import POINTER, c_double, c_float, c_int32, c_int64, c_void_p

from . import _lib

SPNERF_DP_ABI_VERSION = 1

# name → (restype, argtypes); the exact export list of include/spnerf_amd_dp.h
SIGNATURES = {
    "spnerf_dp_abi_version": (c_int32, []),
    # state, plan_rows, perm, cur, batch_idx, global_idx, B, rank, world, rays, ld_rays, clamp, sems, labels_global, stream
    "spnerf_dp_step_begin": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int32,
                                       c_int32, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "spnerf_adam_step_dev_scaled": (c_int32, [c_int32, POINTER(c_void_p), POINTER(c_void_p), POINTER(c_void_p),
                                              POINTER(c_void_p), POINTER(c_int64), c_void_p, c_double, c_double,
                                              c_double, c_float, c_void_p]),
}

lib = _lib.bind(SIGNATURES, "spnerf_dp_abi_version", SPNERF_DP_ABI_VERSION, "data-parallel")
