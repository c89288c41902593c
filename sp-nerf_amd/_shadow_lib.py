"""ctypes signatures of the geometric-shadow exports (include/spnerf_amd_shadow.h), applied to the same
libspnerf_amd.so handle as ``_lib.SIGNATURES``; errors come back through ``_lib.check``."""
from __future__ import annotations

import ctypes
from ctypes import POINTER, c_double, c_float, c_int32, c_int64, c_void_p

from . import _lib

SPNERF_SHADOW_ABI_VERSION = 1
SHADOW_MAX_DIRS = 65535


class ShadowAgreementResult(ctypes.Structure):
    """spnerf_shadow_agreement_result (include/spnerf_amd_shadow.h)."""
    _fields_ = [("sum_sun_lit", c_double), ("sum_sun_shadow", c_double), ("sum_abs", c_double), ("n_lit", c_int64),
                ("n_shadow", c_int64), ("tp", c_int64), ("fp", c_int64), ("fn", c_int64)]


RESULT_BYTES = ctypes.sizeof(ShadowAgreementResult)

# name → (restype, argtypes); the exact export list of include/spnerf_amd_shadow.h
SIGNATURES = {
    "spnerf_shadow_abi_version": (c_int32, []),
    "spnerf_shadow_workspace_bytes": (c_int64, [c_int32, c_int32]),
    "spnerf_shadow_cast": (c_int32, [c_void_p, c_int32, c_int32, c_double, POINTER(c_float), c_int32, c_void_p, c_void_p,
                                     c_void_p, c_void_p]),
    "spnerf_shadow_agreement_workspace_bytes": (c_int64, [c_int64, c_int32]),
    "spnerf_shadow_agreement": (c_int32, [c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_void_p]),
}

lib = _lib.bind(SIGNATURES, "spnerf_shadow_abi_version", SPNERF_SHADOW_ABI_VERSION, "shadow")
