"""ctypes signatures of the evaluation exports (include/spnerf_amd_eval.h), applied to the same
libspnerf_amd.so handle as ``_lib.SIGNATURES``; errors come back through ``_lib.check``."""
from __future__ import annotations

import ctypes
from ctypes import POINTER, c_double, c_int32, c_int64, c_void_p

from . import _lib

SPNERF_EVAL_ABI_VERSION = 1
DSM_MAX_IRANGE = 8
DSM_SUMS_DOUBLES = 2 + 2 * 256


class DsmShift(ctypes.Structure):
    """spnerf_eval_dsm_shift: what a registration leaves on the device (56 bytes)."""
    _fields_ = [("dx", c_int32), ("dy", c_int32), ("muu", c_double), ("muv", c_double), ("sigu", c_double),
                ("sigv", c_double), ("xcorr", c_double), ("count", c_int64)]


# name → (restype, argtypes); the exact export list of include/spnerf_amd_eval.h
SIGNATURES = {
    "spnerf_eval_abi_version": (c_int32, []),
    "spnerf_eval_dsm_register_workspace_bytes": (c_int64, [c_int32, c_int32, c_int32]),
    "spnerf_eval_dsm_down2x": (c_int32, [c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    "spnerf_eval_dsm_register": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p,
                                           c_void_p, c_void_p, c_void_p]),
    "spnerf_eval_dsm_apply_shift": (c_int32, [c_void_p, c_int32, c_int32, c_void_p, c_int32, c_int32, c_int32, c_double,
                                              c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
}

lib = _lib.bind(SIGNATURES, "spnerf_eval_abi_version", SPNERF_EVAL_ABI_VERSION, "evaluation")
