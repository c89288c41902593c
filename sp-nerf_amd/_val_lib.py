"""ctypes signatures of the validation-loss exports (include/spnerf_amd_val.h), applied to the same
libspnerf_amd.so handle as ``_lib.SIGNATURES``; errors come back through ``_lib.check``."""
from __future__ import annotations

import ctypes
from ctypes import POINTER, c_double, c_float, c_int32, c_int64, c_void_p

from . import _lib

SPNERF_VAL_ABI_VERSION = 1


class ValLossResult(ctypes.Structure):
    """spnerf_val_loss_result: what the loss finish leaves on the device (7 doubles)."""
    _fields_ = [("n", c_double), ("color", c_double), ("color_coarse", c_double), ("logbeta", c_double),
                ("sc_term2", c_double), ("sc_term3", c_double), ("loss", c_double)]


RESULT_BYTES = ctypes.sizeof(ValLossResult)

# name → (restype, argtypes); the exact export list of include/spnerf_amd_val.h
SIGNATURES = {
    "spnerf_val_abi_version": (c_int32, []),
    "spnerf_val_solar_terms": (c_int32, [c_int64, c_int32, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_float, c_int64,
                                         c_void_p, c_void_p, POINTER(_lib.Rng), c_void_p]),
    "spnerf_val_loss_workspace_bytes": (c_int64, [c_int64]),
    "spnerf_val_loss": (c_int32, [c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_double, c_double,
                                  c_void_p, c_void_p, c_void_p]),
}

lib = _lib.bind(SIGNATURES, "spnerf_val_abi_version", SPNERF_VAL_ABI_VERSION, "validation-loss")
