"""ctypes signatures of the relighting exports (include/spnerf_amd_relight.h), applied to the same
libspnerf_amd.so handle as ``_lib.SIGNATURES``; errors come back through ``_lib.check``."""
from __future__ import annotations

from ctypes import POINTER, c_float, c_int32, c_int64, c_void_p

from . import _lib

SPNERF_RELIGHT_ABI_VERSION = 1

# name → (restype, argtypes); the exact export list of include/spnerf_amd_relight.h
SIGNATURES = {
    "spnerf_relight_abi_version": (c_int32, []),
    "spnerf_relight_workspace_bytes": (c_int64, [POINTER(_lib.ModelCfg), c_int32]),
    "spnerf_relight_directions": (c_int32, [POINTER(_lib.ModelCfg), c_void_p, c_void_p, c_int32, c_void_p, c_void_p]),
    "spnerf_relight_sun": (c_int32, [POINTER(_lib.ModelCfg), c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_int32,
                                     c_void_p, c_void_p]),
    "spnerf_relight_composite": (c_int32, [c_int64, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_float,
                                           POINTER(_lib.Rng), c_int32, c_void_p, c_void_p, c_int64, c_int64, c_void_p,
                                           c_void_p, c_void_p, c_void_p]),
}

lib = _lib.bind(SIGNATURES, "spnerf_relight_abi_version", SPNERF_RELIGHT_ABI_VERSION, "relighting")
