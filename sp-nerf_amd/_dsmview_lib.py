"""ctypes signatures of the DSM-view exports (include/spnerf_amd_dsmview.h), applied to the same
libspnerf_amd.so handle as ``_lib.SIGNATURES``; errors come back through ``_lib.check``."""
from __future__ import annotations

from ctypes import POINTER, c_double, c_int32, c_int64, c_void_p

from . import _lib
from ._ortho_lib import OrthoGrid

SPNERF_DSMVIEW_ABI_VERSION = 1
DSMVIEW_NEAREST, DSMVIEW_BILINEAR = 0, 1

# name → (restype, argtypes); the exact export list of include/spnerf_amd_dsmview.h
SIGNATURES = {
    "spnerf_dsmview_abi_version": (c_int32, []),
    "spnerf_dsmview_workspace_bytes": (c_int64, [c_int32, c_int32]),
    "spnerf_dsmview_cast": (c_int32, [POINTER(OrthoGrid), c_void_p, c_void_p, c_double, c_double, c_int32, c_int32, c_int32, c_int32,
                                      c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "spnerf_dsmview_sample": (c_int32, [c_void_p, c_int32, c_int32, c_void_p, c_int64, c_int32, c_void_p, c_void_p]),
    "spnerf_dsmview_ecef": (c_int32, [c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p]),
}

lib = _lib.bind(SIGNATURES, "spnerf_dsmview_abi_version", SPNERF_DSMVIEW_ABI_VERSION, "DSM-view")
