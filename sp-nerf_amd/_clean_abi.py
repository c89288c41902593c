"""ctypes signatures of the DSM-cleaning exports (include/staged/spnerf_amd_clean.h), applied to the same
libspnerf_amd.so handle as ``_lib.SIGNATURES``; errors come back through ``_lib.check``.

STAGED: this table is not named ``_clean_lib.py`` and is not in ``_lib.BINDING_MODULES`` because
tests/test_abi_tables.py pins the list of ``_*_lib.py`` modules and of headers in include/; it moves to
``_clean_lib.py`` (and the header to include/spnerf_amd_clean.h) in the first change that may touch that test.
tests/test_clean_abi.py holds it to what the other tables are held to."""
from __future__ import annotations

from ctypes import POINTER, c_float, c_int32, c_int64, c_void_p

from . import _lib

SPNERF_CLEAN_ABI_VERSION = 1
CLEAN_TILE = 16
CLEAN_MAX_RADIUS = 3
CLEAN_MAX_REACH = 4096
CLEAN_LOWEST, CLEAN_NEAREST = 0, 1
CLEAN_E_BOUND = -4

# name → (restype, argtypes); the exact export list of include/staged/spnerf_amd_clean.h
SIGNATURES = {
    "spnerf_clean_abi_version": (c_int32, []),
    "spnerf_clean_workspace_bytes": (c_int32, [c_int32, c_int32, POINTER(c_int64)]),
    "spnerf_clean_speckle": (c_int32, [c_void_p, c_int32, c_int32, c_float, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "spnerf_clean_median": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "spnerf_clean_fill": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
}

lib = _lib.bind(SIGNATURES, "spnerf_clean_abi_version", SPNERF_CLEAN_ABI_VERSION, "DSM cleaning")
