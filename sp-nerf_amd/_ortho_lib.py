"""ctypes signatures of the ground-grid exports (include/spnerf_amd_ortho.h), applied to the same
libspnerf_amd.so handle as ``_lib.SIGNATURES``; errors come back through ``_lib.check``."""
from __future__ import annotations

import ctypes
from ctypes import POINTER, c_double, c_float, c_int32, c_int64, c_void_p

from . import _lib

SPNERF_ORTHO_ABI_VERSION = 1
ORTHO_MAX_SUPERSAMPLE = 4


class OrthoGrid(ctypes.Structure):
    """spnerf_ortho_grid (include/spnerf_amd_ortho.h)."""
    _fields_ = [("xoff", c_double), ("ytop", c_double), ("resolution", c_double), ("xsize", c_int32), ("ysize", c_int32),
                ("zone", c_int32), ("south", c_int32), ("supersample", c_int32), ("reserved", c_int32 * 3)]


# name → (restype, argtypes); the exact export list of include/spnerf_amd_ortho.h
SIGNATURES = {
    "spnerf_ortho_abi_version": (c_int32, []),
    "spnerf_ortho_rays": (c_int32, [POINTER(OrthoGrid), c_int32, c_int32, c_double, c_double, POINTER(c_double), c_double,
                                    POINTER(c_float), c_void_p, c_int32, c_void_p]),
    "spnerf_ortho_reduce": (c_int32, [c_void_p, c_void_p, c_int64, c_int64, c_int32, c_int32, c_int32, c_void_p]),
    "spnerf_ortho_classes": (c_int32, [c_void_p, c_int64, c_int32, c_void_p, c_void_p]),
}

_bound = False


def lib():
    """The library handle of ``_lib.lib()`` with the ground-grid signatures applied (once).  A
    library without these exports is an error: there is no fallback."""
    global _bound
    handle = _lib.lib()
    if not _bound:
        for name, (res, args) in SIGNATURES.items():
            try:
                fn = getattr(handle, name)
            except AttributeError:
                raise _lib.SpnerfError(f"{_lib.LIB_PATH} does not export {name}: rebuild it "
                                       "(`make -C sp-nerf_amd`)") from None
            fn.restype = res
            fn.argtypes = args
        if handle.spnerf_ortho_abi_version() != SPNERF_ORTHO_ABI_VERSION:
            raise _lib.SpnerfError("libspnerf_amd.so: ground-grid ABI version mismatch, rebuild it")
        _bound = True
    return handle
