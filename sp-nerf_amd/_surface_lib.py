"""ctypes signatures of the surface-sweep exports (include/spnerf_amd_surface.h), applied to the same
libspnerf_amd.so handle as ``_lib.SIGNATURES``; errors come back through ``_lib.check``."""
from __future__ import annotations

from ctypes import POINTER, c_double, c_int32, c_int64, c_void_p

from . import _lib
from ._ortho_lib import OrthoGrid

SPNERF_SURFACE_ABI_VERSION = 1
SURFACE_MAX_FACTOR = 8

# name → (restype, argtypes); the exact export list of include/spnerf_amd_surface.h
SIGNATURES = {
    "spnerf_surface_abi_version": (c_int32, []),
    "spnerf_surface_grey": (c_int32, [POINTER(OrthoGrid), c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_double, c_void_p, c_void_p,
                                      c_void_p]),
    "spnerf_surface_lift": (c_int32, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "spnerf_surface_upsample": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "spnerf_surface_sweep": (c_int32, [POINTER(OrthoGrid), c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_double, c_double, c_int32,
                                       c_int32, c_int32, c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
}

_bound = False


def lib():
    """The library handle of ``_lib.lib()`` with the surface-sweep signatures applied (once).  A library
    without these exports is an error: there is no fallback."""
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
        if handle.spnerf_surface_abi_version() != SPNERF_SURFACE_ABI_VERSION:
            raise _lib.SpnerfError("libspnerf_amd.so: surface-sweep ABI version mismatch, rebuild it")
        _bound = True
    return handle
