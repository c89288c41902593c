"""ctypes signatures of the training-set exports (include/spnerf_amd_data.h), applied to the same
libspnerf_amd.so handle as ``_lib.SIGNATURES``; errors come back through ``_lib.check``."""
from __future__ import annotations

from ctypes import POINTER, c_double, c_float, c_int32, c_int64, c_void_p

from . import _lib

SPNERF_DATA_ABI_VERSION = 1
DATA_WORKSPACE_BYTES = 4096
VOID_LABEL = -100

# name → (restype, argtypes); the exact export list of include/spnerf_amd_data.h
SIGNATURES = {
    "spnerf_data_abi_version": (c_int32, []),
    "spnerf_rpc_rays_f64": (c_int32, [POINTER(c_double), c_double, c_double, c_double, c_void_p, c_int64,
                                      POINTER(c_float), c_float, POINTER(c_float), c_void_p, c_int32, c_void_p]),
    "spnerf_depth_priors": (c_int32, [POINTER(c_double), c_double, c_double, c_int32, c_int32, POINTER(c_float), c_float,
                                      c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "spnerf_scene_bounds": (c_int32, [POINTER(c_double), c_double, c_double, c_double, c_int32, c_int32, c_void_p,
                                      c_void_p]),
    "spnerf_semantic_labels": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_int32, c_int32, c_int32,
                                         c_int32, c_void_p, c_void_p, c_void_p]),
}

_bound = False


def lib():
    """The library handle of ``_lib.lib()`` with the training-set signatures applied (once).  A
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
        if handle.spnerf_data_abi_version() != SPNERF_DATA_ABI_VERSION:
            raise _lib.SpnerfError("libspnerf_amd.so: data ABI version mismatch, rebuild it")
        _bound = True
    return handle
