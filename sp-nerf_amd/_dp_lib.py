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

_bound = False


def lib():
    """The library handle of ``_lib.lib()`` with the data-parallel signatures applied (once).  A
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
        if handle.spnerf_dp_abi_version() != SPNERF_DP_ABI_VERSION:
            raise _lib.SpnerfError("libspnerf_amd.so: data-parallel ABI version mismatch, rebuild it")
        _bound = True
    return handle
