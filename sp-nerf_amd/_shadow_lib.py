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

_bound = False


def lib():
    """The library handle of ``_lib.lib()`` with the shadow signatures applied (once).  A library
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
        if handle.spnerf_shadow_abi_version() != SPNERF_SHADOW_ABI_VERSION:
            raise _lib.SpnerfError("libspnerf_amd.so: shadow ABI version mismatch, rebuild it")
        _bound = True
    return handle
