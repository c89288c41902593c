"""ctypes signatures of the image-score exports (include/spnerf_amd_image.h), applied to the same
libspnerf_amd.so handle as ``_lib.SIGNATURES``; errors come back through ``_lib.check``."""
from __future__ import annotations

import ctypes
from ctypes import c_double, c_int32, c_int64, c_void_p

from . import _lib

SPNERF_IMAGE_ABI_VERSION = 1
IMAGE_MAX_CHANNELS = 4
IMAGE_MAX_WINDOW = 11


class SsimResult(ctypes.Structure):
    """spnerf_image_ssim_result: what the SSIM finish leaves on the device (48 bytes)."""
    _fields_ = [("ssim", c_double), ("channel_mean", c_double * IMAGE_MAX_CHANNELS), ("n", c_int64)]


# name → (restype, argtypes); the exact export list of include/spnerf_amd_image.h
SIGNATURES = {
    "spnerf_image_abi_version": (c_int32, []),
    "spnerf_image_ssim_workspace_bytes": (c_int64, [c_int32, c_int32, c_int32, c_int32]),
    "spnerf_image_ssim": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int64, c_int64, c_int64, c_int32,
                                    c_double, c_void_p, c_void_p, c_void_p, c_void_p]),
}

lib = _lib.bind(SIGNATURES, "spnerf_image_abi_version", SPNERF_IMAGE_ABI_VERSION, "image")
