"""ctypes signatures of the orthorectification exports (include/spnerf_amd_rectify.h), applied to the same
libspnerf_amd.so handle as ``_lib.SIGNATURES``; errors come back through ``_lib.check``."""
from __future__ import annotations

import ctypes
from ctypes import POINTER, c_double, c_int32, c_int64, c_void_p

from . import _lib
from ._ortho_lib import OrthoGrid

SPNERF_RECTIFY_ABI_VERSION = 1
RECTIFY_MAX_VIEWS = 64
RECTIFY_MAX_CHANNELS = 4
RECTIFY_CAMERA_DOUBLES = 90
RECTIFY_MEAN, RECTIFY_MEDIAN = 0, 1


class RectifyImage(ctypes.Structure):
    """spnerf_rectify_image (include/spnerf_amd_rectify.h): an entry of a call's image table."""
    _fields_ = [("pixels", c_void_p), ("height", c_int32), ("width", c_int32)]


IMAGE_BYTES = ctypes.sizeof(RectifyImage)

# name → (restype, argtypes); the exact export list of include/spnerf_amd_rectify.h
SIGNATURES = {
    "spnerf_rectify_abi_version": (c_int32, []),
    "spnerf_rectify_project": (c_int32, [c_void_p, POINTER(OrthoGrid), c_void_p, c_int32, c_void_p, c_void_p]),
    "spnerf_rectify_sample": (c_int32, [c_void_p, c_int32, c_int32, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "spnerf_rectify": (c_int32, [c_void_p, POINTER(OrthoGrid), c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                                 c_void_p]),
    "spnerf_rectify_view_dirs": (c_int32, [POINTER(OrthoGrid), c_void_p, c_int32, c_double, c_double, c_void_p, c_void_p, c_void_p]),
    "spnerf_rectify_mosaic": (c_int32, [c_void_p, c_void_p, c_int32, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                                        c_void_p]),
}

lib = _lib.bind(SIGNATURES, "spnerf_rectify_abi_version", SPNERF_RECTIFY_ABI_VERSION, "orthorectification")
