"""ctypes structs and signatures of the training-step exports (include/spnerf_amd_train.h), applied
to the same libspnerf_amd.so handle as ``_lib.SIGNATURES``; errors come back through ``_lib.check``."""
from __future__ import annotations

import ctypes
from ctypes import POINTER, c_double, c_float, c_int32, c_int64, c_void_p

from . import _lib

SPNERF_TRAIN_ABI_VERSION = 1

ERR_PAST_END = 1
ERR_BATCH = 2


class StepScalars(ctypes.Structure):
    """spnerf_train_step_scalars: one step's row of the epoch plan."""
    _fields_ = [("noise_std", c_float), ("lr", c_float), ("adam_step_size", c_float), ("adam_bc2_sqrt", c_float),
                ("step", c_int64)]


class TrainState(ctypes.Structure):
    """spnerf_train_state: the device-resident description of the uploaded plan."""
    _fields_ = [("cursor", c_int64), ("n_steps", c_int64), ("B", c_int64), ("error", c_int64)]


# name → (restype, argtypes); the exact export list of include/spnerf_amd_train.h
SIGNATURES = {
    "spnerf_train_abi_version": (c_int32, []),
    "spnerf_train_step_begin": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "spnerf_adam_step_dev": (c_int32, [c_int32, POINTER(c_void_p), POINTER(c_void_p), POINTER(c_void_p),
                                       POINTER(c_void_p), POINTER(c_int64), c_void_p, c_double, c_double, c_double,
                                       c_void_p]),
    "spnerf_composite_forward_dev": (c_int32, [c_int64, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_int32,
                                               c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                               POINTER(_lib.Rng), c_void_p]),
    "spnerf_composite_backward_dev": (c_int32, [c_int64, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_int32,
                                                c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                c_void_p, POINTER(_lib.Rng), c_void_p]),
}

lib = _lib.bind(SIGNATURES, "spnerf_train_abi_version", SPNERF_TRAIN_ABI_VERSION, "training-step")
