"""ctypes structs and signatures of the training-loss exports (include/spnerf_amd_loss.h), applied
to the same libspnerf_amd.so handle as ``_lib.SIGNATURES``; errors come back through ``_lib.check``."""
from __future__ import annotations

import ctypes
from ctypes import POINTER, c_float, c_int32, c_int64, c_void_p

from . import _lib

SPNERF_LOSS_ABI_VERSION = 1

LOSS_BETA = 1
LOSS_DEPTH_TERM_ONLY = 2
LOSS_SEM_TERM_ONLY = 4

DEPTH_NONE, DEPTH_SUBSET_MSE, DEPTH_SUBSET_GNLL, DEPTH_ALL = 0, 1, 2, 3

RESULT_FLOATS = 18
PASS_BASE = 2
PASS_TERMS = 8
# slot of each term in a pass's part of the result block
TERM_SLOTS = {"color": 0, "logbeta": 1, "sc_term2": 2, "sc_term3": 3, "ds": 4, "ss": 5, "mse": 6, "psnr": 7}


class TrainLossPass(ctypes.Structure):
    """spnerf_train_loss_pass: one pass's render tensors and, for the backward, its gradients."""
    _fields_ = [("n_samples", c_int32), ("ld_sun", c_int32),
                ("rgb", c_void_p), ("weights", c_void_p), ("z_vals", c_void_p), ("depth", c_void_p),
                ("sun_sc", c_void_p), ("transparency_sc", c_void_p), ("weights_sc", c_void_p), ("sem_logits", c_void_p),
                ("d_rgb", c_void_p), ("d_weights", c_void_p), ("d_depth", c_void_p), ("d_sun", c_void_p),
                ("d_logits", c_void_p)]


class TrainLossOpts(ctypes.Structure):
    """spnerf_train_loss_opts: the shared targets and options."""
    _fields_ = [("n_rays", c_int64), ("n_classes", c_int32), ("flags", c_int32), ("depth_form", c_int32),
                ("world", c_int32), ("lambda_sc", c_float), ("lambda_ds", c_float), ("lambda_ss", c_float),
                ("ld_beta", c_int32), ("ld_td", c_int32), ("reserved", c_int32),
                ("target", c_void_p), ("beta", c_void_p), ("target_depth", c_void_p), ("target_weight", c_void_p),
                ("valid", c_void_p), ("target_std", c_void_p), ("labels", c_void_p), ("labels_global", c_void_p),
                ("n_global", c_int64), ("d_beta", c_void_p)]


# name → (restype, argtypes); the exact export list of include/spnerf_amd_loss.h
SIGNATURES = {
    "spnerf_loss_abi_version": (c_int32, []),
    "spnerf_train_loss_workspace_bytes": (c_int64, [c_int64]),
    "spnerf_train_loss_forward": (c_int32, [POINTER(TrainLossOpts), POINTER(TrainLossPass), POINTER(TrainLossPass),
                                            c_void_p, c_void_p, c_void_p]),
    "spnerf_train_loss_backward": (c_int32, [POINTER(TrainLossOpts), POINTER(TrainLossPass), POINTER(TrainLossPass),
                                             c_void_p, c_void_p, c_void_p]),
}

lib = _lib.bind(SIGNATURES, "spnerf_loss_abi_version", SPNERF_LOSS_ABI_VERSION, "loss")
