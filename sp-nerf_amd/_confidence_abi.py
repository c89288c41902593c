"""ctypes signatures of the confidence exports (include/staged/spnerf_amd_confidence.h), applied to the same
libspnerf_amd.so handle as ``_lib.SIGNATURES``; errors come back through ``_lib.check``.

STAGED: this table is not named ``_confidence_lib.py`` and is not in ``_lib.BINDING_MODULES`` because
tests/test_abi_tables.py pins the list of ``_*_lib.py`` modules and of headers in include/; it moves to
``_confidence_lib.py`` (and the header to include/spnerf_amd_confidence.h) in the first change that may touch that
test.  tests/test_confidence_abi.py holds it to what the other tables are held to."""
from __future__ import annotations

from ctypes import c_double, c_float, c_int32, c_int64, c_void_p

from . import _lib

SPNERF_CONF_ABI_VERSION = 1
CONF_MAX_PLANES = 512
# the output planes in the order of spnerf_conf_volume's pointers, with their element types
CONF_OUTPUTS = (("scored", "int32"), ("index", "int32"), ("margin", "float32"), ("peak_margin", "float32"), ("peaks", "int32"),
                ("support", "int32"), ("curvature", "float32"), ("mlm", "float32"), ("spread", "float32"))

# name → (restype, argtypes); the exact export list of include/staged/spnerf_amd_confidence.h
SIGNATURES = {
    "spnerf_conf_abi_version": (c_int32, []),
    "spnerf_conf_volume": (c_int32, [c_void_p, c_int32, c_int64, c_double, c_double, c_float, c_float, c_int32] + [c_void_p] * 9 + [c_void_p]),
}

lib = _lib.bind(SIGNATURES, "spnerf_conf_abi_version", SPNERF_CONF_ABI_VERSION, "confidence")
