"""What holds across all the ctypes tables of one libspnerf_amd.so (spnerf_amd._lib and the modules it names in
BINDING_MODULES): no export is bound twice, every header's ABI version is what it was, the base header's
prototypes have the table's argument types, and ``_lib.bind`` keeps each ``lib()``'s contract — no GPU needed."""
import ctypes
import glob
import importlib
import os

import pytest

import abi_util
from spnerf_amd import _lib

MODULES = [_lib] + [importlib.import_module("spnerf_amd." + m) for m in _lib.BINDING_MODULES]
# version export → value; the header, the module constant and the library are each held to it
VERSIONS = {"spnerf_abi_version": 2, "spnerf_eval_abi_version": 1, "spnerf_view_abi_version": 1, "spnerf_image_abi_version": 1,
            "spnerf_loss_abi_version": 1, "spnerf_data_abi_version": 1, "spnerf_lpips_abi_version": 1, "spnerf_val_abi_version": 1,
            "spnerf_train_abi_version": 1, "spnerf_dp_abi_version": 1, "spnerf_relight_abi_version": 1, "spnerf_ortho_abi_version": 1,
            "spnerf_shadow_abi_version": 1, "spnerf_rectify_abi_version": 1, "spnerf_sweep_abi_version": 1, "spnerf_sgm_abi_version": 1,
            "spnerf_occlusion_abi_version": 1, "spnerf_surface_abi_version": 1, "spnerf_dsmview_abi_version": 1}


def test_every_binding_module_and_header_is_named():
    files = sorted(os.path.basename(p)[:-3] for p in glob.glob(os.path.join(os.path.dirname(_lib.__file__), "_*_lib.py")))
    assert files == sorted(_lib.BINDING_MODULES)
    headers = sorted(os.path.basename(p) for p in glob.glob(abi_util.header_path("*.h")))
    assert headers == sorted(["spnerf_amd.h"] + ["spnerf_amd" + m[:-4] + ".h" for m in _lib.BINDING_MODULES])


def test_all_tables_are_pairwise_disjoint():
    for i, a in enumerate(MODULES):
        for b in MODULES[i + 1:]:
            assert not set(a.SIGNATURES) & set(b.SIGNATURES), (a.__name__, b.__name__)


def test_every_header_keeps_its_abi_version():
    assert len(VERSIONS) == len(MODULES)
    for mod in MODULES:
        (symbol,) = [n for n in mod.SIGNATURES if n.endswith("abi_version")]
        stem = symbol[len("spnerf_"):-len("abi_version")].upper()          # "", "EVAL_", ...
        if mod is _lib:                                                    # the base header has no #define of it
            assert mod.lib().spnerf_abi_version() == VERSIONS[symbol]
            continue
        header = abi_util.header_path("spnerf_amd" + mod.__name__.split(".")[-1][:-4] + ".h")
        define = abi_util.defines(header, "SPNERF_" + stem)["SPNERF_" + stem + "ABI_VERSION"]
        assert define == getattr(mod, "SPNERF_" + stem + "ABI_VERSION") == getattr(mod.lib(), symbol)() == VERSIONS[symbol], symbol


def test_base_header_has_the_tables_argument_types():
    P = ctypes.POINTER
    # host arrays and host out-values of the base header; every other pointer is a device pointer
    host = {("spnerf_param_info", 4): P(ctypes.c_int64), ("spnerf_param_info", 5): P(ctypes.c_int64),
            ("spnerf_mlp_trunk_wgrad", 3): P(ctypes.c_int64), ("spnerf_mlp_trunk_wgrad", 4): P(ctypes.c_int32),
            ("spnerf_mlp_trunk_wgrad", 5): P(ctypes.c_int32), ("spnerf_rpc_rays", 0): P(ctypes.c_double),
            ("spnerf_rpc_rays", 10): P(ctypes.c_float), ("spnerf_rpc_rays", 12): P(ctypes.c_float),
            ("spnerf_dsm_points", 4): P(ctypes.c_double), ("spnerf_get_option", 1): P(ctypes.c_int32),
            ("spnerf_adam_step", 5): P(ctypes.c_int64), ("spnerf_gather_rows", 4): P(ctypes.c_int64),
            ("spnerf_gather_rows", 5): P(ctypes.c_int32), ("spnerf_grad_marks", 1): P(ctypes.c_int32),
            ("spnerf_prof_read", 1): P(ctypes.c_int64), ("spnerf_prof_read", 2): P(ctypes.c_double),
            ("spnerf_prof_read", 3): P(ctypes.c_double), ("spnerf_prof_read", 4): P(ctypes.c_double)}
    assert len(abi_util.check_table(_lib, abi_util.header_path("spnerf_amd.h"), "spnerf_", host)) == 40


def test_bind_reports_a_missing_export():
    lib = _lib.bind({"spnerf_no_such_export": (ctypes.c_int32, [])}, "spnerf_abi_version", 2, "test")
    with pytest.raises(_lib.SpnerfError, match="does not export spnerf_no_such_export: rebuild it"):
        lib()


def test_bind_reports_a_version_mismatch_and_binds_once():
    from spnerf_amd import _sgm_lib
    stale = _lib.bind(_sgm_lib.SIGNATURES, "spnerf_sgm_abi_version", _sgm_lib.SPNERF_SGM_ABI_VERSION + 1, "semi-global aggregation")
    with pytest.raises(_lib.SpnerfError, match="libspnerf_amd.so: semi-global aggregation ABI version mismatch, rebuild it"):
        stale()
    lib = _lib.bind(_sgm_lib.SIGNATURES, "spnerf_sgm_abi_version", _sgm_lib.SPNERF_SGM_ABI_VERSION, "semi-global aggregation")
    assert lib() is lib() is _sgm_lib.lib() is _lib.lib()
