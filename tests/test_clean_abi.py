"""The DSM-cleaning C ABI (include/staged/spnerf_amd_clean.h, spnerf_amd._clean_abi): what tests/test_abi_tables.py
holds the tables of ``_lib.BINDING_MODULES`` to, for the one table that is staged outside that list; and argument
errors come back as codes or are raised before any device is used — no GPU needed."""
import ctypes
import importlib
from ctypes import POINTER, c_int64

import pytest
import torch

import abi_util
import clean_cases as cc
import spnerf_amd
from abi_util import A, B, C, D, refused
from spnerf_amd import _clean_abi, _lib, clean
from spnerf_amd.ortho import GroundGrid
from spnerf_amd.satellite import load_cameras

HEADER = abi_util.header_path("staged/spnerf_amd_clean.h")
E = ctypes.c_void_p(5 << 32)


def test_clean_exports_match_the_header():
    assert abi_util.check_table(_clean_abi, HEADER, "spnerf_clean", {"int64_t*": POINTER(c_int64)}) == [
        "spnerf_clean_abi_version", "spnerf_clean_fill", "spnerf_clean_median", "spnerf_clean_speckle", "spnerf_clean_workspace_bytes"]
    consts = abi_util.defines(HEADER, "SPNERF_CLEAN_")
    assert consts["SPNERF_CLEAN_ABI_VERSION"] == _clean_abi.SPNERF_CLEAN_ABI_VERSION == _clean_abi.lib().spnerf_clean_abi_version() == 1
    assert consts["SPNERF_CLEAN_TILE"] == _clean_abi.CLEAN_TILE == clean.TILE == cc.T
    assert consts["SPNERF_CLEAN_MAX_RADIUS"] == _clean_abi.CLEAN_MAX_RADIUS == 3 and consts["SPNERF_CLEAN_MAX_REACH"] == _clean_abi.CLEAN_MAX_REACH == 4096
    assert (consts["SPNERF_CLEAN_LOWEST"], consts["SPNERF_CLEAN_NEAREST"]) == (_clean_abi.CLEAN_LOWEST, _clean_abi.CLEAN_NEAREST) == (0, 1)
    assert clean.MODES == {"lowest": 0, "nearest": 1}
    assert consts["SPNERF_CLEAN_E_BOUND"] == _clean_abi.CLEAN_E_BOUND == -4
    assert _clean_abi.CLEAN_E_BOUND not in (_lib.SPNERF_OK, _lib.SPNERF_E_ARG, _lib.SPNERF_E_HIP, _lib.SPNERF_E_UNSUPPORTED)


def test_the_staged_table_is_disjoint_from_every_other_and_shares_the_handle():
    assert "_clean_abi" not in _lib.BINDING_MODULES and "_clean_lib" not in _lib.BINDING_MODULES
    assert _clean_abi.lib() is _lib.lib()
    for mod in [_lib] + [importlib.import_module("spnerf_amd." + m) for m in _lib.BINDING_MODULES]:
        assert not set(_clean_abi.SIGNATURES) & set(mod.SIGNATURES), mod.__name__


def test_c_argument_errors_are_reported():
    L = _clean_abi.lib()
    nan, inf = float("nan"), float("inf")
    n = c_int64(-1)
    assert L.spnerf_clean_workspace_bytes(9, 15, ctypes.byref(n)) == 0 and n.value == 9 * 15 * 8 + 16
    assert L.spnerf_clean_workspace_bytes(1, 2 ** 31 - 1, ctypes.byref(n)) == 0 and n.value == (2 ** 31 - 1) * 8 + 16
    refused(L, L.spnerf_clean_workspace_bytes(9, 15, None), b"clean_workspace_bytes: NULL bytes", "bytes")
    refused(L, L.spnerf_clean_workspace_bytes(0, 15, ctypes.byref(n)), b"clean_workspace_bytes: grid of 15 x 0 cells", "H")
    refused(L, L.spnerf_clean_workspace_bytes(9, -1, ctypes.byref(n)), b"clean_workspace_bytes: grid of -1 x 9 cells", "W")
    refused(L, L.spnerf_clean_workspace_bytes(2, 2 ** 30, ctypes.byref(n)), b"grid of 1073741824 x 2 cells is too large", "cells")

    need = 9 * 15 * 8 + 16

    def speckle(dsm=A, H=9, W=15, max_diff=0.5, max_size=10, out=B, label=C, size=D, work=E, work_bytes=need):
        return L.spnerf_clean_speckle(dsm, H, W, max_diff, max_size, out, label, size, work, work_bytes, None)

    for kw in (dict(dsm=None), dict(out=None), dict(label=None), dict(size=None), dict(work=None)):
        refused(L, speckle(**kw), b"clean_speckle: NULL", kw)
    for kw, text in ((dict(H=0), b"grid of 15 x 0 cells"), (dict(W=-3), b"grid of -3 x 9 cells"), (dict(H=2 ** 16, W=2 ** 15), b"grid of 32768 x 65536 cells is too large"),
                     (dict(max_diff=nan), b"max_diff nan must be finite and >= 0"), (dict(max_diff=-0.5), b"max_diff -0.5 must be"),
                     (dict(max_diff=inf), b"max_diff inf must be"), (dict(max_size=-1), b"max_size -1 must be >= 0"),
                     (dict(work_bytes=need - 1), b"workspace of 1095 bytes, 1096 needed"), (dict(work=ctypes.c_void_p((5 << 32) + 2)), b"workspace is not 4-byte aligned"),
                     (dict(out=A), b"out overlaps dsm"), (dict(out=ctypes.c_void_p((1 << 32) + 9 * 15 * 4 - 4)), b"out overlaps dsm"),
                     (dict(label=A), b"label or size overlaps dsm"), (dict(size=A), b"label or size overlaps dsm"), (dict(work=A), b"workspace overlaps"),
                     (dict(work=ctypes.c_void_p((2 << 32) - need + 4)), b"workspace overlaps"), (dict(label=B), b"out, label and size overlap"),
                     (dict(size=C), b"out, label and size overlap")):
        refused(L, speckle(**kw), b"clean_speckle: " + text, kw)

    def median(dsm=A, H=9, W=15, radius=1, min_count=1, fill=0, out=B):
        return L.spnerf_clean_median(dsm, H, W, radius, min_count, fill, out, None)

    for kw in (dict(dsm=None), dict(out=None)):
        refused(L, median(**kw), b"clean_median: NULL", kw)
    for kw, text in ((dict(H=0), b"grid of 15 x 0 cells"), (dict(H=2 ** 16, W=2 ** 15), b"grid of 32768 x 65536 cells is too large"), (dict(radius=0), b"radius 0 outside [1, 3]"),
                     (dict(radius=4), b"radius 4 outside [1, 3]"), (dict(min_count=0), b"min_count 0 outside [1, 9]"), (dict(min_count=10), b"min_count 10 outside [1, 9]"),
                     (dict(radius=3, min_count=50), b"min_count 50 outside [1, 49]"), (dict(fill=2), b"fill 2 must be 0 or 1"), (dict(out=A), b"out overlaps dsm")):
        refused(L, median(**kw), b"clean_median: " + text, kw)

    def fill(dsm=A, H=9, W=15, reach=4, mode=0, min_dirs=1, out=B, filled=C):
        return L.spnerf_clean_fill(dsm, H, W, reach, mode, min_dirs, out, filled, None)

    for kw in (dict(dsm=None), dict(out=None), dict(filled=None)):
        refused(L, fill(**kw), b"clean_fill: NULL", kw)
    for kw, text in ((dict(W=0), b"grid of 0 x 9 cells"), (dict(H=2 ** 16, W=2 ** 15), b"grid of 32768 x 65536 cells is too large"), (dict(reach=0), b"reach 0 outside [1, 4096]"),
                     (dict(reach=4097), b"reach 4097 outside"), (dict(mode=2), b"mode 2 is neither"), (dict(mode=-1), b"mode -1 is neither"),
                     (dict(min_dirs=0), b"min_dirs 0 outside [1, 8]"), (dict(min_dirs=9), b"min_dirs 9 outside [1, 8]"), (dict(out=A), b"out overlaps dsm"),
                     (dict(filled=A), b"filled overlaps dsm or out"), (dict(filled=B), b"filled overlaps dsm or out")):
        refused(L, fill(**kw), b"clean_fill: " + text, kw)


def test_python_argument_errors_come_before_any_device_use():
    for name in ("speckle_filter", "median_dsm", "fill_holes", "clean_dsm", "bootstrap_sweep"):
        assert getattr(spnerf_amd, name) is getattr(clean, name)
    assert spnerf_amd.clean is clean and clean.SPECKLE_CELLS >= 1
    nan, inf = float("nan"), float("inf")
    dsm = torch.zeros(9, 15)
    bad_rasters = ((dsm.double(), "must be a non-empty \\(H, W\\) float32"), (dsm[0], "must be"), (dsm[:, :0], "must be"), (dsm.numpy(), "must be"),
                   (torch.zeros(2, 2 ** 30, device="meta"), "a grid of 1073741824 x 2 cells is too large"))
    speckle_errors = ((dict(max_diff=nan), "max_diff nan must be finite and >= 0"), (dict(max_diff=-1.0), "max_diff -1.0 must be"), (dict(max_diff=inf), "max_diff inf must be"),
                      (dict(max_diff=1e39), "max_diff 1e\\+39 must be"), (dict(max_diff="1"), "max_diff '1' must be"), (dict(max_size=-1), "max_size -1 must be an integer in 0"),
                      (dict(max_size=2.0), "max_size 2.0 must be"), (dict(max_size=True), "max_size True must be"))
    fill_errors = ((dict(reach=0), "reach 0 must be an integer in 1..4096"), (dict(reach=4097), "reach 4097 must be"), (dict(reach=2.0), "reach 2.0 must be"),
                   (dict(mode="linear"), "mode 'linear' is neither 'lowest' nor 'nearest'"), (dict(mode=0), "mode 0 is neither"),
                   (dict(min_dirs=0), "min_dirs 0 must be an integer in 1..8"), (dict(min_dirs=9), "min_dirs 9 must be"))

    for bad, text in bad_rasters:
        for call in (lambda d: clean.speckle_filter(d, max_diff=1.0, max_size=4), lambda d: clean.median_dsm(d), lambda d: clean.fill_holes(d, reach=2),
                     lambda d: clean.clean_dsm(d, max_diff=1.0, max_size=4)):
            with pytest.raises(ValueError, match=text):
                call(bad)
    for kw, text in speckle_errors:
        with pytest.raises(ValueError, match=text):
            clean.speckle_filter(dsm, **dict(dict(max_diff=1.0, max_size=4), **kw))
        with pytest.raises(ValueError, match=text):
            clean.clean_dsm(dsm, **dict(dict(max_diff=1.0, max_size=4), **kw))
    with pytest.raises(TypeError):
        clean.clean_dsm(dsm)                                             # max_diff and max_size have no default
    with pytest.raises(_lib.SpnerfError, match="MI355X"):                # only now the raster's device matters
        clean.speckle_filter(dsm, max_diff=1.0, max_size=4)

    for kw, text in ((dict(radius=0), "radius 0 must be an integer in 1..3"), (dict(radius=4), "radius 4 must be"), (dict(radius=1.0), "radius 1.0 must be"),
                     (dict(min_count=0), "min_count 0 must be an integer in 1..9"), (dict(min_count=10), "min_count 10 must be"),
                     (dict(radius=2, min_count=26), "min_count 26 must be an integer in 1..25"), (dict(fill=1), "fill 1 must be a bool")):
        with pytest.raises(ValueError, match=text):
            clean.median_dsm(dsm, **kw)
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        clean.median_dsm(dsm, radius=3, min_count=49, fill=True)

    for kw, text in fill_errors:
        with pytest.raises(ValueError, match=text):
            clean.fill_holes(dsm, **dict(dict(reach=2), **kw))
        with pytest.raises(ValueError, match=text):
            clean.clean_dsm(dsm, max_diff=1.0, max_size=4, **dict(dict(reach=2), **kw))
    with pytest.raises(TypeError):
        clean.fill_holes(dsm)                                            # reach has no default
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        clean.fill_holes(dsm, reach=4096, mode="nearest", min_dirs=8)

    # clean_dsm: the weight, the median's radius (0 is "none" here), and a bad fill argument even without a fill
    for kw, text in ((dict(weight=dsm), "weight and min_weight go together"), (dict(min_weight=0.25), "weight and min_weight go together"),
                     (dict(weight=dsm.double(), min_weight=0.25), "weight must be a non-empty \\(H, W\\) float32"),
                     (dict(weight=dsm[:8], min_weight=0.25), "weight \\(8, 15\\) is not the grid's \\(9, 15\\)"), (dict(weight=dsm, min_weight=nan), "min_weight nan must be finite"),
                     (dict(weight=dsm, min_weight="0.25"), "min_weight '0.25' must be"), (dict(radius=-1), "radius -1 must be an integer in 0..3"),
                     (dict(radius=4), "radius 4 must be"), (dict(mode="mean"), "mode 'mean' is neither"), (dict(min_dirs=9), "min_dirs 9 must be")):
        with pytest.raises(ValueError, match=text):
            clean.clean_dsm(dsm, max_diff=1.0, max_size=4, **kw)
    with pytest.raises(ValueError, match="on one device"):
        clean.clean_dsm(dsm, weight=dsm.to("meta"), min_weight=0.25, max_diff=1.0, max_size=4)
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        clean.clean_dsm(dsm, weight=dsm, min_weight=0.25, max_diff=1.0, max_size=4, radius=0, reach=8)

    # bootstrap_sweep: refine_sweep's checks, then the chain's, then the device
    metas = load_cameras()["images"]
    cams = [spnerf_amd.rectify.Camera.from_meta(m, 4) for m in list(metas.values())[:2]]
    imgs = [torch.zeros(c.shape + (1,)) for c in cams]
    grid = GroundGrid(438638.0, 3353655.0, 15, 9, 0.5, 17)

    def boot(imgs=imgs, cams=cams, grid=grid, alt_lo=-20.0, step=1.0, planes=5, **kw):
        return clean.bootstrap_sweep(imgs, cams, grid, alt_lo, step, planes, **kw)

    for kw, text in ((dict(grid=0.5), "grid must be a GroundGrid"), (dict(imgs=imgs[:1]), "1 images for 2 views"), (dict(step=0.0), "step"), (dict(planes=1), "planes 1 must be an integer in 2"),
                     (dict(sweep_radius=0), "radius"), (dict(min_views=3), "min_views"), (dict(p1=-1.0), "p1 -1.0 must be"), (dict(paths=5), "paths 5 must be 4 or 8"),
                     (dict(slack=-1.0), "slack -1.0 must be"), (dict(volume=1), "volume 1 must be a bool"), (dict(max_diff=-1.0), "max_diff -1.0 must be"),
                     (dict(max_size=-1), "max_size -1 must be"), (dict(radius=4), "radius 4 must be an integer in 0..3"), (dict(reach=0), "reach 0 must be"),
                     (dict(mode="mean"), "mode 'mean' is neither"), (dict(min_dirs=0), "min_dirs 0 must be"), (dict(min_weight=nan), "min_weight nan must be finite")):
        with pytest.raises(ValueError, match=text):
            boot(**kw)
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        boot()
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        boot(max_diff=2.0, max_size=25, radius=0, min_weight=0.25, reach=8, mode="nearest", min_dirs=2, slack=2.0, sweep_radius=1)
