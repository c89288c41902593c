"""The DSM-view C ABI (include/spnerf_amd_dsmview.h, spnerf_amd._dsmview_lib): the header, the ctypes table and
the built library agree, and argument errors come back as codes or are raised before any device is used — no
GPU needed."""
import ctypes

import pytest
import torch

import abi_util
import spnerf_amd
from abi_util import A, B, C, D, refused
from spnerf_amd import _dsmview_lib, _lib, _ortho_lib, dsm_view, rectify
from spnerf_amd.ortho import GroundGrid
from spnerf_amd.satellite import load_cameras

HEADER = abi_util.header_path("spnerf_amd_dsmview.h")


def test_dsmview_exports_match_the_header():
    assert abi_util.check_table(_dsmview_lib, HEADER, "spnerf_dsmview") == [
        "spnerf_dsmview_abi_version", "spnerf_dsmview_cast", "spnerf_dsmview_ecef", "spnerf_dsmview_sample", "spnerf_dsmview_workspace_bytes"]
    consts = abi_util.defines(HEADER, "SPNERF_DSMVIEW_")
    assert (consts["SPNERF_DSMVIEW_NEAREST"], consts["SPNERF_DSMVIEW_BILINEAR"]) == (_dsmview_lib.DSMVIEW_NEAREST, _dsmview_lib.DSMVIEW_BILINEAR) == (0, 1)
    assert dsm_view.MODES == {"nearest": 0, "bilinear": 1}


def test_c_argument_errors_are_reported():
    L = _dsmview_lib.lib()
    nan, inf = float("nan"), float("inf")
    good = dict(xoff=438638.0, ytop=3353655.0, res=0.5, W=15, H=9, zone=17)

    def grid(**kw):
        g = dict(good, **kw)
        return ctypes.byref(_ortho_lib.OrthoGrid(g["xoff"], g["ytop"], g["res"], g["W"], g["H"], g["zone"], 0, 1))

    assert L.spnerf_dsmview_workspace_bytes(9, 15) == 16 and L.spnerf_dsmview_workspace_bytes(512, 512) == 1024
    assert L.spnerf_dsmview_workspace_bytes(4096, 4096) == 1024
    refused(L, L.spnerf_dsmview_workspace_bytes(0, 15), b"dsmview_workspace_bytes: grid of 15 x 0", "H")
    refused(L, L.spnerf_dsmview_workspace_bytes(9, -1), b"dsmview_workspace_bytes: grid of -1 x 9", "W")
    refused(L, L.spnerf_dsmview_workspace_bytes(2 ** 31 - 1, 2 ** 31 - 1), b"cells is too large", "cells")

    def cast(grid=grid(), dsm=A, cam=B, lo=-30.0, hi=-2.0, col0=0, row0=0, stride=1, nc=7, nr=5, ws=C, hit=D, alt=D, ground=D, cell=D, depth=D):
        return L.spnerf_dsmview_cast(grid, dsm, cam, lo, hi, col0, row0, stride, nc, nr, ws, hit, alt, ground, cell, depth, None)

    for kw in (dict(grid=None), dict(dsm=None), dict(cam=None), dict(ws=None), dict(hit=None), dict(alt=None), dict(ground=None), dict(cell=None),
               dict(depth=None)):
        refused(L, cast(**kw), b"dsmview_cast: NULL", kw)
    for kw, text in ((dict(grid=grid(W=0)), b"grid of 0 x 9 cells"), (dict(grid=grid(zone=61)), b"UTM zone 61"), (dict(grid=grid(res=0.0)), b"resolution 0"),
                     (dict(grid=grid(xoff=nan)), b"non-finite grid origin"), (dict(lo=nan), b"altitudes nan, -2 are not finite"),
                     (dict(hi=inf), b"altitudes -30, inf are not finite"), (dict(lo=-2.0), b"alt_hi -2 must be above alt_lo -2"),
                     (dict(lo=0.0), b"alt_hi -2 must be above alt_lo 0"), (dict(stride=0), b"stride 0 must be at least 1"),
                     (dict(stride=-3), b"stride -3 must be"), (dict(nc=0), b"lattice of 0 x 5 pixels"), (dict(nr=-1), b"lattice of 7 x -1 pixels"),
                     (dict(col0=2 ** 31 - 4), b"the lattice from (2147483644, 0), 7 x 5 pixels of stride 1, leaves the int32 range"),
                     (dict(stride=2 ** 30, nr=4), b"7 x 4 pixels of stride 1073741824, leaves the int32 range"),
                     (dict(ws=ctypes.c_void_p((3 << 32) + 8)), b"workspace not 16-byte aligned"),
                     (dict(nr=65535 * 16 + 1), b"1048561 lattice rows in one call")):
        refused(L, cast(**kw), text, kw)

    def sample(raster=A, H=9, W=15, cell=B, n=7, mode=0, out=C):
        return L.spnerf_dsmview_sample(raster, H, W, cell, n, mode, out, None)

    for kw in (dict(raster=None), dict(cell=None), dict(out=None)):
        refused(L, sample(**kw), b"dsmview_sample: NULL", kw)
    for kw, text in ((dict(H=0), b"grid of 15 x 0 cells"), (dict(W=2 ** 31 - 1, H=2 ** 31 - 1), b"grid of 2147483647 x 2147483647 cells is too large"), (dict(n=0), b"count 0 outside"),
                     (dict(n=2 ** 32 + 1), b"count 4294967297"), (dict(mode=2), b"mode 2 is neither"), (dict(mode=-1), b"mode -1 is neither")):
        refused(L, sample(**kw), b"dsmview_sample: " + text, kw)

    def ecef(ground=A, alt=B, n=7, zone=17, south=0, out=C):
        return L.spnerf_dsmview_ecef(ground, alt, n, zone, south, out, None)

    for kw in (dict(ground=None), dict(alt=None), dict(out=None)):
        refused(L, ecef(**kw), b"dsmview_ecef: NULL", kw)
    for kw, text in ((dict(n=0), b"count 0 outside"), (dict(n=2 ** 32 + 1), b"count 4294967297"), (dict(zone=0), b"UTM zone 0"), (dict(zone=61), b"UTM zone 61")):
        refused(L, ecef(**kw), b"dsmview_ecef: " + text, kw)


def test_python_argument_errors_come_before_any_device_use():
    for name in ("view_dsm", "sample_at", "hit_ecef", "normalised_depth", "dsm_depth_priors"):
        assert getattr(spnerf_amd, name) is getattr(dsm_view, name)
    assert spnerf_amd.dsm_view is dsm_view
    nan, inf = float("nan"), float("inf")
    metas = list(load_cameras()["images"].values())
    cam = rectify.Camera.from_meta(metas[0], 1)
    grid = GroundGrid(438638.0, 3353655.0, 15, 9, 0.5, 17)
    dsm = torch.zeros(9, 15)
    bad_rasters = ((dsm.double(), "must be a non-empty \\(H, W\\) float32"), (dsm[0], "must be"), (dsm[:, :0], "must be"), (dsm.numpy(), "must be"),
                   (dsm[:8], "\\(8, 15\\) is not the grid's \\(9, 15\\)"), (dsm.t(), "\\(15, 9\\) is not the grid's"))

    def view(dsm=dsm, grid=grid, cam=cam, lo=-30.0, hi=-2.0, rect=(0, 0, 7, 5), stride=1):
        return dsm_view.view_dsm(dsm, grid, cam, alt_lo=lo, alt_hi=hi, rect=rect, stride=stride)

    for bad, text in bad_rasters:
        with pytest.raises(ValueError, match="dsm " + text):
            view(dsm=bad)
    for kw, text in ((dict(grid=0.5), "grid must be a GroundGrid"), (dict(cam=metas[0]), "camera must be a rectify.Camera"),
                     (dict(lo=nan), "alt_lo nan must be finite"), (dict(hi=inf), "alt_hi inf must be finite"), (dict(lo="0"), "alt_lo '0' must be"),
                     (dict(lo=-2.0), "alt_hi -2.0 must be above alt_lo -2.0"), (dict(stride=0), "stride 0 must be an integer in 1"),
                     (dict(stride=1.0), "stride 1.0 must be"), (dict(stride=True), "stride True must be"), (dict(rect=(0, 0, 7)), "rect .* must be \\(col0"),
                     (dict(rect=(0, 0, 0, 5)), "rect .* must be"), (dict(rect=(0.0, 0, 7, 5)), "rect .* must be"), (dict(rect=None), "rect None must be"),
                     (dict(rect=(2 ** 31 - 4, 0, 7, 5)), "is too large for one call"), (dict(rect=(0, 0, 7, 5), stride=2 ** 30), "is too large")):
        with pytest.raises(ValueError, match=text):
            view(**kw)
    with pytest.raises(ValueError, match="on one device"):
        dsm_view.sample_at(dsm, torch.zeros(4, 2).to("meta"))
    with pytest.raises(_lib.SpnerfError, match="MI355X"):                # only now the raster's device matters
        view()
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        view(rect=(-40, 12, 1, 1), stride=3, lo=-46.0, hi=14.0)

    # sample_at
    cell = torch.zeros(5, 7, 2)
    for bad, text in bad_rasters[:4]:
        with pytest.raises(ValueError, match="raster " + text):
            dsm_view.sample_at(bad, cell)
    for bad in (cell.double(), cell[..., :1], cell[:0], torch.zeros(()), cell.numpy()):
        with pytest.raises(ValueError, match="cell must be a non-empty \\(..., 2\\) float32"):
            dsm_view.sample_at(dsm, bad)
    for mode in ("linear", 0, None):
        with pytest.raises(ValueError, match="mode .* is neither 'nearest' nor 'bilinear'"):
            dsm_view.sample_at(dsm, cell, mode)
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        dsm_view.sample_at(dsm, cell, "bilinear")

    # hit_ecef
    ground, alt = torch.zeros(5, 7, 2, dtype=torch.float64), torch.zeros(5, 7)
    for bad in (ground.float(), ground[..., :1], ground[:0], ground.numpy()):
        with pytest.raises(ValueError, match="ground must be a non-empty \\(..., 2\\) float64"):
            dsm_view.hit_ecef(bad, alt, grid)
    for bad in (alt.double(), alt[:4], alt.numpy()):
        with pytest.raises(ValueError, match="altitude must be a float32 tensor of shape \\(5, 7\\)"):
            dsm_view.hit_ecef(ground, bad, grid)
    with pytest.raises(ValueError, match="grid must be a GroundGrid"):
        dsm_view.hit_ecef(ground, alt, None)
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        dsm_view.hit_ecef(ground, alt, grid)

    # normalised_depth is torch alone
    d = dsm_view.normalised_depth(torch.tensor([128.0, float("nan")]), 256.0)
    assert d[0] == 0.5 and torch.isnan(d[1])
    for depth, rng, text in (([1.0], 1.0, "depth must be a float32 tensor"), (torch.zeros(3).double(), 1.0, "depth must be a float32 tensor"),
                             (torch.zeros(3), 0.0, "range 0.0 must be finite and > 0"), (torch.zeros(3), nan, "range nan must be"),
                             (torch.zeros(3), "1", "range '1' must be")):
        with pytest.raises(ValueError, match=text):
            dsm_view.normalised_depth(depth, rng)

    # dsm_depth_priors
    def priors(dsm=dsm, weight=dsm, grid=grid, metas=metas[:2], lo=-30.0, hi=-2.0, **kw):
        return dsm_view.dsm_depth_priors(dsm, weight, grid, metas, alt_lo=lo, alt_hi=hi, **kw)

    for bad, text in bad_rasters:
        with pytest.raises(ValueError, match="dsm " + text):
            priors(dsm=bad)
        with pytest.raises(ValueError, match="weight " + text):
            priors(weight=bad)
    h, w = int(metas[0]["height"]), int(metas[0]["width"])
    for kw, text in ((dict(metas=[]), "metas must be a non-empty list"), (dict(metas=metas[0]), "metas must be a non-empty list"),
                     (dict(metas=[{"rpc": metas[0]["rpc"]}]), "metas\\[0\\] must be a dict with rpc, height"), (dict(lo=nan), "alt_lo nan must be"),
                     (dict(lo=0.0), "alt_hi -2.0 must be above alt_lo 0.0"), (dict(stride=0), "stride 0 must be"), (dict(min_weight=nan), "min_weight nan must be"),
                     (dict(min_weight="0.25"), "min_weight '0.25' must be"), (dict(rect=(0, 0, w + 1, 5)), f"leaves the {h} x {w} image of metas\\[0\\]"),
                     (dict(rect=(-1, 0, 4, 4)), "leaves the"), (dict(rect=(0, 0, 4, (h + 1) // 2 + 1), stride=2), "leaves the"),
                     (dict(rect=(0, 0, 4)), "rect .* must be")):
        with pytest.raises(ValueError, match=text):
            priors(**kw)
    with pytest.raises(ValueError, match="on one device"):
        priors(weight=dsm.to("meta"))
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        priors()
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        priors(rect=(10, 20, 64, 64), stride=4, min_weight=0.25)
