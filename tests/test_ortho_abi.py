"""The ground-grid C ABI (include/spnerf_amd_ortho.h, spnerf_amd._ortho_lib): the header, the ctypes
table and the built library agree, and argument errors come back as codes or are raised before any
device is used — no GPU needed."""
import ctypes
import re
import types

import numpy as np
import pytest
import torch

import abi_util
import spnerf_amd
from abi_util import ONE
from spnerf_amd import _lib, _ortho_lib
from spnerf_amd.ortho import GroundGrid

HEADER = abi_util.header_path("spnerf_amd_ortho.h")
CENTER = (ctypes.c_double * 3)(801532.875, -5452266.5, 3200266.75)
SUN = (ctypes.c_float * 3)(0.0, 0.6, 0.8)


def test_ortho_exports_match_the_header():
    # the scene centre and the sun direction are host arrays
    host = {("spnerf_ortho_rays", 5): ctypes.POINTER(ctypes.c_double), ("spnerf_ortho_rays", 7): ctypes.POINTER(ctypes.c_float)}
    assert abi_util.check_table(_ortho_lib, HEADER, "spnerf_", host) == [
        "spnerf_ortho_abi_version", "spnerf_ortho_classes", "spnerf_ortho_rays", "spnerf_ortho_reduce"]
    txt = open(HEADER).read()
    consts = abi_util.defines(HEADER, "SPNERF_ORTHO_")
    assert consts["SPNERF_ORTHO_MAX_SUPERSAMPLE"] == _ortho_lib.ORTHO_MAX_SUPERSAMPLE == 4
    # the struct of the header, field for field
    body = re.search(r"typedef struct spnerf_ortho_grid \{(.*?)\} spnerf_ortho_grid;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n.split("[")[0] for decl in re.findall(r"(?:double|int32_t)\s+([^;]+);", body) for n in re.split(r",\s*", decl)]
    assert fields == [f for f, _ in _ortho_lib.OrthoGrid._fields_]
    assert ctypes.sizeof(_ortho_lib.OrthoGrid) == 3 * 8 + 8 * 4


def grid(xoff=438638.996411, ytop=3353655.999928, res=0.5, xsize=5, ysize=3, zone=17, south=0, s=1):
    return ctypes.byref(_ortho_lib.OrthoGrid(xoff, ytop, res, xsize, ysize, zone, south, s))


def test_ray_argument_errors_are_reported():
    L = _ortho_lib.lib()

    def rays(g=None, row0=0, n_rows=3, lo=-30.0, hi=-2.0, center=CENTER, rng=141.21875, sun=SUN, out=ONE, stride=11):
        return L.spnerf_ortho_rays(None if g == "NULL" else g or grid(), row0, n_rows, lo, hi, center, rng, sun, out, stride, None)

    for kw, text in ((dict(g="NULL"), b"NULL"), (dict(center=None), b"NULL"), (dict(out=None), b"NULL"),
                     (dict(g=grid(zone=0)), b"UTM zone 0"), (dict(g=grid(zone=61)), b"UTM zone 61"),
                     (dict(g=grid(s=0)), b"supersample 0"), (dict(g=grid(s=5)), b"supersample 5"),
                     (dict(g=grid(xsize=0)), b"grid of 0 x 3"), (dict(g=grid(ysize=-1)), b"grid of 5 x -1"),
                     (dict(g=grid(res=0.0)), b"resolution 0"), (dict(g=grid(res=-0.5)), b"resolution -0.5"),
                     (dict(g=grid(res=float("nan"))), b"resolution"), (dict(g=grid(xoff=float("inf"))), b"non-finite"),
                     (dict(lo=-2.0), b"must be above"), (dict(lo=5.0), b"must be above"), (dict(hi=float("nan")), b"must be above"),
                     (dict(rng=0.0), b"range 0"),
                     (dict(row0=-1), b"outside the grid"), (dict(row0=1), b"outside the grid"), (dict(n_rows=4), b"outside the grid"),
                     (dict(n_rows=-1), b"outside the grid"), (dict(row0=3, n_rows=1), b"outside the grid"),
                     (dict(row0=2 ** 31 - 1, n_rows=2 ** 31 - 1), b"outside the grid"),
                     (dict(stride=9), b"neither 8 nor 11"), (dict(stride=12), b"neither 8 nor 11"), (dict(stride=6), b"neither 8 nor 11"),
                     (dict(sun=None), b"needs the sun direction")):
        assert rays(**kw) == -1, kw
        assert text in L.spnerf_last_error(), (kw, L.spnerf_last_error())
    assert rays(g=grid(xsize=2 ** 31 - 1, ysize=2 ** 31 - 1, s=4), n_rows=2 ** 31 - 1) == -1
    assert b"in one launch" in L.spnerf_last_error()
    assert rays(n_rows=0) == 0 and rays(row0=3, n_rows=0) == 0          # nothing to do, nothing launched
    assert rays(sun=None, stride=8, n_rows=0) == 0


def test_reduce_and_class_argument_errors_are_reported():
    L = _ortho_lib.lib()
    two = ctypes.c_void_p(512)

    def reduce(src=ONE, dst=two, images=1, cells=7, width=3, s=2, dtype=0):
        return L.spnerf_ortho_reduce(src, dst, images, cells, width, s, dtype, None)

    for kw, text in ((dict(src=None), b"NULL"), (dict(dst=None), b"NULL"), (dict(s=0), b"supersample 0"), (dict(s=5), b"supersample 5"),
                     (dict(images=-1), b"bad sizes"), (dict(cells=-1), b"bad sizes"), (dict(width=0), b"bad sizes"),
                     (dict(dtype=2), b"dtype 2"), (dict(dtype=-1), b"dtype -1"), (dict(dst=ONE), b"cannot be the input"),
                     (dict(images=1 << 20, cells=1 << 30, width=5), b"in one launch")):
        assert reduce(**kw) == -1, kw
        assert text in L.spnerf_last_error(), (kw, L.spnerf_last_error())
    assert reduce(s=1) == 0 and reduce(cells=0) == 0 and reduce(images=0) == 0       # nothing launched

    def classes(logits=ONE, cells=7, C=3, labels=two):
        return L.spnerf_ortho_classes(logits, cells, C, labels, None)

    for kw, text in ((dict(logits=None), b"NULL"), (dict(labels=None), b"NULL"), (dict(cells=-1), b"cells -1"),
                     (dict(C=0), b"n_classes 0")):
        assert classes(**kw) == -1, kw
        assert text in L.spnerf_last_error(), (kw, L.spnerf_last_error())
    assert classes(cells=0) == 0


def test_ground_grid():
    g = GroundGrid.from_roi((438638.996411, 3353399.999928, 512, 0.5), 17)
    assert g == GroundGrid(438638.996411, 3353399.999928 + 256.0, 512, 512, 0.5, 17) and g.shape == (512, 512) and not g.south
    e, n = g.cell_centres()
    assert e.shape == n.shape == (512, 512) and e.dtype == n.dtype == np.float64
    assert e[7, 0] == g.xoff + 0.25 and e[0, 511] == g.xoff + 255.75 and n[0, 3] == g.ytop - 0.25 and n[511, 0] == g.ytop - 255.75
    # the snapping get_dsm_from_nerf_prediction applies to a cloud's bounds
    b = GroundGrid.from_bounds(100.3, 103.9, 50.2, 52.6, 0.5, 33, south=True)
    assert (b.xoff, b.ytop, b.xsize, b.ysize, b.south) == (100.0, 53.0, 8, 7, True)
    from oracle import dsm_ref
    assert dsm_ref.dsm_grid([100.3, 103.9], [50.2, 52.6], resolution=0.5) == (b.xoff, b.ytop, b.xsize, b.ysize, 0.5)
    assert dsm_ref.dsm_grid(None, None, roi=(438638.996411, 3353399.999928, 512, 0.5)) == (g.xoff, g.ytop, 512, 512, 0.5)
    for kw, text in ((dict(zone=0), "zone 0"), (dict(zone=61), "zone 61"), (dict(xsize=0), "0 x 3"), (dict(ysize=-2), "5 x -2"),
                     (dict(resolution=0.0), "resolution"), (dict(xoff=float("nan")), "not finite"), (dict(xsize=2.5), "integer")):
        with pytest.raises(ValueError, match=text):
            GroundGrid(**{**dict(xoff=1.0, ytop=2.0, xsize=5, ysize=3, resolution=0.5, zone=17), **kw})
    with pytest.raises(ValueError, match="ROI"):
        GroundGrid.from_roi((1.0, 2.0, 3.0), 17)


def test_python_argument_errors_come_before_any_device_use():
    assert spnerf_amd.render_ortho is spnerf_amd.ortho.render_ortho and spnerf_amd.relight_ortho is spnerf_amd.ortho.relight_ortho
    assert spnerf_amd.ortho_rays is spnerf_amd.ortho.ortho_rays and spnerf_amd.GroundGrid is GroundGrid
    model = spnerf_amd.SPNeRF(feat=64, mapping=True)
    args = types.SimpleNamespace(model="sp-nerf", n_samples=8, n_importance=0, guidedsample=False, beta=False,
                                 sc_lambda=0.0, noise_std=0.0)
    g = GroundGrid(438638.996411, 3353655.999928, 5, 3, 0.5, 17)
    center, rng = np.array([801532.84375, -5452266.5, 3200266.875], np.float32), 141.21875

    def rays(grid=g, lo=-30.0, hi=-2.0, center=center, rng=rng, **kw):
        return spnerf_amd.ortho_rays(grid, lo, hi, center, rng, **kw)

    def render(grid=g, lo=-30.0, hi=-2.0, center=center, rng=rng, sun=(60.0, 140.0), **kw):
        return spnerf_amd.render_ortho({"coarse": model}, args, grid, lo, hi, center, rng, sun, **kw)

    def relight(grid=g, lo=-30.0, hi=-2.0, center=center, rng=rng, dirs=torch.tensor([[0.0, 0.6, 0.8]]), **kw):
        return spnerf_amd.relight_ortho({"coarse": model}, args, grid, lo, hi, center, rng, dirs, **kw)

    for call in (render, relight):
        with pytest.raises(ValueError, match="sc product"):
            call(products=("rgb", "sc"))
        with pytest.raises(ValueError, match="unknown products"):
            call(products=("rgb", "shadow"))
        with pytest.raises(ValueError, match="n_importance > 0"):
            call(products=("rgb", "rgb_coarse"))
        with pytest.raises(ValueError, match="one int"):
            call(ts=torch.zeros(15, dtype=torch.long))
        with pytest.raises(ValueError, match="one label per cell"):
            call(semantics=torch.zeros(5, 3, dtype=torch.long))
        with pytest.raises(_lib.SpnerfError, match="MI355X"):   # only now the model's device matters
            call()
    for call in (rays, render, relight):
        with pytest.raises(ValueError, match="must be a GroundGrid"):
            call(grid=(438638.0, 3353655.0, 5, 3, 0.5, 17))
        for bad in (0, 5, 2.0, True):
            with pytest.raises(ValueError, match="supersample"):
                call(supersample=bad)
        for bad in ((0, 4), (2, 2), (-1, 2), (2, 1), (0.0, 2.0), 3, (0, 1, 2)):
            with pytest.raises(ValueError, match="rows"):
                call(rows=bad)
        with pytest.raises(ValueError, match="must be above min_alt"):
            call(lo=-2.0)
        with pytest.raises(ValueError, match="center must be 3 finite"):
            call(center=np.zeros(4))
        with pytest.raises(ValueError, match="rng .* must be positive"):
            call(rng=0.0)
    for bad in ((1.0,), (1.0, 2.0, 3.0, 4.0)):
        with pytest.raises(ValueError, match="pair in degrees or a 3-vector"):
            render(sun=bad)
        with pytest.raises(ValueError, match="pair in degrees or a 3-vector"):
            rays(sun=bad)
    with pytest.raises(ValueError, match="non-finite"):
        render(sun=(float("nan"), 10.0))
    with pytest.raises(ValueError, match=r"must be \(K, 3\)"):
        relight(dirs=torch.zeros(3))
    with pytest.raises(ValueError, match="K = 0"):
        relight(dirs=torch.zeros(0, 3))
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        rays(device="cpu")
    args.model = "nerf"
    with pytest.raises(ValueError, match="not valid"):
        render()
    with pytest.raises(ValueError, match="not valid"):
        relight()
    # the reduction's own checks
    with pytest.raises(ValueError, match="supersample"):
        spnerf_amd.ortho.reduce_subrays(torch.zeros(8), 5)
    with pytest.raises(ValueError, match="float32 or float64"):
        spnerf_amd.ortho.reduce_subrays(torch.zeros(8, dtype=torch.int32), 2)
    with pytest.raises(ValueError, match="whole cells"):
        spnerf_amd.ortho.reduce_subrays(torch.zeros(6), 2)
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        spnerf_amd.ortho.reduce_subrays(torch.zeros(8), 2)
