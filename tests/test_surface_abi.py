"""The surface-sweep C ABI (include/spnerf_amd_surface.h, spnerf_amd._surface_lib): the header, the ctypes
table and the built library agree, and argument errors come back as codes or are raised before any device is
used — no GPU needed."""
import ctypes

import pytest
import torch

import abi_util
import spnerf_amd
from abi_util import A, B, C, D, refused
from spnerf_amd import _lib, _ortho_lib, _surface_lib, rectify, sgm, surface
from spnerf_amd.ortho import GroundGrid
from spnerf_amd.satellite import load_cameras

HEADER = abi_util.header_path("spnerf_amd_surface.h")


def test_surface_exports_match_the_header():
    names = abi_util.check_table(_surface_lib, HEADER, "spnerf_surface")
    assert names == ["spnerf_surface_abi_version", "spnerf_surface_grey", "spnerf_surface_lift", "spnerf_surface_sweep", "spnerf_surface_upsample"]
    assert all(_surface_lib.SIGNATURES[n][0] is ctypes.c_int32 for n in names)
    consts = abi_util.defines(HEADER, "SPNERF_SURFACE_")
    assert consts["SPNERF_SURFACE_MAX_FACTOR"] == _surface_lib.SURFACE_MAX_FACTOR == surface.MAX_FACTOR == 8


def test_c_argument_errors_are_reported():
    L = _surface_lib.lib()
    nan, inf = float("nan"), float("inf")
    grid = _ortho_lib.OrthoGrid(438638.0, 3353655.0, 0.5, 15, 9, 17, 0, 1)

    def lift(base=A, rel=B, n=7, out=C):
        return L.spnerf_surface_lift(base, rel, n, out, None)

    for kw in (dict(base=None), dict(rel=None), dict(out=None)):
        refused(L, lift(**kw), b"surface_lift: NULL", kw)
    refused(L, lift(n=0), b"surface_lift: count 0 outside", "n")
    refused(L, lift(n=2 ** 32 + 1), b"surface_lift: count 4294967297", "n")

    def up(coarse=A, f=2, H=9, W=15, out=B):
        return L.spnerf_surface_upsample(coarse, f, H, W, out, None)

    for kw in (dict(coarse=None), dict(out=None)):
        refused(L, up(**kw), b"surface_upsample: NULL", kw)
    for kw, text in ((dict(f=0), b"factor 0 outside [1, 8]"), (dict(f=9), b"factor 9 outside [1, 8]"), (dict(H=0), b"grid of 15 x 0"),
                     (dict(W=-1), b"grid of -1 x 9"), (dict(H=2 ** 31 - 1, W=2 ** 31 - 1), b"grid of 2147483647 x 2147483647 cells is too large")):
        refused(L, up(**kw), b"surface_upsample: " + text, kw)

    def grey(grid=ctypes.byref(grid), cams=A, images=B, V=4, C=3, base=C, offset=0.0, grey=D, valid=D):
        return L.spnerf_surface_grey(grid, cams, images, V, C, base, offset, grey, valid, None)

    for kw in (dict(grid=None), dict(cams=None), dict(images=None), dict(base=None), dict(grey=None), dict(valid=None)):
        refused(L, grey(**kw), b"surface_grey: NULL", kw)
    for kw, text in ((dict(V=1), b"n_views 1 outside [2, 16]"), (dict(V=17), b"n_views 17"), (dict(C=5), b"channels 5 outside [1, 4]"),
                     (dict(offset=nan), b"offset nan is not finite"), (dict(offset=inf), b"offset inf")):
        refused(L, grey(**kw), b"surface_grey: " + text, kw)

    def sweep(grid=ctypes.byref(grid), cams=A, images=B, V=4, C=3, base=C, lo=-3.0, step=0.5, K=13, radius=2, mv=2, std=0.0, alt=D, score=D,
              index=D, views=D):
        return L.spnerf_surface_sweep(grid, cams, images, V, C, base, lo, step, K, radius, mv, std, alt, score, index, views, None, None)

    for kw in (dict(grid=None), dict(cams=None), dict(images=None), dict(base=None), dict(alt=None), dict(score=None), dict(index=None),
               dict(views=None)):
        refused(L, sweep(**kw), b"surface_sweep: NULL", kw)
    for kw, text in ((dict(V=1), b"n_views 1 outside"), (dict(C=0), b"channels 0"), (dict(K=0), b"n_planes 0 outside [1, 4096]"),
                     (dict(K=4097), b"n_planes 4097"), (dict(lo=nan), b"alt_lo nan is not finite"), (dict(step=0.0), b"step 0 must be"),
                     (dict(radius=0), b"radius 0 outside [1, 4]"), (dict(radius=5), b"radius 5"), (dict(mv=1), b"min_views 1 outside [2, 4]"),
                     (dict(mv=5), b"min_views 5"), (dict(std=-1.0), b"min_std -1 must be")):
        refused(L, sweep(**kw), b"surface_sweep: " + text, kw)


def test_python_argument_errors_come_before_any_device_use():
    for name in ("surface_grey", "surface_lift", "surface_sweep", "upsample_dsm", "pyramid_sweep", "coarsen"):
        assert getattr(spnerf_amd, name) is getattr(surface, name)
    assert spnerf_amd.surface is surface
    nan, inf = float("nan"), float("inf")
    metas = load_cameras()["images"]
    cams = [rectify.Camera.from_meta(m, 4) for m in metas.values()][:4]
    grid = GroundGrid(438638.0, 3353655.0, 15, 9, 0.5, 17)
    images = [torch.zeros(c.shape + (3,)) for c in cams]
    base = torch.zeros(9, 15)
    bad_bases = ((base.double(), "base must be a non-empty \\(H, W\\) float32"), (base[0], "base must be"), (base[:, :0], "base must be"),
                 (base.numpy(), "base must be"), (base[:8], "base \\(8, 15\\) is not the grid's \\(9, 15\\)"),
                 (base.t(), "base \\(15, 9\\) is not the grid's"), (base.to("meta"), "on one device"))

    # coarsen
    assert surface.coarsen(grid, 1) == grid
    assert surface.coarsen(grid, 4) == GroundGrid(438638.0, 3353655.0, 4, 3, 2.0, 17) and surface.coarsen(grid, 8).shape == (2, 2)
    assert surface.coarsen(surface.coarsen(grid, 2), 2) == surface.coarsen(grid, 4)
    for f in (0, 9, 2.0, True, "2"):
        with pytest.raises(ValueError, match="factor .* must be an integer in 1..8"):
            surface.coarsen(grid, f)
    with pytest.raises(ValueError, match="grid must be a GroundGrid"):
        surface.coarsen(0.5, 2)

    # upsample_dsm
    coarse = torch.zeros(3, 4)
    for f in (0, 9, 2.5, True):
        with pytest.raises(ValueError, match="factor .* must be an integer in 1..8"):
            surface.upsample_dsm(coarse, f, (9, 15))
    for shape in ((9,), (9, 15, 1), (0, 15), (9, -1), (9.0, 15), None):
        with pytest.raises(ValueError, match="shape .* must be \\(H, W\\)"):
            surface.upsample_dsm(coarse, 4, shape)
    for bad in (coarse.double(), coarse[0], coarse[:, :0], coarse.numpy()):
        with pytest.raises(ValueError, match="coarse must be a non-empty \\(H, W\\) float32"):
            surface.upsample_dsm(bad, 4, (9, 15))
    with pytest.raises(ValueError, match="coarse \\(3, 4\\) is not \\(5, 8\\)"):
        surface.upsample_dsm(coarse, 2, (9, 15))
    with pytest.raises(ValueError, match="coarse \\(3, 4\\) is not \\(3, 5\\)"):
        surface.upsample_dsm(coarse, 4, (9, 17))
    with pytest.raises(_lib.SpnerfError, match="MI355X"):                # only now the raster's device matters
        surface.upsample_dsm(coarse, 4, (9, 15))
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        surface.upsample_dsm(coarse, 4, (12, 16))

    # surface_lift
    for bad in (base.double(), base[0], base[:, :0], base.numpy()):
        with pytest.raises(ValueError, match="base must be"):
            surface.surface_lift(bad, base)
    for bad in (base.double(), base[:8], base[0], base.numpy()):
        with pytest.raises(ValueError, match="rel must be|rel \\(8, 15\\) is not"):
            surface.surface_lift(base, bad)
    with pytest.raises(ValueError, match="on one device"):
        surface.surface_lift(base, base.to("meta"))
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        surface.surface_lift(base, base)

    # surface_grey
    for bad, text in bad_bases:
        with pytest.raises(ValueError, match=text):
            surface.surface_grey(images, cams, grid, bad, 0.0)
    for off in (nan, inf, "0", True):
        with pytest.raises(ValueError, match="offset .* must be finite"):
            surface.surface_grey(images, cams, grid, base, off)
    with pytest.raises(ValueError, match="3 images for 4 views"):
        surface.surface_grey(images[:3], cams, grid, base, 0.0)
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        surface.surface_grey(images, cams, grid, base, 0.0)

    # surface_sweep
    def sweep(images=images, cams=cams, grid=grid, base=base, lo=-3.0, step=0.5, planes=13, **kw):
        return surface.surface_sweep(images, cams, grid, base, lo, step, planes, **kw)

    for bad, text in bad_bases:
        with pytest.raises(ValueError, match=text):
            sweep(base=bad)
    window = ((dict(radius=5), "radius 5 must be"), (dict(radius=0), "radius 0 must be"), (dict(min_views=5), "min_views 5 must be"),
              (dict(min_views=1), "min_views 1 must be"), (dict(min_std=-1e-3), "min_std -0.001 must be"), (dict(min_std=nan), "min_std nan must be"))
    scene = ((dict(cams=cams[:1], images=images[:1]), "1 views in one sweep"), (dict(grid=0.5), "grid must be a GroundGrid"),
             (dict(images=images[:3]), "3 images for 4 views"), (dict(step=0.0), "step 0.0 must be"), (dict(step=nan), "step nan must be"))
    for kw, text in scene + window + ((dict(lo=inf), "off_lo inf must be finite"), (dict(lo="0"), "off_lo '0' must be"),
                                      (dict(planes=0), "planes 0 must be"), (dict(planes=4097), "planes 4097 must be")):
        with pytest.raises(ValueError, match=text):
            sweep(**kw)
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        sweep()
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        sweep(volume=True, radius=4, min_views=4, min_std=0.01, planes=1)

    # pyramid_sweep
    def pyramid(images=images, cams=cams, grid=grid, lo=-30.0, step=0.5, planes=64, **kw):
        return surface.pyramid_sweep(images, cams, grid, lo, step, planes, **kw)

    for factors, text in (((2, 4), "strictly descending"), ((4, 4), "strictly descending"), ((2, 2, 1), "integers in 2..8"),
                          ((6, 4), "6 is not an integer multiple of 4"), ((8, 3), "8 is not an integer multiple of 3"),
                          ((9,), "integers in 2..8"), ((1,), "integers in 2..8"), ((16, 4), "integers in 2..8"), ((), "non-empty tuple"),
                          (4, "non-empty tuple"), ((4.0,), "integers in 2..8"), ((True,), "integers in 2..8")):
        with pytest.raises(ValueError, match=text):
            pyramid(factors=factors)
    for reach in (0, -1, nan, inf, "3", True):
        with pytest.raises(ValueError, match="reach .* must be finite and > 0"):
            pyramid(reach=reach)
    penalties = ((dict(p1=-0.125), "p1 -0.125 must be"), (dict(p1=0.5, p2=0.25), "p2 0.25 must be finite and >= p1 0.5"),
                 (dict(unscored=nan), "unscored nan must be"), (dict(paths=3), "paths 3 must be 4 or 8"))
    for kw, text in scene + window + penalties + ((dict(lo=inf), "alt_lo inf must be"), (dict(planes=0), "planes 0 must be"),
                                                  (dict(planes=1025), "planes of the level of factor 4: 513 must be an integer in 1..512"),
                                                  (dict(reach=300), "planes of the level of factor 1: 1201 must be")):
        with pytest.raises(ValueError, match=text):
            pyramid(**kw)
    assert surface.level_plan((4,), 64, 3) == [(4, 2, 32), (1, 1, 13)]
    assert surface.level_plan((4, 2), 63, 3) == [(4, 2, 32), (2, 2, 7), (1, 1, 13)]
    assert surface.level_plan((8, 4, 2), 9, 1.5) == [(8, 2, 5), (4, 2, 5), (2, 2, 5), (1, 1, 7)]
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        pyramid()
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        pyramid(factors=(8, 4, 2), reach=1, radius=1, paths=4, p1=0.125, p2=0.75, planes=1024)
    assert sgm.P1 == 0.25 and sgm.P2 == 2.0
