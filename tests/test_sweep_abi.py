"""The plane-sweep C ABI (include/spnerf_amd_sweep.h, spnerf_amd._sweep_lib): the header, the ctypes
table and the built library agree, and argument errors come back as codes or are raised before any
device is used — no GPU needed."""
import ctypes

import pytest
import torch

import abi_util
import spnerf_amd
from abi_util import ONE, grid_of, refused
from spnerf_amd import _lib, _sweep_lib, rectify, sweep
from spnerf_amd.ortho import GroundGrid
from spnerf_amd.satellite import load_cameras

HEADER = abi_util.header_path("spnerf_amd_sweep.h")
TWO = ctypes.c_void_p(512)   # like ONE, a non-NULL pointer that is never dereferenced


def test_sweep_exports_match_the_header():
    names = abi_util.check_table(_sweep_lib, HEADER, "spnerf_sweep")
    assert names == ["spnerf_sweep", "spnerf_sweep_abi_version", "spnerf_sweep_grey", "spnerf_sweep_pick", "spnerf_sweep_score"]
    assert all(_sweep_lib.SIGNATURES[n][0] is ctypes.c_int32 for n in names)
    txt = open(HEADER).read()
    consts = abi_util.defines(HEADER, "SPNERF_SWEEP_")
    assert consts["SPNERF_SWEEP_MIN_VIEWS"] == _sweep_lib.SWEEP_MIN_VIEWS == sweep.MIN_VIEWS == 2
    assert consts["SPNERF_SWEEP_MAX_VIEWS"] == _sweep_lib.SWEEP_MAX_VIEWS == sweep.MAX_VIEWS == 16
    assert consts["SPNERF_SWEEP_MAX_PLANES"] == _sweep_lib.SWEEP_MAX_PLANES == sweep.MAX_PLANES == 4096
    assert consts["SPNERF_SWEEP_MAX_RADIUS"] == _sweep_lib.SWEEP_MAX_RADIUS == sweep.MAX_RADIUS == 4
    assert consts["SPNERF_SWEEP_TILE"] == _sweep_lib.SWEEP_TILE == 16
    assert "Occlusion is not modelled" in txt


VIEW_ERRORS = ((dict(v=1), b"n_views 1 outside [2, 16]"), (dict(v=17), b"n_views 17 outside [2, 16]"), (dict(v=0), b"n_views 0"))
PLANE_ERRORS = ((dict(K=0), b"n_planes 0 outside [1, 4096]"), (dict(K=4097), b"n_planes 4097"), (dict(step=0.0), b"step 0 must be"),
                (dict(step=-1.0), b"step -1 must be"), (dict(step=float("nan")), b"step"), (dict(lo=float("inf")), b"alt_lo inf"))
WINDOW_ERRORS = ((dict(r=0), b"radius 0 outside [1, 4]"), (dict(r=5), b"radius 5 outside [1, 4]"), (dict(mv=1), b"min_views 1 outside [2, 4]"),
                 (dict(mv=5), b"min_views 5 outside [2, 4]"), (dict(ms=-0.5), b"min_std -0.5"), (dict(ms=float("nan")), b"min_std"))
GRID_ERRORS = ((dict(xsize=0), b"grid of 0 x 9"), (dict(zone=61), b"UTM zone 61"), (dict(res=0.0), b"resolution 0"))


def test_c_argument_errors_are_reported():
    L = _sweep_lib.lib()

    def fused(cams=ONE, images=ONE, v=4, c=3, lo=-20.0, step=1.0, K=9, r=2, mv=2, ms=0.0, alt=TWO, score=TWO, index=TWO, views=TWO, **g):
        return L.spnerf_sweep(grid_of(**g), cams, images, v, c, lo, step, K, r, mv, ms, alt, score, index, views, None, None)

    for kw in (dict(cams=None), dict(images=None), dict(alt=None), dict(score=None), dict(index=None), dict(views=None)):
        refused(L, fused(**kw), b"sweep: NULL", kw)
    for kw, text in GRID_ERRORS + VIEW_ERRORS + PLANE_ERRORS + WINDOW_ERRORS + ((dict(c=0), b"channels 0 outside [1, 4]"),
                                                                            (dict(c=5), b"channels 5")):
        refused(L, fused(**kw), text, kw)

    def grey(cams=ONE, images=ONE, v=4, c=3, alt=-20.0, out=TWO, valid=TWO, **g):
        return L.spnerf_sweep_grey(grid_of(**g), cams, images, v, c, alt, out, valid, None)

    for kw in (dict(cams=None), dict(images=None), dict(out=None), dict(valid=None)):
        refused(L, grey(**kw), b"sweep_grey: NULL", kw)
    for kw, text in GRID_ERRORS + VIEW_ERRORS + ((dict(c=5), b"channels 5"), (dict(alt=float("nan")), b"alt nan")):
        refused(L, grey(**kw), text, kw)

    def score(grey=ONE, valid=ONE, v=4, H=9, W=15, r=2, mv=2, ms=0.0, out=TWO, views=TWO):
        return L.spnerf_sweep_score(grey, valid, v, H, W, r, mv, ms, out, views, None)

    for kw in (dict(grey=None), dict(valid=None), dict(out=None), dict(views=None)):
        refused(L, score(**kw), b"sweep_score: NULL", kw)
    for kw, text in VIEW_ERRORS + WINDOW_ERRORS + ((dict(H=0), b"grid of 15 x 0"), (dict(W=-1), b"grid of -1 x 9"),
                                                   (dict(H=2 ** 31 - 1, W=2 ** 31 - 1), b"too large")):
        refused(L, score(**kw), text, kw)

    def pick(vol=ONE, vv=ONE, K=9, cells=7, lo=-20.0, step=1.0, alt=TWO, score=TWO, index=TWO, views=TWO):
        return L.spnerf_sweep_pick(vol, vv, K, cells, lo, step, alt, score, index, views, None)

    for kw in (dict(vol=None), dict(vv=None), dict(alt=None), dict(score=None), dict(index=None), dict(views=None)):
        refused(L, pick(**kw), b"sweep_pick: NULL", kw)
    for kw, text in PLANE_ERRORS + ((dict(cells=0), b"cells 0"), (dict(cells=2 ** 32 + 1), b"cells 4294967297")):
        refused(L, pick(**kw), text, kw)


def test_python_argument_errors_come_before_any_device_use():
    assert spnerf_amd.plane_sweep is sweep.plane_sweep
    metas = load_cameras()["images"]
    cams = [rectify.Camera.from_meta(m, 4) for m in metas.values()][:4]
    grid = GroundGrid(438638.0, 3353655.0, 15, 9, 0.5, 17)
    images = [torch.zeros(c.shape + (3,)) for c in cams]

    def call(images=images, cams=cams, grid=grid, lo=-20.0, step=1.0, planes=9, **kw):
        return spnerf_amd.plane_sweep(images, cams, grid, lo, step, planes, **kw)

    for bad, text in ((dict(cams=cams[:1], images=images[:1]), "1 views in one sweep"),
                      (dict(cams=cams * 5, images=images * 5), "20 views in one sweep"), (dict(cams=[], images=[]), "cameras in one call"),
                      (dict(cams=[cams[0], None]), r"cameras\[1\] must be a rectify.Camera"), (dict(grid=0.5), "grid must be a GroundGrid"),
                      (dict(images=images[:3]), "3 images for 4 views"), (dict(images=[im.double() for im in images]), r"images\[0\] must be"),
                      (dict(images=[torch.zeros(c.shape + (5,)) for c in cams]), "C <= 4"),
                      (dict(images=images[:3] + [images[3][:, :, :2]]), r"images\[3\] has 2 channels"),
                      (dict(images=images[:3] + [images[3][:-1]]), r"images\[3\] is .* its camera's image is"),
                      (dict(planes=0), "planes 0 must be"), (dict(planes=4097), "planes 4097 must be"), (dict(planes=2.0), "planes 2.0 must be"),
                      (dict(step=0.0), "step 0.0 must be"), (dict(step=-2), "step -2 must be"), (dict(step=float("nan")), "step nan must be"),
                      (dict(lo=float("inf")), "alt_lo inf must be"), (dict(lo="0"), "alt_lo '0' must be"),
                      (dict(radius=0), "radius 0 must be"), (dict(radius=5), "radius 5 must be"), (dict(radius=1.5), "radius 1.5 must be"),
                      (dict(min_views=1), "min_views 1 must be"), (dict(min_views=5), "min_views 5 must be an integer in 2..4"),
                      (dict(min_std=-1e-3), "min_std -0.001 must be"), (dict(min_std=float("inf")), "min_std inf must be")):
        with pytest.raises(ValueError, match=text):
            call(**bad)
    mixed = [images[0].to("meta")] + images[1:]
    with pytest.raises(ValueError, match="on one device"):
        call(images=mixed)
    with pytest.raises(_lib.SpnerfError, match="MI355X"):                # only now the images' device matters
        call()
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        call(volume=True, radius=4, min_views=4, min_std=0.01)

    with pytest.raises(ValueError, match="alt nan must be"):
        sweep.plane_grey(images, cams, grid, float("nan"))
    with pytest.raises(ValueError, match="1 views in one sweep"):
        sweep.plane_grey(images[:1], cams[:1], grid, -20.0)
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        sweep.plane_grey(images, cams, grid, -20.0)

    grey, valid = torch.zeros(4, 9, 15), torch.ones(4, 9, 15, dtype=torch.uint8)
    for bad in (grey.double(), grey[0], grey[:, :0], grey.numpy()):
        with pytest.raises(ValueError, match="grey must be"):
            sweep.window_score(bad, valid)
    for bad in (valid.bool(), valid[:3], valid[0], valid.numpy()):
        with pytest.raises(ValueError, match="valid must be"):
            sweep.window_score(grey, bad)
    with pytest.raises(ValueError, match="17 views in one sweep"):
        sweep.window_score(torch.zeros(17, 2, 2), torch.ones(17, 2, 2, dtype=torch.uint8))
    for kw, text in ((dict(radius=0), "radius 0"), (dict(min_views=5), "min_views 5"), (dict(min_std=-1.0), "min_std -1.0")):
        with pytest.raises(ValueError, match=text):
            sweep.window_score(grey, valid, **kw)
    with pytest.raises(ValueError, match="on one device"):
        sweep.window_score(grey, valid.to("meta"))
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        sweep.window_score(grey, valid)

    volume, views = torch.zeros(9, 9, 15), torch.ones(9, 9, 15, dtype=torch.uint8)
    for bad in (volume.double(), volume[0], volume[:, :0], volume.numpy()):
        with pytest.raises(ValueError, match="volume must be"):
            sweep.pick_plane(bad, views, -20.0, 1.0)
    for bad in (views.int(), views[:3], views.numpy()):
        with pytest.raises(ValueError, match="views must be"):
            sweep.pick_plane(volume, bad, -20.0, 1.0)
    with pytest.raises(ValueError, match="step 0 must be"):
        sweep.pick_plane(volume, views, -20.0, 0)
    with pytest.raises(ValueError, match="planes 4097 must be"):
        sweep.pick_plane(torch.zeros(4097, 1, 1), torch.ones(4097, 1, 1, dtype=torch.uint8), -20.0, 1.0)
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        sweep.pick_plane(volume, views, -20.0, 1.0)
