"""The orthorectification C ABI (include/spnerf_amd_rectify.h, spnerf_amd._rectify_lib): the header, the
ctypes table and the built library agree, and argument errors come back as codes or are raised before
any device is used — no GPU needed."""
import ctypes
import re

import numpy as np
import pytest
import torch

import abi_util
import spnerf_amd
from abi_util import ONE, grid_of, refused
from spnerf_amd import _lib, _ortho_lib, _rectify_lib, rectify
from spnerf_amd.ortho import GroundGrid
from spnerf_amd.satellite import RPCModel, load_cameras, rescale_rpc

HEADER = abi_util.header_path("spnerf_amd_rectify.h")
TWO = ctypes.c_void_p(512)   # like ONE, a non-NULL pointer that is never dereferenced


def test_rectify_exports_match_the_header():
    assert abi_util.check_table(_rectify_lib, HEADER, "spnerf_rectify") == [
        "spnerf_rectify", "spnerf_rectify_abi_version", "spnerf_rectify_mosaic", "spnerf_rectify_project", "spnerf_rectify_sample",
        "spnerf_rectify_view_dirs"]
    txt = open(HEADER).read()
    consts = abi_util.defines(HEADER, "SPNERF_RECTIFY_")
    assert consts["SPNERF_RECTIFY_MAX_VIEWS"] == _rectify_lib.RECTIFY_MAX_VIEWS == rectify.MAX_VIEWS == 64
    assert consts["SPNERF_RECTIFY_MAX_CHANNELS"] == _rectify_lib.RECTIFY_MAX_CHANNELS == 4
    assert consts["SPNERF_RECTIFY_CAMERA_DOUBLES"] == _rectify_lib.RECTIFY_CAMERA_DOUBLES == 90
    assert (consts["SPNERF_RECTIFY_MEAN"], consts["SPNERF_RECTIFY_MEDIAN"]) == (_rectify_lib.RECTIFY_MEAN, _rectify_lib.RECTIFY_MEDIAN) == (0, 1)
    # the struct of the header, field for field
    body = re.search(r"typedef struct spnerf_rectify_image \{(.*?)\} spnerf_rectify_image;", txt, re.S).group(1)
    fields = [n.strip("* ") for decl in re.findall(r"(?:const float\*|int32_t)\s+([^;]+);", body) for n in re.split(r",\s*", decl)]
    assert fields == [f for f, _ in _rectify_lib.RectifyImage._fields_]
    assert ctypes.sizeof(_rectify_lib.RectifyImage) == _rectify_lib.IMAGE_BYTES == 16


GRID_ERRORS = ((dict(xsize=0), b"grid of 0 x 9"), (dict(ysize=-3), b"grid of 15 x -3"),
               (dict(xsize=2 ** 31 - 1, ysize=2 ** 31 - 1), b"too large"), (dict(zone=0), b"UTM zone 0"), (dict(zone=61), b"UTM zone 61"),
               (dict(res=0.0), b"resolution 0"), (dict(res=float("nan")), b"resolution"), (dict(res=float("inf")), b"resolution"),
               (dict(xoff=float("nan")), b"non-finite grid origin"), (dict(ytop=float("inf")), b"non-finite grid origin"))


def test_project_and_fused_argument_errors_are_reported():
    L = _rectify_lib.lib()

    def project(dsm=ONE, grid=None, cams=ONE, v=2, pix=TWO, **g):
        return L.spnerf_rectify_project(dsm, grid_of(**g) if grid is None else grid, cams, v, pix, None)

    def fused(dsm=ONE, grid=None, cams=ONE, images=ONE, v=2, c=3, rgb=TWO, valid=TWO, pix=None, **g):
        return L.spnerf_rectify(dsm, grid_of(**g) if grid is None else grid, cams, images, v, c, rgb, valid, pix, None)

    for kw in (dict(dsm=None), dict(cams=None), dict(pix=None), dict(grid=ctypes.POINTER(_ortho_lib.OrthoGrid)())):
        refused(L, project(**kw), b"rectify_project: NULL", kw)
    for kw in (dict(dsm=None), dict(cams=None), dict(images=None), dict(rgb=None), dict(valid=None),
               dict(grid=ctypes.POINTER(_ortho_lib.OrthoGrid)())):
        refused(L, fused(**kw), b"rectify: NULL", kw)
    for kw, text in GRID_ERRORS + ((dict(v=0), b"n_views 0"), (dict(v=-1), b"n_views -1"), (dict(v=65), b"n_views 65 outside [1, 64]")):
        refused(L, project(**kw), text, kw)
        refused(L, fused(**kw), text, kw)
    for c in (0, -1, 5):
        refused(L, fused(c=c), f"channels {c} outside [1, 4]".encode(), c)


def test_sample_view_dirs_and_mosaic_argument_errors_are_reported():
    L = _rectify_lib.lib()

    def sample(images=ONE, v=2, c=3, pix=ONE, cells=7, rgb=TWO, valid=TWO):
        return L.spnerf_rectify_sample(images, v, c, pix, cells, rgb, valid, None)

    for kw, text in ((dict(images=None), b"NULL"), (dict(pix=None), b"NULL"), (dict(rgb=None), b"NULL"), (dict(valid=None), b"NULL"),
                     (dict(cells=0), b"cells 0"), (dict(cells=-4), b"cells -4"), (dict(cells=2 ** 32 + 1), b"cells 4294967297"),
                     (dict(v=0), b"n_views 0"), (dict(v=65), b"n_views 65"), (dict(c=0), b"channels 0"), (dict(c=5), b"channels 5")):
        refused(L, sample(**kw), text, kw)

    def view_dirs(grid=None, cams=ONE, v=2, lo=-30.0, hi=-2.0, dirs=TWO, spread=TWO, **g):
        return L.spnerf_rectify_view_dirs(grid_of(**g) if grid is None else grid, cams, v, lo, hi, dirs, spread, None)

    for kw in (dict(cams=None), dict(dirs=None), dict(spread=None), dict(grid=ctypes.POINTER(_ortho_lib.OrthoGrid)())):
        refused(L, view_dirs(**kw), b"rectify_view_dirs: NULL", kw)
    for kw, text in GRID_ERRORS + ((dict(v=0), b"n_views 0"), (dict(v=65), b"n_views 65"), (dict(lo=-2.0, hi=-2.0), b"alt_hi -2 must be above alt_lo -2"),
                                   (dict(lo=5.0, hi=1.0), b"alt_hi 1 must be above alt_lo 5"), (dict(hi=float("nan")), b"must be above"),
                                   (dict(lo=float("-inf")), b"must be above")):
        refused(L, view_dirs(**kw), text, kw)

    def mosaic(rgb=ONE, usable=ONE, v=2, cells=7, c=3, mode=1, out=TWO, count=TWO, spread=TWO):
        return L.spnerf_rectify_mosaic(rgb, usable, v, cells, c, mode, out, count, spread, None)

    for kw, text in ((dict(rgb=None), b"NULL"), (dict(usable=None), b"NULL"), (dict(out=None), b"NULL"), (dict(count=None), b"NULL"),
                     (dict(spread=None), b"NULL"), (dict(cells=0), b"cells 0"), (dict(cells=2 ** 40), b"cells 1099511627776"),
                     (dict(v=0), b"n_views 0"), (dict(v=65), b"n_views 65"), (dict(c=0), b"channels 0"), (dict(c=5), b"channels 5"),
                     (dict(mode=2), b"mode 2 is neither"), (dict(mode=-1), b"mode -1 is neither")):
        refused(L, mosaic(**kw), text, kw)


def test_camera_is_the_rescaled_model():
    meta = load_cameras()["images"]["JAX_269_006_RGB"]
    cam = rectify.Camera.from_meta(meta, 4)
    assert cam.downscale == 4.0 and cam.shape == (meta["height"] // 4, meta["width"] // 4)
    want = np.array(list(rescale_rpc(RPCModel(meta["rpc"]), 1.0 / 4).packed()))
    assert cam.packed().dtype == np.float64 and np.array_equal(cam.packed(), want)
    assert np.array_equal(rectify.Camera(RPCModel(meta["rpc"])).packed(), np.array(list(RPCModel(meta["rpc"]).packed())))
    for bad in (0, -1.0, float("nan"), float("inf"), "4", True, None):
        with pytest.raises(ValueError, match="downscale"):
            rectify.Camera(RPCModel(meta["rpc"]), bad)
    with pytest.raises(ValueError, match="RPCModel"):
        rectify.Camera(meta["rpc"])


def test_python_argument_errors_come_before_any_device_use():
    assert spnerf_amd.orthorectify is rectify.orthorectify
    metas = load_cameras()["images"]
    cams = [rectify.Camera.from_meta(m, 4) for m in metas.values()]
    grid = GroundGrid(438638.0, 3353655.0, 15, 9, 0.5, 17)
    dsm = torch.full((9, 15), -20.0, dtype=torch.float64)
    images = [torch.zeros(c.shape + (3,)) for c in cams]

    # the DSM, the grid and the cameras: every entry that takes them
    for call in (lambda **k: rectify.project_cells(k.get("dsm", dsm), k.get("grid", grid), k.get("cams", cams)),
                 lambda **k: rectify.orthorectify(k.get("images", images), k.get("cams", cams), k.get("dsm", dsm), k.get("grid", grid), -30.0, -2.0)):
        for bad in (np.zeros((9, 15)), torch.zeros(9), torch.zeros(2, 9, 15), torch.zeros(0, 15), torch.zeros(9, 15, dtype=torch.int32),
                    torch.zeros(9, 15, dtype=torch.float16)):
            with pytest.raises(ValueError, match="dsm must be"):
                call(dsm=bad)
        with pytest.raises(ValueError, match="is not the grid's"):
            call(grid=GroundGrid(438638.0, 3353655.0, 9, 15, 0.5, 17))               # 15 rows of 9 cells, not 9 of 15
        for bad in (0.5, None):
            with pytest.raises(ValueError, match="grid must be a GroundGrid"):
                call(grid=bad)
        with pytest.raises(ValueError, match="cameras in one call"):
            call(cams=[], images=[])
        with pytest.raises(ValueError, match="65 cameras in one call"):
            call(cams=cams[:1] * 65, images=images[:1] * 65)
        with pytest.raises(ValueError, match=r"cameras\[1\] must be a rectify.Camera"):
            call(cams=[cams[0], metas["JAX_269_007_RGB"]], images=images[:2])
        with pytest.raises(_lib.SpnerfError, match="MI355X"):                       # only now the DSM's device matters
            call()
        with pytest.raises(_lib.SpnerfError, match="MI355X"):
            call(dsm=dsm.float())

    ortho = spnerf_amd.orthorectify
    for bad, text in ((images[:3], "3 images for 4 views"), (None, "images must be"), ([im.double() for im in images], r"images\[0\] must be"),
                      ([images[0], images[1][..., 0], images[2], images[3]], r"images\[1\] must be"),
                      ([images[0], images[1], images[2][:, :, :2], images[3]], r"images\[2\] has 2 channels"),
                      ([torch.zeros(c.shape + (5,)) for c in cams], r"C <= 4"),
                      ([images[0], images[1], images[2], images[3][:-1]], r"images\[3\] is .* its camera's image is")):
        with pytest.raises(ValueError, match=text):
            ortho(bad, cams, dsm, grid, -30.0, -2.0)
    for lo, hi in ((-2.0, -30.0), (-2.0, -2.0), (float("nan"), 0.0), (0.0, float("inf"))):
        with pytest.raises(ValueError, match="must be above"):
            ortho(images, cams, dsm, grid, lo, hi)
    with pytest.raises(ValueError, match="neither 'mean' nor 'median'"):
        ortho(images, cams, dsm, grid, -30.0, -2.0, mosaic="mode")
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        ortho(images, cams, dsm, grid, -30.0, -2.0, mosaic="median", pix=True)

    pix = torch.zeros(4, 9, 15, 2, dtype=torch.float64)
    for bad in (pix.float(), pix[0], pix[..., :1], pix[:, :0], pix.numpy()):
        with pytest.raises(ValueError, match="pix must be"):
            rectify.sample_images(images, bad)
    with pytest.raises(ValueError, match="4 images for 3 views"):
        rectify.sample_images(images, pix[:3])
    with pytest.raises(ValueError, match=r"images\[0\] must be"):
        rectify.sample_images([im.numpy() for im in images], pix)
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        rectify.sample_images(images, pix)
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        rectify.sample_images(torch.zeros(4, 6, 5, 1), pix)                          # a (V, h, w, C) tensor is V images

    for lo, hi in ((-2.0, -30.0), (1.0, 1.0), (float("nan"), 0.0)):
        with pytest.raises(ValueError, match="must be above"):
            rectify.view_directions(grid, cams, lo, hi)
    with pytest.raises(ValueError, match="grid must be a GroundGrid"):
        rectify.view_directions(None, cams, -30.0, -2.0)
    with pytest.raises(ValueError, match="cameras in one call"):
        rectify.view_directions(grid, [], -30.0, -2.0)
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        rectify.view_directions(grid, cams, -30.0, -2.0, device="cpu")

    rgb, usable = torch.zeros(4, 9, 15, 3), torch.ones(4, 9, 15, dtype=torch.uint8)
    for bad in (rgb.double(), rgb[0], rgb[:, :0], torch.zeros(65, 2, 2, 3), torch.zeros(2, 2, 2, 5), rgb.numpy()):
        with pytest.raises(ValueError, match="rgb must be"):
            rectify.mosaic(bad, usable)
    for bad in (usable.bool(), usable[:3], usable[0], usable.numpy()):
        with pytest.raises(ValueError, match="usable must be"):
            rectify.mosaic(rgb, bad)
    with pytest.raises(ValueError, match="neither 'mean' nor 'median'"):
        rectify.mosaic(rgb, usable, "max")
    for mode in ("mean", "median"):
        with pytest.raises(_lib.SpnerfError, match="MI355X"):
            rectify.mosaic(rgb, usable, mode)
