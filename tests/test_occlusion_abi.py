"""The occlusion C ABI (include/spnerf_amd_occlusion.h, spnerf_amd._occlusion_lib): the header, the ctypes
table and the built library agree, and argument errors come back as codes or are raised before any
device is used — no GPU needed."""
import ctypes
import re

import numpy as np
import pytest
import torch

import abi_util
import spnerf_amd
from abi_util import ONE, grid_of, refused
from spnerf_amd import _lib, _occlusion_lib, _shadow_lib, _sweep_lib, occlusion, rectify
from spnerf_amd.ortho import GroundGrid
from spnerf_amd.satellite import load_cameras

HEADER = abi_util.header_path("spnerf_amd_occlusion.h")
TWO = ctypes.c_void_p(512)   # like ONE, a non-NULL pointer that is never dereferenced


def test_occlusion_exports_match_the_header():
    # `dirs` is a host pointer to floats
    assert abi_util.check_table(_occlusion_lib, HEADER, "spnerf_occlusion", {("spnerf_occlusion_floor", 4): ctypes.POINTER(ctypes.c_float)}) == [
        "spnerf_occlusion_abi_version", "spnerf_occlusion_floor", "spnerf_occlusion_gate", "spnerf_occlusion_sweep", "spnerf_occlusion_workspace_bytes"]
    L = _occlusion_lib.lib()
    txt = open(HEADER).read()
    consts = abi_util.defines(HEADER, "SPNERF_OCCLUSION_")
    assert consts["SPNERF_OCCLUSION_MAX_VIEWS"] == _occlusion_lib.OCCLUSION_MAX_VIEWS == occlusion.MAX_VIEWS == _sweep_lib.SWEEP_MAX_VIEWS == 16
    # the march is stated in the words of the cast's header
    cast = re.sub(r"\s*\*\s*", " ", open(abi_util.header_path("spnerf_amd_shadow.h")).read())
    mine = re.sub(r"\s*\*\s*", " ", txt)
    for words in ("step m = 1, 2, ... visits column i' = i + m·sign(a) at row position y = j + m·q, q = b/|a|.",
                  "kept within [min(h0, h1), max(h0, h1)]; a step that needs a NaN height contributes nothing.",
                  "march ends when i' leaves the grid or y leaves [0, H - 1]."):
        assert words in cast and words in mine, words
    assert L.spnerf_occlusion_workspace_bytes(512, 512) == _shadow_lib.lib().spnerf_shadow_workspace_bytes(512, 512) == 2048


def test_c_argument_errors_are_reported():
    L = _occlusion_lib.lib()
    up = (ctypes.c_float * 6)(0.1, 0.2, 0.9, -0.1, 0.0, 0.8)

    def floor(dsm=ONE, H=9, W=15, res=0.5, dirs=up, v=2, ws=TWO, out=TWO):
        return L.spnerf_occlusion_floor(dsm, H, W, res, dirs, v, ws, out, None)

    for kw in (dict(dsm=None), dict(dirs=None), dict(ws=None), dict(out=None)):
        refused(L, floor(**kw), b"occlusion_floor: NULL", kw)
    for kw, text in ((dict(H=0), b"grid of 15 x 0"), (dict(W=-1), b"grid of -1 x 9"), (dict(H=2 ** 30, W=2 ** 30), b"too large"),
                     (dict(v=0), b"n_views 0 outside [1, 16]"), (dict(v=17), b"n_views 17 outside [1, 16]"), (dict(res=0.0), b"resolution 0"),
                     (dict(res=float("nan")), b"resolution"), (dict(ws=ctypes.c_void_p(520)), b"workspace not 16-byte aligned"),
                     (dict(dirs=(ctypes.c_float * 6)(0.1, 0.2, 0.9, 0.0, float("nan"), 0.8)), b"direction 1 is not finite"),
                     (dict(dirs=(ctypes.c_float * 6)(0.1, 0.2, 0.0, 0.0, 0.1, 0.8)), b"direction 0 has up 0")):
        refused(L, floor(**kw), text, kw)
    assert L.spnerf_occlusion_workspace_bytes(0, 4) == -1 and b"grid of 4 x 0" in L.spnerf_last_error()

    def gate(grey=ONE, valid=ONE, fl=TWO, v=4, cells=7, alt=-20.0, slack=0.5):
        return L.spnerf_occlusion_gate(grey, valid, fl, v, cells, alt, slack, None)

    for kw in (dict(grey=None), dict(valid=None), dict(fl=None)):
        refused(L, gate(**kw), b"occlusion_gate: NULL", kw)
    for kw, text in ((dict(v=0), b"n_views 0"), (dict(v=17), b"n_views 17"), (dict(cells=0), b"cells 0"), (dict(cells=2 ** 32 + 1), b"cells 4294967297"),
                     (dict(alt=float("inf")), b"alt inf"), (dict(slack=-0.5), b"slack -0.5 must be"), (dict(slack=float("nan")), b"slack"),
                     (dict(slack=float("inf")), b"slack inf")):
        refused(L, gate(**kw), text, kw)

    def fused(cams=ONE, images=ONE, v=4, c=3, lo=-20.0, step=1.0, K=9, r=2, mv=2, ms=0.0, fl=ONE, slack=0.5, alt=TWO, score=TWO, index=TWO,
              views=TWO, **g):
        return L.spnerf_occlusion_sweep(grid_of(**g), cams, images, v, c, lo, step, K, r, mv, ms, fl, slack, alt, score, index, views, None, None)

    for kw in (dict(cams=None), dict(images=None), dict(fl=None), dict(alt=None), dict(score=None), dict(index=None), dict(views=None)):
        refused(L, fused(**kw), b"occlusion_sweep: NULL", kw)
    for kw, text in ((dict(slack=-1.0), b"slack -1 must be"), (dict(slack=float("inf")), b"slack inf"), (dict(xsize=0), b"grid of 0 x 9"),
                     (dict(zone=61), b"UTM zone 61"), (dict(v=1), b"n_views 1 outside [2, 16]"), (dict(v=17), b"n_views 17"),
                     (dict(c=5), b"channels 5"), (dict(K=0), b"n_planes 0 outside [1, 4096]"), (dict(step=0.0), b"step 0 must be"),
                     (dict(lo=float("inf")), b"alt_lo inf"), (dict(r=0), b"radius 0 outside [1, 4]"), (dict(r=5), b"radius 5"),
                     (dict(mv=5), b"min_views 5 outside [2, 4]"), (dict(ms=-0.5), b"min_std -0.5")):
        refused(L, fused(**kw), text, kw)


def test_python_argument_errors_come_before_any_device_use():
    assert spnerf_amd.visibility_floor is occlusion.visibility_floor and spnerf_amd.gate_plane is occlusion.gate_plane
    assert spnerf_amd.visible_sweep is occlusion.visible_sweep and spnerf_amd.refine_sweep is occlusion.refine_sweep
    metas = load_cameras()["images"]
    cams = [rectify.Camera.from_meta(m, 4) for m in metas.values()][:4]
    grid = GroundGrid(438638.0, 3353655.0, 15, 9, 0.5, 17)
    images = [torch.zeros(c.shape + (3,)) for c in cams]
    dsm, dirs = torch.zeros(9, 15, dtype=torch.float64), np.array([[0.1, 0.2, 0.9], [-0.2, 0.0, 0.8]], np.float32)

    for bad in (dsm.int(), dsm[0], dsm[:, :0], dsm.numpy()):
        with pytest.raises(ValueError, match="dsm must be"):
            spnerf_amd.visibility_floor(bad, grid, dirs)
    with pytest.raises(ValueError, match="is not the grid's"):
        spnerf_amd.visibility_floor(dsm[:8], grid, dirs)
    with pytest.raises(ValueError, match="resolution"):
        spnerf_amd.visibility_floor(dsm, -0.5, dirs)
    for bad, text in ((dirs[:, :2], "dirs must be"), (dirs[0], "dirs must be"), (np.zeros((0, 3), np.float32), "0 directions"),
                      (np.tile(dirs, (9, 1)), "18 directions"), (np.array([[0.1, np.nan, 0.9]]), "non-finite"),
                      (np.array([[0.1, 0.2, 0.9], [0.1, 0.2, 0.0]]), r"dirs\[1\] has up = 0.0"), (np.array([["a", "b", "c"]]), "dirs must be")):
        with pytest.raises(ValueError, match=text):
            spnerf_amd.visibility_floor(dsm, grid, bad)
    with pytest.raises(_lib.SpnerfError, match="MI355X"):                # only now the device matters
        spnerf_amd.visibility_floor(dsm, grid, torch.tensor(dirs))
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        spnerf_amd.visibility_floor(dsm.float(), 0.5, dirs[:1])

    grey, valid, floor = torch.zeros(4, 9, 15), torch.ones(4, 9, 15, dtype=torch.uint8), torch.zeros(4, 9, 15)
    for bad in (grey.double(), grey[0], grey[:, :0], grey.numpy()):
        with pytest.raises(ValueError, match="grey must be"):
            spnerf_amd.gate_plane(bad, valid, floor, -20.0)
    with pytest.raises(ValueError, match="17 views in one call"):
        spnerf_amd.gate_plane(torch.zeros(17, 2, 2), torch.ones(17, 2, 2, dtype=torch.uint8), torch.zeros(17, 2, 2), -20.0)
    for bad in (valid.bool(), valid[:3], valid.numpy()):
        with pytest.raises(ValueError, match="valid must be"):
            spnerf_amd.gate_plane(grey, bad, floor, -20.0)
    for bad in (floor.double(), floor[:3], floor[0], floor.numpy()):
        with pytest.raises(ValueError, match="floor must be"):
            spnerf_amd.gate_plane(grey, valid, bad, -20.0)
    for kw, text in ((dict(alt=float("nan")), "alt nan must be"), (dict(alt="0"), "alt '0' must be"), (dict(slack=-0.5), "slack -0.5 must be"),
                     (dict(slack=float("inf")), "slack inf must be"), (dict(slack=None), "slack None must be")):
        with pytest.raises(ValueError, match=text):
            spnerf_amd.gate_plane(grey, valid, floor, **{"alt": -20.0, **kw})
    with pytest.raises(ValueError, match="on one device"):
        spnerf_amd.gate_plane(grey, valid, floor.to("meta"), -20.0)
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        spnerf_amd.gate_plane(grey, valid, floor, -20.0, slack=0.5)

    def sweep(images=images, cams=cams, grid=grid, lo=-20.0, step=1.0, planes=9, floor=floor, slack=0.5, **kw):
        return spnerf_amd.visible_sweep(images, cams, grid, lo, step, planes, floor, slack=slack, **kw)

    with pytest.raises(TypeError, match="slack"):                        # no default: the caller chooses it
        spnerf_amd.visible_sweep(images, cams, grid, -20.0, 1.0, 9, floor)
    for bad, text in ((dict(cams=cams[:1], images=images[:1]), "1 views in one sweep"), (dict(grid=0.5), "grid must be a GroundGrid"),
                      (dict(images=images[:3]), "3 images for 4 views"), (dict(planes=0), "planes 0 must be"), (dict(step=0.0), "step 0.0 must be"),
                      (dict(lo=float("inf")), "alt_lo inf must be"), (dict(radius=5), "radius 5 must be"), (dict(min_views=5), "min_views 5 must be"),
                      (dict(min_std=-1e-3), "min_std -0.001 must be"), (dict(floor=floor[:3]), "floor must be a"),
                      (dict(floor=floor.double()), "floor must be a"), (dict(floor=torch.zeros(4, 15, 9)), r"floor must be a \(4, 9, 15\)"),
                      (dict(floor=None), "floor must be a"), (dict(slack=-1.0), "slack -1.0 must be"), (dict(slack=float("nan")), "slack nan must be"),
                      (dict(slack=True), "slack True must be")):
        with pytest.raises(ValueError, match=text):
            sweep(**bad)
    with pytest.raises(ValueError, match="on one device"):
        sweep(floor=floor.to("meta"))
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        sweep()
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        sweep(volume=True, radius=4, min_views=4, min_std=0.01, slack=0.0)

    def refine(images=images, cams=cams, grid=grid, lo=-20.0, step=1.0, planes=9, **kw):
        return spnerf_amd.refine_sweep(images, cams, grid, lo, step, planes, **kw)

    for bad, text in ((dict(planes=1), "planes 1 must be an integer in 2"), (dict(planes=4097), "planes 4097 must be"), (dict(step=-1), "step -1 must be"),
                      (dict(radius=0), "radius 0 must be"), (dict(slack=-0.5), "slack -0.5 must be"), (dict(p1=-1.0), "p1 -1.0 must be"),
                      (dict(p2=0.1), "p2 0.1 must be"), (dict(paths=5), "paths 5 must be 4 or 8"), (dict(volume=1), "volume 1 must be a bool"),
                      (dict(prior=dsm[:8]), "is not the grid's"), (dict(prior=dsm.int()), "prior must be"), (dict(prior=dsm.numpy()), "prior must be"),
                      (dict(cams=cams * 5, images=images * 5), "20 views in one sweep")):
        with pytest.raises(ValueError, match=text):
            refine(**bad)
    with pytest.raises(ValueError, match="on one device"):
        refine(prior=dsm.to("meta"))
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        refine()
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        refine(prior=dsm, slack=0.0, paths=4)
