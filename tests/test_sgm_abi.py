"""The semi-global aggregation C ABI (include/spnerf_amd_sgm.h, spnerf_amd._sgm_lib): the header, the
ctypes table and the built library agree, and argument errors come back as codes or are raised before
any device is used — no GPU needed."""
import ctypes

import pytest
import torch

import abi_util
import spnerf_amd
from abi_util import A as VOL, B as OUT, C as WORK, D as FOUR, refused
from spnerf_amd import _lib, _sgm_lib, rectify, sgm
from spnerf_amd.ortho import GroundGrid
from spnerf_amd.satellite import load_cameras

HEADER = abi_util.header_path("spnerf_amd_sgm.h")


def test_sgm_exports_match_the_header():
    names = abi_util.check_table(_sgm_lib, HEADER, "spnerf_sgm", {"int64_t*": ctypes.POINTER(ctypes.c_int64)})
    assert names == ["spnerf_sgm_abi_version", "spnerf_sgm_aggregate", "spnerf_sgm_pick", "spnerf_sgm_workspace_bytes"]
    assert all(_sgm_lib.SIGNATURES[n][0] is ctypes.c_int32 for n in names)
    txt = open(HEADER).read()
    consts = abi_util.defines(HEADER, "SPNERF_SGM_")
    assert consts["SPNERF_SGM_MAX_PLANES"] == _sgm_lib.SGM_MAX_PLANES == sgm.MAX_PLANES == 512
    assert consts["SPNERF_SGM_TILE"] == _sgm_lib.SGM_TILE == 64
    assert "There is no `views` output" in txt and "Occlusion is not modelled" in txt


SIZE_ERRORS = ((dict(K=0), b"n_planes 0 outside [1, 512]"), (dict(K=513), b"n_planes 513 outside [1, 512]"), (dict(H=0), b"grid of 15 x 0"),
               (dict(W=-1), b"grid of -1 x 9"), (dict(H=2 ** 31 - 1, W=2 ** 31 - 1), b"grid of 2147483647 x 2147483647 cells is too large"), (dict(paths=3), b"paths 3 must be 4 or 8"),
               (dict(paths=0), b"paths 0 must be"), (dict(paths=16), b"paths 16 must be"))


def test_c_argument_errors_are_reported():
    L = _sgm_lib.lib()
    n = ctypes.c_int64(-1)

    def size(K=9, H=9, W=15, paths=8, out=ctypes.byref(n)):
        return L.spnerf_sgm_workspace_bytes(K, H, W, paths, out)

    assert size() == 0 and n.value == 9 * 9 * 9 * 15 * 4 + 9 * 15
    assert size(paths=4) == 0 and n.value == 5 * 9 * 9 * 15 * 4 + 9 * 15
    assert size(K=512, H=65536, W=65536) == 0 and n.value == (9 * 512 * 4 + 1) << 32
    refused(L, size(out=None), b"sgm_workspace_bytes: NULL", "bytes")
    for kw, text in SIZE_ERRORS:
        refused(L, size(**kw), b"sgm_workspace_bytes: " + text, kw)

    need = 9 * 9 * 9 * 15 * 4 + 9 * 15

    def agg(vol=VOL, K=9, H=9, W=15, p1=0.125, p2=1.0, unscored=1.0, paths=8, out=OUT, work=WORK, nbytes=1 << 30):
        return L.spnerf_sgm_aggregate(vol, K, H, W, p1, p2, unscored, paths, out, work, nbytes, None)

    for kw in (dict(vol=None), dict(out=None), dict(work=None)):
        refused(L, agg(**kw), b"sgm: NULL", kw)
    for kw, text in SIZE_ERRORS:
        refused(L, agg(**kw), b"sgm: " + text, kw)
    nan, inf = float("nan"), float("inf")
    for kw, text in ((dict(p1=-0.5), b"p1 -0.5 must be"), (dict(p1=nan), b"p1 nan must be"), (dict(p1=inf, p2=inf), b"p1 inf must be"),
                     (dict(p1=0.5, p2=0.25), b"p2 0.25 must be finite and >= p1 0.5"), (dict(p2=nan), b"p2 nan must be"),
                     (dict(p2=inf), b"p2 inf must be"), (dict(unscored=nan), b"unscored nan"), (dict(unscored=-inf), b"unscored -inf"),
                     (dict(nbytes=need - 1), b"workspace of %d bytes, %d needed" % (need - 1, need)), (dict(nbytes=0), b"workspace of 0 bytes"),
                     (dict(paths=4, nbytes=5 * 9 * 9 * 15 * 4), b"workspace of 24300 bytes, 24435 needed"), (dict(work=ctypes.c_void_p((3 << 32) + 2)), b"workspace is not 4-byte aligned"),
                     (dict(out=VOL), b"out overlaps volume"), (dict(out=ctypes.c_void_p((1 << 32) + 9 * 9 * 15 * 4 - 4)), b"out overlaps volume"),
                     (dict(vol=ctypes.c_void_p((2 << 32) + 4)), b"out overlaps volume"), (dict(work=OUT), b"workspace overlaps"),
                     (dict(work=ctypes.c_void_p((1 << 32) - 16)), b"workspace overlaps")):
        refused(L, agg(**kw), b"sgm: " + text, kw)
    refused(L, agg(nbytes=need, out=ctypes.c_void_p((1 << 32) + 9 * 9 * 15 * 4), work=ctypes.c_void_p((1 << 32) - need - 2)), b"sgm: workspace is not 4-byte aligned", "adjacent")

    def pick(agg=VOL, vol=OUT, K=9, cells=7, lo=-20.0, step=1.0, alt=FOUR, score=FOUR, index=FOUR, photo=FOUR):
        return L.spnerf_sgm_pick(agg, vol, K, cells, lo, step, alt, score, index, photo, None)

    for kw in (dict(agg=None), dict(vol=None), dict(alt=None), dict(score=None), dict(index=None), dict(photo=None)):
        refused(L, pick(**kw), b"sgm_pick: NULL", kw)
    for kw, text in ((dict(K=0), b"n_planes 0 outside [1, 512]"), (dict(K=513), b"n_planes 513"), (dict(step=0.0), b"step 0 must be"),
                     (dict(step=nan), b"step"), (dict(lo=inf), b"alt_lo inf"), (dict(cells=0), b"cells 0"),
                     (dict(cells=2 ** 32 + 1), b"cells 4294967297")):
        refused(L, pick(**kw), b"sgm_pick: " + text, kw)


def test_python_argument_errors_come_before_any_device_use():
    assert spnerf_amd.smooth_sweep is sgm.smooth_sweep and spnerf_amd.sgm is sgm
    assert sgm.workspace_bytes(9, 9, 15) == 9 * 9 * 9 * 15 * 4 + 9 * 15 and sgm.workspace_bytes(9, 9, 15, 4) == 5 * 9 * 9 * 15 * 4 + 9 * 15
    assert 0 <= sgm.P1 <= sgm.P2
    volume = torch.zeros(9, 9, 15)
    for bad in (volume.double(), volume[0], volume[:, :0], volume.numpy(), torch.zeros(513, 1, 1)):
        with pytest.raises(ValueError, match="volume must be|planes 513 must be"):
            sgm.aggregate(bad, p1=0.125, p2=1.0)
    nan, inf = float("nan"), float("inf")
    penalties = ((dict(p1=-0.125), "p1 -0.125 must be finite and >= 0"), (dict(p1=nan), "p1 nan must be"), (dict(p1="1"), "p1 '1' must be"),
                 (dict(p1=0.5, p2=0.25), "p2 0.25 must be finite and >= p1 0.5"), (dict(p2=inf), "p2 inf must be"),
                 (dict(p2=1e39), "p2 1e\\+39 must be"), (dict(p2=True), "p2 True must be"), (dict(unscored=nan), "unscored nan must be finite"),
                 (dict(unscored=-1e39), "unscored -1e\\+39 must be"), (dict(paths=3), "paths 3 must be 4 or 8"),
                 (dict(paths=8.0), "paths 8.0 must be 4 or 8"), (dict(paths=True), "paths True must be"))
    for kw, text in penalties:
        with pytest.raises(ValueError, match=text):
            sgm.aggregate(volume, **{**dict(p1=0.125, p2=1.0), **kw})
    with pytest.raises(_lib.SpnerfError, match="MI355X"):                # only now the volume's device matters
        sgm.aggregate(volume, p1=0.125, p2=1.0)
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        sgm.aggregate(volume, p1=0.0, p2=0.0, unscored=-2.0, paths=4)
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        sgm.aggregate(volume)

    for bad in (volume.double(), volume[0], volume[:, :0], volume.numpy()):
        with pytest.raises(ValueError, match="aggregated must be"):
            sgm.pick(bad, volume, -20.0, 1.0)
    for bad in (volume.double(), volume[:3], volume[0], volume.numpy()):
        with pytest.raises(ValueError, match="volume must be a \\(9, 9, 15\\) float32"):
            sgm.pick(volume, bad, -20.0, 1.0)
    with pytest.raises(ValueError, match="planes 513 must be"):
        sgm.pick(torch.zeros(513, 1, 1), torch.zeros(513, 1, 1), -20.0, 1.0)
    with pytest.raises(ValueError, match="step 0 must be"):
        sgm.pick(volume, volume, -20.0, 0)
    with pytest.raises(ValueError, match="alt_lo inf must be"):
        sgm.pick(volume, volume, inf, 1.0)
    with pytest.raises(ValueError, match="on one device"):
        sgm.pick(volume, volume.to("meta"), -20.0, 1.0)
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        sgm.pick(volume, volume, -20.0, 1.0)

    metas = load_cameras()["images"]
    cams = [rectify.Camera.from_meta(m, 4) for m in metas.values()][:4]
    grid = GroundGrid(438638.0, 3353655.0, 15, 9, 0.5, 17)
    images = [torch.zeros(c.shape + (3,)) for c in cams]

    def call(images=images, cams=cams, grid=grid, lo=-20.0, step=1.0, planes=9, **kw):
        return spnerf_amd.smooth_sweep(images, cams, grid, lo, step, planes, **{**dict(p1=0.125, p2=1.0), **kw})

    for bad, text in ((dict(cams=cams[:1], images=images[:1]), "1 views in one sweep"), (dict(grid=0.5), "grid must be a GroundGrid"),
                      (dict(images=images[:3]), "3 images for 4 views"), (dict(planes=0), "planes 0 must be"),
                      (dict(planes=513), "planes 513 must be an integer in 1..512"), (dict(step=0.0), "step 0.0 must be"),
                      (dict(lo=inf), "alt_lo inf must be"), (dict(radius=5), "radius 5 must be"), (dict(min_views=5), "min_views 5 must be"),
                      (dict(min_std=-1e-3), "min_std -0.001 must be"), (dict(volume=1), "volume 1 must be a bool")) + penalties:
        with pytest.raises(ValueError, match=text):
            call(**bad)
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        call()
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        call(volume=True, paths=4, radius=4, min_views=4, min_std=0.01, unscored=0.5)
