"""The geometric-shadow C ABI (include/spnerf_amd_shadow.h, spnerf_amd._shadow_lib): the header, the
ctypes table and the built library agree, and argument errors come back as codes or are raised before
any device is used — no GPU needed."""
import ctypes
import re
import types

import numpy as np
import pytest
import torch

import abi_util
import spnerf_amd
from abi_util import ONE
from spnerf_amd import _lib, _shadow_lib
from spnerf_amd.ortho import GroundGrid

HEADER = abi_util.header_path("spnerf_amd_shadow.h")
TWO = ctypes.c_void_p(512)   # like ONE, a non-NULL, 16-byte aligned pointer that is never dereferenced


def dirs_of(*rows):
    return (ctypes.c_float * (3 * len(rows)))(*[v for r in rows for v in r])


def test_shadow_exports_match_the_header():
    # `dirs` is a host pointer to floats
    assert abi_util.check_table(_shadow_lib, HEADER, "spnerf_", {("spnerf_shadow_cast", 4): ctypes.POINTER(ctypes.c_float)}) == [
        "spnerf_shadow_abi_version", "spnerf_shadow_agreement", "spnerf_shadow_agreement_workspace_bytes", "spnerf_shadow_cast",
        "spnerf_shadow_workspace_bytes"]
    txt = open(HEADER).read()
    consts = abi_util.defines(HEADER, "SPNERF_SHADOW_")
    assert consts["SPNERF_SHADOW_MAX_DIRS"] == _shadow_lib.SHADOW_MAX_DIRS == 65535
    # the struct of the header, field for field
    body = re.search(r"typedef struct spnerf_shadow_agreement_result \{(.*?)\} spnerf_shadow_agreement_result;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n for decl in re.findall(r"(?:double|int64_t)\s+([^;]+);", body) for n in re.split(r",\s*", decl)]
    assert fields == [f for f, _ in _shadow_lib.ShadowAgreementResult._fields_]
    assert ctypes.sizeof(_shadow_lib.ShadowAgreementResult) == _shadow_lib.RESULT_BYTES == 8 * 8


def test_workspace_sizes():
    L = _shadow_lib.lib()
    # one partial maximum per workgroup of 1024 cells, at most 256 of them, 16-byte granules
    assert L.spnerf_shadow_workspace_bytes(1, 1) == 16 and L.spnerf_shadow_workspace_bytes(33, 65) == 32
    assert L.spnerf_shadow_workspace_bytes(130, 257) == 33 * 8 + 8 and L.spnerf_shadow_workspace_bytes(512, 512) == 256 * 8
    assert L.spnerf_shadow_workspace_bytes(4096, 4096) == 256 * 8
    for h, w, text in ((0, 5, b"grid of 5 x 0"), (5, -1, b"grid of -1 x 5"), (2 ** 31 - 1, 2 ** 31 - 1, b"too large")):
        assert L.spnerf_shadow_workspace_bytes(h, w) == -1 and text in L.spnerf_last_error()
    # one 64-byte partial per workgroup of 256 cells and direction, at most 256 workgroups per direction
    assert L.spnerf_shadow_agreement_workspace_bytes(1, 1) == 64 and L.spnerf_shadow_agreement_workspace_bytes(257, 3) == 2 * 3 * 64
    assert L.spnerf_shadow_agreement_workspace_bytes(512 * 512, 16) == 256 * 16 * 64
    for cells, k, text in ((0, 1, b"cells 0"), (5, 0, b"n_dirs 0"), (5, 65536, b"n_dirs 65536")):
        assert L.spnerf_shadow_agreement_workspace_bytes(cells, k) == -1 and text in L.spnerf_last_error()


def test_cast_argument_errors_are_reported():
    L = _shadow_lib.lib()
    good = dirs_of((0.5, 0.5, 0.7), (0.0, 0.0, 1.0))

    def cast(dsm=ONE, h=9, w=15, res=0.5, dirs=good, k=2, ws=ONE, shadow=TWO, excess=None):
        return L.spnerf_shadow_cast(dsm, h, w, res, dirs, k, ws, shadow, excess, None)

    for kw, text in ((dict(dsm=None), b"NULL"), (dict(dirs=None), b"NULL"), (dict(ws=None), b"NULL"), (dict(shadow=None), b"NULL"),
                     (dict(h=0), b"grid of 15 x 0"), (dict(h=-3), b"grid of 15 x -3"), (dict(w=0), b"grid of 0 x 9"),
                     (dict(w=-1), b"grid of -1 x 9"), (dict(h=2 ** 31 - 1, w=2 ** 31 - 1), b"too large"),
                     (dict(k=0), b"n_dirs 0"), (dict(k=-1), b"n_dirs -1"), (dict(k=65536), b"n_dirs 65536"),
                     (dict(res=0.0), b"resolution 0"), (dict(res=-0.5), b"resolution -0.5"), (dict(res=float("nan")), b"resolution"),
                     (dict(res=float("inf")), b"resolution"),
                     (dict(ws=ctypes.c_void_p(264)), b"16-byte aligned"),
                     (dict(dirs=dirs_of((0.5, 0.5, 0.7), (0.6, 0.8, 0.0))), b"direction 1 has up 0"),
                     (dict(dirs=dirs_of((0.5, 0.5, -0.25), (0.0, 0.0, 1.0))), b"direction 0 has up -0.25"),
                     (dict(dirs=dirs_of((0.5, 0.5, 0.7), (float("nan"), 0.0, 1.0))), b"direction 1 is not finite"),
                     (dict(dirs=dirs_of((0.5, float("inf"), 0.7), (0.0, 0.0, 1.0))), b"direction 0 is not finite"),
                     (dict(dirs=dirs_of((0.5, 0.5, float("nan")), (0.0, 0.0, 1.0))), b"direction 0 is not finite")):
        assert cast(**kw) == _lib.SPNERF_E_ARG == -1, kw
        assert text in L.spnerf_last_error(), (kw, L.spnerf_last_error())
    assert cast(dirs=dirs_of((0.6, 0.8, 0.0)), k=1) == -1 and b"above the horizon" in L.spnerf_last_error()


def test_agreement_argument_errors_are_reported():
    L = _shadow_lib.lib()

    def agree(sun=ONE, shadow=TWO, cells=7, k=2, ws=ONE, res=TWO):
        return L.spnerf_shadow_agreement(sun, shadow, cells, k, ws, res, None)

    for kw, text in ((dict(sun=None), b"NULL"), (dict(shadow=None), b"NULL"), (dict(ws=None), b"NULL"), (dict(res=None), b"NULL"),
                     (dict(cells=0), b"cells 0"), (dict(cells=-4), b"cells -4"), (dict(k=0), b"n_dirs 0"), (dict(k=65536), b"n_dirs 65536"),
                     (dict(cells=2 ** 40), b"in one call"), (dict(ws=ctypes.c_void_p(264)), b"16-byte aligned")):
        assert agree(**kw) == -1, kw
        assert text in L.spnerf_last_error(), (kw, L.spnerf_last_error())


def test_python_argument_errors_come_before_any_device_use():
    assert spnerf_amd.cast_shadows is spnerf_amd.shadow.cast_shadows
    assert spnerf_amd.shadow_agreement is spnerf_amd.shadow.shadow_agreement
    dsm = torch.zeros(9, 15, dtype=torch.float64)
    good = np.array([[0.5, 0.5, 0.7]], np.float32)
    cast = spnerf_amd.cast_shadows
    for bad in (np.zeros((9, 15)), torch.zeros(9), torch.zeros(2, 9, 15), torch.zeros(0, 15), torch.zeros(9, 15, dtype=torch.int32),
                torch.zeros(9, 15, dtype=torch.float16)):
        with pytest.raises(ValueError, match="dsm must be"):
            cast(bad, 0.5, good)
    for bad in (0.0, -0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="resolution .* must be positive"):
            cast(dsm, bad, good)
    for bad in ("0.5", None, True, (0.5,)):
        with pytest.raises(ValueError, match="GroundGrid or the cell size"):
            cast(dsm, bad, good)
    with pytest.raises(ValueError, match="is not the grid's"):
        cast(dsm, GroundGrid(438638.0, 3353655.0, 9, 15, 0.5, 17), good)      # 15 rows of 9 cells, not 9 of 15
    for bad in (np.zeros(3), np.zeros((2, 4)), np.zeros((0, 3)), np.zeros((0, 2)), torch.zeros(2, 3, 1)):
        with pytest.raises(ValueError, match=r"\(K, 3\)|K = 0"):
            cast(dsm, 0.5, bad)
    with pytest.raises(ValueError, match="non-finite"):
        cast(dsm, 0.5, np.array([[0.5, float("nan"), 0.7]]))
    with pytest.raises(ValueError, match="non-finite"):
        cast(dsm, 0.5, np.array([[float("inf"), 140.0]]))
    for bad, k in (([[0.5, 0.5, 0.7], [0.6, 0.8, 0.0]], 1), ([[0.6, 0.8, -0.1]], 0), ([[30.0, 90.0], [-5.0, 90.0]], 1), ([[0.0, 10.0]], 0)):
        with pytest.raises(ValueError, match=rf"sun_dirs\[{k}\] has up"):
            cast(dsm, 0.5, np.array(bad))
    with pytest.raises(_lib.SpnerfError, match="MI355X"):          # only now the DSM's device matters
        cast(dsm, 0.5, good)
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        cast(dsm.float(), GroundGrid(438638.0, 3353655.0, 15, 9, 0.5, 17), np.array([[30.0, 90.0], [60.0, 200.0]]), excess=True)
    # (elevation, azimuth) pairs are satellite.sun_direction's vectors
    d = spnerf_amd.shadow.sun_directions(np.array([[30.0, 90.0], [60.0, 200.0]]))
    want = np.stack([spnerf_amd.satellite.sun_direction(30.0, 90.0), spnerf_amd.satellite.sun_direction(60.0, 200.0)]).astype(np.float32)
    assert d.dtype == torch.float32 and np.array_equal(d.numpy(), want)
    assert np.array_equal(spnerf_amd.shadow.sun_directions(torch.tensor(want)).numpy(), want)

    agree = spnerf_amd.shadow_agreement
    sun, sh = torch.zeros(2, 3, 4), torch.zeros(2, 3, 4, dtype=torch.uint8)
    for a, b, text in ((sun[0], sh, "sun must be"), (sun.double(), sh, "sun must be"), (sun, sh.int(), "shadow must be"),
                       (sun, sh[0], "shadow must be"), (sun[:, :0], sh[:, :0], "sun must be"), (sun.numpy(), sh, "sun must be"),
                       (sun, sh[:1], "same shape")):
        with pytest.raises(ValueError, match=text):
            agree(a, b)
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        agree(sun, sh)


def test_relight_ortho_cast_argument_errors():
    model = spnerf_amd.SPNeRF(feat=64, mapping=True)
    args = types.SimpleNamespace(model="sp-nerf", n_samples=8, n_importance=0, guidedsample=False, beta=False,
                                 sc_lambda=0.0, noise_std=0.0)
    g = GroundGrid(438638.996411, 3353655.999928, 5, 3, 0.5, 17)
    center, rng = np.array([801532.84375, -5452266.5, 3200266.875], np.float32), 141.21875

    def relight(dirs=torch.tensor([[0.0, 0.6, 0.8]]), **kw):
        return spnerf_amd.relight_ortho({"coarse": model}, args, g, -30.0, -2.0, center, rng, dirs, **kw)

    with pytest.raises(ValueError, match='needs "depth"'):
        relight(cast=True)
    with pytest.raises(ValueError, match='needs "depth"'):
        relight(cast=True, products=("rgb", "sun"))
    with pytest.raises(ValueError, match="needs the whole grid"):
        relight(cast=True, products=("sun", "depth"), rows=(0, 2))
    with pytest.raises(ValueError, match=r"sun_dirs\[1\] has up"):
        relight(cast=True, products=("sun", "depth"), dirs=torch.tensor([[0.0, 0.6, 0.8], [0.6, 0.8, 0.0]]))
    with pytest.raises(ValueError, match="rows"):                  # the checks of the call without cast= come first
        relight(cast=True, products=("sun", "depth"), rows=(0, 4))
    with pytest.raises(_lib.SpnerfError, match="MI355X"):          # only now the model's device matters
        relight(cast=True, products=("sun", "depth"))
    with pytest.raises(_lib.SpnerfError, match="MI355X"):          # without cast= a sun below the horizon is the network's business
        relight(products=("sun", "depth"), dirs=torch.tensor([[0.0, 0.6, 0.8], [0.6, 0.8, 0.0]]), rows=(0, 2))
