"""The confidence C ABI (include/staged/spnerf_amd_confidence.h, spnerf_amd._confidence_abi): what
tests/test_abi_tables.py holds the tables of ``_lib.BINDING_MODULES`` to, for a table that is staged outside that
list; and argument errors come back as codes or are raised before any device is used — no GPU needed."""
import ctypes
import importlib

import pytest
import torch

import abi_util
import spnerf_amd
from abi_util import A, refused
from spnerf_amd import _clean_abi, _confidence_abi, _lib, clean, confidence, sgm
from spnerf_amd.ortho import GroundGrid
from spnerf_amd.satellite import load_cameras

HEADER = abi_util.header_path("staged/spnerf_amd_confidence.h")
OUTS = [ctypes.c_void_p(k << 32) for k in range(2, 11)]   # nine non-NULL pointers far apart, never dereferenced


def test_confidence_exports_match_the_header():
    assert abi_util.check_table(_confidence_abi, HEADER, "spnerf_conf") == ["spnerf_conf_abi_version", "spnerf_conf_volume"]
    consts = abi_util.defines(HEADER, "SPNERF_CONF_")
    assert consts["SPNERF_CONF_ABI_VERSION"] == _confidence_abi.SPNERF_CONF_ABI_VERSION == _confidence_abi.lib().spnerf_conf_abi_version() == 1
    assert consts["SPNERF_CONF_MAX_PLANES"] == _confidence_abi.CONF_MAX_PLANES == sgm.MAX_PLANES == 512
    assert consts["SPNERF_CONF_OUTPUTS"] == len(_confidence_abi.CONF_OUTPUTS) == len(OUTS)


def test_the_staged_table_is_disjoint_from_every_other_and_shares_the_handle():
    assert "_confidence_abi" not in _lib.BINDING_MODULES and "_confidence_lib" not in _lib.BINDING_MODULES
    assert _confidence_abi.lib() is _lib.lib()
    for mod in [_lib, _clean_abi] + [importlib.import_module("spnerf_amd." + m) for m in _lib.BINDING_MODULES]:
        assert not set(_confidence_abi.SIGNATURES) & set(mod.SIGNATURES), mod.__name__


def test_c_argument_errors_are_reported():
    L = _confidence_abi.lib()
    nan, inf = float("nan"), float("inf")

    def conf(volume=A, K=5, cells=9 * 15, alt_lo=-20.0, step=0.5, tau=0.05, temperature=0.1, exclude=1, outs=OUTS):
        return L.spnerf_conf_volume(volume, K, cells, alt_lo, step, tau, temperature, exclude, *outs, None)

    for kw, text in ((dict(volume=None), b"NULL volume"), (dict(K=0), b"n_planes 0 outside [1, 512]"), (dict(K=513), b"n_planes 513 outside [1, 512]"),
                     (dict(cells=0), b"cells 0 outside [1, 2^32]"), (dict(cells=2 ** 32 + 1), b"cells 4294967297 outside [1, 2^32]"),
                     (dict(alt_lo=nan), b"alt_lo nan is not finite"), (dict(step=0.0), b"step 0 must be finite and > 0"), (dict(step=inf), b"step inf must be"),
                     (dict(tau=-0.5), b"tau -0.5 must be finite and >= 0"), (dict(tau=nan), b"tau nan must be"), (dict(tau=inf), b"tau inf must be"),
                     (dict(temperature=0.0), b"temperature 0 must be finite and > 0"), (dict(temperature=nan), b"temperature nan must be"),
                     (dict(temperature=-1.0), b"temperature -1 must be"), (dict(temperature=inf), b"temperature inf must be"),
                     (dict(exclude=0), b"exclude 0 must be >= 1"), (dict(exclude=-3), b"exclude -3 must be >= 1"),
                     (dict(outs=[None] * 9), b"every output is NULL"),
                     (dict(outs=[None] * 4 + [A] + [None] * 4), b"an output overlaps volume"),
                     (dict(outs=[ctypes.c_void_p((1 << 32) + 5 * 9 * 15 * 4 - 4)] + [None] * 8), b"an output overlaps volume")):
        refused(L, conf(**kw), b"conf_volume: " + text, kw)


def test_python_argument_errors_come_before_any_device_use():
    for name in ("volume_confidence", "sparsification"):
        assert getattr(spnerf_amd, name) is getattr(confidence, name)
    assert spnerf_amd.confidence is confidence
    nan, inf = float("nan"), float("inf")
    vol = torch.zeros(5, 9, 15)

    def call(volume=vol, alt_lo=-20.0, step=0.5, **kw):
        return confidence.volume_confidence(volume, alt_lo, step, **kw)

    for bad, text in ((vol.double(), "volume must be a non-empty \\(K, H, W\\) float32"), (vol[0], "volume must be"), (vol[:, :0], "volume must be"),
                      (vol.numpy(), "volume must be"), (torch.zeros(513, 2, 2), "planes 513 must be an integer in 1..512"),
                      (torch.zeros(2, 2 ** 17, 2 ** 16, device="meta"), "a grid of 65536 x 131072 cells is too large")):
        with pytest.raises(ValueError, match=text):
            call(volume=bad)
    for kw, text in ((dict(alt_lo=nan), "alt_lo nan must be finite"), (dict(step=0.0), "step 0.0 must be finite and > 0"), (dict(step="1"), "step '1' must be"),
                     (dict(tau=-0.1), "tau -0.1 must be finite and >= 0"), (dict(tau=nan), "tau nan must be"), (dict(tau=1e39), "tau 1e\\+39 must be"),
                     (dict(tau=True), "tau True must be"), (dict(temperature=0.0), "temperature 0.0 must be finite and > 0"),
                     (dict(temperature=1e-50), "temperature 1e-50 must be"), (dict(temperature=inf), "temperature inf must be"),
                     (dict(temperature=1e39), "temperature 1e\\+39 must be"), (dict(exclude=0), "exclude 0 must be an integer in 1"),
                     (dict(exclude=1.0), "exclude 1.0 must be"), (dict(planes=[]), "planes \\[\\] must be None or a non-empty list of names among scored, index"),
                     (dict(planes="mlm"), "planes 'mlm' must be"), (dict(planes=["mlm", "photo"]), "planes \\['mlm', 'photo'\\] must be"),
                     (dict(planes=[0]), "planes \\[0\\] must be")):
        with pytest.raises(ValueError, match=text):
            call(**kw)
    with pytest.raises(_lib.SpnerfError, match="MI355X"):               # only now the volume's device matters
        call()
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        call(tau=0.0, temperature=0.02, exclude=7, planes=("index", "margin"))

    # smooth_sweep and bootstrap_sweep: the new arguments are checked with the others, before the device
    metas = load_cameras()["images"]
    cams = [spnerf_amd.rectify.Camera.from_meta(m, 4) for m in list(metas.values())[:2]]
    imgs = [torch.zeros(c.shape + (1,)) for c in cams]
    grid = GroundGrid(438638.0, 3353655.0, 15, 9, 0.5, 17)
    with pytest.raises(ValueError, match="confidence 1 must be a bool"):
        sgm.smooth_sweep(imgs, cams, grid, -20.0, 1.0, 5, confidence=1)
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        sgm.smooth_sweep(imgs, cams, grid, -20.0, 1.0, 5, confidence=True)
    assert clean.WEIGHTS == ("photo", "margin", "peak_margin", "curvature", "mlm")
    for bad in ("score", "spread", None, 0):
        with pytest.raises(ValueError, match="weight .* must be one of 'photo', 'margin', 'peak_margin', 'curvature', 'mlm'"):
            clean.bootstrap_sweep(imgs, cams, grid, -20.0, 1.0, 5, weight=bad)
    for name in clean.WEIGHTS:
        with pytest.raises(_lib.SpnerfError, match="MI355X"):
            clean.bootstrap_sweep(imgs, cams, grid, -20.0, 1.0, 5, weight=name, min_weight=0.1)
