"""The relighting C ABI (include/spnerf_amd_relight.h, spnerf_amd._relight_lib): the header, the
ctypes table and the built library agree, and argument errors come back as codes or are raised
before any device is used — no GPU needed."""
import ctypes
import re
import types

import numpy as np
import pytest
import torch

import abi_util
import spnerf_amd
from abi_util import ONE
from spnerf_amd import _lib, _relight_lib

HEADER = abi_util.header_path("spnerf_amd_relight.h")


def cfg(width=64, dtype=1):
    c = _lib.ModelCfg()
    c.width, c.layers, c.skip, c.n_freq, c.dtype = width, 8, 4, 10, dtype
    return ctypes.byref(c)


def test_relight_exports_match_the_header():
    assert abi_util.check_table(_relight_lib, HEADER, "spnerf_") == [
        "spnerf_relight_abi_version", "spnerf_relight_composite", "spnerf_relight_directions", "spnerf_relight_sun",
        "spnerf_relight_workspace_bytes"]
    # the new MLP flag is the header's
    main = open(abi_util.header_path("spnerf_amd.h")).read()
    assert int(re.search(r"#define SPNERF_MLP_KEEP_FEAT (\d+)\b", main).group(1)) == _lib.SPNERF_MLP_KEEP_FEAT == 32


def test_workspace_bytes_and_unsupported_widths():
    L = _relight_lib.lib()
    wsb = L.spnerf_relight_workspace_bytes
    assert wsb(cfg(64), 1) == 16 + 32 * 4 and wsb(cfg(256), 5) == 5 * (16 + 128 * 4)
    assert wsb(cfg(256, 0), 16) == 16 * (16 + 128 * 4)       # the fp32 model alike
    assert all(wsb(cfg(w), k) % 16 == 0 for w in (64, 128, 192, 256) for k in (1, 3, 16))
    for w in (512, 320, 384):
        assert wsb(cfg(w), 4) == -3 and b"width" in L.spnerf_last_error(), w     # SPNERF_E_UNSUPPORTED
    assert wsb(cfg(64), 0) == -1 and b"n_dirs 0" in L.spnerf_last_error()
    assert wsb(None, 1) == -1


def test_launch_argument_errors_are_reported():
    L = _relight_lib.lib()
    assert L.spnerf_relight_directions(cfg(), ONE, None, 2, ONE, None) == -1 and b"NULL" in L.spnerf_last_error()
    assert L.spnerf_relight_directions(cfg(), ONE, ONE, 0, ONE, None) == -1 and b"n_dirs 0" in L.spnerf_last_error()
    assert L.spnerf_relight_directions(cfg(), ONE, ONE, 2, ctypes.c_void_p(264), None) == -1
    assert b"not 16-byte aligned" in L.spnerf_last_error()
    assert L.spnerf_relight_directions(cfg(512), ONE, ONE, 2, ONE, None) == -3

    def sun(c=None, packed=ONE, ws=ONE, n=4, S=8, dws=ONE, K=2, sv=ONE):
        return L.spnerf_relight_sun(c or cfg(), packed, ws, n, S, dws, K, sv, None)

    for kw, text in ((dict(packed=None), b"NULL"), (dict(ws=None), b"NULL"), (dict(sv=None), b"NULL"), (dict(dws=None), b"NULL"),
                     (dict(n=-1), b"bad sizes"), (dict(S=0), b"bad sizes"), (dict(K=0), b"n_dirs 0"),
                     (dict(dws=ctypes.c_void_p(264)), b"not 16-byte aligned"), (dict(n=1 << 40), b"too many points")):
        assert sun(**kw) == -1, kw
        assert text in L.spnerf_last_error(), (kw, L.spnerf_last_error())
    assert sun(c=cfg(512)) == -3
    assert sun(n=0) == 0                                    # nothing to do, nothing launched

    def comp(n=4, S=48, z=ONE, out=ONE, NO=8, K=2, sv=ONE, dws=ONE, begin=0, rays=4):
        return L.spnerf_relight_composite(n, S, z, out, NO, None, 0.0, None, K, sv, dws, begin, rays, ONE, ONE, ONE, None)

    for kw, text in ((dict(z=None), b"NULL z or out"), (dict(out=None), b"NULL z or out"), (dict(sv=None), b"NULL sun_v"),
                     (dict(dws=None), b"NULL sun_v"), (dict(n=-1), b"n_rays -1"), (dict(S=0), b"n_samples 0"),
                     (dict(S=257), b"n_samples 257"), (dict(NO=7), b"n_out 7"), (dict(S=256, NO=40), b"too large"),
                     (dict(K=0), b"n_dirs 0"), (dict(begin=-1), b"outside a plane"), (dict(begin=1), b"outside a plane"),
                     (dict(rays=3), b"outside a plane")):
        assert comp(**kw) == -1, kw
        assert text in L.spnerf_last_error(), (kw, L.spnerf_last_error())
    assert comp(n=0, rays=0) == 0


def test_keep_feat_goes_with_a_whole_inference_forward():
    L = _lib.lib()
    for flags in (32 | 1, 32 | 2, 32 | 4):
        assert L.spnerf_mlp_forward(cfg(), ONE, ONE, 11, 3, 4, 8, ONE, None, None, flags, ONE, ONE, None) == -1, flags
        assert b"SPNERF_MLP_KEEP_FEAT" in L.spnerf_last_error()


def test_relight_image_argument_errors_come_before_any_device_use():
    assert spnerf_amd.relight_image is spnerf_amd.relight.relight_image
    model = spnerf_amd.SPNeRF(feat=64, mapping=True)
    args = types.SimpleNamespace(model="sp-nerf", n_samples=8, n_importance=0, guidedsample=False, beta=False,
                                 sc_lambda=0.0, noise_std=0.0)
    rays, good = torch.zeros(4, 11), torch.tensor([[0.0, 0.6, 0.8]])

    def call(dirs=good, **kw):
        return spnerf_amd.relight_image({"coarse": model}, args, rays, dirs, **kw)

    with pytest.raises(ValueError, match="sc product"):
        call(products=("rgb", "sc"))
    with pytest.raises(ValueError, match="unknown products"):
        call(products=("rgb", "shadow"))
    for bad in (torch.zeros(3), torch.zeros(2, 4), np.zeros((2, 3, 1), np.float32)):
        with pytest.raises(ValueError, match=r"must be \(K, 3\)"):
            call(bad)
    with pytest.raises(ValueError, match="K = 0"):
        call(torch.zeros(0, 3))
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="non-finite"):
            call(torch.tensor([[0.0, 1.0, 0.0], [0.0, bad, 0.0]]))
    with pytest.raises(ValueError, match="n_importance > 0"):
        call(products=("rgb", "rgb_coarse"))
    with pytest.raises(_lib.SpnerfError, match="MI355X"):   # only now the tensors' device matters
        call()
    args.model = "nerf"
    with pytest.raises(ValueError, match="not valid"):
        call()
