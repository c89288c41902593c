"""The validation-loss C ABI (include/spnerf_amd_val.h, spnerf_amd._val_lib): the header, the ctypes
table and the built library agree, and argument errors come back as codes — no GPU needed."""
import ctypes
import re

import pytest

import abi_util
from abi_util import ONE
from spnerf_amd import _lib, _val_lib

HEADER = abi_util.header_path("spnerf_amd_val.h")


def test_val_exports_match_the_header():
    assert abi_util.check_table(_val_lib, HEADER, "spnerf_") == [
        "spnerf_val_abi_version", "spnerf_val_loss", "spnerf_val_loss_workspace_bytes", "spnerf_val_solar_terms"]


def test_val_result_layout_matches_the_header():
    hdr = open(HEADER).read()
    body = re.search(r"typedef struct spnerf_val_loss_result \{(.*?)\} spnerf_val_loss_result;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = [m.strip() for decl in body.split(";") if decl.strip() for m in re.sub(r"^\s*double", "", decl.strip()).split(",")]
    assert members == [f for f, _ in _val_lib.ValLossResult._fields_]
    assert ctypes.sizeof(_val_lib.ValLossResult) == _val_lib.RESULT_BYTES == 7 * 8


def test_solar_terms_argument_errors_are_reported():
    L = _val_lib.lib()

    def solar(n=4, S=48, z=ONE, out=ONE, stride=8, sun_col=4, begin=0, t2=ONE, t3=ONE):
        return L.spnerf_val_solar_terms(n, S, z, out, stride, sun_col, None, 0.0, begin, t2, t3, None, None)

    for kw, text in ((dict(z=None), b"NULL z or out"), (dict(out=None), b"NULL z or out"),
                     (dict(t2=None), b"NULL term2 or term3"), (dict(t3=None), b"NULL term2 or term3"),
                     (dict(S=0), b"n_samples 0"), (dict(S=257), b"n_samples 257"), (dict(n=-1), b"n_rays -1"),
                     (dict(sun_col=-1), b"sun_col -1 outside the row"), (dict(stride=3, sun_col=2), b"outside the row"),
                     (dict(sun_col=8), b"out_stride 8 is below sun_col + 1 = 9"), (dict(stride=4), b"out_stride 4 is below"),
                     (dict(S=256, stride=40), b"too large"), (dict(begin=-1), b"ray_begin -1")):
        assert solar(**kw) == -1, kw
        assert text in L.spnerf_last_error(), (kw, L.spnerf_last_error())
    assert solar(n=0) == 0                                  # nothing to do, nothing launched


def test_val_loss_argument_errors_are_reported():
    L = _val_lib.lib()

    def loss(n=100, rgb=ONE, tgt=ONE, coarse=None, beta=None, t2=None, t3=None, lam=0.1, bmin=0.05, ws=ONE, res=ONE):
        return L.spnerf_val_loss(n, rgb, tgt, coarse, beta, t2, t3, lam, bmin, ws, res, None)

    for kw, text in ((dict(rgb=None), b"val_loss: NULL"), (dict(tgt=None), b"val_loss: NULL"), (dict(ws=None), b"val_loss: NULL"),
                     (dict(res=None), b"val_loss: NULL"), (dict(n=0), b"n_rays 0"),
                     (dict(ws=ctypes.c_void_p(264)), b"not 16-byte aligned"), (dict(t2=ONE), b"go together"),
                     (dict(t3=ONE), b"go together"), (dict(beta=ONE, coarse=ONE), b"beta with rgb_coarse"),
                     (dict(beta=ONE, bmin=0.0), b"beta_min 0 must be positive")):
        assert loss(**kw) == -1, kw
        assert text in L.spnerf_last_error(), (kw, L.spnerf_last_error())
    wsb = L.spnerf_val_loss_workspace_bytes
    assert wsb(0) == -1 and b"n_rays 0" in L.spnerf_last_error()
    # six doubles per workgroup of 256 rays, a fixed function of the view's size; the grid is capped
    assert wsb(1) == wsb(256) == 48 and wsb(257) == 96
    assert 0 < wsb(70001) < wsb(1 << 24) == wsb(1 << 30) == 1024 * 48
    assert all(wsb(n) % 16 == 0 for n in (1, 255, 300, 70001))


def test_python_surface_refuses_cpu_tensors_and_bad_arguments():
    import types
    import torch
    import spnerf_amd
    assert spnerf_amd.view_loss is spnerf_amd.view.view_loss
    assert "sc" in spnerf_amd.view.PRODUCTS and "rgb_coarse" in spnerf_amd.view.PRODUCTS
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        spnerf_amd.view_loss({"rgb": torch.zeros(4, 3)}, torch.zeros(4, 3), 0.0)
    model = spnerf_amd.SPNeRF(feat=64, mapping=True)
    args = types.SimpleNamespace(model="sp-nerf", n_samples=8, n_importance=0, guidedsample=False, beta=False,
                                 sc_lambda=0.0, noise_std=0.0)
    with pytest.raises(ValueError, match="sc_lambda > 0"):
        spnerf_amd.render_image({"coarse": model}, args, torch.zeros(4, 11), products=("rgb", "sc"))
    with pytest.raises(ValueError, match="n_importance > 0"):
        spnerf_amd.render_image({"coarse": model}, args, torch.zeros(4, 11), products=("rgb", "rgb_coarse"))
    args.sc_lambda, args.n_importance = 0.1, 8
    with pytest.raises(ValueError, match="KeyError"):
        spnerf_amd.render_image({"coarse": model, "fine": model}, args, torch.zeros(4, 11), products=("rgb", "sc"))
