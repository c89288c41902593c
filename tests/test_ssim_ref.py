"""SSIM — CPU only.  The numpy restatement (tests/ssim_numpy.py) against a second, independently
written form and the closed form for constant images, and the image interface of the library
(include/spnerf_amd_image.h) without a compute call."""
import ctypes
import os
import re

import numpy as np
import pytest

import ssim_numpy as sn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spnerf_amd_image.h")


def mirror(i, n):
    """torch's 'reflect' index: mirrored about the first / last value, which is not repeated."""
    if i < 0:
        i = -i
    if i >= n:
        i = 2 * (n - 1) - i
    assert 0 <= i < n
    return i


def ssim_map_loops(x, y, ws, max_val=1.0):
    """The definition written out: for every output value a gather of the ws x ws neighbourhood
    through the mirrored index, weighted by the 2-D window outer(g, g)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    C, H, W = x.shape
    r = ws // 2
    g = [np.exp(-((i - r) ** 2) / (2 * 1.5 ** 2)) for i in range(ws)]
    total = sum(g)
    win = [[(a / total) * (b / total) for b in g] for a in g]
    c1, c2 = (0.01 * max_val) ** 2, (0.03 * max_val) ** 2
    out = np.empty((C, H, W))
    for c in range(C):
        for i in range(H):
            for j in range(W):
                m = [0.0] * 5
                for di in range(ws):
                    for dj in range(ws):
                        u = x[c, mirror(i + di - r, H), mirror(j + dj - r, W)]
                        v = y[c, mirror(i + di - r, H), mirror(j + dj - r, W)]
                        w = win[di][dj]
                        for q, t in enumerate((u, v, u * u, v * v, u * v)):
                            m[q] += w * t
                mu1, mu2 = m[0], m[1]
                s1, s2, s12 = m[2] - mu1 * mu1, m[3] - mu2 * mu2, m[4] - mu1 * mu2
                out[c, i, j] = ((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s1 + s2 + c2) + 1e-12)
    return out


@pytest.mark.parametrize("C,H,W,ws", [(1, 2, 2, 3), (3, 6, 6, 11), (1, 3, 17, 3), (3, 9, 7, 5), (2, 8, 13, 7), (1, 12, 10, 9)])
def test_restatement_matches_the_written_out_definition(C, H, W, ws):
    g = np.random.default_rng(C * 1000 + H * 100 + W + ws)
    x = g.uniform(0, 1, (C, H, W)).astype(np.float32)
    y = np.clip(x + 0.1 * g.standard_normal((C, H, W)), 0, 1).astype(np.float32)
    ref = ssim_map_loops(x, y, ws)
    got = sn.ssim_map(x, y, ws)
    err = float(np.abs(got - ref).max())
    print(f"({C},{H},{W}) ws {ws}: map max diff {err:.2e}, mean diff {abs(sn.ssim(x, y, ws) - ref.mean()):.2e}")
    assert err <= 1e-12
    assert abs(sn.ssim(x, y, ws) - float(ref.mean())) <= 1e-12
    with pytest.raises(ValueError):
        sn.ssim_map(x[:, :ws // 2], y[:, :ws // 2], ws)        # torch's reflect refuses these too


@pytest.mark.parametrize("ws", [3, 5, 7, 9, 11])
@pytest.mark.parametrize("a,b,max_val", [(0.5, 0.5, 1.0), (0.25, 0.75, 1.0), (0.0, 1.0, 1.0), (0.0, 0.0, 1.0), (40.0, 200.0, 255.0)])
def test_constant_images_have_the_closed_form(a, b, max_val, ws):
    c1, c2 = (0.01 * max_val) ** 2, (0.03 * max_val) ** 2
    want = (2 * a * b + c1) * c2 / ((a * a + b * b + c1) * c2 + 1e-12)
    x, y = np.full((2, 7, 9), a, np.float32), np.full((2, 7, 9), b, np.float32)
    m = sn.ssim_map(x, y, ws, max_val)
    assert float(np.abs(m - want).max()) <= 1e-12, (float(np.abs(m - want).max()), want)
    assert abs(sn.ssim(x, y, ws, max_val) - want) <= 1e-12


def test_layouts_of_a_flat_buffer():
    flat = np.arange(2 * 3 * 3, dtype=np.float32).reshape(6, 3)          # (H * W, C) with H, W = 2, 3
    hwc, chw = sn.chw_of(flat, (2, 3), "hwc"), sn.chw_of(flat, (2, 3), "chw")
    assert hwc.shape == chw.shape == (3, 2, 3)
    assert hwc[1, 0, 2] == flat[2, 1] and chw[1, 0, 2] == flat.ravel()[1 * 6 + 2]


def image_header_symbols():
    txt = open(HEADER).read()
    return sorted(set(re.findall(r"\b(spnerf_image_[a-z0-9_]+)\s*\(", txt)))


def test_image_exports_match_the_header():
    from spnerf_amd import _eval_lib, _image_lib, _lib, _view_lib
    syms = image_header_symbols()
    assert syms == ["spnerf_image_abi_version", "spnerf_image_ssim", "spnerf_image_ssim_workspace_bytes"]
    L = _image_lib.lib()
    assert L is _lib.lib()                                  # one library, four signature tables
    for s in syms:
        assert hasattr(L, s), s
    assert sorted(_image_lib.SIGNATURES) == syms, "image signature table out of sync with the header"
    for other in (_lib, _eval_lib, _view_lib):
        assert not set(_image_lib.SIGNATURES) & set(other.SIGNATURES)
    hdr = open(HEADER).read()
    consts = {k: int(v) for k, v in re.findall(r"#define (SPNERF_IMAGE_[A-Z_]+) (\d+)\b", hdr)}
    assert L.spnerf_image_abi_version() == consts["SPNERF_IMAGE_ABI_VERSION"] == _image_lib.SPNERF_IMAGE_ABI_VERSION == 1
    assert consts["SPNERF_IMAGE_MAX_CHANNELS"] == _image_lib.IMAGE_MAX_CHANNELS == 4
    assert consts["SPNERF_IMAGE_MAX_WINDOW"] == _image_lib.IMAGE_MAX_WINDOW == 11
    assert ctypes.sizeof(_image_lib.SsimResult) == 48
    assert L.spnerf_abi_version() == 2                      # the three older ABIs are untouched
    _eval_lib.lib()
    _view_lib.lib()
    assert L.spnerf_eval_abi_version() == 1 and L.spnerf_view_abi_version() == 1


def test_image_argument_errors_are_reported():
    from spnerf_amd import _image_lib
    L = _image_lib.lib()
    one = ctypes.c_void_p(256)      # never dereferenced: the arguments are refused first

    def ssim(x=one, y=one, C=3, H=12, W=10, cs=120, rs=10, ps=1, ws=3, wsp=one, res=one, mp=None):
        return L.spnerf_image_ssim(x, y, C, H, W, cs, rs, ps, ws, 1.0, wsp, mp, res, None)

    for kw, text in ((dict(x=None), b"NULL image"), (dict(y=None), b"NULL image"), (dict(wsp=None), b"NULL workspace or result"),
                     (dict(res=None), b"NULL workspace or result"), (dict(ws=4), b"window size 4"), (dict(ws=1), b"window size 1"),
                     (dict(ws=13), b"window size 13"), (dict(ws=-3), b"window size -3"), (dict(C=0), b"0 channels"),
                     (dict(C=5), b"5 channels"), (dict(H=-1), b"is negative"), (dict(W=-4), b"is negative"),
                     (dict(H=1), b"too small"), (dict(W=5, ws=11), b"too small"), (dict(H=0), b"too small"),
                     (dict(cs=-1), b"negative stride"), (dict(rs=-10), b"negative stride"), (dict(ps=-1), b"negative stride"),
                     (dict(H=1 << 21), b"larger than"), (dict(wsp=ctypes.c_void_p(264)), b"not 16-byte aligned"),
                     (dict(res=ctypes.c_void_p(260)), b"not 8-byte aligned"), (dict(mp=ctypes.c_void_p(260)), b"not 8-byte aligned")):
        assert ssim(**kw) == -1, kw
        assert text in L.spnerf_last_error(), (kw, L.spnerf_last_error())
    wsb = L.spnerf_image_ssim_workspace_bytes
    assert wsb(3, 12, 10, 4) == -1 and wsb(0, 12, 10, 3) == -1 and wsb(5, 12, 10, 3) == -1 and wsb(3, 1, 10, 3) == -1
    assert wsb(3, 5, 10, 11) == -1 and b"too small" in L.spnerf_last_error()
    assert wsb(3, -1, 10, 3) == -1 and b"is negative" in L.spnerf_last_error()
    # one double per 16 x 32 tile per channel, a fixed function of the image's size
    assert wsb(1, 2, 2, 3) == 16 and wsb(3, 16, 32, 3) == 32 and wsb(3, 17, 33, 3) == 96
    assert wsb(3, 1024, 1024, 3) == wsb(3, 1024, 1024, 11) == 3 * 64 * 32 * 8
    assert all(wsb(c, h, w, 3) % 16 == 0 for c in (1, 2, 3, 4) for h in (2, 17, 65) for w in (2, 33, 70))


def test_python_surface_refuses_cpu_tensors_and_bad_arguments():
    import torch
    import spnerf_amd
    from spnerf_amd import _lib, losses
    assert spnerf_amd.ssim is spnerf_amd.image.ssim is losses.ssim
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        spnerf_amd.ssim(torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 8))
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        spnerf_amd.view_metrics(torch.zeros(120, 3), torch.zeros(120, 3), hw=(12, 10))
