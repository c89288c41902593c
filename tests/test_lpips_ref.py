"""LPIPS — CPU only.  The fp64 restatement's shapes and sanity (tests/lpips_torch.py), the weight
naming of ``LpipsWeights`` and the LPIPS interface of the library (include/spnerf_amd_lpips.h)
without a compute call."""
import ctypes
import os
import re

import pytest
import torch

import lpips_torch as lt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spnerf_amd_lpips.h")


def lpips_header_symbols():
    txt = open(HEADER).read()
    return sorted(set(re.findall(r"\b(spnerf_lpips_?[a-z0-9_]*)\s*\(", txt)))


def test_lpips_exports_match_the_header():
    from spnerf_amd import _data_lib, _eval_lib, _image_lib, _lib, _loss_lib, _lpips_lib, _view_lib
    syms = lpips_header_symbols()
    assert syms == ["spnerf_lpips", "spnerf_lpips_abi_version", "spnerf_lpips_bands", "spnerf_lpips_features_floats",
                    "spnerf_lpips_pack_weights", "spnerf_lpips_weights_floats", "spnerf_lpips_workspace_bytes"]
    L = _lpips_lib.lib()
    assert L is _lib.lib()
    for s in syms:
        assert hasattr(L, s), s
    assert sorted(_lpips_lib.SIGNATURES) == syms, "lpips signature table out of sync with the header"
    for other in (_lib, _eval_lib, _view_lib, _image_lib, _loss_lib, _data_lib):
        assert not set(_lpips_lib.SIGNATURES) & set(other.SIGNATURES)
    hdr = open(HEADER).read()
    consts = {k: int(v) for k, v in re.findall(r"#define (SPNERF_LPIPS_[A-Z_]+) (\d+)\b", hdr)}
    assert L.spnerf_lpips_abi_version() == consts["SPNERF_LPIPS_ABI_VERSION"] == _lpips_lib.SPNERF_LPIPS_ABI_VERSION == 1
    assert consts["SPNERF_LPIPS_TAPS"] == _lpips_lib.LPIPS_TAPS == 5
    assert consts["SPNERF_LPIPS_MIN_SIDE"] == _lpips_lib.LPIPS_MIN_SIDE == 31
    assert consts["SPNERF_LPIPS_MAX_SIDE"] == _lpips_lib.LPIPS_MAX_SIDE
    assert ctypes.sizeof(_lpips_lib.LpipsResult) == 88
    # per tap [C_out][K rounded up to 32] weights, C_out biases, C_out lin weights
    want = sum(co * ((ci * k * k + 31) // 32 * 32 + 2) for ci, co, k, *_ in lt.LAYERS)
    assert L.spnerf_lpips_weights_floats() == want == 2472192
    assert L.spnerf_abi_version() == 2 and L.spnerf_image_abi_version() == 1       # the older ABIs are untouched


# 35 x 47 divides evenly under conv1's stride ((35 + 4 - 11) % 4 == 0) and gives 8 x 11; 34 x 46 leaves a
# remainder of 3 in both axes and gives the 7 x 10, 3 x 4, 1 x 1 taps where both pools drop a column
@pytest.mark.parametrize("H,W,want", [(31, 31, [(7, 7), (3, 3), (1, 1), (1, 1), (1, 1)]),
                                      (35, 47, [(8, 11), (3, 5), (1, 2), (1, 2), (1, 2)]),
                                      (34, 46, [(7, 10), (3, 4), (1, 1), (1, 1), (1, 1)]),
                                      (224, 224, [(55, 55), (27, 27), (13, 13), (13, 13), (13, 13)])])
def test_tap_sizes_of_the_restatement(H, W, want):
    from spnerf_amd import perceptual
    convs, biases, _ = lt.seeded_weights()
    taps = lt.features(torch.zeros(3, H, W), convs, biases)
    assert [tuple(t.shape[1:]) for t in taps] == want
    assert [t.shape[0] for t in taps] == [64, 192, 384, 256, 256] == list(perceptual.CHANNELS)
    assert perceptual.tap_sizes(H, W) == want


def test_restatement_is_a_distance():
    w = lt.seeded_weights()
    a, b = lt.pair(35, 47)
    score, layers, _, _ = lt.lpips(a, b, w)
    assert all(d > 0 for d in layers) and abs(score - sum(layers)) == 0
    assert 1e-3 < score < 1e-2, score                       # the issue's restatement scored 3.6e-3 to 3.8e-3
    assert lt.lpips(a, a, w)[0] == 0.0
    assert lt.lpips(b, a, w)[0] == score
    pre = lt.lpips(2 * a.double() - 1, 2 * b.double() - 1, w, normalize=False)[0]
    assert abs(pre - score) <= 1e-15
    f32 = lt.lpips(a, b, w, dtype=torch.float32)
    print(f"35x47: score {score:.6e}, torch fp32 off by {abs(float(f32[0]) - score) / score:.1e} relative")
    assert abs(float(f32[0]) - score) <= 1e-5 * score       # the bar the GPU is held to holds for torch's own fp32
    with pytest.raises(RuntimeError):
        lt.features(torch.zeros(3, 30, 40), w[0], w[1])     # the second pool has no window


def test_state_dict_namings_give_the_same_tensors():
    from spnerf_amd import perceptual
    w = lt.seeded_weights()
    want = perceptual._checked(*w)
    pkg = lt.package_state_dict(w)
    tv, lin = lt.split_state_dicts(w)
    for got in (perceptual.state_dict_tensors(pkg), perceptual.state_dict_tensors(tv, lin),
                perceptual.state_dict_tensors({**tv, **lin})):
        got = perceptual._checked(*got)
        for seq_g, seq_w in zip(got, want):
            assert len(seq_g) == 5 and all(torch.equal(g, t) for g, t in zip(seq_g, seq_w))
    assert [tuple(t.shape) for t in want[2]] == [(c,) for c in perceptual.CHANNELS]
    for key in ("net.slice3.6.weight", "net.slice5.10.bias", "lin2.model.1.weight"):
        sd = dict(pkg)
        del sd[key]
        with pytest.raises(ValueError, match=re.escape(key)):
            perceptual.LpipsWeights.from_state_dict(sd, "cpu")
    with pytest.raises(ValueError, match=re.escape("lin0.model.1.weight")):
        perceptual.LpipsWeights.from_state_dict(tv, "cpu")
    bad = dict(pkg)
    bad["net.slice2.3.weight"] = torch.zeros(192, 64, 3, 3)
    with pytest.raises(ValueError, match=r"convs\[1\]"):
        perceptual.LpipsWeights.from_state_dict(bad, "cpu")
    bad = dict(pkg)
    bad["lin4.model.1.weight"] = torch.zeros(1, 255, 1, 1)
    with pytest.raises(ValueError, match=r"lins\[4\]"):
        perceptual.LpipsWeights.from_state_dict(bad, "cpu")
    with pytest.raises(ValueError, match="biases has 4 entries"):
        perceptual.LpipsWeights.from_tensors(w[0], w[1][:4], w[2])


def test_lpips_argument_errors_are_reported():
    from spnerf_amd import _lpips_lib
    L = _lpips_lib.lib()
    one = ctypes.c_void_p(256)      # never dereferenced: the arguments are refused first
    full = L.spnerf_lpips_workspace_bytes(40, 40, 0)

    def call(x=one, y=one, H=40, W=40, cs=1600, rs=40, ps=1, wts=one, wsp=one, nbytes=full, res=one):
        return L.spnerf_lpips(x, y, H, W, cs, rs, ps, 1, wts, wsp, nbytes, None, res, None)

    for kw, text in ((dict(x=None), b"NULL image"), (dict(y=None), b"NULL image"), (dict(wts=None), b"NULL weights"),
                     (dict(wsp=None), b"NULL weights"), (dict(res=None), b"NULL weights"),
                     (dict(H=30), b"image 30 x 40 smaller than 31"), (dict(W=30), b"smaller than 31"), (dict(H=-1), b"smaller than 31"),
                     (dict(H=1 << 20), b"larger than"), (dict(cs=-1), b"negative stride"), (dict(rs=-40), b"negative stride"),
                     (dict(wsp=ctypes.c_void_p(264)), b"not 16-byte aligned"), (dict(res=ctypes.c_void_p(260)), b"not 8-byte aligned"),
                     (dict(nbytes=1024), b"too small"), (dict(nbytes=0), b"too small")):
        assert call(**kw) == -1, kw
        assert text in L.spnerf_last_error(), (kw, L.spnerf_last_error())
    wsb = L.spnerf_lpips_workspace_bytes
    assert wsb(30, 40, 0) == -1 and b"smaller than 31" in L.spnerf_last_error()
    assert L.spnerf_lpips_features_floats(40, 30) == -1
    least = wsb(97, 130, 1)
    assert 0 < least < wsb(97, 130, 0) and least % 16 == 0 and wsb(97, 130, least) == least
    assert wsb(97, 130, 1 << 40) == wsb(97, 130, 0) == wsb(97, 130, wsb(97, 130, 0))
    bands = (ctypes.c_int32 * 5)()
    assert L.spnerf_lpips_bands(97, 130, wsb(97, 130, 0), bands) == 0 and list(bands) == [1] * 5
    assert L.spnerf_lpips_bands(97, 130, least, bands) == 0 and bands[0] >= 3 and bands[1] >= 2
    assert L.spnerf_lpips_bands(97, 130, least - 16, bands) == -1 and b"too small" in L.spnerf_last_error()
    taps = [(23, 31), (11, 15), (5, 7), (5, 7), (5, 7)]
    assert L.spnerf_lpips_features_floats(97, 130) == sum(2 * h * w * c for (h, w), c in zip(taps, (64, 192, 384, 256, 256)))


def test_python_surface_refuses_cpu_tensors_and_bad_arguments():
    import spnerf_amd
    from spnerf_amd import _lib
    assert spnerf_amd.lpips is spnerf_amd.perceptual.lpips and spnerf_amd.LpipsWeights is spnerf_amd.perceptual.LpipsWeights
    w = lt.seeded_weights()
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        spnerf_amd.LpipsWeights.from_tensors(*w)                       # CPU weights and no device
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        spnerf_amd.LpipsWeights.from_state_dict(lt.package_state_dict(w), "cpu")
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        spnerf_amd.lpips(torch.zeros(40, 40, 3), torch.zeros(40, 40, 3), None)
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        spnerf_amd.view_metrics(torch.zeros(1600, 3), torch.zeros(1600, 3), hw=(40, 40), lpips=object())
