"""LPIPS (AlexNet, lpips 0.1, spatial=False) restated with torch's CPU operators in float64, and
seeded stand-in weights — a helper of the tests, not a test.

The definition (include/spnerf_amd_lpips.h): the scaling layer, five taps of AlexNet taken after
their ReLUs, unit-normalised over channels with eps 1e-10 added to the norm, the squared difference
weighted by each tap's lin vector, averaged over positions and summed over taps.
"""
import functools

import torch
import torch.nn.functional as F

SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
# (C_in, C_out, kernel, stride, padding, max-pool 3/2 in front of it)
LAYERS = ((3, 64, 11, 4, 2, False), (64, 192, 5, 1, 2, True), (192, 384, 3, 1, 1, True), (384, 256, 3, 1, 1, False),
          (256, 256, 3, 1, 1, False))
FEATURE_INDEX = (0, 3, 6, 8, 10)


@functools.lru_cache(maxsize=None)
def seeded_weights(seed=0):
    """(convs, biases, lins) as float32 CPU tensors: convolution weights randn · sqrt(2 / fan_in),
    biases 0.1 · randn, lin weights rand / C (not negative, as the trained ones are)."""
    g = torch.Generator().manual_seed(seed)
    convs, biases, lins = [], [], []
    for ci, co, k, _, _, _ in LAYERS:
        convs.append(torch.randn(co, ci, k, k, generator=g) * (2.0 / (ci * k * k)) ** 0.5)
        biases.append(0.1 * torch.randn(co, generator=g))
        lins.append(torch.rand(co, generator=g) / co)
    return tuple(convs), tuple(biases), tuple(lins)


def features(img, convs, biases, dtype=torch.float64):
    """The five post-ReLU taps, each (C, h, w), of a (3, H, W) image in [−1, 1]."""
    x = img.to(dtype)[None]
    shift, scale = (torch.tensor(v, dtype=dtype, device=x.device).view(1, 3, 1, 1) for v in (SHIFT, SCALE))
    x = (x - shift) / scale
    taps = []
    for (ci, co, k, stride, pad, pool), w, b in zip(LAYERS, convs, biases):
        if pool:
            x = F.max_pool2d(x, 3, 2)
        x = F.relu(F.conv2d(x, w.to(dtype), b.to(dtype), stride=stride, padding=pad))
        taps.append(x[0])
    return taps


def lpips(a, b, weights, normalize=True, dtype=torch.float64):
    """(score, [d_l], [taps of a], [taps of b]) for two (3, H, W) images."""
    convs, biases, lins = weights
    a, b = a.to(dtype), b.to(dtype)
    if normalize:
        a, b = 2 * a - 1, 2 * b - 1
    fa, fb = features(a, convs, biases, dtype), features(b, convs, biases, dtype)
    layers = []
    for u, v, lin in zip(fa, fb, lins):
        nu = u / (u.pow(2).sum(0, keepdim=True).sqrt() + 1e-10)
        nv = v / (v.pow(2).sum(0, keepdim=True).sqrt() + 1e-10)
        d = ((nu - nv) ** 2 * lin.to(dtype).view(-1, 1, 1)).sum(0)
        layers.append(float(d.mean()) if dtype == torch.float64 else d.mean())
    return sum(layers), layers, fa, fb


def pair(H, W, seed=None):
    """Two float32 (3, H, W) images in [0, 1]: b = clamp(a + 0.25 · randn, 0, 1)."""
    g = torch.Generator().manual_seed(1000 * H + W if seed is None else seed)
    a = torch.rand(3, H, W, generator=g)
    b = (a + 0.25 * torch.randn(3, H, W, generator=g)).clamp(0, 1)
    return a, b


def package_state_dict(weights):
    """The weights under the `lpips` package's names (written from its published source)."""
    convs, biases, lins = weights
    sd = {}
    for l, idx in enumerate(FEATURE_INDEX):
        sd[f"net.slice{l + 1}.{idx}.weight"] = convs[l]
        sd[f"net.slice{l + 1}.{idx}.bias"] = biases[l]
        sd[f"lin{l}.model.1.weight"] = lins[l].view(1, -1, 1, 1)
    sd["scaling_layer.shift"] = torch.tensor(SHIFT).view(1, 3, 1, 1)
    sd["scaling_layer.scale"] = torch.tensor(SCALE).view(1, 3, 1, 1)
    return sd


def split_state_dicts(weights):
    """(torchvision alexnet features state_dict, the lin file's state_dict)."""
    convs, biases, lins = weights
    tv, lin = {}, {}
    for l, idx in enumerate(FEATURE_INDEX):
        tv[f"features.{idx}.weight"] = convs[l]
        tv[f"features.{idx}.bias"] = biases[l]
        lin[f"lin{l}.model.1.weight"] = lins[l].view(1, -1, 1, 1)
    tv["classifier.1.weight"] = torch.zeros(2, 2)   # the rest of the classifier is ignored
    return tv, lin
