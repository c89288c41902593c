"""float64 numpy / scipy restatement of the SSIM the reference's validation step logs
(modules/metrics.py ssim :210-215 -> ``kornia.losses.ssim(img1, img2, window_size=3)`` of kornia
0.5.3, whose mean is the score), as include/spnerf_amd_image.h states it.

For images x, y of shape (C, H, W), an odd window size ws and r = ws // 2:
  g[i] = exp(-(i - r)^2 / (2 * 1.5^2)) normalised to sum 1; the window is outer(g, g);
  f(.) = the correlation with that window per channel, the border mirrored without repeating the
         edge value (torch's 'reflect' padding) — ``scipy.ndimage.correlate1d(mode='mirror')``
         along both axes;
  mu1 = f(x), mu2 = f(y), s1 = f(x x) - mu1^2, s2 = f(y y) - mu2^2, s12 = f(x y) - mu1 mu2;
  map = ((2 mu1 mu2 + C1)(2 s12 + C2)) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2) + 1e-12),
  C1 = (0.01 max_val)^2, C2 = (0.03 max_val)^2; the score is the mean of the map.

kornia is not a dependency of this repository and its own outputs are not among the fixtures: the
restatement is held to a second, independently written form instead (tests/test_ssim_ref.py)."""
from __future__ import annotations

import numpy as np
from scipy.ndimage import correlate1d

EPS = 1e-12


def gaussian(ws: int, sigma: float = 1.5) -> np.ndarray:
    i = np.arange(ws, dtype=np.float64) - ws // 2
    g = np.exp(-(i * i) / (2.0 * sigma * sigma))
    return g / g.sum()


def constants(max_val: float = 1.0):
    return (0.01 * max_val) ** 2, (0.03 * max_val) ** 2


def blur(img: np.ndarray, ws: int) -> np.ndarray:
    """f(.) of a (C, H, W) float64 image."""
    g = gaussian(ws)
    if img.shape[1] <= ws // 2 or img.shape[2] <= ws // 2:
        raise ValueError(f"image {img.shape[1:]} too small for a mirrored border of {ws // 2}")
    return correlate1d(correlate1d(img, g, axis=2, mode="mirror"), g, axis=1, mode="mirror")


def ssim_map(x, y, ws: int = 3, max_val: float = 1.0) -> np.ndarray:
    """The (C, H, W) float64 SSIM map of two (C, H, W) images."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    assert x.shape == y.shape and x.ndim == 3 and ws % 2 == 1
    c1, c2 = constants(max_val)
    mu1, mu2 = blur(x, ws), blur(y, ws)
    s1 = blur(x * x, ws) - mu1 * mu1
    s2 = blur(y * y, ws) - mu2 * mu2
    s12 = blur(x * y, ws) - mu1 * mu2
    return ((2.0 * mu1 * mu2 + c1) * (2.0 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s1 + s2 + c2) + EPS)


def ssim(x, y, ws: int = 3, max_val: float = 1.0) -> float:
    return float(np.mean(ssim_map(x, y, ws, max_val)))


def chw_of(flat, hw, layout: str) -> np.ndarray:
    """The (C, H, W) image an (H * W, C) buffer is under ``layout``: "hwc" the interleaved image it
    holds (eval.py:393), "chw" the C planes main.py:261's ``.view(1, C, H, W)`` reads it as."""
    flat = np.ascontiguousarray(flat)
    H, W = hw
    C = flat.shape[-1]
    if layout == "hwc":
        return flat.reshape(H, W, C).transpose(2, 0, 1)
    assert layout == "chw"
    return flat.reshape(C, H, W)
