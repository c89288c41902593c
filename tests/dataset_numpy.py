"""numpy restatement of the reference's dataset construction — TEST INFRASTRUCTURE ONLY.

datasets/satellite_scene.py load_depth_data (:223-297), load_semantic_data (:299-389) and
init_scaling_params (:391-413) on arrays instead of files, built on oracle/rpc_ref.  Pinned to the
reference's own functions by tests/golden/dataset.npz (tests/test_dataset_ref.py); the GPU kernels of
csrc/dataset.hip are held to it where no fixture exists.
"""
from __future__ import annotations

import numpy as np

from oracle import rpc_ref

F32 = np.float32
VOID = -100


def rpc_of(packed, downscale=1.0):
    d = dict(zip(rpc_ref.KEYS, packed[:10]))
    d.update(row_num=packed[10:30], row_den=packed[30:50], col_num=packed[50:70], col_den=packed[70:90])
    return rpc_ref.RPC(d, downscale)


def fma32(a, b, c):
    """fp32 fused multiply-add: torch's CPU vector norm accumulates acc = fma(x, x, acc) along the
    row.  The product of two fp32 values is exact in fp64; the sum is then rounded twice (fp64,
    fp32), which differs from a true fma only on a tie of the 2^-29-relative kind."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def depth_image(rpc, min_alt, max_alt, height, width, pts2d, pts3d, correl, center, rng, stdscale, margin):
    """One image of load_depth_data at img_downscale 1: the padded planes before the global scale and
    (depth_min, depth_max).  Keypoints strictly increasing in row * width + col (the k-th keypoint
    is then the k-th set pixel, :270-278)."""
    cols, rows = np.asarray(pts2d, np.int64).T
    rays = rpc_ref.normalize_rays(rpc_ref.get_rays(cols.astype(float), rows.astype(float), rpc, min_alt, max_alt),
                                  center, rng)
    c = np.asarray(correl, F32)
    with np.errstate(invalid="ignore", divide="ignore"):
        w = ((c - c.min()) / (c.max() - c.min())).astype(F32)                           # :248-249
    p = ((np.asarray(pts3d, F32) - np.asarray(center, F32)) / F32(rng)).astype(F32)     # :258
    diff = (p - rays[:, :3]).astype(F32)
    depth = np.sqrt(fma32(diff[:, 2], diff[:, 2], fma32(diff[:, 1], diff[:, 1], diff[:, 0] * diff[:, 0])))  # :261
    std = (F32(stdscale) * (F32(1) - w) + F32(margin)).astype(F32)                      # :262
    n = height * width
    idx = rows * width + cols
    planes = {"deprays": np.zeros((n, 8), F32), "depths": np.zeros((n, 2), F32), "valid_depth": np.zeros(n, F32),
              "depth_std": np.zeros(n, F32)}
    planes["deprays"][idx] = rays
    planes["depths"][idx, 0] = depth
    planes["depths"][idx, 1] = w
    planes["valid_depth"][idx] = 1
    planes["depth_std"][idx] = std
    return planes, (depth.min(), depth.max())


def load_depth_data(images, center, rng, stdscale=1, margin=0):
    """images: dicts with rpc (rpc_ref.RPC), min_alt, max_alt, height, width, pts2d, pts3d, correl."""
    parts, lo, hi = [], None, None
    for im in images:
        planes, (a, b) = depth_image(im["rpc"], im["min_alt"], im["max_alt"], im["height"], im["width"], im["pts2d"],
                                     im["pts3d"], im["correl"], center, rng, stdscale, margin)
        parts.append(planes)
        lo = a if lo is None else min(lo, a)
        hi = b if hi is None else max(hi, b)
    cat = {k: np.concatenate([p[k] for p in parts], 0) for k in parts[0]}
    return cat["deprays"], cat["depths"], cat["valid_depth"], (cat["depth_std"] * F32(hi - lo)).astype(F32), (lo, hi)


def nearest_index(n_out, n_in):
    """Source index of F.interpolate(mode='nearest'): floor(dst * scale) with the scale formed in
    fp32 as in / out, clamped to the last source index."""
    scale = F32(n_in) / F32(n_out)
    return np.minimum(np.floor(np.arange(n_out, dtype=F32) * scale).astype(np.int64), n_in - 1)


def semantic_image(raster, mapping, height, width, dense_ss=False, sem_downscale=8):
    """One image of load_semantic_data: labels int64 (H*W, 1), valid float32 (H*W,)."""
    raster = np.asarray(raster).astype(np.int64)
    mapped = np.full(raster.shape, VOID, np.int64)
    for k, v in mapping.items():
        mapped[raster == k] = v
    hs, ws = mapped.shape
    if dense_ss:
        mapped = mapped[np.ix_(nearest_index(hs // sem_downscale, hs), nearest_index(ws // sem_downscale, ws))]
        lab = mapped[np.ix_(nearest_index(height, mapped.shape[0]), nearest_index(width, mapped.shape[1]))]
        valid = (lab != VOID).astype(F32)
    else:
        lab = mapped[np.ix_(nearest_index(height, hs), nearest_index(width, ws))].copy()
        mask = np.zeros((height, width), F32)
        mask[np.ix_(np.arange(0, height, sem_downscale), np.arange(0, width, sem_downscale))] = 1
        valid = mask * (lab != VOID).astype(F32)
        lab[valid == 0] = VOID
    return lab.reshape(-1, 1), valid.reshape(-1)


def load_semantic_data(raster, metas, mapping, dense_ss=False, sem_downscale=8):
    parts = [semantic_image(raster, mapping, m["height"], m["width"], dense_ss, sem_downscale) for m in metas]
    return np.concatenate([p[0] for p in parts], 0), np.concatenate([p[1] for p in parts], 0)


def scene_points(rpc, min_alt, max_alt, h, w):
    """near and far points of every pixel of an h x w image in fp32 (:401-406)."""
    cols, rows = np.meshgrid(np.arange(w), np.arange(h))
    rays = rpc_ref.get_rays(cols.flatten().astype(float), rows.flatten().astype(float), rpc, min_alt, max_alt)
    far = (rays[:, :3] + (rays[:, 7:8] * rays[:, 3:6]).astype(F32)).astype(F32)
    return np.concatenate([rays[:, :3], far], 0)


def scaling_params(points):
    """utils.rpc_scaling_params per axis on the float32 points → the scene.loc dict (float32 values)."""
    out = {}
    for k, name in enumerate("XYZ"):
        v = points[:, k]
        scale = (v.max() - v.min()) / F32(2)
        out[f"{name}_scale"], out[f"{name}_offset"] = scale, v.min() + scale
    return out
