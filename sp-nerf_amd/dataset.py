"""The training set's depth, label and scaling tensors on the GPU — the rest of the reference's
datasets/satellite_scene.py after the ray generator (``satellite``): ``load_depth_data``
(:223-297), ``load_semantic_data`` (:299-389) and ``init_scaling_params`` (:391-413), backed by
csrc/dataset.hip (include/spnerf_amd_data.h).

Only the file reading of those methods is left to the caller: each function takes the arrays the
reference reads from the JSON, ``*_2DPts.txt`` / ``*_3DPts_ecef.txt`` / ``*_Correl.txt`` and CLS
raster files and returns what the method returns, on the device — the tensors ``render_rays``
(``valid_depth``, ``target_depths``, ``target_std``), ``FusedTrainLoss`` and ``BatchGather``
consume.  Argument errors are raised on the host before the library is loaded.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from .satellite import RPCModel

VOID_LABEL = -100
LOC_KEYS = ("X_scale", "X_offset", "Y_scale", "Y_offset", "Z_scale", "Z_offset")


def _device(device):
    """The device to allocate on; anything but a GPU is an error, as elsewhere."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.SpnerfError("spnerf_amd builds the training set on the MI355X (HIP) only; got device "
                               f"{dev}.")
    return dev


def _on_device(x, dtype, device):
    """``x`` as a contiguous ``dtype`` tensor on ``device``; a CPU *tensor* is refused like everywhere
    else in the package, host arrays are uploaded."""
    if isinstance(x, torch.Tensor):
        _lib.require_device(x)
        return x.to(device=device, dtype=dtype).contiguous()
    return torch.tensor(np.asarray(x), device=device).to(dtype).contiguous()


def _px(p):
    return (int(p[0]), int(p[1]))


def _keypoints(i, im, height, width):
    """The (K, 2) int64 host keypoints of image ``i``, checked: strictly increasing in
    row * width + col (the reference assigns the k-th keypoint to the k-th set pixel) and inside
    the image."""
    p = im["pts2d"]
    p = p.cpu().numpy() if isinstance(p, torch.Tensor) else np.asarray(p)
    if p.size == 0:
        raise ValueError(f"load_depth_data: image {i} has K == 0 keypoints (the min of no correlation is undefined)")
    if p.ndim != 2 or p.shape[1] != 2:
        raise ValueError(f"load_depth_data: image {i}: pts2d must be (K, 2) [col, row], got {p.shape}")
    if not np.issubdtype(p.dtype, np.integer):
        if not np.array_equal(p, np.floor(p)):
            raise ValueError(f"load_depth_data: image {i}: pts2d must be whole pixels")
    p = p.astype(np.int64)
    if (p[:, 0] < 0).any() or (p[:, 0] >= width).any() or (p[:, 1] < 0).any() or (p[:, 1] >= height).any():
        bad = int(np.flatnonzero((p[:, 0] < 0) | (p[:, 0] >= width) | (p[:, 1] < 0) | (p[:, 1] >= height))[0])
        raise ValueError(f"load_depth_data: image {i}: keypoint {bad} {_px(p[bad])} is outside the "
                         f"{height} x {width} image")
    flat = p[:, 1] * width + p[:, 0]
    step = np.diff(flat)
    if (step <= 0).any():
        bad = int(np.flatnonzero(step <= 0)[0]) + 1
        what = "repeats" if step[bad - 1] == 0 else "comes before"
        raise ValueError(f"load_depth_data: image {i}: keypoints must be strictly increasing in row * width + col; "
                         f"keypoint {bad} {_px(p[bad])} {what} keypoint {bad - 1} {_px(p[bad - 1])}")
    return p


def depth_planes(images, *, center, range, stdscale=1, margin=0, img_downscale=1.0, device="cuda"):
    """``load_depth_data`` before its last step: ``(deprays, depths, valid_depth, depth_std,
    depth_range)`` with ``depth_std`` not yet scaled and ``depth_range`` the (2,) device tensor
    [min, max] of the depths of all images, which scales it."""
    if float(img_downscale) != 1.0:
        raise ValueError(f"depth priors need img_downscale == 1 (got {img_downscale}): at any other scale the "
                         "reference indexes its planes with fractional pixels and its padded assignment no longer "
                         "matches in count")
    images = list(images)
    if not images:
        raise ValueError("load_depth_data: no images")
    checked = []
    for i, im in enumerate(images):
        h, w = int(im["height"]), int(im["width"])
        p = _keypoints(i, im, h, w)
        k = p.shape[0]
        if tuple(im["pts3d"].shape) != (k, 3) or tuple(im["correl"].shape) != (k,):
            raise ValueError(f"load_depth_data: image {i}: {k} keypoints but pts3d {tuple(im['pts3d'].shape)} "
                             f"and correl {tuple(im['correl'].shape)}")
        checked.append((h, w, p))
    for im in images:
        for key in ("pts3d", "correl"):
            if isinstance(im[key], torch.Tensor):
                _lib.require_device(im[key])
    dev = _device(device)

    from . import _data_lib
    L = _data_lib.lib()
    cen = (ctypes.c_float * 3)(*[float(v) for v in np.asarray(center, np.float32)])
    n_total = sum(h * w for h, w, _ in checked)
    deprays = torch.empty(n_total, 8, device=dev)
    depths = torch.empty(n_total, 2, device=dev)
    valid = torch.empty(n_total, device=dev)
    stds = torch.empty(n_total, device=dev)
    drange = torch.tensor([float("inf"), float("-inf")], device=dev)
    ws = torch.empty(_data_lib.DATA_WORKSPACE_BYTES, dtype=torch.uint8, device=dev)
    at = 0
    with torch.cuda.device(dev):
        for im, (h, w, p) in zip(images, checked):
            pix = torch.as_tensor(p.astype(np.float64), device=dev).contiguous()
            pts3d = _on_device(im["pts3d"], torch.float32, dev)
            correl = _on_device(im["correl"], torch.float32, dev)
            rpc = im["rpc"] if isinstance(im["rpc"], RPCModel) else RPCModel(im["rpc"])
            n = h * w
            _lib.check(L.spnerf_depth_priors(rpc.packed(), float(im["min_alt"]), float(im["max_alt"]), h, w, cen,
                                             float(np.float32(range)), _lib.ptr(pix), _lib.ptr(pts3d), _lib.ptr(correl),
                                             p.shape[0], float(np.float32(stdscale)), float(np.float32(margin)),
                                             _lib.ptr(deprays[at:at + n]), _lib.ptr(depths[at:at + n]),
                                             _lib.ptr(valid[at:at + n]), _lib.ptr(stds[at:at + n]), _lib.ptr(drange),
                                             _lib.ptr(ws), _lib.stream_of(deprays)), "depth_priors")
            at += n
    return deprays, depths, valid, stds, drange


def load_depth_data(images, *, center, range, stdscale=1, margin=0, img_downscale=1.0, device="cuda"):
    """satellite_scene.py:223-297.  ``images``: one dict per image with the camera metadata
    (``rpc``, ``height``, ``width``, ``min_alt``, ``max_alt``) and the arrays ``pts2d`` (K, 2)
    [col, row], ``pts3d`` (K, 3) ECEF, ``correl`` (K,).  ``center`` / ``range`` as
    ``satellite.scene_normalisation`` gives them.  Returns ``all_deprays`` (N, 8),
    ``all_depths`` (N, 2) [depth, weight], ``all_valid_depth`` (N,), ``all_depth_stds`` (N,), all
    float32 on the device, N the images' height * width summed; rows without a keypoint are zero.

    One launch pair per image (``spnerf_depth_priors``); the global depth range accumulates on the
    device and scales the std planes after the last image (:295).  Only ``img_downscale == 1`` is
    supported, and the keypoints of an image must be strictly increasing in row * width + col."""
    deprays, depths, valid, stds, drange = depth_planes(images, center=center, range=range, stdscale=stdscale,
                                                        margin=margin, img_downscale=img_downscale, device=device)
    stds *= drange[1] - drange[0]
    return deprays, depths, valid, stds


def scene_bounds(metas, img_downscale=1.0, device="cuda"):
    """Per-axis minimum and maximum, as a (6,) float32 device tensor [min xyz, max xyz], of the near
    and far points of every ray of every image in ``metas`` (satellite_scene.py:394-406): one
    ``spnerf_scene_bounds`` launch per image folding into one buffer; no ray is stored."""
    metas = list(metas)
    if not metas:
        raise ValueError("scene_bounds: no images")
    if not float(img_downscale) > 0:
        raise ValueError(f"scene_bounds: bad img_downscale {img_downscale}")
    dev = _device(device)
    from . import _data_lib
    L = _data_lib.lib()
    inf = float("inf")
    bounds = torch.tensor([inf, inf, inf, -inf, -inf, -inf], device=dev)
    with torch.cuda.device(dev):
        for d in metas:
            h, w = int(d["height"] // img_downscale), int(d["width"] // img_downscale)
            rpc = d["rpc"] if isinstance(d["rpc"], RPCModel) else RPCModel(d["rpc"])
            _lib.check(L.spnerf_scene_bounds(rpc.packed(), float(img_downscale), float(d["min_alt"]), float(d["max_alt"]),
                                             h, w, _lib.ptr(bounds), _lib.stream_of(bounds)), "scene_bounds")
    return bounds


def init_scaling_params(metas, img_downscale=1.0, device="cuda"):
    """satellite_scene.py:391-413: the ``scene.loc`` dict (X/Y/Z ``_scale`` and ``_offset`` as Python
    floats; the caller writes the JSON) over every pixel of every image in ``metas`` at
    ``img_downscale``.  scale = (max − min) / 2 and offset = min + scale per axis in float32, as
    ``utils.rpc_scaling_params`` evaluates them on the float32 points."""
    b = scene_bounds(metas, img_downscale, device).cpu().numpy()
    loc = {}
    for k, axis in enumerate("XYZ"):
        scale = (b[3 + k] - b[k]) / np.float32(2)
        loc[f"{axis}_scale"], loc[f"{axis}_offset"] = float(scale), float(b[k] + scale)
    return loc


def label_lut(label_mapping) -> np.ndarray:
    """The 256-entry int32 table of a ``{original: mapped}`` dict, −100 where unmapped."""
    lut = np.full(256, VOID_LABEL, np.int32)
    for k, v in dict(label_mapping).items():
        if not 0 <= int(k) < 256:
            raise ValueError(f"load_semantic_data: class code {k} outside [0, 256)")
        lut[int(k)] = int(v)
    return lut


def load_semantic_data(labels, metas, label_mapping, dense_ss=False, sem_downscale=8, device="cuda"):
    """satellite_scene.py:299-389.  ``labels``: the (Hs, Ws) class-code raster as read from the CLS
    file (uint8 or an integer type); ``metas``: dicts with ``height`` and ``width``;
    ``label_mapping``: ``SEMANTIC_CONFIG[n]["label_mapping"]``.  Returns ``all_semantics`` (N, 1)
    int64 and ``all_valid_semantics`` (N,) float32 on the device, one ``spnerf_semantic_labels``
    launch per image.  ``sem_downscale`` defaults to 8 like the reference method's argument (which
    it uses instead of the dataset's ``sem_downscale``)."""
    metas = list(metas)
    if not metas:
        raise ValueError("load_semantic_data: no images")
    sd = int(sem_downscale)
    if sd < 1 or sd != sem_downscale:
        raise ValueError(f"load_semantic_data: sem_downscale must be a positive integer, got {sem_downscale}")
    if len(labels.shape) != 2 or 0 in tuple(labels.shape):
        raise ValueError(f"load_semantic_data: the label raster must be (Hs, Ws), got {tuple(labels.shape)}")
    hs, ws = (int(v) for v in labels.shape)
    if dense_ss and (hs // sd < 1 or ws // sd < 1):
        raise ValueError(f"load_semantic_data: a {hs} x {ws} raster has no 1/{sd} downsampling")
    lut_host = label_lut(label_mapping)
    sizes = [(int(d["height"]), int(d["width"])) for d in metas]
    if any(h < 1 or w < 1 for h, w in sizes):
        raise ValueError("load_semantic_data: empty target image")
    if isinstance(labels, torch.Tensor):
        _lib.require_device(labels)
        is_u8 = labels.dtype == torch.uint8
        if not is_u8 and labels.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64):
            raise ValueError(f"load_semantic_data: integer class codes expected, got {labels.dtype}")
    else:
        labels = np.asarray(labels)
        is_u8 = labels.dtype == np.uint8
        if not np.issubdtype(labels.dtype, np.integer):
            raise ValueError(f"load_semantic_data: integer class codes expected, got {labels.dtype}")
        if not is_u8:
            labels = labels.astype(np.int64).clip(-1, 256).astype(np.int32)
    dev = _device(device)

    from . import _data_lib
    L = _data_lib.lib()
    if isinstance(labels, torch.Tensor) and not is_u8:
        labels = labels.clamp(-1, 256)
    raster = _on_device(labels, torch.uint8 if is_u8 else torch.int32, dev)
    lut = torch.as_tensor(lut_host, device=dev)
    n_total = sum(h * w for h, w in sizes)
    out = torch.empty(n_total, 1, dtype=torch.int64, device=dev)
    valid = torch.empty(n_total, device=dev)
    at = 0
    with torch.cuda.device(dev):
        for h, w in sizes:
            _lib.check(L.spnerf_semantic_labels(_lib.ptr(raster), 0 if is_u8 else 1, hs, ws, _lib.ptr(lut), h, w, sd,
                                                1 if dense_ss else 0, _lib.ptr(out[at:at + h * w]),
                                                _lib.ptr(valid[at:at + h * w]), _lib.stream_of(out)), "semantic_labels")
            at += h * w
    return out, valid
