"""Whole views: what a user does with a trained model after each epoch — the reference's
``NeRF_pl.forward(mode='test')`` + ``validation_step`` (main.py:59-89, 188-299) and
``save_nerf_output_to_images`` (eval.py:27-101) — on the GPU (csrc/view.hip,
include/spnerf_amd_view.h).

``render_image`` renders N rays chunk by chunk into image planes left on the device: the final
pass's MLP rows go to ``k_composite_products``, which writes per-ray values only (rgb, depth, the
shadow / albedo / sky / uncertainty sums of eval.py:76-101, the mean semantic logits and their
argmax) — the per-sample dictionary of ``render_rays`` is never materialised.  ``view_metrics``
scores a rendered view against its targets in one pass (psnr, miou, overall accuracy of
modules/metrics.py:206-246) with one device-to-host copy.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _image_lib, _lib, _lpips_lib, _view_lib, image, perceptual
from .rendering import _coarse_rows, _fine_rows
from .rng import current_random_source, device_key
from .spnerf import composite, max_points_per_call

PRODUCTS = ("rgb", "depth", "sun", "albedo", "sky", "beta", "sem")
# plane name -> (trailing shape given the class count, dtype)
_PLANES = {"rgb": (lambda c: (3,), torch.float32), "depth": (lambda c: (), torch.float32),
           "sun": (lambda c: (), torch.float32), "albedo": (lambda c: (3,), torch.float32),
           "sky": (lambda c: (3,), torch.float32), "beta": (lambda c: (), torch.float32),
           "sem_logits": (lambda c: (c,), torch.float32), "sem_class": (lambda c: (), torch.int32)}


def composite_products(model, out, z, noise_std, planes: dict, ray_begin: int = 0) -> None:
    """``spnerf_view_composite_products`` on one chunk's final-pass rows: ray r of the chunk goes
    to entry ``ray_begin + r`` of every plane in ``planes`` (name -> contiguous device tensor; the
    names of ``spnerf_view_planes``, a missing name is a skipped plane).  Takes the σ-noise draw the
    composite of that pass takes (spnerf.py:122)."""
    B, S = z.shape
    key, keep = device_key(z.device)   # on-device σ noise: a slot per inference call, drawn or not
    noise = None if key is not None else current_random_source().noise((B, S), z.device, noise_std)
    if noise is not None:
        noise = noise.contiguous().float()
    z = z.contiguous()
    n_sem = model.num_sem_classes if model.sem else 0
    p = _view_lib.ViewPlanes()
    for name, t in planes.items():
        shape, dtype = _PLANES[name]
        if not t.is_cuda or t.dtype != dtype or not t.is_contiguous() or tuple(t.shape[1:]) != shape(n_sem):
            raise ValueError(f"plane {name!r}: expected a contiguous {dtype} device tensor (N, *{shape(n_sem)}), got "
                             f"{t.dtype} {tuple(t.shape)} on {t.device}")
        if t.shape[0] < ray_begin + B:
            raise ValueError(f"plane {name!r} has {t.shape[0]} rays, the chunk ends at ray {ray_begin + B}")
        setattr(p, name, t.data_ptr())
    _lib.check(_view_lib.lib().spnerf_view_composite_products(
        B, S, _lib.ptr(z), _lib.ptr(out), out.shape[1], _lib.ptr(noise), float(noise_std), 8 + (1 if model.beta else 0),
        n_sem, 8 if model.beta else -1, int(ray_begin), ctypes.byref(p), _lib.rng_ref(key if noise_std != 0 else None),
        _lib.stream_of(out)), "view_composite_products")


def _final_rows(models, args, rays, ts, semantics, clamp_near_far=None):
    """(model, out, z_vals) of the pass whose composite is the image: render_rays(mode='test')
    with ``sc_lambda`` taken as 0 (no product reads the solar march), up to that composite."""
    model, pk, sem, rays_t, out, z_vals, _ = _coarse_rows(models, args, rays, ts, semantics, "test", None, None, None,
                                                                 clamp_near_far)
    if args.n_importance > 0:
        # the coarse weights alone: the σ-only composite takes the same noise draw and marches alike
        _, _, w, _, _ = composite(model, out, z_vals, args.noise_std, weights_only=True)
        model, pk, sem, rays_t, out, z_vals = _fine_rows(models, args, rays, ts, z_vals, w, semantics)
    return model, out, z_vals


def render_image(models, args, rays, ts=None, semantics=None, *, chunk=None,
                 products=("rgb", "depth", "sun", "albedo", "sky", "sem"), out=None, ray_offset=0, center=None,
                 rng=None, clamp_near_far=None) -> dict:
    """Render the N = rays.shape[0] rays of a view (or of a shard of its rows) into image planes
    on the device, under ``torch.no_grad()``, ``chunk`` rays at a time (default: what one MLP call
    takes, ``max_points_per_call``).  The image is that of the coarse model, or of the fine one
    when ``args.n_importance > 0`` (the reference's ``typ``, eval.py:33); the sampling passes and
    the order of the random draws are those of ``render_rays(mode='test')`` with ``sc_lambda`` 0.

    ``products`` names what to write: "rgb" (N, 3), "depth" (N), "sun" (N), "albedo" (N, 3), "sky"
    (N, 3), "beta" (N; a model with the β head) and "sem" — ``sem_logits`` (N, C) and
    ``sem_class`` (N) int32, skipped for a model without the semantic head.  With ``out`` (a dict
    of caller-owned planes of a larger image, the returned names) ray i is written at entry
    ``ray_offset + i``; without it the planes are new and hold the N rays.  With ``center=`` and
    ``rng=`` (the scene's normalisation, SatelliteSceneDataset.center / .range) the altitude of
    every ray comes back as "alt" (N) float64 (get_latlonalt_from_nerf_prediction, eval.py:44).

    Guided sampling clamps its depths to one ray's near / far (rendering.py:95): here that of the
    call's first ray for every chunk, as ``render_rays`` on all N rays at once does, or
    ``clamp_near_far`` (an extension beyond the reference's arguments, as in ``render_rays``: a
    device tensor of 2 floats; a shard passes the whole view's first ray).

    With an on-device random source (``PhiloxRandom``) every chunk draws as step 0 of the global
    ray ids ``ray_offset + i``, so the image does not depend on the chunking or the sharding."""
    if args.model != "sp-nerf":
        raise ValueError(f'model {args.model} is not valid')
    _lib.require_device(rays, ts, semantics)
    unknown = [p for p in products if p not in PRODUCTS]
    if unknown:
        raise ValueError(f"unknown products {unknown}; the products are {PRODUCTS}")
    rays = rays.contiguous().float()
    N, dev = rays.shape[0], rays.device
    model = models["fine" if args.n_importance > 0 else "coarse"]
    if "beta" in products and not model.beta:
        raise ValueError("the beta product needs a model with the beta head")
    if (center is None) != (rng is None):
        raise ValueError("the altitude needs both center= and rng=")
    n_sem = model.num_sem_classes if model.sem else 0
    names = [p for p in products if p != "sem"]
    if "sem" in products and n_sem:
        names += ["sem_logits", "sem_class"]
    if center is not None and "depth" not in names:
        names.append("depth")
    begin = int(ray_offset) if out is not None else 0
    if out is not None:
        missing = [n for n in names if n not in out]
        if missing:
            raise ValueError(f"out= lacks the planes {missing}")
        planes = {n: out[n] for n in names}
    else:
        planes = {n: torch.empty((N,) + _PLANES[n][0](n_sem), dtype=_PLANES[n][1], device=dev) for n in names}
    S = (2 if args.guidedsample else 1) * args.n_samples + args.n_importance
    if chunk is None:
        chunk = max(1, max_points_per_call(model) // S)
    if clamp_near_far is None and args.guidedsample and N:
        clamp_near_far = rays[0, 6:8]
    src = current_random_source()
    keyed = getattr(src, "on_device", False)
    offset0 = src.ray_offset if keyed else 0
    try:
        with torch.no_grad():
            for i0 in range(0, N, int(chunk)):
                i1 = min(N, i0 + int(chunk))
                if keyed:
                    src.ray_offset = int(ray_offset) + i0
                    src.reset_step(-1)
                m, rows, z = _final_rows(models, args, rays[i0:i1], None if ts is None else ts[i0:i1],
                                         None if semantics is None else semantics[i0:i1], clamp_near_far)
                composite_products(m, rows, z, args.noise_std, planes, begin + i0)
    finally:
        if keyed:
            src.ray_offset = offset0
    res = dict(planes)
    if center is not None:
        from .dsm import _points
        lla, _ = _points(rays, planes["depth"][begin:begin + N], center, rng)
        res["alt"] = lla[:, 2]
    return res


def view_metrics(planes_or_rgb, target_rgb, sem_class=None, labels=None, num_classes=0, hw=None, ssim_layout="hwc",
                 window_size=3, lpips=None) -> dict:
    """The scores the validation step logs, of a rendered view against its targets, in one pass on
    the device and one device-to-host copy: ``mse``, ``psnr`` (metrics.py:197-207, summed in fp64)
    and — with ``labels`` (int64, any label outside [0, num_classes) ignored, −100 included) and
    the predicted ``sem_class`` — ``miou``, ``oa`` (metrics.py:218-246) and the (num_classes + 1,
    num_classes) ``confusion`` table [label, prediction], ignored labels in the last row.
    ``planes_or_rgb`` is the rgb image or ``render_image``'s dictionary (its ``sem_class`` is then
    the default).  The IoUs follow the reference's float32 arithmetic: a class whose union is 0
    contributes 0 to the mean, and ``oa`` divides by the number of labels, ignored ones included.

    With ``hw=(H, W)`` the view is also scored as an H x W image: ``ssim`` (metrics.py:210-215 with
    ``window_size``, evaluated in fp64: ``spnerf_amd.ssim``) and ``ssim_channels``, its mean per
    channel, on the same stream and in the same copy.  ``ssim_layout="hwc"`` reads the (H·W, 3)
    buffers as the interleaved image they are (eval.py:393); ``"chw"`` reads them as three H x W
    planes, which is what main.py:261's ``.view(1, 3, H, W)`` scores.  Without ``hw`` the result has
    neither key.

    With ``hw`` and ``lpips=`` an ``LpipsWeights`` the view is scored with LPIPS too (eval.py:128-135,
    399: AlexNet features, the images taken as [0, 1] and read in ``ssim_layout``):
    ``lpips`` and ``lpips_layers``, its five per-tap terms, again on the same stream and in the same
    copy.  Without the argument neither key nor any of its launches is there."""
    if isinstance(planes_or_rgb, dict):
        rgb = planes_or_rgb["rgb"]
        if sem_class is None and labels is not None:
            sem_class = planes_or_rgb.get("sem_class")
    else:
        rgb = planes_or_rgb
    _lib.require_device(rgb, target_rgb, sem_class, labels)
    C = int(num_classes)
    if not 0 <= C <= _view_lib.VIEW_MAX_CLASSES:
        raise ValueError(f"num_classes {C} outside [0, {_view_lib.VIEW_MAX_CLASSES}]")
    rgb = rgb.contiguous().float()
    tgt = target_rgb.to(rgb.device).contiguous().float()
    if rgb.numel() != tgt.numel() or rgb.numel() % 3 or rgb.numel() == 0:
        raise ValueError(f"rgb {tuple(rgb.shape)} and target {tuple(tgt.shape)} must be the same non-empty (..., 3) image")
    n = rgb.numel() // 3
    scored = labels is not None and C > 0
    if scored:
        if sem_class is None:
            raise ValueError("labels need the predicted sem_class")
        sem_class = sem_class.reshape(-1).to(torch.int32).contiguous()
        labels = labels.reshape(-1).to(torch.int64).contiguous()
        if sem_class.numel() != n or labels.numel() != n:
            raise ValueError(f"sem_class and labels must have one entry per ray ({n})")
    if hw is not None:
        H, W = int(hw[0]), int(hw[1])
        if H * W != n:
            raise ValueError(f"hw {tuple(hw)} is not the view's {n} rays")
        if ssim_layout not in ("hwc", "chw"):
            raise ValueError(f"ssim_layout {ssim_layout!r} is neither 'hwc' nor 'chw'")
    elif lpips is not None:
        raise ValueError("lpips= scores the view as an image: it needs hw=(H, W)")
    L = _view_lib.lib()
    nbytes = L.spnerf_view_metrics_workspace_bytes(n, C)
    if nbytes < 0:
        _lib.check(int(nbytes), "view_metrics_workspace_bytes")
    ws = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=rgb.device)
    vm_bytes = ctypes.sizeof(_view_lib.ViewMetricsResult)      # both result structs in one buffer: one copy
    lp_off = vm_bytes + image.RESULT_BYTES
    res = torch.zeros(vm_bytes + (image.RESULT_BYTES if hw is not None else 0) + (perceptual.RESULT_BYTES if lpips is not None else 0),
                      dtype=torch.uint8, device=rgb.device)
    _lib.check(L.spnerf_view_metrics(n, _lib.ptr(rgb), _lib.ptr(tgt), _lib.ptr(sem_class if scored else None),
                                     _lib.ptr(labels if scored else None), C, _lib.ptr(ws), _lib.ptr(res),
                                     _lib.stream_of(rgb)), "view_metrics")
    if hw is not None:
        image.launch_ssim(rgb, tgt, 3, H, W, (1, 3 * W, 3) if ssim_layout == "hwc" else (H * W, W, 1), window_size, 1.0,
                          res.data_ptr() + vm_bytes)
        if lpips is not None:
            perceptual.launch_lpips(rgb, tgt, H, W, (1, 3 * W, 3) if ssim_layout == "hwc" else (H * W, W, 1), True, lpips,
                                    res.data_ptr() + lp_off)
    raw = res.cpu().numpy().tobytes()                          # the one copy
    host = _view_lib.ViewMetricsResult.from_buffer_copy(raw)
    result = {"mse": host.mse, "psnr": host.psnr, "n": host.n, "miou": None, "oa": None, "correct": None, "confusion": None}
    if scored:
        table = np.array(host.table[:(C + 1) * C], np.int64).reshape(C + 1, C)
        result.update(confusion=table, correct=int(host.correct), **scores_from_table(table, n))
    if hw is not None:
        sr = _image_lib.SsimResult.from_buffer_copy(raw, vm_bytes)
        result.update(ssim=sr.ssim, ssim_channels=[sr.channel_mean[c] for c in range(3)])
        if lpips is not None:
            lr = _lpips_lib.LpipsResult.from_buffer_copy(raw, lp_off)
            result.update(lpips=lr.lpips, lpips_layers=list(lr.layer))
    return result


def scores_from_table(table: np.ndarray, n: int) -> dict:
    """miou and overall accuracy from the (C + 1, C) confusion table with the reference's rules
    and its float32 arithmetic (metrics.py:218-246): per class intersection / union as float32
    (0 where the union is 0), their float32 mean; correct / numel(gt) as float32."""
    C = table.shape[1]
    ious = []
    for c in range(C):
        inter = int(table[c, c])
        union = int(table[c, :].sum()) + int(table[:, c].sum()) - inter
        ious.append(np.float32(0.0) if union == 0 else np.float32(inter) / np.float32(union))
    miou = np.float32(sum(ious, np.float32(0.0))) / np.float32(C)
    oa = np.float32(int(np.trace(table[:C]))) / np.float32(n)
    return {"miou": float(miou), "oa": float(oa)}
