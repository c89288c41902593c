"""Whole views: what a user does with a trained model after each epoch — the reference's
``NeRF_pl.forward(mode='test')`` + ``validation_step`` (main.py:59-89, 188-299) and
``save_nerf_output_to_images`` (eval.py:27-101) — on the GPU (csrc/view.hip,
include/spnerf_amd_view.h).

``render_image`` renders N rays chunk by chunk into image planes left on the device: the final
pass's MLP rows go to ``k_composite_products``, which writes per-ray values only (rgb, depth, the
shadow / albedo / sky / uncertainty sums of eval.py:76-101, the mean semantic logits and their
argmax) — the per-sample dictionary of ``render_rays`` is never materialised.  ``view_metrics``
scores a rendered view against its targets in one pass (psnr, miou, overall accuracy of
modules/metrics.py:206-246) with one device-to-host copy.  With the "sc" product the solar-correction
march of every chunk is reduced to two numbers per ray (csrc/val.hip, include/spnerf_amd_val.h) and
``view_loss`` forms the loss the validation step logs (modules/metrics.py:27-65) from the planes.
"""
from __future__ import annotations

import contextlib
import ctypes

import numpy as np
import torch

from . import _image_lib, _lib, _lpips_lib, _val_lib, _view_lib, image, perceptual
from .rendering import _coarse_rows, _fine_rows
from .rng import current_random_source, device_key
from .spnerf import composite, max_points_per_call, run_mlp

PRODUCTS = ("rgb", "depth", "sun", "albedo", "sky", "beta", "sem", "sc", "rgb_coarse")
# plane name -> (trailing shape given the class count, dtype)
_PLANES = {"rgb": (lambda c: (3,), torch.float32), "depth": (lambda c: (), torch.float32),
           "sun": (lambda c: (), torch.float32), "albedo": (lambda c: (3,), torch.float32),
           "sky": (lambda c: (3,), torch.float32), "beta": (lambda c: (), torch.float32),
           "sem_logits": (lambda c: (c,), torch.float32), "sem_class": (lambda c: (), torch.int32),
           "sc_term2": (lambda c: (), torch.float32), "sc_term3": (lambda c: (), torch.float32),
           "rgb_coarse": (lambda c: (3,), torch.float32)}
# the planes spnerf_view_composite_products writes (spnerf_view_planes); the others have launches of their own
_COMPOSITE_PLANES = ("rgb", "depth", "sun", "albedo", "sky", "beta", "sem_logits", "sem_class")


def sigma_noise_draw(z, noise_std):
    """The σ-noise draw the composite of a pass takes (spnerf.py:122): (key, keep-alive, noise) —
    an on-device key, or a host-side draw (None when ``noise_std`` is 0)."""
    B, S = z.shape
    key, keep = device_key(z.device)   # on-device σ noise: a slot per inference call, drawn or not
    noise = None if key is not None else current_random_source().noise((B, S), z.device, noise_std)
    if noise is not None:
        noise = noise.contiguous().float()
    return key, keep, noise


def composite_products(model, out, z, noise_std, planes: dict, ray_begin: int = 0, draw=None) -> None:
    """``spnerf_view_composite_products`` on one chunk's final-pass rows: ray r of the chunk goes
    to entry ``ray_begin + r`` of every plane in ``planes`` (name -> contiguous device tensor; the
    names of ``spnerf_view_planes``, a missing name is a skipped plane).  Takes the σ-noise draw the
    composite of that pass takes (spnerf.py:122), or ``draw`` (``sigma_noise_draw``'s result: a
    draw shared with another launch over the same rows)."""
    B, S = z.shape
    key, keep, noise = sigma_noise_draw(z, noise_std) if draw is None else draw
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


def _chunk_plan(model, args, rays, chunk, clamp_near_far):
    """(rays per chunk, guided-sampling clamp) of a whole-view loop: the defaults of ``render_image``."""
    S = (2 if args.guidedsample else 1) * args.n_samples + args.n_importance
    if chunk is None:
        chunk = max(1, max_points_per_call(model) // S)
    if clamp_near_far is None and args.guidedsample and rays.shape[0]:
        clamp_near_far = rays[0, 6:8]
    return int(chunk), clamp_near_far


def _check_coarse_plane(coarse, n_rays):
    if coarse is not None and (not coarse.is_cuda or coarse.dtype != torch.float32 or not coarse.is_contiguous() or
                               tuple(coarse.shape[1:]) != (3,) or coarse.shape[0] < n_rays):
        raise ValueError(f"plane 'rgb_coarse': expected a contiguous float32 device tensor of at least {n_rays} x 3, got "
                         f"{coarse.dtype} {tuple(coarse.shape)} on {coarse.device}")


def _ray_chunks(N, chunk, ray_offset):
    """The (i0, i1) of a whole-view loop over N rays.  With an on-device random source every chunk
    draws as step 0 of the global ray ids ``ray_offset + i``; the source's own offset is put back
    when the generator is closed (use it under ``contextlib.closing``)."""
    src = current_random_source()
    keyed = getattr(src, "on_device", False)
    offset0 = src.ray_offset if keyed else 0
    try:
        for i0 in range(0, N, int(chunk)):
            if keyed:
                src.ray_offset = int(ray_offset) + i0
                src.reset_step(-1)
            yield i0, min(N, i0 + int(chunk))
    finally:
        if keyed:
            src.ray_offset = offset0


def _final_rows(models, args, rays, ts, semantics, clamp_near_far=None, rgb_coarse=None, solar=False, rows_mlp=None):
    """(model, out, z_vals) of the pass whose composite is the image: render_rays(mode='test')
    up to that composite, the solar march (``sc_lambda``) left to the caller.  ``rgb_coarse`` (with
    a fine model): a (B, 3) slice of the coarse image's plane, filled here.  With ``solar`` a
    fourth value follows: (weight pack, semantics or None, t-embedding or None) of the model, what
    the solar pass at the same depths needs.  ``rows_mlp``: what runs the forwards of the
    returned rows in ``run_mlp``'s place (relight.py)."""
    model, pk, sem, rays_t, out, z_vals, _ = _coarse_rows(models, args, rays, ts, semantics, "test", None, None, None,
                                                                 clamp_near_far,
                                                                 None if args.n_importance > 0 else rows_mlp)
    if args.n_importance > 0:
        if rgb_coarse is None:
            # the coarse weights alone: the σ-only composite takes the same noise draw and marches alike
            _, _, w, _, _ = composite(model, out, z_vals, args.noise_std, weights_only=True)
        else:   # the coarse image as well: the full composite, the same draw, the same march and weights
            rgb, _, w, _, _ = composite(model, out, z_vals, args.noise_std)
            rgb_coarse.copy_(rgb)
        model, pk, sem, rays_t, out, z_vals = _fine_rows(models, args, rays, ts, z_vals, w, semantics, rows_mlp)
    if solar:
        return model, out, z_vals, (pk, sem, rays_t)
    return model, out, z_vals


def solar_terms(model, rays, z, noise_std, pack, semantics, rays_t, term2, term3, ray_begin: int = 0) -> None:
    """The solar pass of one chunk at the final depths ``z`` (rendering.py:171-177: the sun-only
    forward along the sun direction, what ``inference_rays(mode="sun")`` launches) reduced by
    ``spnerf_val_solar_terms`` to ``term2[ray_begin + r]`` = Σ (T − sun)² and ``term3[ray_begin + r]``
    = 1 − Σ w·sun (metrics.py:20-21).  Takes the σ-noise draw the composite of that pass takes."""
    B, S = z.shape
    out = run_mlp(model, rays, z, 8, semantics if model.sem else None, rays_t if model.beta else None, sun_only=True,
                  pack=pack)
    key, keep = device_key(z.device)   # on-device σ noise: a slot per inference call, drawn or not
    noise = None if key is not None else current_random_source().noise((B, S), z.device, noise_std)
    if noise is not None:
        noise = noise.contiguous().float()
    z = z.contiguous()
    for name, t in (("sc_term2", term2), ("sc_term3", term3)):
        if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 1:
            raise ValueError(f"plane {name!r}: expected a contiguous float32 device tensor (N,), got {t.dtype} "
                             f"{tuple(t.shape)} on {t.device}")
        if t.shape[0] < ray_begin + B:
            raise ValueError(f"plane {name!r} has {t.shape[0]} rays, the chunk ends at ray {ray_begin + B}")
    _lib.check(_val_lib.lib().spnerf_val_solar_terms(
        B, S, _lib.ptr(z), _lib.ptr(out), out.shape[1], 4, _lib.ptr(noise), float(noise_std), int(ray_begin),
        _lib.ptr(term2), _lib.ptr(term3), _lib.rng_ref(key if noise_std != 0 else None), _lib.stream_of(out)),
        "val_solar_terms")


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

    "sc" (``args.sc_lambda > 0``, no fine model) adds the solar-correction march of
    rendering.py:171-177 after every chunk's composite, reduced to ``sc_term2`` (N) = Σ (T − sun)² and
    ``sc_term3`` (N) = 1 − Σ w·sun (metrics.py:20-21); the draws are then those of
    ``render_rays(mode='test')`` at the args' ``sc_lambda``: the solar pass's σ noise right after
    the main pass's.  "rgb_coarse" (N, 3), with a fine model, is the coarse model's image: the
    composite that places the importance samples writes it, with the draws it takes anyway.
    ``view_loss`` scores these planes with the loss the validation step logs.

    Guided sampling clamps its depths to one ray's near / far (rendering.py:95): here that of the
    call's first ray for every chunk, as ``render_rays`` on all N rays at once does, or
    ``clamp_near_far`` (an extension beyond the reference's arguments, as in ``render_rays``: a
    device tensor of 2 floats; a shard passes the whole view's first ray).

    With an on-device random source (``PhiloxRandom``) every chunk draws as step 0 of the global
    ray ids ``ray_offset + i``, so the image does not depend on the chunking or the sharding."""
    if args.model != "sp-nerf":
        raise ValueError(f'model {args.model} is not valid')
    solar = "sc" in products
    if solar and not args.sc_lambda > 0:
        raise ValueError("the sc product is the solar-correction march: it needs args.sc_lambda > 0")
    if solar and args.n_importance > 0:
        raise ValueError("the sc product with n_importance > 0: the reference's own dictionary loses its *_coarse keys "
                         "there (rendering.py:207 overwrites result_), so its validation step raises KeyError")
    if "rgb_coarse" in products and not args.n_importance > 0:
        raise ValueError("the rgb_coarse product is the coarse image beside a fine model's: it needs n_importance > 0")
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
    n_sem =model.num_sem_classes if model.sem else 0
    names = [p for p in products if p not in ("sem", "sc")]
    if "sem" in products and n_sem:
        names += ["sem_logits", "sem_class"]
    if solar:
        names += ["sc_term2", "sc_term3"]
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
    chunk, clamp_near_far = _chunk_plan(model, args, rays, chunk, clamp_near_far)
    composited = {n: t for n, t in planes.items() if n in _COMPOSITE_PLANES}
    coarse = planes.get("rgb_coarse")
    _check_coarse_plane(coarse, begin + N)
    with contextlib.closing(_ray_chunks(N, chunk, ray_offset)) as chunks:
        with torch.no_grad():
            for i0, i1 in chunks:
                ts_c = None if ts is None else ts[i0:i1]
                sem_c = None if semantics is None else semantics[i0:i1]
                m, rows, z, *extra = _final_rows(models, args, rays[i0:i1], ts_c, sem_c, clamp_near_far,
                                                 None if coarse is None else coarse[begin + i0:begin + i1], solar)
                composite_products(m, rows, z, args.noise_std, composited, begin + i0)
                if solar:   # its σ-noise draw comes right after the main pass's (rendering.py:169-173)
                    pk, sem, rays_t = extra[0]
                    solar_terms(m, rays[i0:i1], z, args.noise_std, pk, sem, rays_t, planes["sc_term2"], planes["sc_term3"],
                                begin + i0)
    res = dict(planes)
    if center is not None:
        from .dsm import _points
        lla, _ = _points(rays, planes["depth"][begin:begin + N], center, rng)
        res["alt"] = lla[:, 2]
    return res


def _loss_inputs(planes, tgt, lambda_sc, beta, beta_min):
    """The planes ``spnerf_val_loss`` reads for that loss, checked: (rgb, rgb_coarse or None, beta
    or None, term2 or None, term3 or None), contiguous fp32 on the target's device."""
    if not isinstance(planes, dict):
        raise ValueError("the validation loss reads render_image's dictionary of planes, not a bare rgb image")
    n = tgt.numel() // 3

    def plane(name, per_ray):
        if name not in planes:
            raise ValueError(f"the validation loss needs the {name!r} plane (render_image's products)")
        t = planes[name]
        _lib.require_device(t)
        t = t.contiguous().float()
        if t.numel() != n * per_ray or t.device != tgt.device:
            raise ValueError(f"plane {name!r} {tuple(t.shape)} on {t.device} is not the target's {n} rays on {tgt.device}")
        return t

    rgb = plane("rgb", 3)
    coarse = plane("rgb_coarse", 3) if "rgb_coarse" in planes else None
    if beta and coarse is not None:
        raise ValueError("beta=True with a fine model: the reference multiplies weights_fine by beta_coarse per sample "
                         "(metrics.py:11), which no plane holds")
    if beta and not beta_min > 0:
        raise ValueError(f"beta_min {beta_min} must be positive")
    b = plane("beta", 1) if beta else None
    solar = lambda_sc > 0
    if solar and coarse is not None:
        raise ValueError("lambda_sc > 0 with a fine model: the reference's validation step raises KeyError there")
    return rgb, coarse, b, plane("sc_term2", 1) if solar else None, plane("sc_term3", 1) if solar else None


def _launch_loss(inputs, tgt, lambda_sc, beta_min, result_ptr):
    """``spnerf_val_loss`` on the target's stream into a device result; returns what must stay alive."""
    rgb, coarse, b, t2, t3 = inputs
    n = tgt.numel() // 3
    L = _val_lib.lib()
    nbytes = L.spnerf_val_loss_workspace_bytes(n)
    if nbytes < 0:
        _lib.check(int(nbytes), "val_loss_workspace_bytes")
    ws = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=tgt.device)
    _lib.check(L.spnerf_val_loss(n, _lib.ptr(rgb), _lib.ptr(tgt), _lib.ptr(coarse), _lib.ptr(b), _lib.ptr(t2), _lib.ptr(t3),
                                 float(lambda_sc), float(beta_min), _lib.ptr(ws), result_ptr, _lib.stream_of(tgt)), "val_loss")
    return ws


def _loss_terms(host, inputs) -> dict:
    """The reference's ``loss_dict`` and ``loss`` (metrics.py:27-65) from a host spnerf_val_loss_result."""
    _, coarse, b, t2, _ = inputs
    out = {"loss": host.loss}
    if coarse is not None:
        out.update(coarse_color=host.color_coarse, fine_color=host.color)
    else:
        out["coarse_color"] = host.color
    if b is not None:
        out["coarse_logbeta"] = host.logbeta
    if t2 is not None:
        out.update(coarse_sc_term2=host.sc_term2, coarse_sc_term3=host.sc_term3)
    return out


def view_loss(planes, target_rgb, lambda_sc, beta=False, beta_min=0.05) -> dict:
    """The loss the validation step logs (main.py:205,289-297), of a rendered view's planes against
    its target image: ``SNerfLoss(lambda_sc)`` or, with ``beta=True``, ``SatNerfLoss(lambda_sc)``
    (metrics.py:27-65), summed in fp64 in one pass on the device (``spnerf_val_loss``), with one
    device-to-host copy and no synchronisation before it.  Returns ``loss`` and the reference's
    ``loss_dict`` keys: ``coarse_color``; with ``lambda_sc > 0`` ``coarse_sc_term2`` and
    ``coarse_sc_term3`` (the "sc" product's planes); with ``beta=True`` ``coarse_logbeta`` (the
    "beta" plane: Σ w·β); with a fine model — the planes hold "rgb_coarse" — ``rgb`` is the fine
    colour and the result has ``fine_color`` too.  ``beta=True`` with a fine model raises
    ``ValueError``: the reference multiplies ``weights_fine`` by ``beta_coarse`` per sample there,
    which no plane holds."""
    _lib.require_device(target_rgb)
    tgt = target_rgb.contiguous().float()
    if tgt.numel() % 3 or tgt.numel() == 0:
        raise ValueError(f"target {tuple(tgt.shape)} must be a non-empty (..., 3) image")
    inputs = _loss_inputs(planes, tgt, float(lambda_sc), bool(beta), float(beta_min))
    res = torch.zeros(_val_lib.RESULT_BYTES, dtype=torch.uint8, device=tgt.device)
    keep = _launch_loss(inputs, tgt, lambda_sc, beta_min, _lib.ptr(res))   # noqa: F841 (alive until the copy)
    host = _val_lib.ValLossResult.from_buffer_copy(res.cpu().numpy().tobytes())   # the one copy
    return _loss_terms(host, inputs)


def view_metrics(planes_or_rgb, target_rgb, sem_class=None, labels=None, num_classes=0, hw=None, ssim_layout="hwc",
                 window_size=3, lpips=None, loss=None) -> dict:
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
    copy.  Without the argument neither key nor any of its launches is there.

    With ``loss=dict(lambda_sc=..., beta=..., beta_min=...)`` (``planes_or_rgb`` the dictionary of
    planes) the keys of ``view_loss`` are added, from the same stream and the same copy.  Without
    the argument neither a key nor a launch of it is there."""
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
    loss_off = vm_bytes + (image.RESULT_BYTES if hw is not None else 0) + (perceptual.RESULT_BYTES if lpips is not None else 0)
    res = torch.zeros(loss_off + (_val_lib.RESULT_BYTES if loss is not None else 0), dtype=torch.uint8, device=rgb.device)
    if loss is not None:
        lkw = dict(lambda_sc=float(loss["lambda_sc"]), beta_min=float(loss.get("beta_min", 0.05)))
        unknown = sorted(set(loss) - {"lambda_sc", "beta", "beta_min"})
        if unknown:
            raise ValueError(f"loss= takes lambda_sc, beta and beta_min, not {unknown}")
        loss_inputs = _loss_inputs(planes_or_rgb, tgt, lkw["lambda_sc"], bool(loss.get("beta", False)), lkw["beta_min"])
        loss_keep = _launch_loss(loss_inputs, tgt, lkw["lambda_sc"], lkw["beta_min"], res.data_ptr() + loss_off)  # noqa: F841
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
    if loss is not None:
        result.update(_loss_terms(_val_lib.ValLossResult.from_buffer_copy(raw, loss_off), loss_inputs))
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
