"""Relighting: a view under K sun directions from one pass over its geometry (csrc/relight.hip,
include/spnerf_amd_relight.h).

Of the per-point network (models/spnerf.py:332-356) only ``sun_v_net`` and ``sky_color`` read the sun
direction: σ, the albedo, the weights, the depth, β and the semantic logits are the same under every
sun.  ``sky_color`` is one 3-vector per direction, and ``sun_v_net.0`` splits into
``W0[:, :feat]·xyz_features + b0`` (once per point) plus ``W0[:, feat:]·d_k`` (one H-vector per
direction).  ``relight_image`` therefore runs the sampling passes, the final-pass forward and the
sun-independent composite once per chunk, and per direction only the rest of ``sun_v_net`` and the
three sums that read it.
"""
from __future__ import annotations

import contextlib
import ctypes

import numpy as np
import torch

from . import _lib, _relight_lib
from .spnerf import WeightPack, max_points_per_call
from .view import (_COMPOSITE_PLANES, _PLANES, _check_coarse_plane, _chunk_plan, _final_rows, _ray_chunks, composite_products,
                   render_image, sigma_noise_draw)

PRODUCTS = ("rgb", "sun", "sky", "depth", "albedo", "beta", "sem", "rgb_coarse")
# the planes that depend on the sun direction: a leading K, then render_image's shape
SUN_PLANES = {"rgb": (3,), "sun": (), "sky": (3,)}
# directions per pass over the geometry: spnerf_merge_samples gathers the guided pass's per-point
# values as rows of K floats beside the depths, 256 x (3 + K) floats of LDS
MAX_DIRS_PER_PASS = 32


class _FeatRows:
    """``run_mlp``'s stand-in for the final-pass forwards of one chunk: the forward with
    SPNERF_MLP_KEEP_FEAT, then ``spnerf_relight_sun`` on its workspace — the sun visibility of every
    point under every direction, (points, K) — after which the workspace is dropped."""

    def __init__(self, dir_ws, n_dirs):
        self.dir_ws, self.K, self.segs = dir_ws, n_dirs, []

    def __call__(self, model, rays, z, dir_offset, labels=None, temb=None, pack=None):
        _lib.require_device(rays, z, labels, temb)
        rays = rays.contiguous().float()
        z = z.contiguous().float()
        if labels is not None:
            labels = labels.reshape(-1).to(torch.int64).contiguous()
        if temb is not None:
            temb = temb.contiguous().float()
        B, S = z.shape
        if B * S > max_points_per_call(model):
            raise ValueError(f"chunk of {B} rays x {S} samples exceeds one MLP call ({max_points_per_call(model)} points)")
        cfg = ctypes.byref(model.cfg())
        L = _relight_lib.lib()
        flags = _lib.SPNERF_MLP_KEEP_FEAT
        wsb = L.spnerf_mlp_workspace_bytes(cfg, B, S, flags)
        if wsb < 0:
            _lib.check(-1, "workspace_bytes")
        ws = torch.empty(wsb // 4 + 1, dtype=torch.float32, device=rays.device)
        out = torch.empty(B * S, model.number_of_outputs, dtype=torch.float32, device=rays.device)
        if pack is None:
            pack = WeightPack(model, owned=False)
        _lib.check(L.spnerf_mlp_forward(cfg, _lib.ptr(pack.buf), _lib.ptr(rays), rays.stride(0), dir_offset, B, S,
                                        _lib.ptr(z), _lib.ptr(labels), _lib.ptr(temb), flags, _lib.ptr(ws), _lib.ptr(out),
                                        _lib.stream_of(rays)), "mlp_forward")
        sv = torch.empty(B * S, self.K, dtype=torch.float32, device=rays.device)
        _lib.check(L.spnerf_relight_sun(cfg, _lib.ptr(pack.buf), _lib.ptr(ws), B, S, _lib.ptr(self.dir_ws), self.K,
                                        _lib.ptr(sv), _lib.stream_of(rays)), "relight_sun")
        self.segs.append(sv)
        return out

    def merged(self, B, S, z_unsort):
        """The guided pass merged its two forwards' rows into the sorted depth order: so are theirs."""
        sv1, sv2 = self.segs
        sv = torch.empty(B * 2 * S, self.K, dtype=torch.float32, device=sv1.device)
        _lib.check(_lib.lib().spnerf_merge_samples(B, S, S, _lib.ptr(z_unsort), _lib.ptr(sv1), _lib.ptr(sv2), self.K,
                                                   _lib.ptr(sv), _lib.stream_of(sv1)), "merge_samples")
        self.segs = [sv]

    def sun_v(self):
        (sv,) = self.segs
        return sv


def _directions(sun_dirs):
    """(K, 3) float32 on the host, checked."""
    if isinstance(sun_dirs, torch.Tensor):
        shape = tuple(sun_dirs.shape)
    else:
        sun_dirs = np.asarray(sun_dirs)
        shape = sun_dirs.shape
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError(f"sun_dirs must be (K, 3), got {tuple(shape)}")
    if shape[0] == 0:
        raise ValueError("sun_dirs holds no direction (K = 0)")
    d = sun_dirs.detach().cpu().float() if isinstance(sun_dirs, torch.Tensor) else torch.from_numpy(
        np.ascontiguousarray(sun_dirs, dtype=np.float32))
    if not bool(torch.isfinite(d).all()):
        raise ValueError("sun_dirs holds a non-finite direction")
    return d.contiguous()


def relight_image(models, args, rays, sun_dirs, ts=None, semantics=None, *, chunk=None,
                  products=("rgb", "sun", "sky"), out=None, ray_offset=0, clamp_near_far=None) -> dict:
    """Render the N rays of a view under the K sun directions ``sun_dirs`` (K, 3) — rows as
    ``satellite.sun_direction`` returns them, every direction applied to every ray as
    ``get_sun_dirs`` does for an image; the rays' own columns 8:11 are ignored — from one pass over
    the view's geometry.

    Plane k equals what ``render_image`` returns for ``rays`` with columns 8:11 set to
    ``sun_dirs[k]``, with ``noise_std = 0`` or an on-device ``PhiloxRandom`` source (whose draws
    repeat per call).  The sun-dependent planes carry a leading K: "rgb" (K, N, 3), clamped to
    [0, 1], "sun" (K, N) = Σ w·sun_v and "sky" (K, N, 3) = Σ w·sky.  The sun-independent products —
    "depth", "albedo", "beta", "sem" (``sem_logits`` and ``sem_class``) and "rgb_coarse" — come back
    once, with ``render_image``'s shapes.  "sc" is refused: its march follows the sun direction
    through other points, so nothing can be shared.

    ``chunk``, ``out=`` / ``ray_offset`` (sun-dependent planes of a larger image are (K, N', ·),
    ray i at entry [k, ray_offset + i]), ``clamp_near_far``, the model choice (the fine one when
    ``args.n_importance > 0``), the sampling passes and the order of the random draws are
    ``render_image``'s: the geometry is drawn once and the K planes share the σ-noise draw.  With
    an on-device random source the result does not depend on the chunking; plane k depends neither
    on K nor on k's position in ``sun_dirs``.

    Per chunk the final-pass forward runs once with its heads in launches of their own, so that
    ``xyz_features`` stays in the workspace; ``spnerf_relight_sun`` evaluates the rest of
    ``sun_v_net`` for the K directions (bf16: one MFMA launch with the weights resident in LDS) and
    ``spnerf_relight_composite`` forms the K images.  More than 32 directions run in groups of 32,
    one pass over the geometry each (with a host-side random source and ``noise_std`` != 0 the
    groups then draw different geometry, as separate ``render_image`` calls would).

    The function works for every model ``render_image`` takes: at a width the relight launches do
    not run (above 256, or not a multiple of 64) it falls back to the definition — the
    sun-independent planes once, then ``render_image`` with the sun columns replaced, per
    direction."""
    if args.model != "sp-nerf":
        raise ValueError(f'model {args.model} is not valid')
    if "sc" in products:
        raise ValueError("the sc product cannot be relit from shared geometry: its march follows the sun direction "
                         "through other points (render_image renders it per direction)")
    unknown = [p for p in products if p not in PRODUCTS]
    if unknown:
        raise ValueError(f"unknown products {unknown}; the products are {PRODUCTS}")
    dirs = _directions(sun_dirs)
    K = dirs.shape[0]
    if "rgb_coarse" in products and not args.n_importance > 0:
        raise ValueError("the rgb_coarse product is the coarse image beside a fine model's: it needs n_importance > 0")
    _lib.require_device(rays, ts, semantics)
    rays = rays.contiguous().float()
    N, dev = rays.shape[0], rays.device
    model = models["fine" if args.n_importance > 0 else "coarse"]
    if "beta" in products and not model.beta:
        raise ValueError("the beta product needs a model with the beta head")
    n_sem = model.num_sem_classes if model.sem else 0
    sun_names = [p for p in products if p in SUN_PLANES]
    geo_names = [p for p in products if p not in SUN_PLANES and p != "sem"]
    if "sem" in products and n_sem:
        geo_names += ["sem_logits", "sem_class"]
    begin = int(ray_offset) if out is not None else 0
    if out is not None:
        missing = [n for n in sun_names + geo_names if n not in out]
        if missing:
            raise ValueError(f"out= lacks the planes {missing}")
        planes = {n: out[n] for n in sun_names + geo_names}
    else:
        planes = {n: torch.empty((K, N) + SUN_PLANES[n], dtype=torch.float32, device=dev) for n in sun_names}
        planes.update({n: torch.empty((N,) + _PLANES[n][0](n_sem), dtype=_PLANES[n][1], device=dev) for n in geo_names})
    plane_rays = None
    for n in sun_names:
        t = planes[n]
        if (not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 2 + len(SUN_PLANES[n]) or
                t.shape[0] != K or tuple(t.shape[2:]) != SUN_PLANES[n] or t.shape[1] < begin + N):
            raise ValueError(f"plane {n!r}: expected a contiguous float32 device tensor ({K}, N' >= {begin + N}, "
                             f"*{SUN_PLANES[n]}), got {t.dtype} {tuple(t.shape)} on {t.device}")
        if plane_rays is not None and t.shape[1] != plane_rays:
            raise ValueError("the sun-dependent planes of out= must hold the same number of rays")
        plane_rays = t.shape[1]
    geo = {n: planes[n] for n in geo_names}
    L = _relight_lib.lib()
    nbytes = L.spnerf_relight_workspace_bytes(ctypes.byref(model.cfg()), min(K, MAX_DIRS_PER_PASS))
    if nbytes == _lib.SPNERF_E_UNSUPPORTED:   # the definition
        _by_definition(models, args, rays, dirs.to(dev), ts, semantics, chunk, sun_names, geo_names, planes, out is not None,
                       int(ray_offset), clamp_near_far)
        return dict(planes)
    if nbytes < 0:
        _lib.check(int(nbytes), "relight_workspace_bytes")
    chunk, clamp_near_far = _chunk_plan(model, args, rays, chunk, clamp_near_far)
    dirs_dev = dirs.to(dev)
    for k0 in range(0, K, MAX_DIRS_PER_PASS):
        k1 = min(K, k0 + MAX_DIRS_PER_PASS)
        _relight_pass(models, args, model, rays, dirs_dev[k0:k1].contiguous(), ts, semantics, chunk,
                      {n: planes[n][k0:k1] for n in sun_names}, geo if k0 == 0 else {}, plane_rays, begin, int(ray_offset),
                      clamp_near_far)
    return dict(planes)


def _relight_pass(models, args, model, rays, dirs, ts, semantics, chunk, sun_planes, geo, plane_rays, begin, ray_offset,
                  clamp_near_far):
    """One pass over the geometry for up to MAX_DIRS_PER_PASS directions: render_image's chunk loop."""
    N, K, dev = rays.shape[0], dirs.shape[0], rays.device
    L = _relight_lib.lib()
    cfg = ctypes.byref(model.cfg())
    composited = {n: t for n, t in geo.items() if n in _COMPOSITE_PLANES}
    coarse = geo.get("rgb_coarse")
    _check_coarse_plane(coarse, begin + N)
    with contextlib.closing(_ray_chunks(N, chunk, ray_offset)) as chunks:
        with torch.no_grad():
            # the terms of the directions alone, from the weights every chunk's forward reads
            pack = WeightPack(model, owned=False)
            dir_ws = torch.empty(int(L.spnerf_relight_workspace_bytes(cfg, K)), dtype=torch.uint8, device=dev)
            _lib.check(L.spnerf_relight_directions(cfg, _lib.ptr(pack.buf), _lib.ptr(dirs), K, _lib.ptr(dir_ws),
                                                   _lib.stream_of(dirs)), "relight_directions")
            for i0, i1 in chunks:
                ts_c = None if ts is None else ts[i0:i1]
                sem_c = None if semantics is None else semantics[i0:i1]
                fwd = _FeatRows(dir_ws, K)
                m, rows, z = _final_rows(models, args, rays[i0:i1], ts_c, sem_c, clamp_near_far,
                                         None if coarse is None else coarse[begin + i0:begin + i1], rows_mlp=fwd)
                z = z.contiguous()
                draw = sigma_noise_draw(z, args.noise_std)   # one draw: the geometry's and the K images'
                key, keep, noise = draw
                if composited:
                    composite_products(m, rows, z, args.noise_std, composited, begin + i0, draw=draw)
                if sun_planes:
                    B, Sz = z.shape
                    _lib.check(L.spnerf_relight_composite(
                        B, Sz, _lib.ptr(z), _lib.ptr(rows), rows.shape[1], _lib.ptr(noise), float(args.noise_std),
                        _lib.rng_ref(key if args.noise_std != 0 else None), K, _lib.ptr(fwd.sun_v()), _lib.ptr(dir_ws),
                        begin + i0, plane_rays, _lib.ptr(sun_planes.get("rgb")), _lib.ptr(sun_planes.get("sun")),
                        _lib.ptr(sun_planes.get("sky")), _lib.stream_of(rows)), "relight_composite")


def _by_definition(models, args, rays, dirs, ts, semantics, chunk, sun_names, geo_names, planes, into_out, ray_offset,
                   clamp_near_far):
    """The fallback: the sun-independent planes once, then render_image per direction with the sun
    columns replaced."""
    def render(r, names, dst):
        prod = tuple(dict.fromkeys("sem" if n.startswith("sem_") else n for n in names))
        kw = dict(chunk=chunk, products=prod, ray_offset=ray_offset, clamp_near_far=clamp_near_far)
        if into_out:
            render_image(models, args, r, ts, semantics, out=dst, **kw)
        else:   # planes of this call's own: the N rays from entry 0, whatever ray_offset keys the draws
            res = render_image(models, args, r, ts, semantics, **kw)
            for n in names:
                dst[n].copy_(res[n])

    if geo_names:
        render(rays, geo_names, {n: planes[n] for n in geo_names})
    if not sun_names:
        return
    lit = rays.clone()
    for k in range(dirs.shape[0]):
        lit[:, 8:11] = dirs[k]
        render(lit, sun_names, {n: planes[n][k] for n in sun_names})
