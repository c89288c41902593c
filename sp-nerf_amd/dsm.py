"""DSM extraction from a rendered depth image: drop-ins for
``SatelliteSceneDataset.get_latlonalt_from_nerf_prediction`` / ``get_dsm_from_nerf_prediction``
(datasets/satellite_scene.py:475-568) and the MAE of ``utils.compute_mae_and_save_dsm_diff``
(modules/utils.py:142-245), on the GPU (csrc/dsm.hip, fp64).

The reference converts the point cloud on the CPU (numpy + pyproj) and rasterises it with
plyflatten; here the lat/lon/alt, UTM and rasterisation run as three kernel launches over the
render's rays, and only the DSM (a few MB) comes back to the host.  pyproj and plyflatten are
not installed here: the UTM projection is the transverse-Mercator algorithm PROJ's utm uses
(Krüger series) and the rasteriser plyflatten's documented behaviour — both parity unpinned
(oracle/dsm_ref.py); lat/lon/alt is pinned to the reference's own function.  The MAE follows the
reference's no-dsmr branch (registration by the mean Z offset, utils.py:197-201) by default and,
with ``register="ncc"``, the branch the reference runs when its modules/dsmr.py imports: the
integer shift that maximises the normalised cross correlation over a 2x pyramid, then the Z
offset (``compute_shift`` / ``apply_shift`` / ``dsm_pointwise_diff`` below, csrc/dsm_register.hip).
The GDAL crop is the array window of the ROI grid.
"""
from __future__ import annotations

import ctypes
import math
import os

import numpy as np
import torch

from . import _eval_lib, _lib

_ZONE_LETTERS = "CDEFGHJKLMNPQRSTUVWXX"


def utm_zone(lat: float, lon: float):
    """utm.latlon_to_zone_number / latitude_to_zone_letter (the reference's zone of the first
    point, utils.py:133-134)."""
    if 56 <= lat < 64 and 3 <= lon < 12:
        n = 32
    elif 72 <= lat <= 84 and lon >= 0 and lon < 42:
        n = 31 if lon < 9 else 33 if lon < 21 else 35 if lon < 33 else 37
    else:
        n = int((lon + 180) / 6) + 1
    letter = _ZONE_LETTERS[int(lat + 80) >> 3] if -80 <= lat <= 84 else None
    return n, letter


def _points(rays: torch.Tensor, depth: torch.Tensor, center, rng, zone=1, south=False, lla=True, ena=False):
    _lib.require_device(rays, depth)
    rays = rays.contiguous().float()
    depth = depth.reshape(-1).contiguous().float()
    n = rays.shape[0]
    if depth.shape[0] != n or rays.dim() != 2 or rays.shape[1] < 6:
        raise ValueError("rays must be (n, >=6) and depth (n,) or (n, 1)")
    cen = (ctypes.c_double * 3)(*[float(v) for v in np.asarray(center, np.float32).reshape(3)])
    out_lla = torch.empty(n, 3, dtype=torch.float64, device=rays.device) if lla else None
    out_ena = torch.empty(n, 3, dtype=torch.float64, device=rays.device) if ena else None
    _lib.check(_lib.lib().spnerf_dsm_points(_lib.ptr(rays), rays.shape[1], n, _lib.ptr(depth), cen,
                                           float(np.float32(rng)), int(zone), 1 if south else 0, _lib.ptr(out_lla),
                                           _lib.ptr(out_ena), _lib.stream_of(rays)), "dsm_points")
    return out_lla, out_ena


def get_latlonalt_from_nerf_prediction(rays: torch.Tensor, depth: torch.Tensor, center, rng):
    """satellite_scene.py:475-505: numpy (lats, lons, alts) of the predicted points.  ``center``
    and ``rng`` are the scene's normalisation (SatelliteSceneDataset.center / .range)."""
    lla, _ = _points(rays, depth, center, rng)
    lla = lla.cpu().numpy()
    return lla[:, 0], lla[:, 1], lla[:, 2]


def get_dsm_from_nerf_prediction(rays: torch.Tensor, depth: torch.Tensor, center, rng, dsm_path=None, roi_txt=None,
                                 resolution=0.5, radius=1, sigma=float("inf")):
    """satellite_scene.py:507-568: the (ysize, xsize, 1) float64 DSM of the predicted points,
    NaN where no point lands.  ``roi_txt`` (the lidar ROI file: xoff, yoff, size, resolution)
    fixes the grid like the reference; otherwise the cloud's bounds at ``resolution``.  With
    ``dsm_path`` the DSM is written as a float32 TIFF (PIL; no GeoTIFF tags — rasterio is not
    installed) with its grid in ``<dsm_path>.txt`` (xoff, yoff-of-the-top-row, xsize, ysize,
    resolution, UTM zone)."""
    lla, _ = _points(rays[:1], depth.reshape(-1)[:1], center, rng)
    lat0, lon0 = float(lla[0, 0]), float(lla[0, 1])
    zone, letter = utm_zone(lat0, lon0)
    # the reference asks pyproj for "+proj=utm +zone=<n><letter>" without +south; PROJ reads the
    # zone number only, so the northern false northing applies everywhere (kept)
    _, ena = _points(rays, depth, center, rng, zone=zone, south=False, lla=False, ena=True)
    if roi_txt is not None:
        meta = np.loadtxt(roi_txt)
        xoff, yoff = float(meta[0]), float(meta[1])
        xsize = ysize = int(meta[2])
        res = float(meta[3])
        yoff += ysize * res
    else:
        lo = ena[:, :2].amin(0).cpu().numpy()
        hi = ena[:, :2].amax(0).cpu().numpy()
        res = float(resolution)
        xoff = math.floor(lo[0] / res) * res
        xsize = int(1 + math.floor((hi[0] - xoff) / res))
        yoff = math.ceil(hi[1] / res) * res
        ysize = int(1 - math.floor((lo[1] - yoff) / res))
    dsm = rasterize(ena, xoff, yoff, res, xsize, ysize, radius=radius, sigma=sigma)
    out = dsm.cpu().numpy()[:, :, None]
    if dsm_path is not None:
        from PIL import Image
        os.makedirs(os.path.dirname(dsm_path) or ".", exist_ok=True)
        Image.fromarray(out[:, :, 0].astype(np.float32), mode="F").save(dsm_path)
        with open(dsm_path + ".txt", "w") as f:
            f.write(f"{xoff:.6f}\n{yoff:.6f}\n{xsize}\n{ysize}\n{res:.6f}\n{zone}{letter or ''}\n")
    return out


def rasterize(ena: torch.Tensor, xoff, yoff, resolution, xsize, ysize, radius=1, sigma=float("inf")) -> torch.Tensor:
    """plyflatten(cloud, xoff, yoff, resolution, xsize, ysize, radius, sigma) on the device:
    ``ena`` (n, 3) float64 easting / northing / altitude -> (ysize, xsize) float64."""
    _lib.require_device(ena)
    ena = ena.contiguous().double()
    acc = torch.empty(2, ysize, xsize, dtype=torch.float64, device=ena.device)
    dsm = torch.empty(ysize, xsize, dtype=torch.float64, device=ena.device)
    _lib.check(_lib.lib().spnerf_dsm_rasterize(_lib.ptr(ena), ena.shape[0], float(xoff), float(yoff), float(resolution),
                                              int(xsize), int(ysize), int(radius), float(sigma), _lib.ptr(acc),
                                              _lib.ptr(dsm), _lib.stream_of(ena)), "dsm_rasterize")
    return dsm


def dsm_mae(pred_dsm, gt_dsm, register="z") -> float:
    """The MAE of utils.compute_mae_and_save_dsm_diff on arrays already on the ground truth's
    grid.  ``register="z"``: the reference's no-dsmr branch (utils.py:197-201: shift by the mean Z
    offset), on the host.  ``register="ncc"``: the branch it runs with modules/dsmr.py —
    ``compute_shift(gt, pred, scaling=False)``, ``apply_shift``, nanmean |.| — on the device, the
    sums coming from the fused shift-and-error kernel (one device-to-host copy)."""
    if register == "z":
        pred = np.asarray(pred_dsm, np.float64).reshape(np.asarray(gt_dsm).shape)
        gt = np.asarray(gt_dsm, np.float64)
        rp = pred + np.nanmean(gt - pred)
        return float(np.nanmean(np.abs(rp - gt)))
    if register != "ncc":
        raise ValueError(f"register must be 'z' or 'ncc', got {register!r}")
    gt, pred = _image_pair(gt_dsm, pred_dsm)
    reg = _register(gt, pred, 5, (0, 0))
    sums = torch.empty(_eval_lib.DSM_SUMS_DOUBLES, dtype=torch.float64, device=gt.device)
    _apply(pred, reg=reg.device_result, ref=gt, sums=sums)
    total, count = sums[:2].cpu().tolist()
    return total / count if count else float("nan")


# ---- DSM registration (modules/dsmr.py) on the device: csrc/dsm_register.hip ------------------

def _image(x, device):
    """An array, a device tensor or the path of a float TIFF -> (H, W) float64 device tensor."""
    if isinstance(x, (str, os.PathLike)):
        from PIL import Image
        with Image.open(x) as im:
            x = np.asarray(im, np.float64)
    if isinstance(x, torch.Tensor):
        t = x
    else:
        t = torch.as_tensor(np.ascontiguousarray(np.asarray(x, np.float64))).to(device)
    _lib.require_device(t)
    if t.dim() == 3 and 1 in (t.shape[0], t.shape[-1]):     # (1, H, W) rasters, (H, W, 1) DSMs
        t = t.reshape(t.shape[1:] if t.shape[0] == 1 else t.shape[:2])
    if t.dim() != 2 or t.numel() == 0:
        raise ValueError(f"a DSM is one (H, W) image, got shape {tuple(t.shape)}")
    return t.to(torch.float64).contiguous()


def _image_pair(a, b):
    dev = next((t.device for t in (a, b) if isinstance(t, torch.Tensor) and t.is_cuda), None)
    if dev is None:
        # CPU tensors are refused before anything looks for a device to move arrays to
        _lib.require_device(*[t for t in (a, b) if isinstance(t, torch.Tensor)])
        dev = torch.device("cuda", torch.cuda.current_device())
    a, b = _image(a, dev), _image(b, dev)
    if a.shape != b.shape:
        raise ValueError(f"DSMs of unequal shape: {tuple(a.shape)} and {tuple(b.shape)}")
    if a.device != b.device:
        raise ValueError(f"DSMs on different devices: {a.device} and {b.device}")
    return a, b


def pyramid_levels(h: int, w: int) -> int:
    """Levels of recursive_ncc's pyramid: 1 + the 2x reductions made while min(H, W) > 100."""
    n = 1
    while min(h, w) > 100:
        h, w = (h + 1) // 2, (w + 1) // 2
        n += 1
    return n


class Registration:
    """Result of ``register_dsm``: reading ``dx``, ``dy``, the moments (``muu``, ``muv``, ``sigu``,
    ``sigv``, ``xcorr``: mean_std at the shift) or ``count`` makes the one device-to-host copy.
    ``tables`` (if asked for): device tensor (levels, (2·irange+1)² + 2), finest level first —
    each level's correlations in scan order (y outer, x inner), then its chosen dx, dy."""

    def __init__(self, device_result, tables, irange):
        self.device_result, self.tables, self.irange = device_result, tables, irange
        self._host = None

    def __getattr__(self, name):
        if name in ("dx", "dy", "muu", "muv", "sigu", "sigv", "xcorr", "count"):
            if self._host is None:
                self._host = _eval_lib.DsmShift.from_buffer_copy(self.device_result.cpu().numpy().tobytes())
            return getattr(self._host, name)
        raise AttributeError(name)

    def transform(self, scaling=True):
        """compute_shift's (dx, dy, a, b)."""
        with np.errstate(invalid="ignore", divide="ignore"):
            a = float(np.float64(self.sigu) / np.float64(self.sigv)) if scaling else 1.0
        return self.dx, self.dy, a, self.muu - self.muv * a


def _register(u, v, irange, init, tables=False):
    h, w = u.shape
    L = _eval_lib.lib()
    nbytes = L.spnerf_eval_dsm_register_workspace_bytes(h, w, int(irange))
    if nbytes < 0:
        _lib.check(int(nbytes), "dsm_register_workspace_bytes")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=u.device)
    res = torch.empty(ctypes.sizeof(_eval_lib.DsmShift), dtype=torch.uint8, device=u.device)
    tab = None
    if tables:
        tab = torch.empty(pyramid_levels(h, w), (2 * irange + 1) ** 2 + 2, dtype=torch.float64, device=u.device)
    _lib.check(L.spnerf_eval_dsm_register(_lib.ptr(u), _lib.ptr(v), h, w, int(irange), int(init[0]), int(init[1]),
                                          _lib.ptr(ws), _lib.ptr(tab), _lib.ptr(res), _lib.stream_of(u)), "dsm_register")
    return Registration(res, tab, irange)


def _apply(v, dx=0, dy=0, a=1.0, b=0.0, reg=None, scaling=False, ref=None, out=None, err=None, sums=None):
    h, w = v.shape
    _lib.check(_eval_lib.lib().spnerf_eval_dsm_apply_shift(_lib.ptr(v), h, w, _lib.ptr(reg), 1 if scaling else 0, int(dx),
                                                           int(dy), float(a), float(b), _lib.ptr(ref), _lib.ptr(out),
                                                           _lib.ptr(err), _lib.ptr(sums), _lib.stream_of(v)),
               "dsm_apply_shift")


def downsample2x(dsm):
    """dsmr.downsample2x on one image: the next pyramid level, (ceil(H/2), ceil(W/2)).  Returns a
    float64 array (a device tensor when given one)."""
    v, _ = _image_pair(dsm, dsm)
    h, w = v.shape
    out = torch.empty((h + 1) // 2, (w + 1) // 2, dtype=torch.float64, device=v.device)
    _lib.check(_eval_lib.lib().spnerf_eval_dsm_down2x(_lib.ptr(v), h, w, _lib.ptr(out), _lib.stream_of(v)), "dsm_down2x")
    return out if isinstance(dsm, torch.Tensor) else out.cpu().numpy()


def register_dsm(dsm_ref, dsm_sec, irange=5, init=(0, 0), tables=False) -> Registration:
    """recursive_ncc + mean_std of modules/dsmr.py on the device: the shift of ``dsm_sec`` onto
    ``dsm_ref`` and the moments there.  ``init`` is recursive_ncc's initial (dx, dy).  Nothing is
    copied to the host until the result is read."""
    u, v = _image_pair(dsm_ref, dsm_sec)
    return _register(u, v, irange, init, tables)


def compute_shift(dsm_ref, dsm_sec, scaling=True, irange=5):
    """dsmr.compute_shift: (dx, dy, a, b) registering ``dsm_sec`` on ``dsm_ref`` — pixel (j, i) of
    the reference meets pixel (j + dy, i + dx) of ``dsm_sec``, whose altitudes map by
    z -> a·z + b (a = 1 unless ``scaling``).  Each image is an array, a device tensor or the path
    of a float TIFF.  One device-to-host copy, at the end."""
    return register_dsm(dsm_ref, dsm_sec, irange).transform(scaling)


def apply_shift(dsm, dx=0, dy=0, a=1, b=0):
    """dsmr.apply_shift on an image instead of a file pair: out[j, i] = a·dsm[j + dy, i + dx] + b,
    NaN where the source pixel is out of range.  Returns a float64 array (a device tensor when
    given one)."""
    v, _ = _image_pair(dsm, dsm)
    out = torch.empty_like(v)
    _apply(v, dx, dy, a, b, out=out)
    return out if isinstance(dsm, torch.Tensor) else out.cpu().numpy()


def dsm_pointwise_diff(pred, gt, gt_mask=None, register="ncc"):
    """utils.dsm_pointwise_diff on images already on the ground truth's grid: the error map
    registered(pred) − gt as a float64 array.  Cells where ``gt_mask`` is 9 (water) are removed
    from ``pred`` before the registration, like the reference.  ``register="ncc"`` is the
    reference's dsmr branch (compute_shift(gt, pred, scaling=False) then apply_shift), on the
    device without a host sync in between; ``"z"`` its mean-offset fallback."""
    if register not in ("ncc", "z"):
        raise ValueError(f"register must be 'z' or 'ncc', got {register!r}")
    g, p = _image_pair(gt, pred)
    if gt_mask is not None:
        m, _ = _image_pair(gt_mask, g)
        p = torch.where(m == 9, torch.full_like(p, float("nan")), p)
    if register == "z":
        pn, gn = p.cpu().numpy(), g.cpu().numpy()
        return (pn + np.nanmean(gn - pn)) - gn
    reg = _register(g, p, 5, (0, 0))
    err = torch.empty_like(g)
    _apply(p, reg=reg.device_result, ref=g, err=err)
    return err.cpu().numpy()
