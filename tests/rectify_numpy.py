"""The fp64 numpy statement of the orthorectification (include/spnerf_amd_rectify.h): the projection of
the cell centres, the bilinear read, the lines of sight and the mosaic, every step in the stated
operation order.  Written apart from the kernels: the inverse transverse Mercator is
``ortho_numpy.utm_inverse`` (a complex series and a fixed point, where the device takes real series and
Newton steps), the forward one ``oracle.dsm_ref.utm``, the camera ``oracle.rpc_ref.RPC``.

A grid is a ``spnerf_amd.GroundGrid`` or anything with its fields; a camera an ``rpc_ref.RPC`` (already
rescaled); an image an (h, w, C) float32 array.  Every product and sum of ``sample`` and ``mosaic`` is
one numpy operation, i.e. rounded once: the kernels are compiled without fused multiply-adds there.
"""
import numpy as np

import ortho_numpy as on
from oracle import dsm_ref


def cell_centres(grid):
    """(E, N) of the cell centres, two (ysize, xsize) float64 arrays."""
    e = grid.xoff + (np.arange(grid.xsize, dtype=np.float64) + 0.5) * grid.resolution
    n = grid.ytop - (np.arange(grid.ysize, dtype=np.float64) + 0.5) * grid.resolution
    return np.broadcast_to(e[None, :], (grid.ysize, grid.xsize)).copy(), np.broadcast_to(n[:, None], (grid.ysize, grid.xsize)).copy()


def project(dsm, grid, cams):
    """pix (V, H, W, 2) float64: [col, row] of every cell centre at its DSM altitude; NaN where the DSM is."""
    dsm = np.asarray(dsm, np.float64)
    E, N = cell_centres(grid)
    lat, lon = on.utm_inverse(E, N, grid.zone, grid.south)
    pix = np.empty((len(cams),) + dsm.shape + (2,), np.float64)
    for v, cam in enumerate(cams):
        pix[v, ..., 0], pix[v, ..., 1] = cam.projection(lon, lat, dsm)
    return pix


def sample_one(image, pix):
    """(rgb (..., C) float32, valid (...) uint8) of one image at pix (..., 2)."""
    image = np.asarray(image, np.float32)
    h, w, _ = image.shape
    col, row = pix[..., 0], pix[..., 1]
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(col) & np.isfinite(row) & (col >= 0.0) & (col <= w - 1.0) & (row >= 0.0) & (row <= h - 1.0)
    c, r = np.where(valid, col, 0.0), np.where(valid, row, 0.0)
    x0, y0 = np.floor(c), np.floor(r)
    fx, fy = (c - x0)[..., None], (r - y0)[..., None]
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    img = image.astype(np.float64)
    p00, p01, p10, p11 = img[y0, x0], img[y0, x1], img[y1, x0], img[y1, x1]
    value = ((1.0 - fx) * p00 + fx * p01) * (1.0 - fy) + ((1.0 - fx) * p10 + fx * p11) * fy
    rgb = value.astype(np.float32)
    rgb[~valid] = np.nan
    return rgb, valid.astype(np.uint8)


def sample(images, pix):
    """rgb (V, H, W, C) float32 and valid (V, H, W) uint8."""
    res = [sample_one(im, pix[v]) for v, im in enumerate(images)]
    return np.stack([a for a, _ in res]), np.stack([b for _, b in res])


def line_of_sight(cam, e, n, zone, south, alt_lo, alt_hi):
    """The unit vector (east, north, up), float64, from the ground point (e, n) towards the camera."""
    lat, lon = on.utm_inverse(np.array([e], np.float64), np.array([n], np.float64), zone, south)
    col, row = cam.projection(lon, lat, np.array([float(alt_lo)]))
    lon2, lat2 = cam.localization(col, row, np.array([float(alt_hi)]))
    e2, n2 = dsm_ref.utm(lat2, lon2, zone, south)
    d = np.array([float(e2[0]) - e, float(n2[0]) - n, float(alt_hi) - float(alt_lo)], np.float64)
    return d / np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])


def view_directions(grid, cams, alt_lo, alt_hi):
    """dirs (V, 3) float32 at the grid's centre and spread (V,) float32: the largest component
    difference, in fp64, between a corner's direction and the centre's."""
    w, h = grid.xsize * grid.resolution, grid.ysize * grid.resolution
    points = [(grid.xoff + w / 2.0, grid.ytop - h / 2.0)] + [(grid.xoff + a * w, grid.ytop - b * h) for b in (0, 1) for a in (0, 1)]
    dirs, spread = [], []
    for cam in cams:
        d = [line_of_sight(cam, e, n, grid.zone, grid.south, alt_lo, alt_hi) for e, n in points]
        dirs.append(d[0].astype(np.float32))
        spread.append(np.float32(max(float(np.abs(x - d[0]).max()) for x in d[1:])))
    return np.stack(dirs), np.array(spread, np.float32)


def visible_from_shadow(shadow):
    """cast_shadows' planes (1 behind higher terrain, 0 not, 255 no data) as "visible": 0 <-> 1, 255 kept."""
    shadow = np.asarray(shadow, np.uint8)
    return np.where(shadow > 1, shadow, 1 - shadow).astype(np.uint8)


def mosaic(rgb, usable, mode):
    """(mosaic (H, W, C) float32, count (H, W) int32, spread (H, W) float32) over the views whose
    ``usable`` is 1, accumulated in view order."""
    rgb = np.asarray(rgb, np.float32)
    use = np.asarray(usable) == 1
    V, H, W, C = rgb.shape
    x = rgb.astype(np.float64)
    count = use.sum(0).astype(np.int32)
    some = count > 0
    n = np.where(some, count, 1).astype(np.float64)
    total = np.zeros((H, W, C))
    for v in range(V):
        total = np.where(use[v][..., None], total + x[v], total)
    mean = total / n[..., None]
    dev = np.zeros((H, W))
    for c in range(C):
        for v in range(V):
            d = x[v, ..., c] - mean[..., c]
            dev = np.where(use[v], dev + d * d, dev)
    spread = np.sqrt(dev / (n * C)).astype(np.float32)
    if mode == "mean":
        out = mean
    elif mode == "median":
        ranked = np.sort(np.where(use[..., None], x, np.nan), axis=0, kind="stable")     # a NaN sorts last: usable NaNs, then the unusable views
        k_lo, k_hi = np.where(some, (count - 1) // 2, 0), np.where(some, count // 2, 0)
        lo = np.take_along_axis(ranked, k_lo[None, ..., None].repeat(C, -1), 0)[0]
        hi = np.take_along_axis(ranked, k_hi[None, ..., None].repeat(C, -1), 0)[0]
        out = (lo + hi) / 2.0
    else:
        raise ValueError(mode)
    out = out.astype(np.float32)
    out[~some] = np.nan
    spread[~some] = np.nan
    return out, count, spread
