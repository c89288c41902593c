"""The fp64 numpy statement of the surface sweep (include/spnerf_amd_surface.h): the greys on a per-cell
altitude, the lift, the upsampling and the coarse-to-fine chain, one numpy operation per stated operation.
Written from the header and apart from the kernels: the camera is ``oracle.rpc_ref.RPC`` called with an
altitude array, the read ``rectify_numpy.sample_one`` (through ``sweep_numpy.grey_at``), score and pick
``sweep_numpy``'s, the aggregation ``sgm_numpy``'s.
"""
import collections
import math

import numpy as np

import rectify_numpy as rn  # noqa: F401  (the read behind sweep_numpy.grey_at)
import sgm_numpy as sg
import sweep_numpy as sw

Grid = collections.namedtuple("Grid", "xoff ytop xsize ysize resolution zone south")


def coarsen(grid, f):
    """The grid at f times the cell size: same origin and zone, ceil(H / f) x ceil(W / f) cells."""
    assert 1 <= f <= 8
    return Grid(grid.xoff, grid.ytop, -(-grid.xsize // f), -(-grid.ysize // f), grid.resolution * f, grid.zone, grid.south)


def pix_on(grid, cams, base, offset, geo=None):
    """pix (V, H, W, 2) float64 of every cell centre at the altitude (double)base + offset; NaN where the base is not finite."""
    lat, lon = sw.latlon(grid) if geo is None else geo
    b = np.asarray(base, np.float32)
    finite = np.isfinite(b)
    alt = np.where(finite, b, np.float32(0.0)).astype(np.float64) + float(offset)
    pix = np.empty((len(cams),) + lat.shape + (2,), np.float64)
    for v, cam in enumerate(cams):
        pix[v, ..., 0], pix[v, ..., 1] = cam.projection(lon, lat, alt)
    pix[:, ~finite] = np.nan
    return pix


def grey(images, cams, grid, base, offset, geo=None):
    """(grey (V, H, W) float32, valid (V, H, W) uint8) on the surface base + offset."""
    return sw.grey_at(images, pix_on(grid, cams, base, offset, geo))


def lift(base, rel):
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(base, np.float32).astype(np.float64) + np.asarray(rel, np.float32).astype(np.float64)).astype(np.float32)


def _axis(n, f, size):
    y = (np.arange(n, dtype=np.float64) + 0.5) / float(f) - 0.5
    y0 = np.floor(y)
    k = y0.astype(np.int64)
    return np.clip(k, 0, size - 1), np.clip(k + 1, 0, size - 1), y - y0


def upsample(coarse, f, shape):
    """out (H, W) float32 of the raster on the grid coarsened by f."""
    c = np.asarray(coarse, np.float32).astype(np.float64)
    H, W = shape
    assert c.shape == (-(-H // f), -(-W // f))
    ja, jb, t = _axis(H, f, c.shape[0])
    ia, ib, s = _axis(W, f, c.shape[1])
    t, s = t[:, None], s[None, :]
    num, den = np.zeros((H, W)), np.zeros((H, W))
    with np.errstate(invalid="ignore", over="ignore"):
        for h, w in ((c[ja][:, ia], (1.0 - t) * (1.0 - s)), (c[ja][:, ib], (1.0 - t) * s), (c[jb][:, ia], t * (1.0 - s)), (c[jb][:, ib], t * s)):
            ok = np.isfinite(h)
            num = np.where(ok, num + w * np.where(ok, h, 0.0), num)
            den = np.where(ok, den + w, den)
        return np.where(den > 0.0, num / np.where(den > 0.0, den, 1.0), np.nan).astype(np.float32)


def volume(images, cams, grid, base, off_lo, step, planes, radius=2, min_views=2, min_std=0.0):
    """(volume (K, H, W) float32, views_vol (K, H, W) uint8): the scores of the surfaces base + (off_lo + k·step)."""
    geo = sw.latlon(grid)
    vol, views = [], []
    for k in range(planes):
        g, ok = grey(images, cams, grid, base, float(off_lo) + float(k) * float(step), geo)
        sc, m = sw.score(g, ok, radius, min_views, min_std)
        vol.append(sc)
        views.append(m)
    return np.stack(vol), np.stack(views)


def sweep(images, cams, grid, base, off_lo, step, planes, radius=2, min_views=2, min_std=0.0):
    """The whole statement: ``sweep_numpy.pick`` at alt_lo = off_lo with the altitude lifted, plus ``volume`` and ``views_vol``."""
    vol, views = volume(images, cams, grid, base, off_lo, step, planes, radius, min_views, min_std)
    out = sw.pick(vol, views, off_lo, step)
    out["altitude"] = lift(base, out["altitude"])
    out["volume"], out["views_vol"] = vol, views
    return out


def level_plan(factors, planes, reach):
    """[(factor, step multiple, surfaces)] from the coarsest level to the implied one of factor 1."""
    fs = tuple(factors) + (1,)
    assert all(2 <= f <= 8 for f in factors) and all(a > b and a % b == 0 for a, b in zip(fs, fs[1:]))
    mult = [min(f, 2) for f in fs]
    plan = [(fs[0], mult[0], math.ceil(planes / mult[0]))]
    for l in range(1, len(fs)):
        plan.append((fs[l], mult[l], 2 * math.ceil(reach * mult[l - 1] / mult[l]) + 1))
    return plan


def later_level(raw, base, off_lo, step, p1, p2, unscored=1.0, paths=8):
    """A later level from its score volume: aggregate, pick at alt_lo = off_lo, lift; plus ``base``."""
    out = sg.pick(sg.aggregate(raw, p1, p2, unscored, paths), raw, off_lo, step)
    out["altitude"] = lift(base, out["altitude"])
    out["base"] = base
    return out


def pyramid(images, cams, grid, alt_lo, step, planes, factors=(4,), reach=3, radius=2, min_views=2, min_std=0.0, p1=0.25, p2=2.0,
            unscored=1.0, paths=8):
    """The chain: a list of the levels' dicts, each with ``shape`` and ``planes``; the last one is the result."""
    plan = level_plan(factors, planes, reach)
    f0, m0, K0 = plan[0]
    g0 = coarsen(grid, f0)
    first = sw.sweep(images, cams, g0, alt_lo, step * m0, K0, radius, min_views, min_std)
    out = sg.pick(sg.aggregate(first["volume"], p1, p2, unscored, paths), first["volume"], alt_lo, step * m0)
    out["shape"], out["planes"] = (g0.ysize, g0.xsize), K0
    levels, f_prev = [out], f0
    for f, m, K in plan[1:]:
        g = coarsen(grid, f)
        base = upsample(levels[-1]["altitude"], f_prev // f, (g.ysize, g.xsize))
        s, off_lo = step * m, -(K // 2) * (step * m)
        raw, _ = volume(images, cams, g, base, off_lo, s, K, radius, min_views, min_std)
        out = later_level(raw, base, off_lo, s, p1, p2, unscored, paths)
        out["shape"], out["planes"], out["off_lo"], out["step"] = (g.ysize, g.xsize), K, off_lo, s
        levels.append(out)
        f_prev = f
    return levels
