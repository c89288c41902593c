"""The fp64 numpy statement of the plane sweep (include/spnerf_amd_sweep.h): the grey planes, the window
score and the pick, one numpy operation per stated operation, i.e. every product, sum, quotient and
square root rounded once.  Written apart from the kernels: the inverse transverse Mercator is
``ortho_numpy.utm_inverse``, the camera ``oracle.rpc_ref.RPC``, the bilinear read
``rectify_numpy.sample_one``; the score is vectorised over the cells and loops over the window offsets
in row-major order, where the device loops over each cell's own clipped window.
"""
import numpy as np

import ortho_numpy as on
import rectify_numpy as rn


def latlon(grid):
    E, N = rn.cell_centres(grid)
    return on.utm_inverse(E, N, grid.zone, grid.south)


def pix_at(grid, cams, alt, geo=None):
    """pix (V, H, W, 2) float64 of every cell centre at the altitude ``alt``."""
    lat, lon = latlon(grid) if geo is None else geo
    pix = np.empty((len(cams),) + lat.shape + (2,), np.float64)
    for v, cam in enumerate(cams):
        pix[v, ..., 0], pix[v, ..., 1] = cam.projection(lon, lat, np.full(lat.shape, float(alt)))
    return pix


def grey_at(images, pix):
    """(grey (V, H, W) float32, valid (V, H, W) uint8) of the images read at ``pix`` (V, H, W, 2)."""
    greys, valids = [], []
    for v, im in enumerate(images):
        rgb, ok = rn.sample_one(im, pix[v])
        s = rgb[..., 0].astype(np.float64)
        for c in range(1, rgb.shape[-1]):
            s = s + rgb[..., c].astype(np.float64)
        g = (s / float(rgb.shape[-1])).astype(np.float32)
        greys.append(g)
        valids.append(((ok == 1) & np.isfinite(g)).astype(np.uint8))
    return np.stack(greys), np.stack(valids)


def grey(images, cams, grid, alt, geo=None):
    return grey_at(images, pix_at(grid, cams, alt, geo))


def _shifts(plane, radius, fill):
    """The plane seen from every window offset (dj, di), row-major: list of (H, W) arrays, ``fill`` outside the grid."""
    H, W = plane.shape
    pad = np.full((H + 2 * radius, W + 2 * radius), fill, plane.dtype)
    pad[radius:radius + H, radius:radius + W] = plane
    return [pad[radius + dj:radius + dj + H, radius + di:radius + di + W] for dj in range(-radius, radius + 1)
            for di in range(-radius, radius + 1)]


def score(grey, valid, radius, min_views=2, min_std=0.0):
    """(score (H, W) float32, views (H, W) uint8) of one plane."""
    g = np.asarray(grey, np.float32).astype(np.float64)
    ok = np.asarray(valid) == 1
    V, H, W = g.shape
    inside = _shifts(np.ones((H, W), bool), radius, False)
    n = np.zeros((H, W))
    for w in inside:
        n = n + w
    floor = n * (float(min_std) * float(min_std))
    safe_n = np.where(n > 0, n, 1.0)
    use, mu, norm, shifted = [], [], [], []
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for v in range(V):
            gs, oks = _shifts(g[v], radius, 0.0), _shifts(ok[v], radius, False)
            total, every = np.zeros((H, W)), np.ones((H, W), bool)
            for w, x, o in zip(inside, gs, oks):
                total = np.where(w, total + x, total)
                every &= o | ~w
            mean = total / safe_n
            ss = np.zeros((H, W))
            for w, x in zip(inside, gs):
                d = x - mean
                ss = np.where(w, ss + d * d, ss)
            use.append(every & (n >= 2) & (ss > floor))
            mu.append(mean)
            norm.append(np.sqrt(ss))
            shifted.append(gs)
        m = np.zeros((H, W))
        for u in use:
            m = m + u
        acc = np.zeros((H, W))
        for k, w in enumerate(inside):
            S = np.zeros((H, W))
            for v in range(V):
                S = np.where(use[v], S + (shifted[v][k] - mu[v]) / norm[v], S)
            acc = np.where(w, acc + S * S, acc)
        out = ((acc - m) / (m * (m - 1.0))).astype(np.float32)
    out[m < min_views] = np.nan
    return out, m.astype(np.uint8)


def pairwise_zncc(grey, valid, radius, j, i, min_std=0.0):
    """The explicit mean of the pairwise ZNCCs of the usable views at cell (j, i), float64; (nan, m) below two views."""
    g = np.asarray(grey, np.float32).astype(np.float64)
    V, H, W = g.shape
    rows, cols = slice(max(j - radius, 0), min(j + radius, H - 1) + 1), slice(max(i - radius, 0), min(i + radius, W - 1) + 1)
    unit = []
    for v in range(V):
        x = g[v, rows, cols].ravel()
        if x.size < 2 or not (np.asarray(valid)[v, rows, cols] == 1).all():
            continue
        d = x - x.sum() / x.size
        ss = float((d * d).sum())
        if ss > x.size * min_std * min_std:
            unit.append(d / np.sqrt(ss))
    m = len(unit)
    if m < 2:
        return np.nan, m
    return float(np.mean([unit[a] @ unit[b] for a in range(m) for b in range(a + 1, m)])), m


def pick(volume, views_vol, alt_lo, step):
    """dict of altitude (float32), score (float32), index (int32), views (uint8) from (K, H, W) planes."""
    vol = np.asarray(volume, np.float32)
    K = vol.shape[0]
    s = vol.astype(np.float64)
    best = np.full(vol.shape[1:], np.nan)
    index = np.full(vol.shape[1:], -1, np.int64)
    with np.errstate(invalid="ignore"):
        for k in range(K):
            take = ~np.isnan(s[k]) & ((index < 0) | (s[k] > best))
            best, index = np.where(take, s[k], best), np.where(take, k, index)
    some = index >= 0
    at = np.where(some, index, 0)[None]
    nan_plane = np.full((1,) + vol.shape[1:], np.nan)
    lower = np.take_along_axis(np.concatenate([nan_plane, s[:-1]]), at, 0)[0]
    upper = np.take_along_axis(np.concatenate([s[1:], nan_plane]), at, 0)[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        den = (lower - 2.0 * best) + upper
        fit = some & (index > 0) & (index < K - 1) & ~np.isnan(lower) & ~np.isnan(upper) & (den < 0.0)
        offset = np.where(fit, np.clip(0.5 * (lower - upper) / den, -0.5, 0.5), 0.0)
    altitude = (float(alt_lo) + (index.astype(np.float64) + offset) * float(step)).astype(np.float32)
    altitude[~some] = np.nan
    return {"altitude": altitude, "score": np.where(some, np.take_along_axis(vol, at, 0)[0], np.float32(np.nan)).astype(np.float32),
            "index": index.astype(np.int32), "views": np.where(some, np.take_along_axis(np.asarray(views_vol, np.uint8), at, 0)[0], 0).astype(np.uint8)}


def sweep(images, cams, grid, alt_lo, step, planes, radius=2, min_views=2, min_std=0.0, pix_shift=0.0):
    """The whole statement: the dict of ``pick`` plus ``volume`` (K, H, W) float32 and ``views_vol``.
    ``pix_shift`` moves every pixel position by that much in col and row (for sensitivity studies)."""
    geo = latlon(grid)
    volume, views_vol = [], []
    for k in range(planes):
        g, ok = grey_at(images, pix_at(grid, cams, float(alt_lo) + float(k) * float(step), geo) + pix_shift)
        sc, m = score(g, ok, radius, min_views, min_std)
        volume.append(sc)
        views_vol.append(m)
    volume, views_vol = np.stack(volume), np.stack(views_vol)
    out = pick(volume, views_vol, alt_lo, step)
    out["volume"], out["views_vol"] = volume, views_vol
    return out
