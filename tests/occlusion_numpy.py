"""The fp64 numpy statement of the occlusion exports (include/spnerf_amd_occlusion.h): the visibility floor
of a ground-grid DSM under V lines of sight, the gate, and the plane sweep with the gate at every plane.
``floor_one`` states the floor one step at a time for the whole grid, with the march of
``shadow_numpy`` (``march``, ``_interp``: the same major axis, steps, interpolated and clamped height);
``floor_cell`` states it again with plain loops for one cell, written on its own
(tests/test_occlusion_ref.py holds the two together and pins them to known answers).  No early stop:
every cell marches to the grid's edge.

Every product, sum and difference below is one numpy operation, i.e. rounded once.
"""
import numpy as np

import shadow_numpy as sn
import sweep_numpy as sw


def floor_one(dsm, resolution, direction):
    """floor (H, W) float64 of one direction, before the cast to float32: the maximum over the
    contributing steps of (height − m·rho), −inf where there is none.  The cell's own height is not read."""
    dsm = np.asarray(dsm, np.float64)
    axis, sgn, q, rho = sn.march(direction, resolution)
    h = dsm.T if axis == 1 else dsm        # the row case is the transpose of the column case
    H, W = h.shape
    out = np.full((H, W), -np.inf)
    if axis is not None:
        jj = np.arange(H, dtype=np.float64)
        ii = np.arange(W)
        with np.errstate(invalid="ignore"):
            for m in range(1, W):
                cols = ii + m * sgn
                okc = (cols >= 0) & (cols < W)
                y = jj + np.float64(m) * q
                okr = (y >= 0.0) & (y <= H - 1.0)
                if not okc.any() or not okr.any():
                    break                                    # y is monotone in m: it has left for good
                fl = np.floor(y)
                f = y - fl
                r0 = np.clip(fl.astype(np.int64), 0, H - 1)
                r1 = np.clip(r0 + 1, 0, H - 1)
                cc = np.clip(cols, 0, W - 1)
                h0, h1 = h[r0[:, None], cc[None, :]], h[r1[:, None], cc[None, :]]
                hs = np.where(f[:, None] == 0.0, h0, sn._interp(h0, h1, f[:, None]))
                e = hs - np.float64(m) * rho
                ok = okr[:, None] & okc[None, :] & ~np.isnan(hs)
                out = np.where(ok, np.maximum(out, np.where(ok, e, -np.inf)), out)
    return out.T if axis == 1 else out


def floor64(dsm, resolution, dirs):
    """(V, H, W) float64: the floors before their one cast."""
    return np.stack([floor_one(dsm, resolution, d) for d in np.asarray(dirs).reshape(-1, 3)])


def floor(dsm, resolution, dirs):
    """(V, H, W) float32, as ``visibility_floor`` returns it."""
    return floor64(dsm, resolution, dirs).astype(np.float32)


def floor_cell(dsm, resolution, direction, j, i):
    """The float64 floor of cell (j, i) under one direction, walked step by step with scalars."""
    dsm = np.asarray(dsm, np.float64)
    H, W = dsm.shape
    e, n, u = (float(np.float32(v)) for v in direction)
    a, b = e, -n
    if a == 0.0 and b == 0.0:
        return -np.inf
    columns = abs(a) >= abs(b)                                # the major axis
    big, small = (a, b) if columns else (b, a)
    q, rho = np.float64(small) / abs(big), np.float64(resolution) * np.float64(u) / abs(big)
    sgn = 1 if big > 0 else -1
    major, minor = (i, j) if columns else (j, i)
    n_major, n_minor = (W, H) if columns else (H, W)
    best = -np.inf
    for m in range(1, n_major):
        c = major + m * sgn
        y = np.float64(minor) + np.float64(m) * q
        if c < 0 or c >= n_major or y < 0.0 or y > n_minor - 1:
            break
        lo = int(np.floor(y))
        f = y - np.floor(y)
        read = (lambda k: dsm[k, c]) if columns else (lambda k: dsm[c, k])
        if f == 0.0:
            height = read(lo)
        else:
            h0, h1 = read(lo), read(lo + 1)
            height = min(max(h0 + f * (h1 - h0), min(h0, h1)), max(h0, h1)) if not (np.isnan(h0) or np.isnan(h1)) else np.nan
        if np.isnan(height):
            continue
        best = max(best, height - np.float64(m) * rho)
    return best


def gated(floor, alt, slack):
    """The (V, H, W) bool mask of the gate at one plane: (alt + slack) < (double)floor, strictly."""
    reach = np.float64(alt) + np.float64(slack)
    with np.errstate(invalid="ignore"):
        return reach < np.asarray(floor, np.float32).astype(np.float64)


def gate(grey, valid, floor, alt, slack=0.0):
    """A new (grey, valid) pair: NaN and 0 where the gate holds, everything else copied."""
    g, ok = np.array(grey, np.float32), np.array(valid, np.uint8)
    off = gated(floor, alt, slack)
    g[off] = np.nan
    ok[off] = 0
    return g, ok


def sweep(images, cams, grid, alt_lo, step, planes, floor, slack, radius=2, min_views=2, min_std=0.0):
    """``sweep_numpy.sweep`` with the gate at every plane: the dict of ``pick`` plus ``volume``, ``views_vol``
    and ``gated`` (K, V, H, W) bool."""
    geo = sw.latlon(grid)
    volume, views_vol, off = [], [], []
    for k in range(planes):
        alt = float(alt_lo) + float(k) * float(step)
        g, ok = sw.grey_at(images, sw.pix_at(grid, cams, alt, geo))
        g, ok = gate(g, ok, floor, alt, slack)
        sc, m = sw.score(g, ok, radius, min_views, min_std)
        volume.append(sc)
        views_vol.append(m)
        off.append(gated(floor, alt, slack))
    volume, views_vol = np.stack(volume), np.stack(views_vol)
    out = sw.pick(volume, views_vol, alt_lo, step)
    out["volume"], out["views_vol"], out["gated"] = volume, views_vol, np.stack(off)
    return out


def in_window(mask, radius):
    """(..., H, W) bool: whether ``mask`` holds anywhere in the (2·radius + 1)² window of a cell, clipped to the grid."""
    mask = np.asarray(mask, bool)
    H, W = mask.shape[-2:]
    pad = np.zeros(mask.shape[:-2] + (H + 2 * radius, W + 2 * radius), bool)
    pad[..., radius:radius + H, radius:radius + W] = mask
    out = np.zeros(mask.shape, bool)
    for dj in range(2 * radius + 1):
        for di in range(2 * radius + 1):
            out |= pad[..., dj:dj + H, di:di + W]
    return out
