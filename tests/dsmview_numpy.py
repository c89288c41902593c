"""The fp64 numpy statement of the DSM view (include/spnerf_amd_dsmview.h): the localisation, the segment, the
walk, the outputs, the raster read and the ECEF points, every step in the stated operation order.  Written
from the header over ``oracle.rpc_ref`` (the camera), ``oracle.dsm_ref.utm`` (the forward projection) and
``ortho_numpy.utm_inverse`` (the inverse one), with the conventions of tests/shadow_numpy.py: no early exit —
every pixel walks its whole segment from step 0, nothing is skipped above the highest cell — and every
product and sum is one numpy operation, i.e. rounded once.

A grid is a ``spnerf_amd.GroundGrid`` or anything with its fields; a camera an ``rpc_ref.RPC`` (already
rescaled); a lattice (col0, row0, n_cols, n_rows) with a stride.
"""
import numpy as np

import ortho_numpy as on
from oracle import dsm_ref, rpc_ref

FAR = 2.0 ** 31


def lattice_pixels(rect, stride=1):
    """(col, row) of the lattice, two (n_rows, n_cols) float64 arrays."""
    col0, row0, n_cols, n_rows = rect
    col = np.float64(col0) + np.arange(n_cols, dtype=np.float64) * np.float64(stride)
    row = np.float64(row0) + np.arange(n_rows, dtype=np.float64) * np.float64(stride)
    return np.broadcast_to(col[None, :], (n_rows, n_cols)).copy(), np.broadcast_to(row[:, None], (n_rows, n_cols)).copy()


def localise(cam, col, row, alt):
    """(lon, lat) in degrees: the header's iteration, every pixel stopping on its own."""
    cn = (np.asarray(col, np.float64) - cam.col_offset) / cam.col_scale
    rn = (np.asarray(row, np.float64) - cam.row_offset) / cam.row_scale
    an = (np.float64(alt) - cam.alt_offset) / cam.alt_scale
    lon, lat = -np.ones_like(cn), -np.ones_like(cn)
    extra = np.full(cn.shape, -1)
    done = np.zeros(cn.shape, bool)
    eps = 2.0
    with np.errstate(all="ignore"):
        for _ in range(101):
            x0, y0 = cam.projection_n(lat, lon, an)
            conv = ((x0 - cn) * (x0 - cn) + (y0 - rn) * (y0 - rn) < 1e-18) & ~done
            extra[conv & (extra < 0)] = 2
            done |= conv & (extra == 0)
            extra[conv] -= 1
            if done.all():
                break
            x1, y1 = cam.projection_n(lat, lon + eps, an)
            x2, y2 = cam.projection_n(lat + eps, lon, an)
            e1x, e1y, e2x, e2y = x1 - x0, y1 - y0, x2 - x0, y2 - y0
            ux, uy = cn - x0, rn - y0
            a1 = (ux * e1x + uy * e1y) / (e1x * e1x + e1y * e1y)
            a2 = (ux * e2x + uy * e2y) / (e2x * e2x + e2y * e2y)
            lon = np.where(done, lon, lon + a1 * eps)
            lat = np.where(done, lat, lat + a2 * eps)
            eps = 0.1
    return lon * cam.lon_scale + cam.lon_offset, lat * cam.lat_scale + cam.lat_offset


def segments(grid, cam, alt_lo, alt_hi, rect, stride=1):
    """The lines of sight of the lattice: a dict of (n_rows, n_cols) float64 arrays — the ends in UTM (e_hi,
    n_hi, e_lo, n_lo) and in grid coordinates (x_hi, y_hi, x_lo, y_lo) — and the geodetic near end (lat_hi,
    lon_hi)."""
    col, row = lattice_pixels(rect, stride)
    s = {}
    for end, alt in (("hi", alt_hi), ("lo", alt_lo)):
        lon, lat = localise(cam, col, row, alt)
        e, n = dsm_ref.utm(lat, lon, grid.zone, grid.south)
        s["e_" + end], s["n_" + end] = e, n
        s["x_" + end] = (e - grid.xoff) / grid.resolution - 0.5
        s["y_" + end] = (grid.ytop - n) / grid.resolution - 0.5
        s["lat_" + end], s["lon_" + end] = lat, lon
    return s


def _height(h, c, y):
    """The height under (column c, row position y) of the (rows, columns) array h, and whether the step contributes."""
    nmin, nmaj = h.shape
    with np.errstate(invalid="ignore"):
        ok = (c >= 0) & (c <= nmaj - 1) & (y >= 0.0) & (y <= nmin - 1.0)
    fl = np.floor(np.where(ok, y, 0.0))
    f = np.where(ok, y, 0.0) - fl
    r0 = fl.astype(np.int64)
    r1 = np.minimum(r0 + 1, nmin - 1)
    cc = np.where(ok, c, 0).astype(np.int64)
    h0, h1 = h[r0, cc], h[r1, cc]
    with np.errstate(invalid="ignore"):
        t = h0 + f * (h1 - h0)
        between = np.minimum(np.maximum(t, np.minimum(h0, h1)), np.maximum(h0, h1))
    whole = f == 0.0
    ok = ok & np.isfinite(h0) & (whole | np.isfinite(h1))
    return np.where(whole, h0, between), ok


def walk(dsm, x_hi, y_hi, x_lo, y_lo, alt_lo, alt_hi):
    """The walk of the header for arrays of segments in grid coordinates: ``hit`` (bool), ``t`` (the crossing's
    parameter t*, NaN at a miss) and ``margin``: the smallest of |excess| over the contributing steps up to the
    hit, of the distance in cells of a step's minor coordinate from the grid's first and last line, and of
    |t* − 1|·|dA| at the deciding step — how far the decision stood from flipping (inf where nothing was near)."""
    dsm = np.asarray(dsm, np.float32).astype(np.float64)
    H, W = dsm.shape
    x_hi, y_hi, x_lo, y_lo = (np.asarray(v, np.float64) for v in (x_hi, y_hi, x_lo, y_lo))
    shape = x_hi.shape
    dA = np.float64(alt_lo) - np.float64(alt_hi)
    dx, dy = x_lo - x_hi, y_lo - y_hi
    with np.errstate(invalid="ignore"):
        near = (np.abs(x_hi) <= FAR) & (np.abs(y_hi) <= FAR) & (np.abs(x_lo) <= FAR) & (np.abs(y_lo) <= FAR)
        nadir = near & (dx == 0.0) & (dy == 0.0)
        rows = near & ~nadir & ~(np.abs(dx) >= np.abs(dy))
        cols = near & ~nadir & ~rows
    hit = np.zeros(shape, bool)
    ts = np.full(shape, np.nan)
    margin = np.full(shape, np.inf)

    # a segment with no horizontal extent reads the cell it stands in
    if nadir.any():
        i, j = np.floor(x_hi[nadir] + 0.5), np.floor(y_hi[nadir] + 0.5)
        inside = (i >= 0) & (i <= W - 1) & (j >= 0) & (j <= H - 1)
        h = dsm[np.where(inside, j, 0).astype(np.int64), np.where(inside, i, 0).astype(np.int64)]
        with np.errstate(invalid="ignore"):
            ok = inside & np.isfinite(h) & ~(h < alt_lo)
            t = np.where(h >= alt_hi, 0.0, (np.float64(alt_hi) - h) / (np.float64(alt_hi) - np.float64(alt_lo)))
        hit[nadir], ts[nadir] = ok, np.where(ok, t, np.nan)

    for sel, h, p0, q0, dmaj, dmin in ((cols, dsm, x_hi, y_hi, dx, dy), (rows, dsm.T, y_hi, x_hi, dy, dx)):
        if not sel.any():
            continue
        p0, q0, dmaj, dmin = p0[sel], q0[sel], dmaj[sel], dmin[sel]
        a, sgn = np.abs(dmaj), np.where(dmaj > 0.0, 1.0, -1.0)
        c0 = np.where(dmaj > 0.0, np.ceil(p0), np.floor(p0))
        n = p0.shape[0]
        got, prev, stop = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool)
        tp, ep, tc, mg = np.zeros(n), np.zeros(n), np.full(n, np.nan), np.full(n, np.inf)
        m = 0
        while True:
            cm = c0 + sgn * np.float64(m)
            u = (cm - p0) * sgn
            live = ~stop                                  # the first step with u > a is still taken
            if not live.any():
                break
            t = u / a
            y = q0 + t * dmin
            z = np.float64(alt_hi) + t * dA
            hs, ok = _height(h, cm, y)
            ok &= live
            e = z - hs
            on_grid = live & (cm >= 0) & (cm <= h.shape[1] - 1)
            edge = np.minimum(np.abs(y), np.abs(y - (h.shape[0] - 1.0)))
            mg = np.where(on_grid, np.minimum(mg, edge), mg)
            mg = np.where(ok, np.minimum(mg, np.abs(e)), mg)
            now = ok & (e <= 0.0)
            with np.errstate(invalid="ignore", divide="ignore"):
                cross = np.where(prev, tp + (t - tp) * (ep / (ep - e)), t)
            mg = np.where(now, np.minimum(mg, np.abs((cross - 1.0) * dA)), mg)
            tc = np.where(now & (cross <= 1.0), cross, tc)
            got |= now & (cross <= 1.0)
            stop |= now | (u > a)
            keep = ok & ~now
            tp, ep, prev = np.where(keep, t, tp), np.where(keep, e, ep), prev | keep
            m += 1
        hit[sel], ts[sel], margin[sel] = got, tc, mg
    return hit, ts, margin


def cast(dsm, grid, cam, alt_lo, alt_hi, rect, stride=1, seg=None):
    """The cast of the header: a dict of ``hit`` uint8, ``altitude`` float32, ``ground`` float64 (..., 2), ``cell``
    float32 (..., 2) and ``depth`` float32, plus ``t`` and ``margin`` of ``walk`` and the segments ``seg``."""
    s = segments(grid, cam, alt_lo, alt_hi, rect, stride) if seg is None else seg
    hit, t, margin = walk(dsm, s["x_hi"], s["y_hi"], s["x_lo"], s["y_lo"], alt_lo, alt_hi)
    dE, dN, dA = s["e_lo"] - s["e_hi"], s["n_lo"] - s["n_hi"], np.float64(alt_lo) - np.float64(alt_hi)
    dx, dy = s["x_lo"] - s["x_hi"], s["y_lo"] - s["y_hi"]
    length = np.sqrt((dE * dE + dN * dN) + dA * dA)
    with np.errstate(invalid="ignore"):
        out = {"hit": hit.astype(np.uint8), "altitude": (np.float64(alt_hi) + t * dA).astype(np.float32),
               "ground": np.stack([s["e_hi"] + t * dE, s["n_hi"] + t * dN], -1),
               "cell": np.stack([np.minimum(np.maximum(s["x_hi"] + t * dx, 0.0), grid.xsize - 1.0),
                                 np.minimum(np.maximum(s["y_hi"] + t * dy, 0.0), grid.ysize - 1.0)], -1).astype(np.float32),
               "depth": (t * length).astype(np.float32), "t": t, "margin": margin, "seg": s}
    for k in ("ground", "cell"):
        out[k][~hit] = np.nan
    return out


def sample(raster, cell, mode):
    """The raster read of the header: ``mode`` 0 nearest, 1 bilinear; float32, the shape of ``cell`` without its last axis."""
    raster = np.asarray(raster, np.float32)
    H, W = raster.shape
    x, y = np.asarray(cell, np.float32)[..., 0].astype(np.float64), np.asarray(cell, np.float32)[..., 1].astype(np.float64)
    with np.errstate(invalid="ignore"):
        ok = (x >= 0.0) & (x <= W - 1.0) & (y >= 0.0) & (y <= H - 1.0)
    x, y = np.where(ok, x, 0.0), np.where(ok, y, 0.0)
    if mode == 0:
        out = raster[np.floor(y + 0.5).astype(np.int64), np.floor(x + 0.5).astype(np.int64)].copy()
    else:
        x0, y0 = np.floor(x), np.floor(y)
        s, t = x - x0, y - y0
        ia, ja = x0.astype(np.int64), y0.astype(np.int64)
        ib, jb = np.minimum(ia + 1, W - 1), np.minimum(ja + 1, H - 1)
        r = raster.astype(np.float64)
        num, den = np.zeros(x.shape), np.zeros(x.shape)
        for h, w in ((r[ja, ia], (1.0 - t) * (1.0 - s)), (r[ja, ib], (1.0 - t) * s), (r[jb, ia], t * (1.0 - s)), (r[jb, ib], t * s)):
            fin = np.isfinite(h)
            num = np.where(fin, num + w * np.where(fin, h, 0.0), num)
            den = np.where(fin, den + w, den)
        with np.errstate(invalid="ignore", divide="ignore"):
            out = np.where(den > 0.0, num / den, np.nan).astype(np.float32)
    out[~ok] = np.nan
    return out


def ecef(ground, altitude, grid):
    """(..., 3) float64 ECEF of the ground points at their float32 altitudes."""
    ground = np.asarray(ground, np.float64)
    lat, lon = on.utm_inverse(ground[..., 0], ground[..., 1], grid.zone, grid.south)
    return np.stack(rpc_ref.geodetic_to_ecef(lat, lon, np.asarray(altitude, np.float32).astype(np.float64)), -1)
