"""Vectorised numpy restatement of the reference's DSM registration (modules/dsmr.py): the 2x
pyramid, the masked two-pass moments, the NCC table of a shift window, the pick rule and the
shift.  Test-only: the package never imports it.  Images are 2-D float arrays (H, W); a shift
(dx, dy) pairs u[j, i] with v[j + dy, i + dx]."""
import numpy as np


def levels_of(h, w):
    """Number of 2x reductions recursive_ncc makes: it goes down while min(H, W) > 100."""
    n = 0
    while min(h, w) > 100:
        h, w = (h + 1) // 2, (w + 1) // 2
        n += 1
    return n


def down2x(u):
    """downsample2x.  The reference loops over every source pixel (j, i), averages the finite
    values of the 2x2 block that STARTS there and stores it at [j // 2, i // 2], so the value
    that stands is the one written last: the block starting at (min(2J + 1, H - 1),
    min(2I + 1, W - 1)).  Its sum runs column by column: (j, i), (j + 1, i), (j, i + 1),
    (j + 1, i + 1)."""
    u = np.asarray(u, np.float64)
    h, w = u.shape
    oh, ow = (h + 1) // 2, (w + 1) // 2
    j0 = np.minimum(2 * np.arange(oh) + 1, h - 1)[:, None]
    i0 = np.minimum(2 * np.arange(ow) + 1, w - 1)[None, :]
    pad = np.full((h + 1, w + 1), np.nan)
    pad[:h, :w] = u
    s = np.zeros((oh, ow))
    n = np.zeros((oh, ow))
    for k, l in ((0, 0), (0, 1), (1, 0), (1, 1)):      # i + k, j + l
        t = pad[j0 + l, i0 + k]
        ok = np.isfinite(t)
        s = s + np.where(ok, t, 0.0)
        n = n + ok
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(n > 0, s / n, np.nan)


def _overlap(u, v, dx, dy):
    h, w = u.shape
    j0, j1 = max(0, -dy), min(h, h - dy)
    i0, i1 = max(0, -dx), min(w, w - dx)
    if j1 <= j0 or i1 <= i0:
        z = np.zeros(0)
        return z, z
    a = u[j0:j1, i0:i1]
    b = v[j0 + dy:j1 + dy, i0 + dx:i1 + dx]
    ok = np.isfinite(a) & np.isfinite(b)
    return a[ok], b[ok]


def moments(u, v, dx=0, dy=0):
    """mean_std, plus the pair count: (muu, muv, sigu, sigv, xcorr, count).  NaN when no pixel of
    u meets a finite pixel of v (numba's 0 / 0)."""
    a, b = _overlap(np.asarray(u, np.float64), np.asarray(v, np.float64), int(dx), int(dy))
    n = a.size
    if n == 0:
        return (np.nan,) * 5 + (0,)
    muu, muv = a.sum() / n, b.sum() / n
    a, b = a - muu, b - muv
    return muu, muv, np.sqrt((a * a).sum() / n), np.sqrt((b * b).sum() / n), (a * b).sum() / n, n


def ncc_table(u, v, irange, cx, cy):
    """ncc of every shift of (cx, cy) +- irange, rows y, columns x (compute_ncc's scan order)."""
    r = int(irange)
    t = np.full((2 * r + 1, 2 * r + 1), np.nan)
    with np.errstate(invalid="ignore", divide="ignore"):
        for y in range(2 * r + 1):
            for x in range(2 * r + 1):
                m = moments(u, v, cx - r + x, cy - r + y)
                t[y, x] = m[4] / (m[2] * m[3])
    return t


def pick(table, cx, cy):
    """compute_ncc's rule: scan y outer, x inner, replace only on strictly greater than the best
    so far (which starts at -inf): a NaN never wins, the first of equal maxima stands, and the
    centre stands when nothing wins."""
    r = table.shape[0] // 2
    dx, dy, best = cx, cy, -np.inf
    for y in range(table.shape[0]):
        for x in range(table.shape[1]):
            if table[y, x] > best:
                dx, dy, best = cx - r + x, cy - r + y, table[y, x]
    return dx, dy


def recursive_ncc(u, v, irange=5, dx=0, dy=0, trace=None):
    """recursive_ncc.  ``trace`` (a list) receives (dx, dy, table) of every level, the coarsest
    first, as the recursion computes them."""
    if min(u.shape) > 100:
        dx, dy = recursive_ncc(down2x(u), down2x(v), irange, dx // 2, dy // 2, trace)
        dx, dy = dx * 2, dy * 2
    t = ncc_table(u, v, irange, dx, dy)
    dx, dy = pick(t, dx, dy)
    if trace is not None:
        trace.append((dx, dy, t))
    return dx, dy


def compute_shift(u, v, scaling=True, irange=5, dx=0, dy=0, trace=None):
    """compute_shift on arrays: (dx, dy, a, b) and the moments at the result."""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    dx, dy = recursive_ncc(u, v, irange, dx, dy, trace)
    m = moments(u, v, dx, dy)
    with np.errstate(invalid="ignore", divide="ignore"):
        a = m[2] / m[3] if scaling else 1.0
        b = m[0] - m[1] * a
    return dx, dy, a, b, m


def apply_shift(v, dx=0, dy=0, a=1.0, b=0.0):
    """apply_shift_: out[j, i] = a * v[j + dy, i + dx] + b, NaN where the source pixel is out of
    range.  (Its c * i + d * j term is identically zero: c is shadowed by the channel index 0
    and d defaults to 0.)"""
    v = np.asarray(v, np.float64)
    h, w = v.shape
    out = np.full((h, w), np.nan)
    j0, j1 = max(0, -dy), min(h, h - dy)
    i0, i1 = max(0, -dx), min(w, w - dx)
    if j1 > j0 and i1 > i0:
        out[j0:j1, i0:i1] = a * v[j0 + dy:j1 + dy, i0 + dx:i1 + dx] + b
    return out
