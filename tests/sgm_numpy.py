"""The numpy float32 statement of the semi-global aggregation (include/spnerf_amd_sgm.h): straight loops
over the directions and the rows, one numpy float32 operation per stated operation, written from the
header and apart from the kernels — no path is enumerated: the rows are visited in an order in which
the previous cell of the direction has already been done.
"""
import numpy as np

import sweep_numpy as sw

F = np.float32
DIRECTIONS = ((0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (-1, -1), (1, -1), (-1, 1))    # (dj, di), the header's order


def cost(volume, unscored=1.0):
    """C (K, H, W) float32: 1 − score where the score is finite, else ``unscored``."""
    v = np.asarray(volume, F)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(np.isfinite(v), F(1.0) - v, F(unscored)).astype(F)


def path_costs(C, direction, p1, p2):
    """L_r (K, H, W) float32 of one direction (dj, di): the rows are visited so that the previous cell's
    row is done, and one row's cells and planes go through each numpy operation together."""
    dj, di = direction
    if dj == 0:                                                          # along a row: the same with rows and columns swapped
        return path_costs(C.transpose(0, 2, 1), (di, 0), p1, p2).transpose(0, 2, 1)
    K, H, W = C.shape
    p1, p2 = F(p1), F(p2)
    L = np.empty((K, H, W), F)
    for j in (range(H) if dj > 0 else range(H - 1, -1, -1)):
        qj = j - dj
        if not 0 <= qj < H:
            L[:, j] = C[:, j]
            continue
        prev, has = np.zeros((K, W), F), np.zeros(W, bool)              # L_r(q, ·) of every cell of the row whose q is in the grid
        if di == 0:
            prev[:], has[:] = L[:, qj], True
        elif di > 0:
            prev[:, 1:], has[1:] = L[:, qj, :-1], True
        else:
            prev[:, :-1], has[:-1] = L[:, qj, 1:], True
        M = prev.min(axis=0)
        m = np.minimum(prev, (M + p2).astype(F)[None])
        m[1:] = np.minimum(m[1:], (prev[:-1] + p1).astype(F))           # k >= 1: L_r(q, k - 1) + p1
        m[:-1] = np.minimum(m[:-1], (prev[1:] + p1).astype(F))          # k <= K - 2: L_r(q, k + 1) + p1
        step = (C[:, j] + (m - M[None]).astype(F)).astype(F)
        L[:, j] = np.where(has[None], step, C[:, j])
    return L


def aggregate(volume, p1, p2, unscored=1.0, paths=8):
    """out (K, H, W) float32: 1 − (L_0 + L_1 + ...)·(1 / paths), NaN at the cells without a finite score."""
    assert paths in (4, 8)
    v = np.asarray(volume, F)
    C = cost(v, unscored)
    S = path_costs(C, DIRECTIONS[0], p1, p2)
    for d in DIRECTIONS[1:paths]:
        S = (S + path_costs(C, d, p1, p2)).astype(F)
    out = (F(1.0) - S * F(1.0 / paths)).astype(F)
    out[:, ~np.isfinite(v).any(axis=0)] = np.nan
    return out


def pick(aggregated, volume, alt_lo, step):
    """dict of altitude, score (float32), index (int32) — the sweep's pick over ``aggregated`` — and photo
    (float32): the raw score at index where it is finite, else NaN."""
    agg, v = np.asarray(aggregated, F), np.asarray(volume, F)
    out = sw.pick(agg, np.zeros(agg.shape, np.uint8), alt_lo, step)
    del out["views"]
    at = np.where(out["index"] >= 0, out["index"], 0)[None]
    raw = np.take_along_axis(v, at, 0)[0]
    out["photo"] = np.where((out["index"] >= 0) & np.isfinite(raw), raw, F(np.nan)).astype(F)
    return out
