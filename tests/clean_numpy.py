"""The statement of include/staged/spnerf_amd_clean.h in plain numpy: the speckle filter by breadth-first search
over the join relation, the median by ``np.sort`` of the finite window values, the fill by eight walks per
hole, and ``clean_dsm``'s chain over the three.  Every raster is (H, W) float32, row 0 the northernmost; a
cell that is not finite is a hole.  Nothing rounds, so the device is held to these bytes
(tests/test_gpu_clean.py); the statement itself is pinned to closed forms by tests/test_clean_ref.py."""
import collections

import numpy as np

DIRECTIONS = ((0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1), (1, 0), (1, 1))   # (dy, dx): E, NE, N, NW, W, SW, S, SE
LOWEST, NEAREST = "lowest", "nearest"
NAN = np.float32(np.nan)


def _raster(dsm):
    dsm = np.asarray(dsm)
    assert dsm.ndim == 2 and dsm.dtype == np.float32 and dsm.size
    return dsm


def joins(dsm, max_diff):
    """(east, south): whether a cell is joined to its eastern / southern neighbour — both finite and
    fabsf(a − b) <= max_diff, the subtraction in fp32."""
    dsm = _raster(dsm)
    fin = np.isfinite(dsm)
    md = np.float32(max_diff)
    east, south = np.zeros(dsm.shape, bool), np.zeros(dsm.shape, bool)
    with np.errstate(invalid="ignore", over="ignore"):
        east[:, :-1] = fin[:, :-1] & fin[:, 1:] & (np.abs(dsm[:, :-1] - dsm[:, 1:]) <= md)
        south[:-1] = fin[:-1] & fin[1:] & (np.abs(dsm[:-1] - dsm[1:]) <= md)
    return east, south


def components(dsm, max_diff):
    """(label, size) int32: the smallest linear index of the cell's component and its number of cells; −1 and 0
    at a hole.  Cells are visited in index order, so a search starts at its component's smallest index."""
    dsm = _raster(dsm)
    H, W = dsm.shape
    east, south = joins(dsm, max_diff)
    fin = np.isfinite(dsm)
    label, size = np.full((H, W), -1, np.int32), np.zeros((H, W), np.int32)
    for y0 in range(H):
        for x0 in range(W):
            if not fin[y0, x0] or label[y0, x0] >= 0:
                continue
            root, cells, queue = y0 * W + x0, [], collections.deque([(y0, x0)])
            label[y0, x0] = root
            while queue:
                y, x = queue.popleft()
                cells.append((y, x))
                for yy, xx, ok in ((y, x + 1, east[y, x]), (y + 1, x, south[y, x]), (y, x - 1, x > 0 and east[y, x - 1]),
                                   (y - 1, x, y > 0 and south[y - 1, x])):
                    if ok and label[yy, xx] < 0:
                        label[yy, xx] = root
                        queue.append((yy, xx))
            for y, x in cells:
                size[y, x] = len(cells)
    return label, size


def speckle(dsm, max_diff, max_size, parts=None):
    """(out, label, size); ``parts`` is ``components(dsm, max_diff)`` where the caller has it."""
    dsm = _raster(dsm)
    label, size = parts if parts is not None else components(dsm, max_diff)
    out = dsm.copy()
    out[(size >= 1) & (size <= max_size)] = NAN
    return out, label, size


def median(dsm, radius, min_count=1, fill=False):
    dsm = _raster(dsm)
    H, W = dsm.shape
    r = int(radius)
    pad = np.full((H + 2 * r, W + 2 * r), NAN, np.float32)
    pad[r:r + H, r:r + W] = np.where(np.isfinite(dsm), dsm, NAN)
    stack = np.stack([pad[j:j + H, i:i + W] for j in range(2 * r + 1) for i in range(2 * r + 1)])
    ordered = np.sort(stack, axis=0)                                     # the NaN go last
    n = np.isfinite(stack).sum(0)
    rank = np.maximum(n - 1, 0) // 2
    value = np.take_along_axis(ordered, rank[None], 0)[0] + np.float32(0.0)   # −0 comes out as +0
    out = np.where(n >= min_count, value, NAN).astype(np.float32)
    if not fill:
        hole = ~np.isfinite(dsm)
        out[hole] = dsm[hole]
    return out


def fill(dsm, reach, mode=LOWEST, min_dirs=1):
    """(out, filled uint8)."""
    dsm = _raster(dsm)
    assert mode in (LOWEST, NEAREST)
    H, W = dsm.shape
    fin = np.isfinite(dsm)
    out, filled = dsm.copy(), np.zeros((H, W), np.uint8)
    for y, x in zip(*np.nonzero(~fin)):
        found, best, best_d2 = 0, None, None
        for dy, dx in DIRECTIONS:
            for n in range(1, int(reach) + 1):
                yy, xx = y + n * dy, x + n * dx
                if not (0 <= yy < H and 0 <= xx < W):
                    break
                if fin[yy, xx]:
                    v, d2 = dsm[yy, xx], (2 if dy and dx else 1) * n * n
                    if found == 0 or (v < best if mode == LOWEST else d2 < best_d2):
                        best, best_d2 = v, d2
                    found += 1
                    break
        if found >= min_dirs:
            out[y, x], filled[y, x] = best, 1
    return out, filled


def chain(dsm, max_diff, max_size, weight=None, min_weight=None, radius=1, reach=None, mode=LOWEST, min_dirs=1):
    """``clean_dsm``'s dict: dsm, rejected (1 weight, 2 speckle, 4 changed by the median), filled, label, size."""
    cur = _raster(dsm)
    rejected = np.zeros(cur.shape, np.uint8)
    if weight is not None:
        with np.errstate(invalid="ignore"):
            low = np.isfinite(cur) & ~(np.asarray(weight, np.float32) >= np.float32(min_weight))
        rejected[low] |= 1
        cur = np.where(low, NAN, cur).astype(np.float32)
    out, label, size = speckle(cur, max_diff, max_size)
    rejected[np.isfinite(cur) & ~np.isfinite(out)] |= 2
    cur = out
    if radius:
        out = median(cur, radius)
        rejected[np.isfinite(cur) & (out != cur)] |= 4
        cur = out
    filled = np.zeros(cur.shape, np.uint8)
    if reach is not None:
        cur, filled = fill(cur, reach, mode, min_dirs)
    return {"dsm": cur, "rejected": rejected, "filled": filled, "label": label, "size": size}
