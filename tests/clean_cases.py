"""The cases the DSM-cleaning exports are checked on, shared by tests/test_clean_ref.py (CPU: the numpy
statement alone) and tests/test_gpu_clean.py (the device against it).  Everything is seeded, computed once
per process and read-only.  Heights are dyadic wherever equality with ``max_diff`` is meant, so the fp32
subtraction is exact.

Grids: 1 x 1, 1 x 7, 7 x 1, (T − 1) x (T + 1), T x T, (T + 1) x (2T + 1) for the tile T of the header, and
65 x 130.  ``PATTERNS`` names the speckle rasters, each with its ``max_diff``; ``median_raster`` and
``fill_raster`` are random heights with 30 % / seeded holes; ``restoration`` is the box of
tests/occlusion_cases.py (flat ground at −16 m, a roof at 0 m: dyadic) with 12 speckles raised by 20 m.
"""
import functools

import numpy as np

import occlusion_cases as occ

T = 16                                                               # SPNERF_CLEAN_TILE; tests/test_clean_abi.py holds the header to it
GRIDS = ((1, 1), (1, 7), (7, 1), (T - 1, T + 1), (T, T), (T + 1, 2 * T + 1), (65, 130))
NAN = np.float32(np.nan)


def _frozen(a):
    a.setflags(write=False)
    return a


def _seed(shape, salt):
    return 26000 + 1000 * salt + 7 * shape[0] + shape[1]


def serpentine(shape, step=0.25):
    """A path one cell wide over the whole grid — every even row, joined at alternating ends through the odd
    rows — as a ramp of ``step`` per cell along the path: (raster, number of cells on the path)."""
    H, W = shape
    dsm, k = np.full(shape, NAN, np.float32), 0
    for y in range(H):
        if y % 2 == 0:
            cols = range(W) if (y // 2) % 2 == 0 else range(W - 1, -1, -1)
        else:
            cols = [W - 1] if (y // 2) % 2 == 0 else [0]
        for x in cols:
            dsm[y, x] = np.float32(k * step)
            k += 1
    return dsm, k


def spiral(shape):
    """A path one cell wide from the corner inwards, clockwise, a one-cell gap between its turns; constant height."""
    H, W = shape
    on = np.zeros(shape, bool)
    y, x, d = 0, 0, 0
    steps = ((0, 1), (1, 0), (0, -1), (-1, 0))
    on[0, 0] = True

    def free(y, x, d):
        y1, x1, y2, x2 = y + steps[d][0], x + steps[d][1], y + 2 * steps[d][0], x + 2 * steps[d][1]
        if not (0 <= y1 < H and 0 <= x1 < W) or on[y1, x1]:
            return False
        return not (0 <= y2 < H and 0 <= x2 < W and on[y2, x2])

    while True:
        if not free(y, x, d):
            d = (d + 1) % 4
            if not free(y, x, d):
                break
        y, x = y + steps[d][0], x + steps[d][1]
        on[y, x] = True
    return np.where(on, np.float32(5.0), NAN).astype(np.float32)


def ulp_ramp(n, step):
    """n fp32 values whose successive differences are exact in fp32 and one ulp (of the sum) above ``step``."""
    out, step = [np.float32(0.0)], np.float32(step)
    for _ in range(n - 1):
        out.append(np.nextafter(np.float32(out[-1] + step), np.float32(np.inf)))
    out = np.array(out, np.float32)
    assert n == 1 or bool(((out[1:] - out[:-1]) > step).all())
    return out


def _random4(shape):
    g = np.random.default_rng(_seed(shape, 1))
    dsm = g.integers(0, 4, shape).astype(np.float32)
    dsm[g.random(shape) < 0.2] = NAN
    dsm[g.random(shape) < 0.02] = np.float32(np.inf)
    dsm[g.random(shape) < 0.02] = np.float32(-np.inf)
    return dsm, 1.0


def _comb(shape):
    H, W = shape
    dsm = np.full(shape, NAN, np.float32)
    dsm[0] = 2.0                                                          # the spine; the teeth run down every other column
    dsm[:, ::2] = 2.0
    return dsm, 0.0


def _checkerboard(shape):
    jj, ii = np.indices(shape)
    return np.where((jj + ii) % 2 == 0, np.float32(0.0), np.float32(10.0)).astype(np.float32), 1.0


def _walls(shape):
    """NaN walls along the first tile border in each direction (the last column / row of the first tile), a single gap each."""
    H, W = shape
    dsm = np.full(shape, 3.0, np.float32)
    if W > T:
        dsm[:, T - 1] = NAN
        dsm[H // 2, T - 1] = 3.0
    if H > T:
        dsm[T - 1, :] = NAN
        dsm[T - 1, W // 3] = 3.0
    return dsm, 0.5


def _diagonal(shape):
    jj, ii = np.indices(shape)
    return np.where((jj + ii) % 2 == 0, np.float32(1.0), NAN).astype(np.float32), 8.0


def _exact(shape):
    """Rows 0, 4, 8, …: a ramp of steps exactly ``max_diff`` (one component each); rows 2, 6, …: a ramp of steps one
    ulp larger (W components each); NaN rows between them."""
    H, W = shape
    dsm = np.full(shape, NAN, np.float32)
    for y in range(0, H, 2):
        dsm[y] = np.arange(W, dtype=np.float32) * np.float32(0.25) if y % 4 == 0 else ulp_ramp(W, 0.25)
    return dsm, 0.25


PATTERNS = {"random4": _random4, "serpentine": lambda s: (serpentine(s)[0], 0.25), "spiral": lambda s: (spiral(s), 0.0), "comb": _comb,
            "checkerboard": _checkerboard, "whole": lambda s: (np.full(s, -7.5, np.float32), 0.0), "walls": _walls, "diagonal": _diagonal,
            "exact": _exact}


@functools.lru_cache(maxsize=None)
def pattern(name, shape):
    """(raster float32 read-only, max_diff)."""
    dsm, max_diff = PATTERNS[name](shape)
    assert dsm.dtype == np.float32 and dsm.shape == tuple(shape)
    return _frozen(dsm), max_diff


@functools.lru_cache(maxsize=None)
def median_raster(shape):
    """Heights on a grid of 1/8 m (many ties), 30 % NaN, a few ±inf, and both zeros."""
    g = np.random.default_rng(_seed(shape, 2))
    dsm = (g.integers(-40, 41, shape) / 8.0).astype(np.float32)
    dsm[dsm == 0.0] = np.where(g.random(int((dsm == 0.0).sum())) < 0.5, np.float32(-0.0), np.float32(0.0))
    dsm[g.random(shape) < 0.3] = NAN
    dsm[g.random(shape) < 0.01] = np.float32(np.inf)
    return _frozen(dsm)


@functools.lru_cache(maxsize=None)
def zeros_raster(shape=(T + 1, 2 * T + 1)):
    """Only −0.0 and +0.0, and 20 % NaN: every median is a zero and must come out as +0."""
    g = np.random.default_rng(_seed(shape, 3))
    dsm = np.where(g.random(shape) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    dsm[g.random(shape) < 0.2] = NAN
    assert np.signbit(dsm).any() and (~np.signbit(dsm) & (dsm == 0)).any()
    return _frozen(dsm)


@functools.lru_cache(maxsize=None)
def fill_raster(shape):
    """Random heights with single-cell holes (10 %), holes at the four corners and along the edges, a square hole of
    9 x 9 cells (wider than a reach of 3) where the grid has room, and an inf."""
    H, W = shape
    g = np.random.default_rng(_seed(shape, 4))
    dsm = (g.integers(-80, 81, shape) / 4.0).astype(np.float32)
    dsm[g.random(shape) < 0.1] = NAN
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H // 2, 0), (H - 1, W // 2), (H // 2, W - 1)):
        dsm[y, x] = NAN
    if H >= 15 and W >= 15:
        dsm[3:12, 4:13] = NAN
        dsm[2, 2] = np.float32(np.inf)
    return _frozen(dsm)


@functools.lru_cache(maxsize=None)
def chain_case(k):
    """(raster, weight): a swept-looking raster on 33 x 50 cells — plateaus on the plane grid of 0.5 m, seeded outlier
    blobs, 5 % holes — and a weight in [0, 1) on a grid of 1/64 with 2 % NaN."""
    shape = (33, 50)
    g = np.random.default_rng(26900 + k)
    jj, ii = np.indices(shape)
    dsm = (np.round(2.0 * (3.0 * np.sin(0.21 * ii + k) + 2.0 * np.cos(0.17 * jj))) / 2.0).astype(np.float32)
    for _ in range(14):
        y, x, h, w = int(g.integers(0, 31)), int(g.integers(0, 48)), int(g.integers(1, 4)), int(g.integers(1, 4))
        dsm[y:y + h, x:x + w] += np.float32(g.integers(8, 40) / 2.0)
    dsm[g.random(shape) < 0.05] = NAN
    weight = (g.integers(0, 64, shape) / 64.0).astype(np.float32)
    weight[g.random(shape) < 0.02] = NAN
    return _frozen(dsm), _frozen(weight)


# ---- the restoration case: the box of tests/occlusion_cases.py with 12 speckles ---------------------------

SPECKLES, SPECKLE_MAX, RAISED = 12, 6, np.float32(20.0)


@functools.lru_cache(maxsize=None)
def restoration():
    """(original, corrupted, speckle mask): the box raster in fp32 — its two heights are dyadic — and the same with 12
    seeded 4-connected speckles of 1 to ``SPECKLE_MAX`` cells raised by 20 m, none within 2 cells of the box or of
    another speckle."""
    original = occ.box_dsm().astype(np.float32)
    assert bool((original.astype(np.float64) == occ.box_dsm()).all()) and set(np.unique(original)) == {np.float32(occ.Z0), np.float32(occ.ROOF)}
    H, W = original.shape
    g = np.random.default_rng(2026)
    taken = original != np.float32(occ.Z0)                              # the box, then every speckle placed
    mask = np.zeros((H, W), bool)

    def near(cells):
        for y, x in cells:
            if taken[max(y - 2, 0):y + 3, max(x - 2, 0):x + 3].any():
                return True
        return False

    sizes = [1, SPECKLE_MAX] + [int(g.integers(1, SPECKLE_MAX + 1)) for _ in range(SPECKLES - 2)]
    for size in sizes:
        for _ in range(10000):
            cells = [(int(g.integers(0, H)), int(g.integers(0, W)))]
            while len(cells) < size:
                y, x = cells[int(g.integers(0, len(cells)))]
                dy, dx = ((0, 1), (1, 0), (0, -1), (-1, 0))[int(g.integers(0, 4))]
                if 0 <= y + dy < H and 0 <= x + dx < W and (y + dy, x + dx) not in cells:
                    cells.append((y + dy, x + dx))
            if not near(cells):
                break
        else:
            raise AssertionError("no room for a speckle")
        for y, x in cells:
            mask[y, x] = taken[y, x] = True
    corrupted = original.copy()
    corrupted[mask] += RAISED
    return _frozen(original), _frozen(corrupted), _frozen(mask)
