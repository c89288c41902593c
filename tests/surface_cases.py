"""The cases the surface sweep is checked on, shared by tests/test_surface_ref.py (CPU: the numpy statement
alone) and tests/test_gpu_surface.py (the device against it).  Inputs and references are computed once per
process and never modified.

Scene ``tilt``: the texture T of tests/sweep_cases.py on the plane z = Z0 + SLOPE·(E − E_centre), imaged into
the four shipped cameras by iterating every pixel's localisation to the tilted plane (the altitude changes by
SLOPE times the easting, the easting by about a third of the altitude: a contraction of 0.1 per round, twelve
rounds), swept on 33 x 65 cells of 0.5 m with radius 4 and 9 offsets one metre apart centred on 0.  Across the
32.5 m of the grid the plane rises by 8.1 m, so no horizontal plane fits a 4.5 m window better than to
±0.56 m and the whole grid needs nine of them.

Bases for the other scenes of tests/sweep_cases.py are seeded: a smooth bump of a few metres around the
middle of the scene's planes, with single NaN and ±inf cells, a NaN block larger than a tile and its halo,
or all NaN.
"""
import functools

import numpy as np

import rectify_cases as rc
import surface_numpy as sn
import sweep_cases as sc
import sweep_numpy as sw
from oracle import dsm_ref

SLOPE = 0.25
TILT = sc.Scene("tilt", sc._jax((33, 65)), (0, 1, 2, 3), "tilt", 1, -4.0, 1.0, 9, 4, 2)    # alt_lo is off_lo here
E_CENTRE = TILT.grid.xoff + 0.5 * TILT.grid.xsize * TILT.grid.resolution
ROUNDS = 12


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def tilt_height(E):
    return sc.Z0 + SLOPE * (E - E_CENTRE)


@functools.lru_cache(maxsize=None)
def tilt_truth():
    """The tilted plane at the cell centres, (33, 65) float32."""
    E, _ = TILT.grid.cell_centres()
    return _frozen(tilt_height(E).astype(np.float32))


@functools.lru_cache(maxsize=None)
def tilt_images():
    out = []
    for v, cam in zip(TILT.views, sc.ref_cameras(TILT)):
        h, w = rc.sizes()[v]
        im = np.zeros((h, w, 1), np.float32)
        reach = np.concatenate([sw.pix_at(TILT.grid, [cam], a)[0].reshape(-1, 2) for a in (sc.Z0 - 12.0, sc.Z0 + 12.0)])
        c0, r0 = np.maximum(np.floor(reach.min(0)).astype(int) - 3, 0)
        c1, r1 = np.minimum(np.ceil(reach.max(0)).astype(int) + 4, (w, h))
        cols, rows = np.meshgrid(np.arange(c0, c1, dtype=np.float64), np.arange(r0, r1, dtype=np.float64))
        z = np.full(cols.size, sc.Z0)
        for _ in range(ROUNDS):
            lon, lat = cam.localization(cols.ravel(), rows.ravel(), z)
            e, n = dsm_ref.utm(lat, lon, TILT.grid.zone, TILT.grid.south)
            z = tilt_height(e)
        im[r0:r1, c0:c1, 0] = sc.texture(e, n).reshape(cols.shape)
        out.append(_frozen(np.ascontiguousarray(im)))
    return out


def images(name):
    return tilt_images() if name == "tilt" else sc.images(name)


def scene(name):
    return TILT if name == "tilt" else sc.BY_NAME[name]


@functools.lru_cache(maxsize=None)
def ref_tilt(shift=0.0):
    """The surface statement on ``tilt`` around truth + shift (a dict of read-only arrays)."""
    base = (tilt_truth().astype(np.float64) + shift).astype(np.float32)
    out = sn.sweep(tilt_images(), sc.ref_cameras(TILT), TILT.grid, base, TILT.alt_lo, TILT.step, TILT.planes, TILT.radius, TILT.min_views)
    out["base"] = base
    _frozen(*out.values())
    return out


def tilt_planes():
    """(alt_lo, step, planes) of the horizontal sweep over the altitudes the nine surfaces around the truth reach."""
    lo = float(np.floor(tilt_truth().min())) + TILT.alt_lo
    hi = float(np.ceil(tilt_truth().max())) - TILT.alt_lo
    return lo, TILT.step, int(round((hi - lo) / TILT.step)) + 1


@functools.lru_cache(maxsize=None)
def ref_tilt_planes():
    lo, step, K = tilt_planes()
    out = sw.sweep(tilt_images(), sc.ref_cameras(TILT), TILT.grid, lo, step, K, TILT.radius, TILT.min_views)
    _frozen(*out.values())
    return out


BASES = ("smooth", "holes", "block", "nan")


@functools.lru_cache(maxsize=None)
def base(shape, kind="smooth", centre=-16.0, seed=0):
    """A seeded (H, W) float32 base: ``smooth`` — a bump of ±3 m around ``centre`` plus 0.1 m of noise; ``holes`` — that
    with NaN, +inf and −inf cells (1 % each kind, and the first cell NaN); ``block`` — that with rows 2..27 and columns
    3..30 NaN (26 x 28 cells: more than a tile and its halo at radius 4; the whole raster on a smaller grid) and the
    ``holes``; ``nan`` — all NaN."""
    H, W = shape
    g = np.random.default_rng(7000 + 100 * H + W + seed)
    j, i = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    b = (centre + 3.0 * np.sin(0.19 * j + 0.4) * np.cos(0.13 * i) + 0.1 * g.standard_normal((H, W))).astype(np.float32)
    if kind in ("holes", "block"):
        u = g.random((H, W))
        b[u < 0.01] = np.nan
        b[(u >= 0.01) & (u < 0.02)] = np.inf
        b[(u >= 0.02) & (u < 0.03)] = -np.inf
        b[0, 0] = np.nan
    if kind == "block":
        b[2:28, 3:31] = np.nan
    if kind == "nan":
        b[:] = np.nan
    return _frozen(b)
