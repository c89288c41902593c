"""The cases the occlusion exports are checked on, shared by tests/test_occlusion_ref.py (CPU: the numpy
statement alone) and tests/test_gpu_occlusion.py (the device against it).  Inputs and references are
computed once per process and never modified.

Floors: DSMs of 1 x 1, 1 x 7, 7 x 1, 17 x 33 and 33 x 65 cells of 0.5 m — smooth relief plus boxes, NaN
cells on the two larger grids — under eleven lines of sight: along each axis (due east, due north),
|a| = |b|, vertical, a grazing one (u = 0.02: the march runs to the grid's edge unless the early stop ends
it), two more, and the four shipped cameras' (``rectify_numpy.view_directions`` on the ``flat`` grid).

``box``: the four shipped cameras and the texture T of tests/sweep_cases.py on a grid of 49 x 65 cells of
0.5 m; the ground at z0 = −16 m, a box of 16 x 16 cells with its roof at z0 + 16 m; 9 planes one metre apart
from z0 − 4, radius 4.  Every pixel is imaged with occlusion: localised at the roof's altitude it takes
the roof's texture — T shifted by (40 m, −25 m), uncorrelated with the ground's — where that point lies in
the footprint; otherwise it is localised at z0 and takes the constant 0.5 of a wall where the segment
between the two points crosses the footprint, else T.  The floor comes from the true DSM; slack 0.5 m.
"""
import functools

import numpy as np

import occlusion_numpy as oc
import rectify_cases as rc
import rectify_numpy as rn
import sweep_cases as sc
import sweep_numpy as sw
from oracle import dsm_ref

RESOLUTION = 0.5
FLOOR_SHAPES = ((1, 1), (1, 7), (7, 1), (17, 33), (33, 65))
_SEEDS = {(1, 1): 11, (1, 7): 12, (7, 1): 13, (17, 33): 14, (33, 65): 15}


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def camera_dirs():
    """The four shipped cameras' lines of sight on the ``flat`` scene's grid, (4, 3) float32."""
    s = sc.BY_NAME["flat"]
    dirs, _ = rn.view_directions(s.grid, sc.ref_cameras(s), s.alt_lo, s.alt_lo + (s.planes - 1) * s.step)
    return _frozen(np.ascontiguousarray(dirs, np.float32))


@functools.lru_cache(maxsize=None)
def dirs():
    """(11, 3) float32: the lines of sight of the floor cases."""
    fixed = np.array([[0.6, 0.0, 0.8],                      # due east: q = 0
                      [0.0, 0.6, 0.8],                      # due north
                      [-0.5, 0.5, np.sqrt(0.5)],            # |a| = |b|
                      [0.0, 0.0, 1.0],                      # vertical: no step
                      [0.8, -0.6, 0.02],                    # grazing
                      [-0.3, -0.7, 0.5], [0.35, 0.2, 0.9]], np.float32)
    assert fixed[0, 1] == 0.0 and fixed[1, 0] == 0.0 and abs(fixed[2, 0]) == abs(fixed[2, 1])
    return _frozen(np.concatenate([fixed, camera_dirs()]))


@functools.lru_cache(maxsize=None)
def heights(shape):
    """The DSM of a floor case, float64 (read-only): relief of ±10 m, boxes of 3 to 25 m, 3 % NaN on the larger grids."""
    H, W = shape
    g = np.random.default_rng(_SEEDS[shape])
    jj, ii = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    h = np.zeros(shape)
    for _ in range(3):
        kx, ky, p = g.uniform(0.02, 0.25), g.uniform(0.02, 0.25), g.uniform(0, 2 * np.pi)
        h += 3.0 * np.sin(kx * ii + ky * jj + p)
    for _ in range(4 if H * W > 64 else 1):
        j0, i0 = int(g.integers(0, H)), int(g.integers(0, W))
        h[j0:j0 + int(g.integers(1, 12)), i0:i0 + int(g.integers(1, 12))] += g.uniform(3.0, 25.0)
    if H * W > 64:
        h[g.random(shape) < 0.03] = np.nan
    return _frozen(h)


@functools.lru_cache(maxsize=None)
def ref_floor64(shape):
    """(11, H, W) float64: the statement's floors of ``heights(shape)`` before the cast."""
    return _frozen(oc.floor64(heights(shape), RESOLUTION, dirs()))


# ---- the box scene -------------------------------------------------------------------------------------

Z0, ROOF = sc.Z0, sc.Z0 + 16.0
BOX_ROWS, BOX_COLS = (26, 42), (24, 40)                     # 16 x 16 cells; view 3's strip lies north of it
SLACK = 0.5
GROUND_PLANE = 4
BOX = sc.Scene("box", sc._jax((49, 65)), (0, 1, 2, 3), "texture", 1, Z0 - 4.0, 1.0, 9, 4, 2)


def footprint():
    """(E0, E1, N0, N1): the box's footprint in UTM metres."""
    g = BOX.grid
    return (g.xoff + BOX_COLS[0] * g.resolution, g.xoff + BOX_COLS[1] * g.resolution,
            g.ytop - BOX_ROWS[1] * g.resolution, g.ytop - BOX_ROWS[0] * g.resolution)


def _crosses(e0, n0, e1, n1, box):
    """Whether the segment (e0, n0) → (e1, n1) meets the rectangle: the slab test."""
    E0, E1, N0, N1 = box
    t_in, t_out = np.zeros(e0.shape), np.ones(e0.shape)
    ok = np.ones(e0.shape, bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        for p, d, lo, hi in ((e0, e1 - e0, E0, E1), (n0, n1 - n0, N0, N1)):
            still = d == 0.0
            ok &= ~still | ((p >= lo) & (p <= hi))
            ta, tb = np.where(still, 0.0, (lo - p) / d), np.where(still, 1.0, (hi - p) / d)
            t_in, t_out = np.maximum(t_in, np.minimum(ta, tb)), np.minimum(t_out, np.maximum(ta, tb))
    return ok & (t_in <= t_out)


@functools.lru_cache(maxsize=None)
def box_dsm():
    dsm = np.full(BOX.grid.shape, Z0)
    dsm[BOX_ROWS[0]:BOX_ROWS[1], BOX_COLS[0]:BOX_COLS[1]] = ROOF
    return _frozen(dsm)


@functools.lru_cache(maxsize=None)
def box_images():
    """The four images of the box scene, (h, w, 1) float32 each (read-only)."""
    box = footprint()
    E0, E1, N0, N1 = box
    out = []
    for v, cam in zip(BOX.views, sc.ref_cameras(BOX)):
        h, w = rc.sizes()[v]
        im = np.zeros((h, w, 1), np.float32)
        reach = np.concatenate([sw.pix_at(BOX.grid, [cam], a)[0].reshape(-1, 2) for a in (Z0 - 5.0, Z0 + 5.0)])
        c0, r0 = np.maximum(np.floor(reach.min(0)).astype(int) - 3, 0)
        c1, r1 = np.minimum(np.ceil(reach.max(0)).astype(int) + 4, (w, h))
        cols, rows = np.meshgrid(np.arange(c0, c1, dtype=np.float64), np.arange(r0, r1, dtype=np.float64))
        cols, rows = cols.ravel(), rows.ravel()
        lon, lat = cam.localization(cols, rows, np.full(cols.size, ROOF))
        er, nr = dsm_ref.utm(lat, lon, BOX.grid.zone, BOX.grid.south)
        lon, lat = cam.localization(cols, rows, np.full(cols.size, Z0))
        eg, ng = dsm_ref.utm(lat, lon, BOX.grid.zone, BOX.grid.south)
        roof = (er >= E0) & (er <= E1) & (nr >= N0) & (nr <= N1)
        wall = ~roof & _crosses(er, nr, eg, ng, box)
        val = np.where(roof, sc.texture(er + 40.0, nr - 25.0), np.where(wall, 0.5, sc.texture(eg, ng)))
        im[r0:r1, c0:c1, 0] = val.reshape(r1 - r0, c1 - c0)
        out.append(_frozen(np.ascontiguousarray(im)))
    return out


@functools.lru_cache(maxsize=None)
def box_dirs():
    d, _ = rn.view_directions(BOX.grid, sc.ref_cameras(BOX), BOX.alt_lo, BOX.alt_lo + (BOX.planes - 1) * BOX.step)
    return _frozen(np.ascontiguousarray(d, np.float32))


@functools.lru_cache(maxsize=None)
def box_floor():
    """(4, 49, 65) float32: the statement's floor of the true DSM under the cameras' lines of sight."""
    return _frozen(oc.floor(box_dsm(), BOX.grid.resolution, box_dirs()))


@functools.lru_cache(maxsize=None)
def box_sweeps():
    """(gated, ungated): the statement with and without the gate (dicts of read-only arrays)."""
    s, imgs, cams = BOX, box_images(), sc.ref_cameras(BOX)
    gated = oc.sweep(imgs, cams, s.grid, s.alt_lo, s.step, s.planes, box_floor(), SLACK, s.radius, s.min_views)
    plain = sw.sweep(imgs, cams, s.grid, s.alt_lo, s.step, s.planes, s.radius, s.min_views)
    _frozen(*gated.values())
    _frozen(*plain.values())
    return gated, plain


def strip():
    """The ground cells where the floor gates at least one view somewhere in the window at the ground plane
    while at least two views stay usable (the gated statement's view count there)."""
    gated, _ = box_sweeps()
    ground = box_dsm() == Z0
    touched = oc.in_window(gated["gated"][GROUND_PLANE], BOX.radius).any(0)
    return ground & touched & (gated["views_vol"][GROUND_PLANE] >= 2)


# ---- floors for the fused sweep against its staged chain ----------------------------------------------

def seeded_floor(V, shape, alt_lo, step, K, slack, seed=0):
    """(V, H, W) float32 straddling the planes, constant per view on blocks of 8 x 8 cells so that windows
    survive: a third of the blocks exactly on some alt_k + slack (fp32 numbers for the dyadic planes used), a
    sixth −inf, the rest uniform from 3 steps below the planes to a step above them; 5 % of the entries NaN
    and 0.3 % +inf on top; and view 0 gated at every plane over the grid's first 24 x 24 cells — more than a
    16-cell tile and its halo, so whole runs are skipped."""
    H, W = shape
    g = np.random.default_rng(7000 + 100 * V + 10 * H + W + K + seed)
    bh, bw = (H + 7) // 8, (W + 7) // 8
    kind = g.random((V, bh, bw))
    on = (np.float64(alt_lo) + g.integers(0, K, (V, bh, bw)).astype(np.float64) * np.float64(step) + np.float64(slack)).astype(np.float32)
    blocks = g.uniform(alt_lo - 3 * step, alt_lo + (K + 1) * step, (V, bh, bw)).astype(np.float32)
    blocks = np.where(kind < 1 / 3, on, np.where(kind < 0.5, np.float32(-np.inf), blocks))
    f = np.repeat(np.repeat(blocks, 8, 1), 8, 2)[:, :H, :W].copy()
    f[g.random((V, H, W)) < 0.05] = np.nan
    f[g.random((V, H, W)) < 0.003] = np.inf
    f[0, :24, :24] = np.float32(alt_lo + (K + 3) * step)
    return f
