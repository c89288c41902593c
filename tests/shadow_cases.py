"""The cases the geometric shadows are checked on, shared by tests/test_shadow_ref.py (CPU: the
numpy statement alone) and tests/test_gpu_shadow.py (the device against it).  The references are
computed once per process and never modified.

Shapes: 1 x 1, 1 x 7 and 7 x 1 (no interpolation partner, marches of no step); 33 x 65, ragged
against a 64-wide wavefront and the 4-row workgroup tile; 130 x 257, several workgroup rows and
columns.  Heights: smooth relief of ±20 m plus a few boxes; on the two larger grids 2 % of the cells
are NaN.  Directions: eleven — one azimuth in each of the eight octants at elevations of 8°…70°,
exactly north-east and exactly due east among them (as vectors: ``sun_direction(el, 90)`` has a north
component of 5e-17, not 0), one at 2° whose march runs to the grid's edge, one more steep one, and
the zenith.
"""
import functools
import math

import numpy as np

import shadow_numpy as sn

RESOLUTION = 0.5
SHAPES = ((1, 1), (1, 7), (7, 1), (33, 65), (130, 257))
SEEDS = {(1, 1): 1, (1, 7): 2, (7, 1): 3, (33, 65): 4, (130, 257): 5}


def _vector(el, az):
    el, az = math.radians(el), math.radians(az)
    return [math.sin(az) * math.cos(el), math.cos(az) * math.cos(el), math.sin(el)]


_C25, _S25 = math.cos(math.radians(25.0)), math.sin(math.radians(25.0))
DIRS = np.array([
    _vector(12.0, 20.0),                                             # octant 0: rows, towards the north
    [_C25 * math.sqrt(0.5), _C25 * math.sqrt(0.5), _S25],            # exactly north-east: |a| = |b|, q = -1
    [math.cos(math.radians(35.0)), 0.0, math.sin(math.radians(35.0))],   # exactly due east: q = 0
    _vector(8.0, 155.0), _vector(40.0, 200.0), _vector(70.0, 245.0), _vector(18.0, 290.0), _vector(55.0, 335.0),
    _vector(2.0, 100.0),                                             # grazing: the march runs to the edge
    _vector(63.0, 110.0),
    [0.0, 0.0, 1.0],                                                 # the zenith: no step
], np.float32)
assert DIRS.shape == (11, 3) and DIRS[1, 0] == DIRS[1, 1] and DIRS[2, 1] == 0.0


@functools.lru_cache(maxsize=None)
def heights(shape):
    """The DSM of a shape, float64 (read-only)."""
    H, W = shape
    g = np.random.default_rng(SEEDS[shape])
    jj, ii = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    h = np.zeros(shape)
    for _ in range(4):
        kx, ky, p = g.uniform(0.02, 0.25), g.uniform(0.02, 0.25), g.uniform(0, 2 * np.pi)
        h += 5.0 * np.sin(kx * ii + ky * jj + p)
    for _ in range(4 if H * W > 64 else 1):                                  # a few boxes
        j0, i0 = int(g.integers(0, H)), int(g.integers(0, W))
        h[j0:j0 + int(g.integers(1, 12)), i0:i0 + int(g.integers(1, 12))] += g.uniform(3.0, 25.0)
    if H * W > 64:
        h[g.random(shape) < 0.02] = np.nan
    h.setflags(write=False)
    return h


@functools.lru_cache(maxsize=None)
def reference(shape):
    """(shadow, excess) of the numpy statement for ``heights(shape)`` under DIRS (read-only)."""
    shadow, excess = sn.cast(heights(shape), RESOLUTION, DIRS)
    shadow.setflags(write=False)
    excess.setflags(write=False)
    return shadow, excess


def in_band(shape):
    """The cells whose reference |excess| is within the tolerance: where ``shadow`` may flip."""
    with np.errstate(invalid="ignore"):
        return np.abs(reference(shape)[1]) <= sn.tolerance(heights(shape))
