"""The cases the DSM view is checked on, shared by tests/test_dsmview_ref.py (CPU: the numpy statement alone) and
tests/test_gpu_dsmview.py (the device against it).  Inputs and references are computed once per process and
never modified.

Grids: 33 x 65 and 17 x 33 cells of 0.5 m on the JAX_269 ROI origin of tests/rectify_cases.py, and its 33 x 65
grid in a southern zone seen by a shipped camera moved there.  DSMs: the seeded relief of tests/rectify_cases.py
within [−30, −2] m with 2 % of its cells NaN (the 17 x 33 one its corner); a 10 m box on flat ground; a constant
plane at −16 m; the tilted plane of tests/surface_cases.py; the relief with single NaN and ±inf cells and a NaN
block; all NaN.  Cameras: the four shipped JAX_269 cameras at full resolution (0.3 m pixels: two pixels a cell)
and at downscale 4.  Pixel lattices are centred, give or take an offset, on the pixel the grid's centre projects
to at the middle altitude: 1 x 1, 1 x 7, 7 x 1, 17 x 33 and 40 x 70 pixels (the last straddles the 16 x 16 patches
of the kernel on both axes), stride 1 and 3, inside the grid's footprint, partly off it and wholly off it.
"""
import collections
import functools

import numpy as np

import dsmview_numpy as dn
import rectify_cases as rc
import surface_cases as fc
import sweep_cases as sc
from oracle import rpc_ref
from spnerf_amd.rectify import Camera

Case = collections.namedtuple("Case", "name grid dsm view downscale alt_lo alt_hi shape stride offset")

G33, G17, GS = sc._jax((33, 65)), sc._jax((17, 33)), rc._south()
PLANE_ALT = -16.0
BOX = dict(ground=-28.0, height=10.0, rows=(10, 20), cols=(22, 40))
ALTS, ALTS60 = (-30.0, -2.0), (-46.0, 14.0)

CASES = (
    Case("relief", G33, "relief", 0, 1, *ALTS, (40, 70), 1, (0, 0)),
    Case("relief_s3", G33, "relief", 1, 1, *ALTS, (40, 70), 3, (0, 0)),
    Case("relief_ds4", G33, "relief", 2, 4, *ALTS, (17, 33), 1, (0, 0)),
    Case("relief_17", G17, "relief", 3, 1, *ALTS, (17, 33), 3, (0, 0)),
    Case("relief_edge", G33, "relief", 3, 1, *ALTS, (40, 70), 1, (45, -30)),
    Case("plane", G33, "plane", 0, 1, *ALTS, (40, 70), 1, (0, 0)),
    Case("plane60", G33, "plane", 2, 1, *ALTS60, (40, 70), 1, (0, 0)),
    Case("tilt", G33, "tilt", 1, 1, *ALTS, (40, 70), 1, (0, 0)),
    Case("tilt60", G33, "tilt", 3, 1, *ALTS60, (40, 70), 1, (0, 0)),
    Case("box", G33, "box", 3, 1, -30.0, -10.0, (40, 70), 2, (0, 0)),
    Case("holes", G33, "holes", 3, 1, *ALTS, (40, 70), 1, (0, 0)),
    Case("nan", G17, "nan", 0, 1, *ALTS, (17, 33), 1, (0, 0)),
    Case("south", GS, "south", 0, 1, *ALTS, (40, 70), 1, (0, 0)),
    Case("1x1", G33, "relief", 0, 1, *ALTS, (1, 1), 1, (0, 0)),
    Case("1x7", G33, "relief", 1, 1, *ALTS, (1, 7), 3, (0, 0)),
    Case("7x1", G33, "relief", 2, 1, *ALTS, (7, 1), 1, (0, 0)),
    Case("off", G33, "relief", 0, 1, *ALTS, (17, 33), 1, (3000, -2000)),
)
BY_NAME = {c.name: c for c in CASES}
NAMES = tuple(BY_NAME)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def meta(case):
    return rc.metas(case.grid.south)[case.view]


def camera(case):
    """The case's camera for the library."""
    return Camera.from_meta(meta(case), case.downscale)


def ref_camera(case):
    """The case's camera for the numpy statement."""
    return rpc_ref.RPC(meta(case)["rpc"], case.downscale)


@functools.lru_cache(maxsize=None)
def dsm(name):
    """The case's DSM, (H, W) float32 (read-only)."""
    case = BY_NAME[name]
    H, W = case.grid.shape
    if case.dsm == "relief":
        h = rc.heights("33x65_r05")[:H, :W]
    elif case.dsm == "south":
        h = rc.heights("south")
    elif case.dsm == "plane":
        h = np.full((H, W), PLANE_ALT)
    elif case.dsm == "tilt":
        h = fc.tilt_truth()
    elif case.dsm == "box":
        h = np.full((H, W), BOX["ground"])
        h[BOX["rows"][0]:BOX["rows"][1], BOX["cols"][0]:BOX["cols"][1]] += BOX["height"]
    elif case.dsm == "holes":
        h = fc.base((H, W), "holes").copy()
        h[12:20, 30:44] = np.nan
    else:
        h = np.full((H, W), np.nan)
    return _frozen(np.ascontiguousarray(h, np.float32))


@functools.lru_cache(maxsize=None)
def rect(name):
    """(col0, row0, n_cols, n_rows) of the case's lattice."""
    case = BY_NAME[name]
    g = case.grid
    e, n = g.xoff + 0.5 * g.xsize * g.resolution, g.ytop - 0.5 * g.ysize * g.resolution
    import ortho_numpy as on
    lat, lon = on.utm_inverse(np.array([e]), np.array([n]), g.zone, g.south)
    col, row = ref_camera(case).projection(lon, lat, np.array([0.5 * (case.alt_lo + case.alt_hi)]))
    n_rows, n_cols = case.shape
    col0 = int(round(float(col[0]))) - (n_cols // 2) * case.stride + case.offset[0]
    row0 = int(round(float(row[0]))) - (n_rows // 2) * case.stride + case.offset[1]
    return col0, row0, n_cols, n_rows


@functools.lru_cache(maxsize=None)
def ref(name):
    """The statement's cast of the case (a dict of read-only arrays, ``seg`` a dict of them)."""
    case = BY_NAME[name]
    out = dn.cast(dsm(name), case.grid, ref_camera(case), case.alt_lo, case.alt_hi, rect(name), case.stride)
    _frozen(*[v for v in out.values() if isinstance(v, np.ndarray)], *out["seg"].values())
    return out


@functools.lru_cache(maxsize=None)
def weight(shape, seed=0):
    """A seeded (H, W) float32 raster with NaN and ±inf entries: what ``sample_at`` reads."""
    g = np.random.default_rng(4200 + shape[0] + seed)
    w = g.uniform(-1.0, 1.0, shape).astype(np.float32)
    u = g.random(shape)
    w[u < 0.05] = np.nan
    w[(u >= 0.05) & (u < 0.07)] = np.inf
    w[(u >= 0.07) & (u < 0.09)] = -np.inf
    return _frozen(w)
