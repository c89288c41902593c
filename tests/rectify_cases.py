"""The cases the orthorectification is checked on, shared by tests/test_rectify_ref.py (CPU: the numpy
statement alone) and tests/test_gpu_rectify.py (the device against it).  Inputs and references are
computed once per process and never modified.

Grids: 1 x 1, 1 x 7 and 7 x 1 (single cells, rows and columns); 33 x 65, ragged against a 256-thread
workgroup; 130 x 257, many workgroups — each at 0.5 m and at 2 m on the JAX_269 ROI origin of
tests/test_gpu_ortho.py (at 2 m the large grids reach far beyond the images: whole regions are
invalid), and one 33 x 65 grid in a southern zone 2.9° from its central meridian, seen by a shipped
camera moved there.  DSMs: seeded relief within [−30, −2] m, 2 % of the cells NaN on the larger grids
and one NaN on the 1 x 7 one; and a 30 m box on flat ground.  Cameras: the four shipped JAX_269
cameras at downscale 4, as V = 1, 3 and 4 of them (a launch loops over its camera table, so there is no
fixed number of views per launch to go beyond; the GPU test repeats cameras up to V = 9 all the same).
Images: seeded noise (C = 3 and 4), a linear ramp a·col + b·row + c whose values are exact in fp32
(C = 1 and 3), and the shipped JAX_269 pixels.
"""
import collections
import copy
import functools
import os

import numpy as np

import rectify_numpy as rn
import shadow_numpy as sn
from oracle import dsm_ref, rpc_ref
from spnerf_amd import GroundGrid
from spnerf_amd.rectify import Camera
from spnerf_amd.satellite import DATA, load_cameras

DOWNSCALE = 4
ROI_XOFF, ROI_YTOP = 438638.996411, 3353399.999928 + 256.0           # tests/test_gpu_ortho.py
ALT_LO, ALT_HI = -30.0, -2.0
VIEWS = ("JAX_269_006_RGB", "JAX_269_007_RGB", "JAX_269_011_RGB", "JAX_269_023_RGB")
SOUTH_LAT, SOUTH_LON, SOUTH_ZONE = -33.9, 15.0 + 2.9, 33                # tests/test_gpu_ortho.py
PIX_TOL = 1e-5                                                          # pixels: the GPU test's bound on pix
RAMP = np.array([[1 / 64, 1 / 128, 0.25], [-1 / 128, 1 / 32, 2.0], [1 / 256, -1 / 64, 4.0]])   # a, b, c per channel

Case = collections.namedtuple("Case", "name grid dsm views images channels alt_lo alt_hi")


def _jax(shape, res):
    return GroundGrid(ROI_XOFF, ROI_YTOP, shape[1], shape[0], res, 17)


def _south():
    e, n = dsm_ref.utm(SOUTH_LAT, SOUTH_LON, SOUTH_ZONE, south=True)
    return GroundGrid(float(e) - 16.0, float(n) + 8.0, 65, 33, 0.5, SOUTH_ZONE, south=True)


CASES = (
    Case("1x1_r05", _jax((1, 1), 0.5), "relief", (0,), "noise", 3, ALT_LO, ALT_HI),
    Case("1x1_r2", _jax((1, 1), 2.0), "relief", (1, 2, 3), "ramp", 3, ALT_LO, ALT_HI),
    Case("1x7_r05", _jax((1, 7), 0.5), "relief", (0, 1, 2, 3), "real", 3, ALT_LO, ALT_HI),
    Case("1x7_r2", _jax((1, 7), 2.0), "relief", (2,), "ramp", 1, ALT_LO, ALT_HI),
    Case("7x1_r05", _jax((7, 1), 0.5), "relief", (3, 0, 1), "noise", 3, ALT_LO, ALT_HI),
    Case("7x1_r2", _jax((7, 1), 2.0), "relief", (0, 1, 2, 3), "ramp", 3, ALT_LO, ALT_HI),
    Case("33x65_r05", _jax((33, 65), 0.5), "relief", (0, 2, 3), "noise", 4, ALT_LO, ALT_HI),
    Case("33x65_r2", _jax((33, 65), 2.0), "relief", (0, 1, 2, 3), "ramp", 3, ALT_LO, ALT_HI),
    Case("130x257_r05", _jax((130, 257), 0.5), "relief", (0, 1, 2, 3), "real", 3, ALT_LO, ALT_HI),
    Case("130x257_r2", _jax((130, 257), 2.0), "relief", (1,), "noise", 3, ALT_LO, ALT_HI),
    Case("box", _jax((130, 257), 0.5), "box", (0, 1, 2, 3), "real", 3, -28.0, 2.0),
    Case("south", _south(), "relief", (0, 1, 3), "noise", 3, ALT_LO, ALT_HI),
)
BY_NAME = {c.name: c for c in CASES}
NAMES = tuple(BY_NAME)
BOX = dict(ground=-28.0, height=30.0, rows=(40, 90), cols=(100, 150))   # of the "box" case


@functools.lru_cache(maxsize=None)
def metas(south=False):
    """The metadata of the four shipped cameras; ``south``: moved over the southern grid."""
    cams = load_cameras()["images"]
    out = [copy.deepcopy(cams[v]) for v in VIEWS]
    if south:
        for m in out:
            m["rpc"]["lat_offset"], m["rpc"]["lon_offset"] = SOUTH_LAT, SOUTH_LON
    return out


def sizes():
    return [(int(m["height"] // DOWNSCALE), int(m["width"] // DOWNSCALE)) for m in metas()]


def cameras(case):
    """The case's cameras for the library (``rectify.Camera``)."""
    ms = metas(case.grid.south)
    return [Camera.from_meta(ms[v], DOWNSCALE) for v in case.views]


def ref_cameras(case):
    """The case's cameras for the numpy statement (``rpc_ref.RPC``, rescaled)."""
    ms = metas(case.grid.south)
    return [rpc_ref.RPC(ms[v]["rpc"], DOWNSCALE) for v in case.views]


@functools.lru_cache(maxsize=None)
def _real():
    with np.load(os.path.join(os.path.dirname(DATA), f"jax269_rgb_ds{DOWNSCALE}.npz"), allow_pickle=False) as z:
        return [z[v].reshape(h, w, 3) for v, (h, w) in zip(VIEWS, sizes())]


@functools.lru_cache(maxsize=None)
def images(name):
    """The case's images, (h, w, C) float32 each (read-only)."""
    case = BY_NAME[name]
    out = []
    for v in case.views:
        h, w = sizes()[v]
        if case.images == "real":
            im = _real()[v]
        elif case.images == "noise":
            im = np.random.default_rng(100 + v).random((h, w, case.channels), dtype=np.float32)
        else:
            col, row = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
            im = np.stack([a * col + b * row + c for a, b, c in RAMP[:case.channels]], -1)
            assert np.array_equal(im.astype(np.float32).astype(np.float64), im)           # exact in fp32
        im = np.ascontiguousarray(im, np.float32)
        im.setflags(write=False)
        out.append(im)
    return out


@functools.lru_cache(maxsize=None)
def heights(name):
    """The case's DSM, float64 (read-only)."""
    case = BY_NAME[name]
    H, W = case.grid.shape
    if case.dsm == "box":
        h = np.full((H, W), BOX["ground"])
        h[BOX["rows"][0]:BOX["rows"][1], BOX["cols"][0]:BOX["cols"][1]] += BOX["height"]
    else:
        g = np.random.default_rng(NAMES.index(name) + 1)
        jj, ii = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
        h = np.full((H, W), -16.0)
        for _ in range(3):
            kx, ky, p = g.uniform(0.02, 0.2), g.uniform(0.02, 0.2), g.uniform(0, 2 * np.pi)
            h += 3.0 * np.sin(kx * ii + ky * jj + p)
        h += g.uniform(-4.0, 4.0, (H, W))
        h = np.clip(h, ALT_LO, ALT_HI)
        if H * W > 64:
            h[g.random((H, W)) < 0.02] = np.nan
        elif (H, W) == (1, 7):
            h[0, 3] = np.nan
    h.setflags(write=False)
    return h


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def ref_pix(name):
    case = BY_NAME[name]
    return _frozen(rn.project(heights(name), case.grid, ref_cameras(case)))


@functools.lru_cache(maxsize=None)
def ref_sample(name):
    """(rgb, valid) of the numpy statement at its own pix."""
    return _frozen(*rn.sample(images(name), ref_pix(name)))


@functools.lru_cache(maxsize=None)
def ref_dirs(name):
    """(dirs, spread) of the numpy statement."""
    case = BY_NAME[name]
    return _frozen(*rn.view_directions(case.grid, ref_cameras(case), case.alt_lo, case.alt_hi))


@functools.lru_cache(maxsize=None)
def ref_visible(name):
    """"visible" of the numpy statement under ``ref_dirs``."""
    case = BY_NAME[name]
    return _frozen(rn.visible_from_shadow(sn.cast(heights(name), case.grid.resolution, ref_dirs(name)[0])[0]))


def border_distance(name):
    """How far every finite pix entry lies from its image's border lines, in pixels: (V, H, W), NaN where pix is."""
    pix = ref_pix(name)
    out = np.empty(pix.shape[:3])
    for v, im in enumerate(images(name)):
        h, w, _ = im.shape
        col, row = pix[v, ..., 0], pix[v, ..., 1]
        out[v] = np.minimum(np.minimum(np.abs(col), np.abs(col - (w - 1.0))), np.minimum(np.abs(row), np.abs(row - (h - 1.0))))
    return out


def neighbour_difference(image):
    """The largest difference between two neighbouring pixels of an image, over its channels."""
    im = np.asarray(image, np.float64)
    dx = np.abs(np.diff(im, axis=1)).max() if im.shape[1] > 1 else 0.0
    dy = np.abs(np.diff(im, axis=0)).max() if im.shape[0] > 1 else 0.0
    return float(max(dx, dy))
