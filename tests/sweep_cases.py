"""The cases the plane sweep is checked on, shared by tests/test_sweep_ref.py (CPU: the numpy statement
alone) and tests/test_gpu_sweep.py (the device against it).  Inputs and references are computed once
per process and never modified.

Scenes, all on the JAX_269 ROI origin of tests/rectify_cases.py with the four shipped cameras at
downscale 4: ``flat`` and ``half`` — a seeded sum of sinusoids T(E, N) with wavelengths of 3 m to 12 m
on the plane z0 = −16 m, imaged into the four cameras by localising every pixel near the grid at z0 —
swept on 33 x 65 cells of 0.5 m by 9 planes one metre apart with a window radius of 4 (the images'
ground sampling is 1.3 m: a 2.5 m window holds two pixels a side and cannot tell the planes apart), z0 on plane 4 (``flat``) or half-way
between planes 4 and 5 (``half``); ``real`` — the shipped pixels, 9 planes two metres apart; ``noise``
(C = 4), ``ramp`` (C = 3, exact in fp32, zero at the image centre so that its values near the grid
stay small against the pixel tolerance) and ``south`` (the southern-zone grid, three cameras moved
there) for the grey planes.  Stored greys for the score: seeded noise with 3 % of the cells invalid
and one constant block.
"""
import collections
import functools

import numpy as np

import rectify_cases as rc
import sweep_numpy as sw
from oracle import dsm_ref
from spnerf_amd import GroundGrid

Z0 = -16.0
SCORE_GRIDS = ((1, 1), (1, 7), (7, 1), (17, 33), (33, 65))
NEAR_TIE = 1e-5

Scene = collections.namedtuple("Scene", "name grid views images channels alt_lo step planes radius min_views")


def _jax(shape, res=0.5):
    return GroundGrid(rc.ROI_XOFF, rc.ROI_YTOP, shape[1], shape[0], res, 17)


SCENES = (
    Scene("flat", _jax((33, 65)), (0, 1, 2, 3), "texture", 1, Z0 - 4.0, 1.0, 9, 4, 2),
    Scene("half", _jax((33, 65)), (0, 1, 2, 3), "texture", 1, Z0 - 4.5, 1.0, 9, 4, 2),
    Scene("real", _jax((33, 65)), (0, 1, 2, 3), "real", 3, -24.0, 2.0, 9, 2, 2),
    Scene("noise", _jax((17, 33)), (0, 2, 3), "noise", 4, -24.0, 2.0, 3, 1, 3),
    Scene("ramp", _jax((33, 65)), (0, 1, 2, 3), "ramp", 3, -24.0, 2.0, 2, 4, 2),
    Scene("south", rc.BY_NAME["south"].grid, (0, 1, 3), "noise", 3, -24.0, 2.0, 3, 2, 2),
)
BY_NAME = {s.name: s for s in SCENES}
RAMP = rc.RAMP[:, :2]                                                    # a, b per channel


def cameras(scene):
    return rc.cameras(scene)


def ref_cameras(scene):
    return rc.ref_cameras(scene)


def texture(E, N):
    """T(E, N): eight seeded sinusoids, wavelengths 3 m to 12 m, every direction; within [0, 1]."""
    g = np.random.default_rng(269)
    t = np.zeros(np.shape(E))
    for _ in range(8):
        lam, th, ph = g.uniform(3.0, 12.0), g.uniform(0.0, np.pi), g.uniform(0.0, 2.0 * np.pi)
        t = t + np.sin(2.0 * np.pi / lam * ((E - rc.ROI_XOFF) * np.cos(th) + (N - rc.ROI_YTOP) * np.sin(th)) + ph)
    return 0.5 + t / 16.0


@functools.lru_cache(maxsize=None)
def _texture_images():
    scene = BY_NAME["flat"]
    out = []
    for v, cam in zip(scene.views, ref_cameras(scene)):
        h, w = rc.sizes()[v]
        im = np.zeros((h, w, 1), np.float32)
        reach = np.concatenate([sw.pix_at(scene.grid, [cam], a)[0].reshape(-1, 2) for a in (Z0 - 5.0, Z0 + 5.0)])
        c0, r0 = np.maximum(np.floor(reach.min(0)).astype(int) - 3, 0)
        c1, r1 = np.minimum(np.ceil(reach.max(0)).astype(int) + 4, (w, h))
        cols, rows = np.meshgrid(np.arange(c0, c1, dtype=np.float64), np.arange(r0, r1, dtype=np.float64))
        lon, lat = cam.localization(cols.ravel(), rows.ravel(), np.full(cols.size, Z0))
        e, n = dsm_ref.utm(lat, lon, scene.grid.zone, scene.grid.south)
        im[r0:r1, c0:c1, 0] = texture(e, n).reshape(cols.shape)
        out.append(im)
    return out


@functools.lru_cache(maxsize=None)
def images(name):
    """The scene's images, (h, w, C) float32 each (read-only)."""
    scene = BY_NAME[name]
    out = []
    for k, v in enumerate(scene.views):
        h, w = rc.sizes()[v]
        if scene.images == "texture":
            im = _texture_images()[k]
        elif scene.images == "real":
            im = rc._real()[v]
        elif scene.images == "noise":
            im = np.random.default_rng(300 + v).random((h, w, scene.channels), dtype=np.float32)
        else:
            col, row = np.meshgrid(np.arange(w, dtype=np.float64) - w // 2, np.arange(h, dtype=np.float64) - h // 2)
            im = np.stack([a * col + b * row for a, b in RAMP[:scene.channels]], -1)
            assert np.array_equal(im.astype(np.float32).astype(np.float64), im)           # exact in fp32
        im = np.ascontiguousarray(im, np.float32)
        im.setflags(write=False)
        out.append(im)
    return out


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def altitude(scene, k):
    return scene.alt_lo + float(k) * scene.step


@functools.lru_cache(maxsize=None)
def ref_pix(name, k):
    scene = BY_NAME[name]
    return _frozen(sw.pix_at(scene.grid, ref_cameras(scene), altitude(scene, k)))


@functools.lru_cache(maxsize=None)
def ref_grey(name, k):
    """(grey, valid) of the numpy statement at plane k."""
    return _frozen(*sw.grey_at(images(name), ref_pix(name, k)))


@functools.lru_cache(maxsize=None)
def ref_sweep(name, pix_shift=0.0):
    """The whole numpy statement of a scene (a dict of read-only arrays)."""
    s = BY_NAME[name]
    out = sw.sweep(images(name), ref_cameras(s), s.grid, s.alt_lo, s.step, s.planes, s.radius, s.min_views, 0.0, pix_shift)
    _frozen(*out.values())
    return out


def border_distance(pix, imgs):
    """rectify_cases.border_distance for any pix (V, H, W, 2): how far every finite entry lies from its
    image's border lines, in pixels."""
    out = np.empty(pix.shape[:3])
    for v, im in enumerate(imgs):
        h, w, _ = im.shape
        col, row = pix[v, ..., 0], pix[v, ..., 1]
        out[v] = np.minimum(np.minimum(np.abs(col), np.abs(col - (w - 1.0))), np.minimum(np.abs(row), np.abs(row - (h - 1.0))))
    return out


def near_tie(volume):
    """The cells whose best and second-best fp32 scores differ by less than NEAR_TIE (cells with one
    scored plane or none are not ties)."""
    with np.errstate(invalid="ignore"):
        s = np.sort(np.where(np.isnan(volume), -np.inf, volume.astype(np.float64)), axis=0)
        if s.shape[0] < 2:
            return np.zeros(volume.shape[1:], bool)
        return np.isfinite(s[-2]) & (s[-1] - s[-2] < NEAR_TIE)


@functools.lru_cache(maxsize=None)
def stored(V, shape, seed=0):
    """Stored planes for the score: (grey (V, H, W) float32, valid (V, H, W) uint8) — correlated seeded
    noise, 3 % of the cells invalid, one constant block in view 0 (the whole plane on the small grids)."""
    H, W = shape
    g = np.random.default_rng(1000 * V + 10 * H + W + seed)
    common = g.random((H, W), dtype=np.float32)
    grey = np.stack([common + np.float32(0.5) * g.random((H, W), dtype=np.float32) for _ in range(V)])
    valid = (g.random((V, H, W)) >= 0.03).astype(np.uint8)
    if H * W > 64:
        grey[0, 4:12, 5:14] = np.float32(0.375)
        valid[0, 4:12, 5:14] = 1
        valid[1, 0, 0] = 255                                             # anything but 1 does not count
    else:
        grey[V - 1] = np.float32(0.25)
    return _frozen(grey, valid)
