"""The cases the semi-global aggregation is checked on, shared by tests/test_sgm_ref.py (CPU: the numpy
statement alone) and tests/test_gpu_sgm.py (the device against it).  Inputs and references are computed
once per process and never modified.
"""
import functools

import numpy as np

import sgm_numpy as sg

F = np.float32
STEP_SHAPE, STEP_PLANES = (17, 33), 9
STEP_OUTLIERS = 51
# (p1, p2, paths) → the cells the statement leaves wrong on the step scene
STEP_WRONG = {(0.125, 1.0, 4): 0, (0.125, 1.0, 8): 3, (0.125, 0.5, 4): 1, (0.125, 0.5, 8): 5}


def _frozen(a):
    a.setflags(write=False)
    return a


def step_truth():
    """The true plane of every cell of the step scene: 2 left of column 16, 6 from there on."""
    H, W = STEP_SHAPE
    return np.where(np.arange(W)[None, :] < 16, 2, 6) + np.zeros((H, 1), int)


@functools.lru_cache(maxsize=None)
def step_scene():
    """(volume (9, 17, 33) float32, truth (17, 33)): 0.5 at the true plane and 0.25 elsewhere; at the cells with
    (7j + 3i) mod 11 = 0 the plane (truth + 3) mod 9 scores 0.75; at the other cells with (5j + 2i) mod 13 = 0
    the odd planes are NaN."""
    H, W = STEP_SHAPE
    truth = step_truth()
    vol = np.full((STEP_PLANES, H, W), 0.25, F)
    j, i = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    np.put_along_axis(vol, truth[None], F(0.5), 0)
    outlier = (7 * j + 3 * i) % 11 == 0
    np.put_along_axis(vol, np.where(outlier, (truth + 3) % STEP_PLANES, truth)[None], np.where(outlier, F(0.75), F(0.5))[None], 0)
    holes = ~outlier & ((5 * j + 2 * i) % 13 == 0)
    vol[1::2, holes] = np.nan
    return _frozen(vol), _frozen(truth)


def raw_index(volume):
    """The per-cell pick of a volume on its own (what plane_sweep does): the sweep's rule."""
    return sg.pick(volume, volume, 0.0, 1.0)["index"]


@functools.lru_cache(maxsize=None)
def step_reference(p1, p2, paths):
    vol, _ = step_scene()
    return _frozen(sg.aggregate(vol, p1, p2, 1.0, paths))


def near_step(wrong):
    """Whether every cell of the mask lies within one cell of the step between columns 15 and 16."""
    cols = np.nonzero(wrong)[1]
    return bool(((cols >= 14) & (cols <= 17)).all())


@functools.lru_cache(maxsize=None)
def random_volume(K, H, W, dyadic=False, seed=0):
    """(K, H, W) float32 scores in (−1, 1) with 20 % NaN, one ±inf pair, a cell without any score (when the grid has
    more than one cell) and equal scores at neighbouring planes; ``dyadic``: multiples of 1/64."""
    g = np.random.default_rng(100000 * K + 1000 * H + 10 * W + seed + (7 if dyadic else 0))
    if dyadic:
        vol = (g.integers(-64, 65, (K, H, W)) / 64.0).astype(F)
    else:
        vol = (2.0 * g.random((K, H, W), dtype=F) - 1.0).astype(F)
    vol[g.random((K, H, W)) < 0.2] = np.nan
    if H * W > 1:
        vol[:, H - 1, W // 2] = np.nan                                   # no score at any plane
        vol[0, 0, 0] = np.inf                                            # unscored as well
        if K > 1:
            vol[K - 1, 0, W - 1] = -np.inf
            vol[1, 0, :] = vol[0, 0, :]                                  # ties between neighbouring planes
    if H * W > 6 and K > 2:
        vol[:, H // 2, W // 3] = F(0.5)                                  # a flat cell: every plane ties
    return _frozen(vol)


@functools.lru_cache(maxsize=None)
def reference(K, H, W, dyadic, p1, p2, unscored, paths):
    return _frozen(sg.aggregate(random_volume(K, H, W, dyadic), p1, p2, unscored, paths))
