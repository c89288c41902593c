"""Geometric shadows on the GPU (csrc/shadow.hip, spnerf_amd.shadow) — needs an MI355X.

``cast_shadows`` is held to the fp64 numpy statement (tests/shadow_numpy.py, itself pinned to known
answers on the CPU by tests/test_shadow_ref.py) on the cases of tests/shadow_cases.py:

* ``excess`` within 64·2⁻⁵²·max(1, max|h|)·max(H, W) metres — the rounding of y = j + m·q times the
  largest height difference — with −inf and NaN matching exactly;
* ``shadow`` equal in every cell whose reference |excess| exceeds that tolerance, and at most 0.1 % of
  a case's cells inside it (the CPU test asserts there is none);
* ``shadow`` bit-equal with and without ``excess`` requested (the exactness of the early exit), from
  run to run, and for a float32 DSM against its widened copy.

``shadow_agreement`` is held to its numpy statement, and ``relight_ortho(cast=True)`` to
``cast_shadows`` of its own DSM with every other plane untouched.
"""
import functools

import numpy as np
import pytest
import torch

import shadow_cases as sc
import shadow_numpy as sn
import spnerf_amd
from spnerf_amd import GroundGrid, PhiloxRandom, cast_shadows, random_source, shadow_agreement
from relight_cases import DIRS as RELIGHT_DIRS
from test_gpu_ortho import CENTER, MAX_ALT, MIN_ALT, RNG, ROI_XOFF, ROI_YTOP, scene
from test_gpu_parity import DEV

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def device_cast(shape):
    """(shadow, excess) of ``cast_shadows(..., excess=True)`` on the case's DSM, on the host."""
    dsm = torch.tensor(sc.heights(shape), device=DEV)
    shadow, excess = cast_shadows(dsm, sc.RESOLUTION, sc.DIRS, excess=True)
    assert shadow.dtype == torch.uint8 and excess.dtype == torch.float64 and shadow.device == excess.device == dsm.device
    assert tuple(shadow.shape) == tuple(excess.shape) == (11,) + shape
    return shadow.cpu().numpy(), excess.cpu().numpy()


@pytest.mark.parametrize("shape", sc.SHAPES)
def test_excess_matches_the_numpy_statement(shape):
    _, got = device_cast(shape)
    _, ref = sc.reference(shape)
    tol = sn.tolerance(sc.heights(shape))
    special = ~np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got == -np.inf, ref == -np.inf)
    assert not (got == np.inf).any()
    err = np.abs(got[~special] - ref[~special])
    print(f"{shape}: tolerance {tol:.3e} m; worst |excess - reference| {float(err.max()) if err.size else 0.0:.3e} m; "
          f"entries that differ: {int((err != 0).sum())} of {err.size}; -inf {int((ref == -np.inf).sum())}, NaN {int(np.isnan(ref).sum())}")
    assert bool((err <= tol).all())


@pytest.mark.parametrize("shape", sc.SHAPES)
def test_shadow_matches_the_numpy_statement_outside_the_tolerance_band(shape):
    got, _ = device_cast(shape)
    ref, _ = sc.reference(shape)
    band = sc.in_band(shape)
    print(f"{shape}: {int(band.sum())} of {band.size} cells inside the band; shadow differs in {int((got != ref).sum())}; "
          f"shadowed {int((ref == 1).sum())}, lit {int((ref == 0).sum())}, no data {int((ref == 255).sum())}")
    assert band.sum() <= 1e-3 * band.size
    assert np.array_equal(got[~band], ref[~band])
    assert set(np.unique(got).tolist()) <= {0, 1, 255}


@pytest.mark.parametrize("shape", sc.SHAPES)
def test_shadow_alone_takes_the_early_exits_and_is_bit_equal(shape):
    with_excess, excess = device_cast(shape)
    dsm = torch.tensor(sc.heights(shape), device=DEV)
    alone = cast_shadows(dsm, sc.RESOLUTION, sc.DIRS)
    assert isinstance(alone, torch.Tensor) and alone.dtype == torch.uint8
    assert np.array_equal(alone.cpu().numpy(), with_excess)
    # two runs give equal bytes
    again, excess2 = cast_shadows(dsm, sc.RESOLUTION, sc.DIRS, excess=True)
    assert np.array_equal(again.cpu().numpy(), with_excess) and excess2.cpu().numpy().tobytes() == excess.tobytes()
    assert torch.equal(cast_shadows(dsm, sc.RESOLUTION, sc.DIRS), alone)
    # a float32 DSM is its widened copy
    low = dsm.float()
    s32, e32 = cast_shadows(low, sc.RESOLUTION, sc.DIRS, excess=True)
    s64, e64 = cast_shadows(low.double(), sc.RESOLUTION, sc.DIRS, excess=True)
    assert torch.equal(s32, s64) and e32.cpu().numpy().tobytes() == e64.cpu().numpy().tobytes()
    assert torch.equal(cast_shadows(low, sc.RESOLUTION, sc.DIRS), s64)


def test_directions_beyond_one_launch_and_as_angles_and_on_a_grid():
    """More directions than one launch carries (32): plane k depends neither on K nor on k's position.
    (elevation, azimuth) pairs are ``sun_direction``'s vectors, and a GroundGrid gives its resolution."""
    shape = (33, 65)
    ref, ref_excess = device_cast(shape)
    dsm = torch.tensor(sc.heights(shape), device=DEV)
    order = [(3 * k + 1) % 11 for k in range(35)]
    shadow, excess = cast_shadows(dsm, sc.RESOLUTION, sc.DIRS[order], excess=True)
    assert tuple(shadow.shape) == (35,) + shape
    assert np.array_equal(shadow.cpu().numpy(), ref[order]) and np.array_equal(excess.cpu().numpy(), ref_excess[order], equal_nan=True)
    assert np.array_equal(cast_shadows(dsm, sc.RESOLUTION, torch.tensor(sc.DIRS[order])).cpu().numpy(), ref[order])
    angles = np.array([[30.0, 100.0], [55.0, 250.0]])
    vectors = np.stack([spnerf_amd.satellite.sun_direction(el, az) for el, az in angles])
    grid = GroundGrid(ROI_XOFF, ROI_YTOP, 65, 33, sc.RESOLUTION, 17)
    a = cast_shadows(dsm, grid, angles)
    assert torch.equal(a, cast_shadows(dsm, sc.RESOLUTION, vectors))
    want, want_excess = sn.cast(sc.heights(shape), sc.RESOLUTION, vectors)
    with np.errstate(invalid="ignore"):
        clear = ~(np.abs(want_excess) <= sn.tolerance(sc.heights(shape)))
    assert np.array_equal(a.cpu().numpy()[clear], want[clear]) and clear.sum() >= 0.999 * clear.size
    # the resolution matters: half the cell size doubles the reach of every shadow
    assert int((cast_shadows(dsm, 0.25, vectors) == 1).sum()) > int((a == 1).sum())


def test_agreement_matches_the_numpy_statement():
    g = np.random.default_rng(11)
    K, H, W = 3, 33, 65
    sun = g.uniform(0.0, 1.0, (K, H, W)).astype(np.float32)
    sun[0, 3, 5], sun[1, 7, 7], sun[2, 0, 0] = np.nan, np.inf, -np.inf
    shadow = (g.random((K, H, W)) < 0.4).astype(np.uint8)
    shadow[g.random((K, H, W)) < 0.03] = 255
    shadow[2][shadow[2] == 1] = 0                                   # a direction with no shadowed cell
    sun[2] = 0.5 + 0.5 * sun[2]                                     # ... that the learnt plane agrees with
    sun[2, 0, 0] = -np.inf
    want_sums, want = sn.agreement_sums(sun, shadow), sn.agreement(sun, shadow)
    sun_d, shadow_d = torch.tensor(sun, device=DEV), torch.tensor(shadow, device=DEV)
    got = shadow_agreement(sun_d, shadow_d)
    for k in ("n_lit", "n_shadow", "tp", "fp", "fn"):
        assert got[k].dtype == np.int64 and np.array_equal(got[k], want_sums[k]), k
    assert np.array_equal(got["n"], want["n"]) and got["n"].tolist() == want["n"].tolist() and (got["n"] < H * W).all()
    for k in ("mae", "mean_sun_lit", "mean_sun_shadow", "iou"):
        assert got[k].shape == (K,) and got[k].dtype == np.float64
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), k
        ok = ~np.isnan(want[k])
        print(k, got[k], "relative", np.abs(got[k][ok] - want[k][ok]) / np.abs(want[k][ok]))
        assert bool((np.abs(got[k][ok] - want[k][ok]) <= 1e-12 * np.abs(want[k][ok])).all()), k
    assert np.isnan(got["iou"][2]) and np.isnan(got["mean_sun_shadow"][2]) and not np.isnan(got["iou"][:2]).any()
    again = shadow_agreement(sun_d, shadow_d)
    for k, v in got.items():
        assert again[k].tobytes() == v.tobytes(), k
    # more than one workgroup per direction, and more cells than workgroups x threads
    big = np.tile(sun, (1, 31, 1)), np.tile(shadow, (1, 31, 1))           # 66 495 cells per direction
    got = shadow_agreement(torch.tensor(big[0], device=DEV), torch.tensor(big[1], device=DEV))
    assert np.array_equal(got["n"], 31 * want["n"]) and np.array_equal(got["tp"], 31 * want_sums["tp"])
    assert bool((np.abs(got["mae"] - want["mae"]) <= 1e-12 * want["mae"]).all())


def test_agreement_of_a_plane_with_its_own_shadows_is_perfect():
    shadow, _ = device_cast((33, 65))
    s = torch.tensor(shadow[:3], device=DEV)
    sun = torch.where(s == 1, 0.0, 1.0).float()
    got = shadow_agreement(sun, s)
    assert got["mae"].tolist() == [0.0] * 3 and got["iou"].tolist() == [1.0] * 3
    assert got["mean_sun_lit"].tolist() == [1.0] * 3 and got["mean_sun_shadow"].tolist() == [0.0] * 3
    assert got["n"].tolist() == [int((shadow[k] != 255).sum()) for k in range(3)]


def test_relight_ortho_cast_adds_the_shadows_of_its_own_dsm():
    models, args, _ = scene()
    grid = GroundGrid(ROI_XOFF + 60.0, ROI_YTOP - 80.0, 16, 16, 0.5, 17)
    labels = torch.tensor(np.random.default_rng(3).integers(0, 3, grid.shape), device=DEV)
    dirs = RELIGHT_DIRS[:3]
    prod = ("rgb", "sun", "sky", "depth", "albedo")

    def relight(**kw):
        with random_source(PhiloxRandom(5)):
            return spnerf_amd.relight_ortho(models, args, grid, MIN_ALT, MAX_ALT, CENTER, RNG, dirs, semantics=labels, products=prod, **kw)

    plain, cast = relight(), relight(cast=True)
    assert sorted(cast) == sorted(list(plain) + ["shadow_geo"]) and "shadow_geo" not in plain
    for k, v in plain.items():
        assert cast[k].dtype == v.dtype and torch.equal(cast[k], v), k
    geo = cast["shadow_geo"]
    assert geo.dtype == torch.uint8 and tuple(geo.shape) == (3, 16, 16)
    assert torch.equal(geo, cast_shadows(cast["dsm"], grid, dirs))
    score = shadow_agreement(cast["sun"], geo)
    print("agreement of the initialisation's sun plane with its own geometry:", {k: v.tolist() for k, v in score.items()})
    assert score["n"].tolist() == [256] * 3
