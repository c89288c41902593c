"""The fp64 numpy statement of the ground-grid rays (tests/ortho_numpy.py) against the project's
independent forward path — oracle/dsm_ref.py: ECEF → lat/lon/alt by the reference's closed form,
then the forward Krüger series — on the CPU.

The inverse series (β, Karney 2011) and the forward one (α) are derived separately: their round
trip closes only if both sets of coefficients are right, which is the forward series' first check
beyond its known-answer values."""
import functools

import numpy as np
import pytest

import ortho_numpy as on
from oracle import dsm_ref
from spnerf_amd.satellite import load_cameras, scene_normalisation

ROI = (438638.996411, 3353399.999928, 512, 0.5)      # the lidar ROI of JAX_269: xoff, yoff, size, resolution
ZONE, MIN_ALT, MAX_ALT = 17, -30.0, -2.0


@pytest.mark.parametrize("south", [False, True])
@pytest.mark.parametrize("zone", [1, 17, 33, 60])
def test_inverse_of_the_forward_series_closes(zone, south):
    """forward(inverse(forward(lat, lon))) against forward(lat, lon): within 1e-7 m.  The fp64 ulp
    at 1e7 m is 1.9e-9 m; a term of order n^k is worth 6.4e6·n^k m — 5e-5 m at n^4, 9e-8 m at n^5 —
    so a wrong coefficient through n^4, in either series, is far above the bound (the n^6 ones are
    below fp64 resolution here).  Observed worst: 8.4e-9 m."""
    g = np.random.default_rng(100 * zone + south)
    n = 100_000
    lat = np.concatenate([g.uniform(-80.0, 84.0, n), [-80.0, 84.0, 0.0, 0.0, 84.0, -80.0]])
    lon0 = 6.0 * zone - 183.0
    lon = lon0 + np.concatenate([g.uniform(-3.5, 3.5, n), [3.5, -3.5, 0.0, 3.5, 0.0, -3.5]])
    e, nn = dsm_ref.utm(lat, lon, zone, south)
    la, lo = on.utm_inverse(e, nn, zone, south)
    e2, n2 = dsm_ref.utm(la, lo, zone, south)
    worst = float(np.hypot(e2 - e, n2 - nn).max())
    print(zone, south, f"round trip worst {worst:.2e} m; lat {np.abs(la - lat).max():.2e} deg, lon {np.abs(lo - lon).max():.2e} deg")
    assert len(lat) >= 10 ** 5 and worst <= 1e-7
    assert bool((nn[lat < 0] > 0).all()) == south             # the false northing is in play


@functools.lru_cache(maxsize=None)
def jax269():
    center, rng = scene_normalisation(load_cameras()["scene_loc"])
    xoff, yoff, size, res = ROI
    grid = (xoff, yoff + size * res, size, size, res)
    rays = on.ortho_rays(*grid, ZONE, False, MIN_ALT, MAX_ALT, center, rng)
    return grid, center, rng, rays


def test_jax269_rays_land_on_their_cell_centres():
    """The fp32 rays pushed through the existing forward path at depths 0, 0.37·far and far land
    on their own cell centres, at altitude max_alt − depth·range, within
    8 · 2⁻²⁴ · range · (max|o| + far) metres: one fp32 rounding each of o, d and the depth, with
    margin — 8.0e-5 m for this scene.  The reference's fp32 rounding of ECEF (0.5 m) or a
    float64 centre where the scene holds float32 (X_offset 801532.84375 is not a float32: 3 cm)
    fails it by orders of magnitude.  Observed worst: 7.6e-6 m horizontally, 6.8e-6 m in altitude."""
    (xoff, ytop, xsize, ysize, res), center, rng, rays64 = jax269()
    rays = rays64.astype(np.float32)
    assert rays.shape == (512 * 512, 8) and np.all(rays[:, 6] == 0)
    far = rays[:, 7].astype(np.float64)
    bound = 8 * 2.0 ** -24 * float(rng) * (np.abs(rays[:, :3]).max() + far.max())
    print(f"bound {bound:.2e} m")
    assert 7.0e-5 < bound < 9.0e-5
    i = np.arange(xsize, dtype=np.float64)[None, :]
    j = np.arange(ysize, dtype=np.float64)[:, None]
    ce = np.broadcast_to(xoff + (i + 0.5) * res, (ysize, xsize)).ravel()
    cn = np.broadcast_to(ytop - (j + 0.5) * res, (ysize, xsize)).ravel()
    for frac in (0.0, 0.37, 1.0):
        depth = (frac * far).astype(np.float32)
        lat, lon, alt = dsm_ref.latlonalt_from_prediction(rays, depth, center, rng)
        e, n = dsm_ref.utm(lat, lon, ZONE)
        horizontal = float(np.hypot(e - ce, n - cn).max())
        vertical = float(np.abs(alt - (MAX_ALT - depth.astype(np.float64) * float(rng))).max())
        print(f"depth {frac} far: horizontal {horizontal:.2e} m, altitude {vertical:.2e} m")
        assert horizontal <= bound and vertical <= bound
    # the ray runs from max_alt to min_alt: far · range is their distance
    assert np.abs(far * float(rng) - (MAX_ALT - MIN_ALT)).max() <= bound


def test_ray_order_supersampling_and_bands():
    """Ray ((j·xsize + i)·s + a)·s + b stands at sub-ray (a, b) of cell (j, i); a band is the
    whole grid's rows; the sun columns are the given vector."""
    grid, center, rng, _ = jax269()
    small = (grid[0], grid[1], 5, 3, grid[4])
    s = 3
    sun = np.array([0.1, 0.2, 0.9], np.float32)
    rays = on.ortho_rays(*small, ZONE, False, MIN_ALT, MAX_ALT, center, rng, sun=sun, s=s)
    assert rays.shape == (3 * 5 * 9, 11) and np.array_equal(rays[:, 8:], np.broadcast_to(sun.astype(np.float64), (135, 3)))
    fine = on.ortho_rays(small[0], small[1], 5 * s, 3 * s, small[4] / s, ZONE, False, MIN_ALT, MAX_ALT, center, rng)
    fine = fine.reshape(3, s, 5, s, 8).transpose(0, 2, 1, 3, 4).reshape(-1, 8)      # (j, a, i, b) -> (j, i, a, b)
    assert np.abs(rays[:, :8] - fine).max() <= 1e-12
    band = on.ortho_rays(*small, ZONE, False, MIN_ALT, MAX_ALT, center, rng, sun=sun, s=s, rows=(1, 3))
    assert np.array_equal(band, rays[5 * 9:])
    # east is +i, south is +j: the origin moves along the local east / north of the scene
    o = on.ortho_rays(*small, ZONE, False, MIN_ALT, MAX_ALT, center, rng)[:, :3].reshape(3, 5, 3) * float(rng)
    lon = np.radians(-81.66)
    east = np.array([-np.sin(lon), np.cos(lon), 0.0])
    assert np.allclose((o[0, 1] - o[0, 0]) @ east, 0.5, atol=1e-3) and abs((o[1, 0] - o[0, 0]) @ east) < 0.01
    assert (o[1, 0] - o[0, 0])[2] < -0.4                # a row down is half a metre south: z falls at 30° N


def test_reduction_statement():
    g = np.random.default_rng(3)
    x = g.standard_normal((3, 36, 5)).astype(np.float32)
    assert on.reduce_subrays(x, 1) is x                                    # s = 1: the identity
    for s in (2, 3, 4):
        c = np.repeat(x[:, :4, :], s * s, axis=1)                          # constant sub-rays per cell
        assert np.array_equal(on.reduce_subrays(c, s), x[:, :4, :]), s      # their mean is that constant, exactly
    r = on.reduce_subrays(x, 3)
    assert r.shape == (3, 4, 5) and r.dtype == np.float32
    want = (x.reshape(3, 4, 9, 5).astype(np.float64).sum(2) / 9).astype(np.float32)
    assert np.abs(r - want).max() <= 2.0 ** -23 * np.abs(want).max()
    alt = g.standard_normal((8, 1))
    assert on.reduce_subrays(alt, 2).dtype == np.float64 and on.reduce_subrays(alt, 2).shape == (2, 1)
    # the class rule: first maximum, a NaN is the maximum (torch.argmax's)
    nan = float("nan")
    logits = np.array([[1, 1, .5], [.5, 2, 2], [3, nan, 2], [nan, 2, nan], [-1, -3, -.5], [.25, .25, np.inf]], np.float32)
    assert on.classes(logits).tolist() == [0, 1, 1, 0, 2, 2]
