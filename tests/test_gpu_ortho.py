"""Ground-grid rays, their reduction and ``render_ortho`` / ``relight_ortho`` on the GPU
(csrc/ortho.hip, spnerf_amd.ortho) — needs an MI355X.

The rays are held to the fp64 numpy statement (tests/ortho_numpy.py, itself pinned on the CPU by
tests/test_ortho_ref.py) and, independently, to the project's existing forward path
(``spnerf_dsm_points``: ECEF → lat/lon/alt → UTM), which must bring every ray back to its own cell
centre.  The reduction is bit-equal to its numpy statement.  ``render_ortho`` and ``relight_ortho``
are held to their definitions: ``render_image`` / ``relight_image`` on ``ortho_rays``, reduced.
"""
import dataclasses
import functools

import numpy as np
import pytest
import torch

import golden_util as gu
import ortho_numpy as on
import spnerf_amd
import view_numpy as vn
from spnerf_amd import GroundGrid, PhiloxRandom, dsm, ortho, random_source
from spnerf_amd.satellite import load_cameras, scene_normalisation
from relight_cases import DIRS, SUN_SCALE
from test_gpu_parity import DEV, make_model

pytestmark = pytest.mark.gpu

MIN_ALT, MAX_ALT = -30.0, -2.0
CENTER, RNG = scene_normalisation(load_cameras()["scene_loc"])          # JAX_269, UTM zone 17
ROI_XOFF, ROI_YTOP = 438638.996411, 3353399.999928 + 256.0
GRID_A = GroundGrid(ROI_XOFF + 100.0, ROI_YTOP - 50.0, 5, 3, 0.5, 17)          # non-square: an x/y swap fails
GRID_B = GroundGrid(ROI_XOFF + 3.0, ROI_YTOP - 7.0, 67, 33, 0.5, 17)           # odd sizes, 8 844 rays at s = 2
SUN = np.array([0.3, -0.5, 0.8], np.float32)


def numpy_rays(grid, center, rng, sun, s, rows=None, lo=MIN_ALT, hi=MAX_ALT):
    return on.ortho_rays(grid.xoff, grid.ytop, grid.xsize, grid.ysize, grid.resolution, grid.zone, grid.south, lo, hi,
                         center, rng, sun=sun, s=s, rows=rows).astype(np.float32)


def assert_rays(got, ref, what):
    """|a − b| ≤ 2⁻²³·|b| + 2⁻²⁴: one fp32 ulp, for the device's few-ulp fp64 libm flipping the
    rounding of the one cast.  Observed on MI355X: at most 0.50 of the tolerance, 4 entries of
    144 358 not bit-equal."""
    got = got.cpu().numpy()
    assert got.shape == ref.shape and got.dtype == np.float32, what
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    tol = 2.0 ** -23 * np.abs(ref.astype(np.float64)) + 2.0 ** -24
    print(what, f"worst |a - b| / tol {float((err / tol).max()):.3f}; entries that differ: {int((got != ref).sum())} of {ref.size}")
    assert bool((err <= tol).all()), what


@pytest.mark.parametrize("s", [1, 3])
def test_rays_of_a_small_grid_match_the_numpy_statement(s):
    rays = spnerf_amd.ortho_rays(GRID_A, MIN_ALT, MAX_ALT, CENTER, RNG, sun=SUN, supersample=s, device=DEV)
    assert_rays(rays, numpy_rays(GRID_A, CENTER, RNG, SUN, s), f"grid A s={s}")
    bare = spnerf_amd.ortho_rays(GRID_A, MIN_ALT, MAX_ALT, CENTER, RNG, supersample=s, device=DEV)
    assert bare.shape == (15 * s * s, 8) and torch.equal(bare, rays[:, :8])
    angles = spnerf_amd.ortho_rays(GRID_A, MIN_ALT, MAX_ALT, CENTER, RNG, sun=(56.0, 320.0), supersample=s, device=DEV)
    want = torch.tensor(spnerf_amd.satellite.sun_direction(56.0, 320.0).astype(np.float32), device=DEV)
    assert bool((angles[:, 8:] == want).all()) and torch.equal(angles[:, :8], bare)


def test_rays_across_blocks_and_in_bands():
    whole = spnerf_amd.ortho_rays(GRID_B, MIN_ALT, MAX_ALT, CENTER, RNG, sun=SUN, supersample=2, device=DEV)
    assert whole.shape == (8844, 11)
    assert_rays(whole, numpy_rays(GRID_B, CENTER, RNG, SUN, 2), "grid B s=2")
    band = spnerf_amd.ortho_rays(GRID_B, MIN_ALT, MAX_ALT, CENTER, RNG, sun=SUN, supersample=2, rows=(5, 20), device=DEV)
    assert_rays(band, numpy_rays(GRID_B, CENTER, RNG, SUN, 2, rows=(5, 20)), "grid B rows 5..20")
    assert torch.equal(band, whole[5 * 67 * 4:20 * 67 * 4])


def test_rays_far_from_the_central_meridian_in_a_southern_zone():
    from oracle import dsm_ref
    e, n = dsm_ref.utm(-33.9, 15.0 + 2.9, 33, south=True)
    grid = GroundGrid(float(e), float(n), 4, 4, 0.5, 33, south=True)
    center = on.geodetic_to_ecef(-33.9, 17.9, 0.0).astype(np.float32)
    rays = spnerf_amd.ortho_rays(grid, -10.0, 90.0, center, 120.0, sun=SUN, supersample=2, device=DEV)
    assert_rays(rays, numpy_rays(grid, center, 120.0, SUN, 2, lo=-10.0, hi=90.0), "southern grid")
    north = spnerf_amd.ortho_rays(dataclasses.replace(grid, south=False), -10.0, 90.0, center, 120.0, supersample=2, device=DEV)
    assert float((north[:, :3] - rays[:, :3]).abs().max()) > 1e3           # the false northing is read


def test_rays_land_on_their_cell_centres_through_the_forward_path():
    """``spnerf_dsm_points`` (the existing forward path) on grid B at depths 0, 0.37·far and far:
    every ray comes back to its own sub-ray position, at altitude max_alt − depth·range, within
    8 · 2⁻²⁴ · range · (max|o| + far) metres — one fp32 rounding each of o, d and the depth, with
    margin — the horizontal bound no tighter than 1e-6 m (device libm).  Observed on MI355X: 6.1e-6 m
    horizontally, 4.0e-6 m in altitude against 7.5e-5 m."""
    s = 2
    rays = spnerf_amd.ortho_rays(GRID_B, MIN_ALT, MAX_ALT, CENTER, RNG, supersample=s, device=DEV)
    far = rays[:, 7].double()
    bound = 8 * 2.0 ** -24 * float(RNG) * (float(rays[:, :3].abs().max()) + float(far.max()))
    E, N = on.cell_points(GRID_B.xoff, GRID_B.ytop, GRID_B.xsize, GRID_B.ysize, GRID_B.resolution, s)
    E, N = E.ravel(), N.ravel()
    for frac in (0.0, 0.37, 1.0):
        depth = (frac * far).float()
        _, ena = dsm._points(rays, depth, CENTER, RNG, zone=17, south=False, lla=False, ena=True)
        ena = ena.cpu().numpy()
        horizontal = float(np.hypot(ena[:, 0] - E, ena[:, 1] - N).max())
        vertical = float(np.abs(ena[:, 2] - (MAX_ALT - depth.double().cpu().numpy() * float(RNG))).max())
        print(f"depth {frac} far: horizontal {horizontal:.2e} m, altitude {vertical:.2e} m, bound {bound:.2e} m")
        assert horizontal <= max(bound, 1e-6) and vertical <= bound


# ---- the reduction ---------------------------------------------------------------------------------

@pytest.mark.parametrize("s", [2, 3, 4])
def test_reduction_is_bit_equal_to_the_numpy_statement(s):
    g = np.random.default_rng(s)
    for cells in (1, 255, 257):
        for K in (1, 3):
            for width in (1, 3, 5):
                x = (g.standard_normal((K, cells * s * s, width)) * g.choice([1e-3, 1.0, 300.0], (K, 1, width))).astype(np.float32)
                got = ortho.reduce_subrays(torch.tensor(x, device=DEV), s, ray_dim=1)
                want = on.reduce_subrays(x, s)
                assert got.dtype == torch.float32 and tuple(got.shape) == (K, cells, width)
                assert np.array_equal(got.cpu().numpy(), want), (cells, K, width)
        alt = g.standard_normal(cells * s * s) * 30.0                      # the float64 altitude plane
        got = ortho.reduce_subrays(torch.tensor(alt, device=DEV), s)
        assert got.dtype == torch.float64 and np.array_equal(got.cpu().numpy(), on.reduce_subrays(alt[:, None], s)[:, 0])
    rgb = torch.tensor(g.uniform(0, 1, (257 * s * s, 3)).astype(np.float32), device=DEV)      # a geometry plane: (N, 3)
    assert np.array_equal(ortho.reduce_subrays(rgb, s).cpu().numpy(), on.reduce_subrays(rgb.cpu().numpy(), s))
    const = torch.tensor(np.repeat(g.standard_normal((40, 3)).astype(np.float32), s * s, axis=0), device=DEV)
    assert torch.equal(ortho.reduce_subrays(const, s), const[::s * s])     # constant sub-rays: that constant


def test_reduction_with_one_sub_ray_returns_the_same_storage():
    for x in (torch.rand(3, 40, 5, device=DEV), torch.rand(40, device=DEV, dtype=torch.float64)):
        assert ortho.reduce_subrays(x, 1, ray_dim=x.dim() - 2 if x.dim() > 1 else 0) is x


def test_classes_ties_and_nans():
    """The cases of test_products_argmax_ties_and_nans: the first maximum; a NaN is the maximum."""
    nan, inf = float("nan"), float("inf")
    rows = [[1.0, 1.0, 0.5], [0.5, 2.0, 2.0], [3.0, nan, 2.0], [nan, 2.0, nan], [-1.0, -3.0, -0.5], [0.25, 0.25, inf]]
    logits = torch.tensor(rows * 43, device=DEV)                             # 258 cells: more than one block
    got = ortho.classes(logits)
    assert got.dtype == torch.int32 and got.tolist() == [0, 1, 1, 0, 2, 2] * 43
    assert got.tolist() == logits.argmax(-1).tolist() == on.classes(logits.cpu().numpy()).tolist()
    one = ortho.classes(torch.tensor([[0.5], [nan]], device=DEV))
    assert one.tolist() == [0, 0]


# ---- render_ortho / relight_ortho by definition ------------------------------------------------------

GRID_R = GroundGrid(ROI_XOFF + 60.0, ROI_YTOP - 80.0, 9, 7, 0.5, 17)
PRODUCTS = ("rgb", "depth", "sun", "albedo", "sky", "sem")


@functools.lru_cache(maxsize=None)
def scene():
    """A width-64 fp32 model on the weights of the view fixture (case b: guided sampling), 16
    samples, σ noise on so that the on-device draws matter; labels on the grid."""
    d = vn.load_case("b")
    meta = d["meta"]
    dims, args = gu.dims_of(meta), gu.args_of(meta)
    args.n_samples, args.noise_std = 16, 0.1
    models = {"coarse": make_model(dims, meta["seed"])}
    with torch.no_grad():
        models["coarse"].sun_v_net[0].weight[:, dims.width:] *= SUN_SCALE        # the directions matter (relight_cases.py)
    labels = torch.tensor(np.random.default_rng(2).integers(0, 3, GRID_R.shape), device=DEV)
    return models, args, labels


def render(s, seed=5, **kw):
    models, args, labels = scene()
    with random_source(PhiloxRandom(seed)):
        return spnerf_amd.render_ortho(models, args, GRID_R, MIN_ALT, MAX_ALT, CENTER, RNG, SUN, semantics=labels,
                                       supersample=s, products=PRODUCTS, **kw)


@functools.lru_cache(maxsize=None)
def rendered(s):
    return render(s)


@functools.lru_cache(maxsize=None)
def by_definition(s):
    """render_image on ortho_rays, every ray's planes."""
    models, args, labels = scene()
    rays = spnerf_amd.ortho_rays(GRID_R, MIN_ALT, MAX_ALT, CENTER, RNG, sun=SUN, supersample=s, device=DEV)
    with random_source(PhiloxRandom(5)):
        return spnerf_amd.render_image(models, args, rays, None, labels.reshape(-1).repeat_interleave(s * s), products=PRODUCTS,
                                       center=CENTER, rng=RNG)


def test_render_ortho_with_one_ray_per_cell_is_render_image():
    got, ref = rendered(1), by_definition(1)
    assert sorted(got) == sorted(list(ref) + ["dsm"])
    for k, v in ref.items():
        assert got[k].shape == (7, 9) + tuple(v.shape[1:]) and got[k].dtype == v.dtype, k
        assert torch.equal(got[k], v.reshape(got[k].shape)), k
    assert got["dsm"].dtype == torch.float64 and torch.equal(got["dsm"], got["alt"])
    # a model of random weights still stops inside the altitude bounds: depth·range metres below max_alt
    assert bool(torch.isfinite(got["dsm"]).all()) and float(got["dsm"].max()) <= MAX_ALT + 1e-3 and float(got["dsm"].min()) >= MIN_ALT - 1e-3


def test_render_ortho_supersampled_is_the_numpy_reduction_of_render_image():
    got, ref = rendered(2), by_definition(2)
    assert sorted(got) == sorted(list(ref) + ["dsm"])
    for k, v in ref.items():
        if k == "sem_class":
            continue
        x = v.cpu().numpy()
        want = on.reduce_subrays(x.reshape(x.shape[0], -1), 2).reshape((7, 9) + x.shape[1:])
        assert got[k].dtype == v.dtype and np.array_equal(got[k].cpu().numpy(), want), k
    assert torch.equal(got["dsm"], got["alt"]) and got["dsm"].dtype == torch.float64
    logits = got["sem_logits"].cpu().numpy().reshape(63, 3)
    assert got["sem_class"].dtype == torch.int32 and got["sem_class"].cpu().numpy().reshape(-1).tolist() == on.classes(logits).tolist()
    # the sub-rays differ, so the filter did something
    assert not np.array_equal(got["depth"].cpu().numpy(), ref["depth"].cpu().numpy().reshape(63, 4)[:, 0].reshape(7, 9))


def test_render_ortho_depends_neither_on_the_chunking_nor_on_the_banding():
    whole = rendered(2)
    for chunk in (50, 7):                   # neither a multiple of the 4 sub-rays of a cell
        parts = render(2, chunk=chunk)
        for k, v in whole.items():
            assert torch.equal(parts[k], v), (chunk, k)
    bands = [render(2, rows=r) for r in ((0, 3), (3, 4), (4, 7))]
    for k, v in whole.items():
        assert bands[1][k].shape[:2] == (1, 9), k
        assert torch.equal(torch.cat([b[k] for b in bands]), v), k


def test_relight_ortho_is_relight_image_reduced():
    models, args, labels = scene()
    prod = ("rgb", "sun", "sky", "depth", "albedo")
    s = 2
    with random_source(PhiloxRandom(5)):
        got = spnerf_amd.relight_ortho(models, args, GRID_R, MIN_ALT, MAX_ALT, CENTER, RNG, DIRS, semantics=labels,
                                       supersample=s, products=prod)
    rays = spnerf_amd.ortho_rays(GRID_R, MIN_ALT, MAX_ALT, CENTER, RNG, sun=DIRS[0], supersample=s, device=DEV)
    with random_source(PhiloxRandom(5)):
        ref = spnerf_amd.relight_image(models, args, rays, torch.tensor(DIRS), None, labels.reshape(-1).repeat_interleave(s * s),
                                       products=prod)
    assert sorted(got) == sorted(list(ref) + ["alt", "dsm"])
    for k, v in ref.items():
        x = v.cpu().numpy()
        lead = (5,) if k in ("rgb", "sun", "sky") else ()
        flat = x.reshape(lead + (252, -1))
        want = on.reduce_subrays(flat, s).reshape(lead + (7, 9) + x.shape[len(lead) + 1:])
        assert got[k].shape == want.shape and np.array_equal(got[k].cpu().numpy(), want), k
    assert float((got["sun"][0] - got["sun"][2]).abs().max()) > 1e-3          # the directions matter
    # the geometry is render_ortho's: the same draws, the same depth, the same DSM
    assert torch.equal(got["depth"], rendered(2)["depth"]) and torch.equal(got["dsm"], rendered(2)["dsm"])


def test_dsm_goes_to_the_score_without_holes():
    models, args, _ = scene()
    grid = GroundGrid(ROI_XOFF + 20.0, ROI_YTOP - 30.0, 24, 20, 0.5, 17)
    labels = torch.zeros(grid.shape, dtype=torch.long, device=DEV)
    with random_source(PhiloxRandom(1)):
        out = spnerf_amd.render_ortho(models, args, grid, MIN_ALT, MAX_ALT, CENTER, RNG, SUN, semantics=labels, products=("depth",))
    assert out["dsm"].shape == grid.shape and not bool(torch.isnan(out["dsm"]).any())
    e, n = grid.cell_centres()
    gt = -15.0 + 3.0 * np.sin(e / 3.0) * np.cos(n / 4.0) + np.random.default_rng(0).normal(0, 0.2, grid.shape)
    mae = dsm.dsm_mae(out["dsm"], gt, register="ncc")
    print("mae", mae, "z-registered", dsm.dsm_mae(out["dsm"].cpu().numpy(), gt))
    assert np.isfinite(mae) and mae >= 0
