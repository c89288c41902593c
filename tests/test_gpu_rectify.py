"""Orthorectification on the GPU (csrc/rectify.hip, spnerf_amd.rectify) — needs an MI355X.

Every step is held to the fp64 numpy statement (tests/rectify_numpy.py, itself pinned to known answers
on the CPU by tests/test_rectify_ref.py) on the cases of tests/rectify_cases.py:

* ``pix`` within 1e-5 px — the project's 1e-6 m device-libm floor is 3.3e-6 px at the finest ground
  sampling here (0.3 m), with a margin of three — NaNs matching exactly;
* ``sample_images`` on the numpy statement's own ``pix``: bit-equal, ``valid`` included;
* the fused call: ``rgb`` within 1e-5·(largest neighbour difference of the image) + 2⁻²⁴·|value|;
  ``valid`` equal outside the cells whose reference ``pix`` is within 1e-5 px of a border, at most
  0.1 % of a case's cells inside that band (the CPU test asserts there is none);
* bytes: fused = project-then-sample, run to run, float32 DSM = its widened copy, and plane v depends
  neither on V nor on v's position;
* ``view_directions`` and its ``spread`` within 2⁻²³ per component, up > 0; ``visible`` is
  ``cast_shadows`` under those directions with 0 and 1 exchanged; ``mosaic`` bit-equal in both modes.

Observed on MI355X (2026-10-21): worst |pix − reference| 2.5e-9 px over all cases; ``rgb`` at most 0.006 of its
tolerance, about 1 entry in 2 000 not bit-equal; directions at most 3.0e-8 and ``spread`` 2.1e-9 from the reference.
"""
import functools

import numpy as np
import pytest
import torch

import rectify_cases as rc
import rectify_numpy as rn
import shadow_numpy as sn
import spnerf_amd
from spnerf_amd import cast_shadows, orthorectify, rectify
from test_gpu_parity import DEV

pytestmark = pytest.mark.gpu


def device_images(name):
    return [torch.tensor(im, device=DEV) for im in rc.images(name)]


@functools.lru_cache(maxsize=None)
def fused(name):
    """``orthorectify(..., mosaic="median", pix=True)`` of a case, as host arrays."""
    case = rc.BY_NAME[name]
    dsm = torch.tensor(rc.heights(name), device=DEV)
    out = orthorectify(device_images(name), rc.cameras(case), dsm, case.grid, case.alt_lo, case.alt_hi, mosaic="median", pix=True)
    V, (H, W), C = len(case.views), case.grid.shape, case.channels
    want = {"rgb": ((V, H, W, C), torch.float32), "valid": ((V, H, W), torch.uint8), "pix": ((V, H, W, 2), torch.float64),
            "visible": ((V, H, W), torch.uint8), "dirs": ((V, 3), torch.float32), "dir_spread": ((V,), torch.float32),
            "mosaic_rgb": ((H, W, C), torch.float32), "count": ((H, W), torch.int32), "spread": ((H, W), torch.float32)}
    assert sorted(out) == sorted(want)
    for k, (shape, dtype) in want.items():
        assert tuple(out[k].shape) == shape and out[k].dtype == dtype and out[k].device == dsm.device, k
    return {k: v.cpu().numpy() for k, v in out.items()}


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


@pytest.mark.parametrize("name", rc.NAMES)
def test_pix_matches_the_numpy_statement(name):
    got, ref = fused(name)["pix"], rc.ref_pix(name)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    err = np.abs(got - ref)[~np.isnan(ref)]
    print(f"{name}: worst |pix - reference| {float(err.max()):.3e} px of {err.size} entries, {int(np.isnan(ref).sum())} NaN")
    assert bool((err <= rc.PIX_TOL).all())


@pytest.mark.parametrize("name", rc.NAMES)
def test_sampling_the_reference_pix_is_bit_equal(name):
    ref_rgb, ref_valid = rc.ref_sample(name)
    rgb, valid = rectify.sample_images(device_images(name), torch.tensor(rc.ref_pix(name), device=DEV))
    assert rgb.dtype == torch.float32 and valid.dtype == torch.uint8
    assert np.array_equal(valid.cpu().numpy(), ref_valid)
    assert rgb.cpu().numpy().tobytes() == ref_rgb.tobytes()


@pytest.mark.parametrize("name", rc.NAMES)
def test_the_fused_call_matches_the_numpy_statement(name):
    out = fused(name)
    ref_rgb, ref_valid = rc.ref_sample(name)
    band = rc.border_distance(name) <= rc.PIX_TOL                      # NaN compares false
    assert band.sum() <= 1e-3 * band.size
    assert np.array_equal(out["valid"][~band], ref_valid[~band]) and set(np.unique(out["valid"]).tolist()) <= {0, 1}
    assert np.array_equal(np.isnan(out["rgb"]), np.broadcast_to((out["valid"] == 0)[..., None], out["rgb"].shape))
    for v, im in enumerate(rc.images(name)):
        both = (out["valid"][v] == 1) & (ref_valid[v] == 1)
        got, ref = out["rgb"][v][both].astype(np.float64), ref_rgb[v][both].astype(np.float64)
        tol = rc.PIX_TOL * rc.neighbour_difference(im) + 2.0 ** -24 * np.abs(ref)
        err = np.abs(got - ref)
        print(f"{name} view {v}: {int(both.sum())} valid cells of {both.size}; worst |rgb - reference| / tolerance "
              f"{float((err / tol).max()) if err.size else 0.0:.3f}; entries that differ: {int((got != ref).sum())} of {got.size}")
        assert bool((err <= tol).all())


@pytest.mark.parametrize("name", ["1x7_r05", "33x65_r05", "130x257_r2", "box", "south"])
def test_bytes_of_the_fused_path_the_two_step_path_and_a_second_run(name):
    case = rc.BY_NAME[name]
    cams, imgs = rc.cameras(case), device_images(name)
    dsm = torch.tensor(rc.heights(name), device=DEV)
    ref = fused(name)
    pix = rectify.project_cells(dsm, case.grid, cams)
    rgb, valid = rectify.sample_images(imgs, pix)
    assert pix.cpu().numpy().tobytes() == ref["pix"].tobytes()
    assert rgb.cpu().numpy().tobytes() == ref["rgb"].tobytes() and valid.cpu().numpy().tobytes() == ref["valid"].tobytes()
    # without the occlusion, the mosaic and the pix plane the planes that remain are the same
    bare = orthorectify(imgs, cams, dsm, case.grid, case.alt_lo, case.alt_hi, occlusion=False)
    assert sorted(bare) == ["rgb", "valid"]
    assert bare["rgb"].cpu().numpy().tobytes() == ref["rgb"].tobytes() and bare["valid"].cpu().numpy().tobytes() == ref["valid"].tobytes()
    again = orthorectify(imgs, cams, dsm, case.grid, case.alt_lo, case.alt_hi, mosaic="median", pix=True)
    for k, v in ref.items():
        assert again[k].cpu().numpy().tobytes() == v.tobytes(), k
    # a float32 DSM is its widened copy
    low = dsm.float()
    a = orthorectify(imgs, cams, low, case.grid, case.alt_lo, case.alt_hi, mosaic="mean", pix=True)
    b = orthorectify(imgs, cams, low.double(), case.grid, case.alt_lo, case.alt_hi, mosaic="mean", pix=True)
    assert sorted(a) == sorted(b)
    for k in a:
        assert same_bytes(a[k], b[k]), k
    assert same_bytes(rectify.project_cells(low, case.grid, cams), a["pix"])


def test_a_plane_depends_neither_on_the_number_of_views_nor_on_its_position():
    name = "33x65_r2"
    case = rc.BY_NAME[name]
    cams, imgs = rc.cameras(case), device_images(name)
    dsm = torch.tensor(rc.heights(name), device=DEV)
    ref = fused(name)
    order = [2, 0, 3, 3, 1, 0, 2, 1, 3]                                  # V = 9, cameras repeated
    out = orthorectify([imgs[v] for v in order], [cams[v] for v in order], dsm, case.grid, case.alt_lo, case.alt_hi, pix=True)
    for k in ("rgb", "valid", "pix", "visible", "dirs", "dir_spread"):
        assert out[k].cpu().numpy().tobytes() == ref[k][order].tobytes(), k
    one = orthorectify(imgs[2:3], cams[2:3], dsm, case.grid, case.alt_lo, case.alt_hi, pix=True)
    for k in ("rgb", "valid", "pix", "visible", "dirs", "dir_spread"):
        assert one[k].cpu().numpy().tobytes() == ref[k][2:3].tobytes(), k
    # a (V, h, w, C) tensor is V images
    stack = torch.stack([imgs[1]] * 3)
    rgb, valid = rectify.sample_images(stack, torch.tensor(ref["pix"][[1, 0, 1]], device=DEV))
    assert rgb[0].cpu().numpy().tobytes() == ref["rgb"][1].tobytes() and torch.equal(valid[0], valid[2])


@pytest.mark.parametrize("name", rc.NAMES)
def test_view_directions_match_the_numpy_statement(name):
    case = rc.BY_NAME[name]
    ref_dirs, ref_spread = rc.ref_dirs(name)
    dirs, spread = rectify.view_directions(case.grid, rc.cameras(case), case.alt_lo, case.alt_hi, device=DEV)
    assert dirs.dtype == spread.dtype == torch.float32 and tuple(dirs.shape) == ref_dirs.shape and tuple(spread.shape) == ref_spread.shape
    dirs, spread = dirs.cpu().numpy(), spread.cpu().numpy()
    print(f"{name}: worst |dirs - reference| {float(np.abs(dirs.astype(np.float64) - ref_dirs).max()):.3e}, "
          f"|spread - reference| {float(np.abs(spread.astype(np.float64) - ref_spread).max()):.3e}, spread {spread.tolist()}")
    assert bool((np.abs(dirs.astype(np.float64) - ref_dirs) <= 2.0 ** -23).all())
    assert bool((np.abs(spread.astype(np.float64) - ref_spread) <= 2.0 ** -23).all())
    assert (dirs[:, 2] > 0).all()
    out = fused(name)
    assert out["dirs"].tobytes() == dirs.tobytes() and out["dir_spread"].tobytes() == spread.tobytes()


@pytest.mark.parametrize("name", ["1x7_r05", "33x65_r05", "130x257_r05", "box"])
def test_visible_is_cast_shadows_under_the_view_directions(name):
    case = rc.BY_NAME[name]
    out = fused(name)
    dsm = torch.tensor(rc.heights(name), device=DEV)
    shadow = cast_shadows(dsm, case.grid, out["dirs"]).cpu().numpy()
    vis = out["visible"]
    assert np.array_equal(vis == 1, shadow == 0) and np.array_equal(vis == 0, shadow == 1) and np.array_equal(vis == 255, shadow == 255)
    assert np.array_equal(vis == 255, np.broadcast_to(np.isnan(rc.heights(name)), vis.shape))
    if name == "box":
        # the strip of the CPU test: the device's directions are the reference's to 2⁻²³, which moves a ray
        # by less than 1e-4 m over the grid; the cells whose reference clearance is smaller may flip
        _, excess = sn.cast(rc.heights(name), case.grid.resolution, rc.ref_dirs(name)[0])
        clear = ~(np.abs(excess) <= 1e-4)
        assert clear.sum() >= 0.999 * clear.size and np.array_equal(vis[clear], rc.ref_visible(name)[clear]) and (vis == 0).sum() > 3000


def _views(seed, V, H, W, C):
    g = np.random.default_rng(seed)
    rgb = g.random((V, H, W, C), dtype=np.float32)
    usable = (g.random((V, H, W)) < 0.6).astype(np.uint8)
    usable[g.random((V, H, W)) < 0.05] = 255
    usable[:, 0, 0], usable[:, 0, 1], usable[0, 0, 1] = 0, 0, 1          # a count of 0, a count of 1
    usable[:, 0, 2:4] = 1                                                # all of them
    rgb[-1, 0, 3] = rgb[0, 0, 3]                                         # ... with a tie
    return rgb, usable


@pytest.mark.parametrize("mode", ["mean", "median"])
def test_mosaic_is_bit_equal_to_the_numpy_statement(mode):
    for V, C, (H, W) in ((1, 3, (5, 7)), (2, 1, (9, 31)), (4, 3, (33, 65)), (5, 4, (9, 31)), (9, 3, (17, 19)), (64, 2, (3, 5))):
        rgb, usable = _views(V, V, H, W, C)
        want, want_count, want_spread = rn.mosaic(rgb, usable, mode)
        out, count, spread = rectify.mosaic(torch.tensor(rgb, device=DEV), torch.tensor(usable, device=DEV), mode)
        assert out.dtype == spread.dtype == torch.float32 and count.dtype == torch.int32
        assert np.array_equal(count.cpu().numpy(), want_count), (V, C)
        assert want_count[0, 0] == 0 and want_count[0, 1] == 1 and want_count[0, 2] == V
        assert out.cpu().numpy().tobytes() == want.tobytes(), (V, C)
        assert spread.cpu().numpy().tobytes() == want_spread.tobytes(), (V, C)
    # a NaN among the usable values sorts last (rectify.mosaic takes any planes; orthorectify's usable cells are valid)
    rgb, usable = _views(7, 5, 9, 31, 3)
    rgb[np.random.default_rng(8).random(rgb.shape) < 0.1] = np.nan
    want = rn.mosaic(rgb, usable, mode)
    got = rectify.mosaic(torch.tensor(rgb, device=DEV), torch.tensor(usable, device=DEV), mode)
    assert np.isnan(want[0]).any() and not np.isnan(want[0]).all()
    for g, w in zip(got, want):
        assert np.array_equal(g.cpu().numpy(), w, equal_nan=True)
    # the mosaic of a case is the mosaic of its own planes
    for name in ("130x257_r05", "box"):
        ref = fused(name)
        usable = ((ref["valid"] == 1) & (ref["visible"] == 1)).astype(np.uint8)
        want = rn.mosaic(ref["rgb"], usable, "median")
        for got, w in zip((ref["mosaic_rgb"], ref["count"], ref["spread"]), want):
            assert got.tobytes() == w.tobytes()
    assert 0 < (fused("box")["count"] < 4).sum() and (fused("box")["count"] == 4).any()


def test_the_shipped_images_over_a_flat_dsm_end_to_end():
    case = rc.BY_NAME["130x257_r05"]
    cams, imgs = rc.cameras(case), device_images("130x257_r05")
    flat = np.full(case.grid.shape, -20.0)
    out = orthorectify(imgs, cams, torch.tensor(flat, device=DEV), case.grid, rc.ALT_LO, rc.ALT_HI, mosaic="median")
    assert sorted(out) == ["count", "dir_spread", "dirs", "mosaic_rgb", "rgb", "spread", "valid", "visible"]
    _, ref_valid = rn.sample(rc.images("130x257_r05"), rn.project(flat, case.grid, rc.ref_cameras(case)))
    count, mosaic = out["count"].cpu().numpy(), out["mosaic_rgb"].cpu().numpy()
    assert bool((out["visible"] == 1).all())                             # nothing hides anything on flat ground
    four = ref_valid.sum(0) == 4
    print(f"count 4 in {int(four.sum())} of {four.size} cells; count 0 in {int((count == 0).sum())}")
    assert four.sum() > 0.9 * four.size and bool((count[four] == 4).all())
    assert np.array_equal(np.isfinite(mosaic).all(-1), count > 0) and np.array_equal(np.isfinite(mosaic).any(-1), count > 0)
    assert np.array_equal(np.isfinite(out["spread"].cpu().numpy()), count > 0)
