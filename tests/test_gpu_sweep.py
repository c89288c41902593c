"""The plane sweep on the GPU (csrc/sweep.hip, spnerf_amd.sweep) — needs an MI355X.

Every step is held to the fp64 numpy statement (tests/sweep_numpy.py, itself pinned to known answers on
the CPU by tests/test_sweep_ref.py) on the cases of tests/sweep_cases.py:

* ``window_score`` on stored greys: ``score`` and ``views`` bit-equal;
* ``plane_grey``: ``valid`` equal wherever the reference pix lies more than PIX_TOL from a border, and
  |Δgrey| <= 2·PIX_TOL·(largest neighbour difference of the image) — a pix off by the 1e-5 px that
  tests/test_gpu_rectify.py asserts, in col and in row, moves a bilinear read by at most that;
* ``pick_plane`` on stored volumes: all four planes bit-equal;
* the fused ``plane_sweep`` against its own staged path (``plane_grey``, ``window_score`` per plane,
  ``pick_plane``): all four planes and the volume bit-equal;
* the fused call against the statement end to end: ``index`` equal except at near-tie cells (best and
  second-best fp32 score of the statement less than 1e-5 apart), at most 1 % of the cells with an index;
  where it agrees, |Δscore| and |Δaltitude| / step within three times the largest distance measured on
  the MI355X (the convention of DESIGN.md §5);
* the synthetic scene is recovered on its plane.

Measured on MI355X (2026-10-21), worst over the scenes "flat", "half" and "real": |score − statement| 1.118e-7,
|altitude − statement| / step 1.907e-6, 2.98e-7 over the whole volumes, no index differs and "half" has 6 near ties
of 2145 cells; ``grey`` at most 0.19 of its bound on the ramp and 0.004 on the other images.
"""
import functools

import numpy as np
import pytest
import torch

import rectify_cases as rc
import sweep_cases as sc
import sweep_numpy as sw
from spnerf_amd import plane_sweep, sweep
from test_gpu_parity import DEV

pytestmark = pytest.mark.gpu

MEASURED_SCORE = 1.118e-7       # largest |score − statement| where index agrees ("real"; 5.96e-8 on "flat" and "half"): two fp32 ulps
MEASURED_ALTITUDE = 1.907e-6    # largest |altitude − statement| / step where index agrees ("flat", "half"; 9.54e-7 on "real"): one fp32 ulp at 16 m
SCORE_TOL, ALTITUDE_TOL = 3 * MEASURED_SCORE, 3 * MEASURED_ALTITUDE


def device_images(name):
    return [torch.tensor(im, device=DEV) for im in sc.images(name)]


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


SCORE_CASES = [(shape, V, radius, mv, 0.0) for shape, V, radius, mv in
               (((1, 1), 2, 1, 2), ((1, 7), 3, 1, 2), ((1, 7), 2, 4, 2), ((7, 1), 4, 2, 4), ((7, 1), 16, 4, 2), ((17, 33), 2, 1, 2),
                ((17, 33), 3, 2, 3), ((17, 33), 4, 4, 2), ((17, 33), 16, 2, 2), ((33, 65), 2, 4, 2), ((33, 65), 3, 1, 2), ((33, 65), 4, 2, 4),
                ((33, 65), 16, 4, 2), ((33, 65), 16, 1, 16), ((33, 65), 8, 2, 2))] + [((33, 65), 4, 2, 2, 0.2), ((17, 33), 5, 1, 2, 0.15)]


@pytest.mark.parametrize("shape,V,radius,min_views,min_std", SCORE_CASES)
def test_window_score_is_bit_equal_to_the_numpy_statement(shape, V, radius, min_views, min_std):
    grey, valid = sc.stored(V, shape)
    want, want_views = sw.score(grey, valid, radius, min_views, min_std)
    score, views = sweep.window_score(torch.tensor(grey, device=DEV), torch.tensor(valid, device=DEV), radius=radius, min_views=min_views,
                                      min_std=min_std)
    assert score.dtype == torch.float32 and views.dtype == torch.uint8 and tuple(score.shape) == tuple(views.shape) == shape
    print(f"{shape} V {V} r {radius}: scored {int(np.isfinite(want).sum())} of {want.size} cells, views {np.bincount(want_views.ravel()).tolist()}")
    if shape[0] * shape[1] > 64:
        assert np.isfinite(want).any() and (want_views < V).any()
    assert np.array_equal(views.cpu().numpy(), want_views)
    assert same(score.cpu().numpy(), want)


@pytest.mark.parametrize("name", ["noise", "ramp", "real", "south", "flat"])
def test_plane_grey_matches_the_numpy_statement(name):
    scene = sc.BY_NAME[name]
    imgs = sc.images(name)
    worst = 0.0
    for k in range(min(scene.planes, 2)):
        grey, valid = sweep.plane_grey(device_images(name), sc.cameras(scene), scene.grid, sc.altitude(scene, k))
        assert grey.dtype == torch.float32 and valid.dtype == torch.uint8 and tuple(grey.shape) == tuple(valid.shape) == (len(imgs),) + scene.grid.shape
        grey, valid = grey.cpu().numpy(), valid.cpu().numpy()
        ref_grey, ref_valid = sc.ref_grey(name, k)
        clear = ~(sc.border_distance(sc.ref_pix(name, k), imgs) <= rc.PIX_TOL)
        assert np.array_equal(valid[clear], ref_valid[clear]) and set(np.unique(valid).tolist()) <= {0, 1}
        assert np.array_equal(np.isnan(grey), valid == 0)
        for v, im in enumerate(imgs):
            both = (valid[v] == 1) & (ref_valid[v] == 1)
            tol = 2 * rc.PIX_TOL * rc.neighbour_difference(im)
            err = np.abs(grey[v][both].astype(np.float64) - ref_grey[v][both].astype(np.float64))
            worst = max(worst, float(err.max()) / tol if err.size else 0.0)
            print(f"{name} plane {k} view {v}: {int(both.sum())} valid cells, worst |grey - reference| / bound {float(err.max()) / tol if err.size else 0.0:.4f}, "
                  f"entries that differ {int((err > 0).sum())}")
            assert bool((err <= tol).all())
    print(f"{name}: worst share of the bound {worst:.4f}")


def _volume(K, H, W, seed):
    g = np.random.default_rng(seed)
    vol = g.random((K, H, W), dtype=np.float32)
    vol[g.random((K, H, W)) < 0.2] = np.nan
    vol[:, 0, 0] = np.nan                                                # no plane at all
    if K > 1:
        vol[1, 0, 1:3] = vol[0, 0, 1:3] = 2.0                            # equal maxima: the lowest plane
        vol[K - 1, 1, :] = 3.0                                           # the best plane is the last one
    if K > 2:
        vol[1, 2, :] = 3.0                                               # an inner best, NaN neighbours among them
        vol[0, 3, :4], vol[1, 3, :4], vol[2, 3, :4] = 1.0, 3.0, 3.0      # a flat top: den < 0, the offset clamped at 0.5
    return vol, g.integers(2, 17, (K, H, W)).astype(np.uint8)


@pytest.mark.parametrize("K,H,W", [(1, 1, 1), (1, 5, 7), (2, 5, 7), (3, 17, 33), (9, 33, 65), (64, 9, 31)])
def test_pick_plane_is_bit_equal_to_the_numpy_statement(K, H, W):
    vol, views = _volume(K, H, W, K)
    want = sw.pick(vol, views, -23.5, 0.75)
    out = host(sweep.pick_plane(torch.tensor(vol, device=DEV), torch.tensor(views, device=DEV), -23.5, 0.75))
    assert sorted(out) == ["altitude", "index", "score", "views"]
    for k in out:
        assert same(out[k], want[k]), k
    assert want["index"][0, 0] == -1 and (K < 2 or H < 2 or (want["index"][0, 1] == 0 and (want["index"][1] == K - 1).all()))


def staged(imgs, cams, grid, alt_lo, step, K, **kw):
    volume, views = [], []
    for k in range(K):
        grey, valid = sweep.plane_grey(imgs, cams, grid, alt_lo + float(k) * step)
        s, m = sweep.window_score(grey, valid, **kw)
        volume.append(s)
        views.append(m)
    out = sweep.pick_plane(torch.stack(volume), torch.stack(views), alt_lo, step)
    out["volume"] = torch.stack(volume)
    return out


@pytest.mark.parametrize("shape", sc.SCORE_GRIDS)
@pytest.mark.parametrize("K", [1, 2, 3, 9])
def test_the_fused_sweep_has_the_bytes_of_its_staged_path(shape, K):
    scene = sc.BY_NAME["real"]
    grid, radius = sc._jax(shape), (1, 2, 4)[(K + shape[0]) % 3]
    imgs, cams = device_images("real"), sc.cameras(scene)
    kw = dict(radius=radius, min_views=2 + K % 2, min_std=0.0 if K != 3 else 0.01)
    want = host(staged(imgs, cams, grid, -24.0, 2.0, K, **kw))
    out = plane_sweep(imgs, cams, grid, -24.0, 2.0, K, volume=True, **kw)
    assert sorted(out) == ["altitude", "index", "score", "views", "volume"]
    assert out["altitude"].dtype == out["score"].dtype == out["volume"].dtype == torch.float32
    assert out["index"].dtype == torch.int32 and out["views"].dtype == torch.uint8 and tuple(out["volume"].shape) == (K,) + shape
    out = host(out)
    for k in want:
        assert same(out[k], want[k]), k
    bare = host(plane_sweep(imgs, cams, grid, -24.0, 2.0, K, **kw))                     # without the volume, and a second run
    assert sorted(bare) == ["altitude", "index", "score", "views"]
    for k in bare:
        assert same(bare[k], want[k]), k


@pytest.mark.parametrize("name,V", [("noise", 3), ("south", 3), ("flat", 4), ("real", 16), ("real", 7)])
def test_the_fused_sweep_on_other_images_channels_zones_and_view_counts(name, V):
    scene = sc.BY_NAME[name]
    order = [k % len(scene.views) for k in range(V)]
    imgs, cams = [device_images(name)[k] for k in order], [sc.cameras(scene)[k] for k in order]
    kw = dict(radius=scene.radius, min_views=scene.min_views)
    K = min(scene.planes, 3)
    want = host(staged(imgs, cams, scene.grid, scene.alt_lo, scene.step, K, **kw))
    out = host(plane_sweep(imgs, cams, scene.grid, scene.alt_lo, scene.step, K, volume=True, **kw))
    for k in want:
        assert same(out[k], want[k]), k
    assert (out["index"] >= 0).any()


@functools.lru_cache(maxsize=None)
def fused(name):
    s = sc.BY_NAME[name]
    return host(plane_sweep(device_images(name), sc.cameras(s), s.grid, s.alt_lo, s.step, s.planes, radius=s.radius, min_views=s.min_views,
                            volume=True))


@pytest.mark.parametrize("name", ["flat", "half", "real"])
def test_the_fused_sweep_matches_the_numpy_statement(name):
    scene, out, ref = sc.BY_NAME[name], fused(name), sc.ref_sweep(name)
    some = ref["index"] >= 0
    ties = sc.near_tie(ref["volume"])
    differ = out["index"] != ref["index"]
    agree = some & ~differ
    d_score = np.abs(out["score"][agree].astype(np.float64) - ref["score"][agree].astype(np.float64))
    d_alt = np.abs(out["altitude"][agree].astype(np.float64) - ref["altitude"][agree].astype(np.float64)) / scene.step
    d_vol = np.abs(out["volume"].astype(np.float64) - ref["volume"].astype(np.float64))
    print(f"{name}: {int(some.sum())} cells with an index, {int(ties.sum())} near ties, {int(differ.sum())} indices differ; "
          f"worst |score - statement| {float(d_score.max()):.3e}, worst |altitude - statement| / step {float(d_alt.max()):.3e}, "
          f"worst over the volume {float(np.nanmax(d_vol)):.3e}")
    assert ties.sum() <= 0.01 * some.sum()
    assert not (differ & ~ties).any()
    assert np.array_equal(np.isnan(out["volume"]), np.isnan(ref["volume"]))
    assert np.array_equal(out["views"][agree], ref["views"][agree])
    assert bool((d_score <= SCORE_TOL).all()) and bool((d_alt <= ALTITUDE_TOL).all())


def test_the_flat_scene_is_recovered_on_the_gpu():
    out = fused("flat")
    four = out["views"] == 4
    print(f"4 views usable at {int(four.sum())} of {four.size} cells; index histogram {np.bincount(out['index'][four], minlength=9).tolist()}")
    assert four.sum() > 0.5 * four.size and bool((out["index"][four] == 4).all())
    half = fused("half")
    four = half["views"] == 4
    assert bool((np.abs(half["altitude"][four].astype(np.float64) - sc.Z0) <= sc.BY_NAME["half"].step / 2).all())
