"""Known answers for the numpy statement of the plane sweep (tests/sweep_numpy.py), which
tests/test_gpu_sweep.py holds the device to — no GPU needed."""
import numpy as np
import pytest

import rectify_cases as rc
import sweep_cases as sc
import sweep_numpy as sw

ONES = lambda V, H, W: np.ones((V, H, W), np.uint8)   # noqa: E731


def noise(V, H, W, seed=0):
    return np.random.default_rng(seed).random((V, H, W), dtype=np.float32)


def test_identical_windows_score_one_and_opposite_ones_minus_one():
    a = noise(1, 9, 11)[0]
    for V in (2, 3, 4, 16):
        score, views = sw.score(np.stack([a] * V), ONES(V, 9, 11), 2)
        assert (views == V).all() and np.abs(score.astype(np.float64) - 1.0).max() <= 1e-6
        # a gain and an offset per view change nothing
        score, _ = sw.score(np.stack([np.float32(v + 1) * a + np.float32(v) for v in range(V)]), ONES(V, 9, 11), 2)
        assert np.abs(score.astype(np.float64) - 1.0).max() <= 1e-5
    score, views = sw.score(np.stack([a, -a]), ONES(2, 9, 11), 1)
    assert (views == 2).all() and np.abs(score.astype(np.float64) + 1.0).max() <= 1e-6


@pytest.mark.parametrize("V,radius", [(2, 1), (3, 2), (5, 4), (16, 2)])
def test_the_s_vector_score_is_the_mean_of_the_pairwise_znccs(V, radius):
    grey, valid = sc.stored(V, (17, 33))
    floor = 0.15 if V == 3 else 0.0
    # the statement in fp64 before its cast: the same function on a copy whose cast is exact enough to compare to 1e-12
    score, views = sw.score(grey, valid, radius, 2, floor)
    worst = 0.0
    for j in range(17):
        for i in range(33):
            want, m = sw.pairwise_zncc(grey, valid, radius, j, i, floor)
            assert views[j, i] == m
            assert np.isnan(score[j, i]) == (m < 2)
            if m >= 2:
                assert np.float32(want) == score[j, i] or abs(float(score[j, i]) - want) <= 2.0 ** -23
                worst = max(worst, abs(_score64(grey, valid, radius, j, i, floor) - want))
    assert worst <= 1e-12, worst


def _score64(grey, valid, radius, j, i, min_std):
    """The S-vector formula at one cell in fp64, uncast."""
    g = grey.astype(np.float64)
    V, H, W = g.shape
    rows, cols = slice(max(j - radius, 0), min(j + radius, H - 1) + 1), slice(max(i - radius, 0), min(i + radius, W - 1) + 1)
    S, m = 0.0, 0
    for v in range(V):
        x = g[v, rows, cols].ravel()
        d = x - x.sum() / x.size
        ss = (d * d).sum()
        if (valid[v, rows, cols] == 1).all() and ss > x.size * min_std * min_std:
            S, m = S + d / np.sqrt(ss), m + 1
    return float(((S * S).sum() - m) / (m * (m - 1)))


def test_a_constant_window_drops_its_view_and_too_few_views_give_nan():
    grey = noise(3, 9, 9, 1)
    grey[1, 2:7, 2:7] = 0.5
    score, views = sw.score(grey, ONES(3, 9, 9), 2)
    assert views[4, 4] == 2 and views[4, 5] == 3 and views[0, 0] == 3 and np.isfinite(score).all()
    score3, _ = sw.score(grey, ONES(3, 9, 9), 2, min_views=3)
    assert np.isnan(score3[4, 4]) and score3[4, 5] == score[4, 5]
    both = grey.copy()
    both[0, 2:7, 2:7] = 0.25
    score, views = sw.score(both, ONES(3, 9, 9), 2)
    assert views[4, 4] == 1 and np.isnan(score[4, 4])
    out = sw.pick(np.stack([score, score]), np.stack([views, views]), -20.0, 1.0)
    assert out["index"][4, 4] == -1 and np.isnan(out["altitude"][4, 4]) and np.isnan(out["score"][4, 4]) and out["views"][4, 4] == 0
    assert out["index"][0, 0] == 0 and out["views"][0, 0] == 3


def test_the_min_std_comparison_is_strict():
    # a 1 x 2 grid: both cells see the window {0, 1}: mean 0.5, ss = 0.5 = n·min_std² at min_std = 0.5 exactly
    grey = np.array([[[0.0, 1.0]], [[1.0, 3.0]]], np.float32)
    for min_std, m in ((0.0, 2), (0.49, 2), (0.5, 1), (0.75, 1), (1.0, 0)):   # view 1: ss = 2 = n·1²
        score, views = sw.score(grey, ONES(2, 1, 2), 1, 2, min_std)
        assert (views == m).all(), min_std
        assert np.isnan(score).all() == (m < 2)


def test_an_invalid_cell_anywhere_in_a_window_drops_that_view_there():
    grey, valid = noise(3, 9, 9, 2), ONES(3, 9, 9)
    valid[2, 4, 4] = 0
    valid[1, 0, 8] = 7                                                   # anything but 1
    for radius in (1, 2):
        _, views = sw.score(grey, valid, radius)
        jj, ii = np.mgrid[:9, :9]
        near = (np.abs(jj - 4) <= radius) & (np.abs(ii - 4) <= radius)
        corner = (jj <= radius) & (ii >= 8 - radius)
        assert np.array_equal(views, 3 - near.astype(int) - corner.astype(int))


def test_windows_are_clipped_at_the_grid_and_a_single_cell_is_nan():
    grey = noise(2, 5, 6, 3)
    score, views = sw.score(grey, ONES(2, 5, 6), 2)
    for (j, i), rows, cols in (((0, 0), slice(0, 3), slice(0, 3)), ((4, 5), slice(2, 5), slice(3, 6)), ((0, 5), slice(0, 3), slice(3, 6))):
        a, b = (grey[v, rows, cols].astype(np.float64).ravel() for v in (0, 1))
        a, b = a - a.mean(), b - b.mean()
        assert abs(float(score[j, i]) - float(a @ b / np.sqrt((a @ a) * (b @ b)))) <= 1e-6 and views[j, i] == 2
    score, views = sw.score(noise(4, 1, 1), ONES(4, 1, 1), 1)
    assert np.isnan(score).all() and (views == 0).all()
    out = sw.pick(score[None], views[None], 0.0, 1.0)
    assert out["index"][0, 0] == -1 and np.isnan(out["altitude"][0, 0])


def test_the_pick_by_hand():
    nan = np.nan
    columns = [[0.1, 0.5, 0.3], [0.5, 0.1, 0.0], [0.0, 0.1, 0.5], [nan, 0.5, 0.3], [0.3, 0.5, nan], [0.5, 0.5, 0.2], [nan, nan, nan],
               [0.2, 0.5, 0.5], [nan, nan, 0.25], [0.5, 0.5, 0.5], [0.0, 0.5, 0.49999]]
    vol = np.array(columns, np.float32).T.reshape(3, 1, -1)
    views = np.arange(3 * vol.shape[2], dtype=np.uint8).reshape(vol.shape) % 5 + 2
    out = sw.pick(vol, views, -20.0, 2.0)
    assert out["index"][0].tolist() == [1, 0, 2, 1, 1, 0, -1, 1, 2, 0, 1]
    s = vol.astype(np.float64)[:, 0, 0]
    offset = 0.5 * (s[0] - s[2]) / ((s[0] - 2.0 * s[1]) + s[2])           # 0.5·(0.1 − 0.3) / (0.1 − 1 + 0.3) = 1/6
    assert abs(offset - 1.0 / 6.0) < 1e-7
    want = [np.float32(-20.0 + (1.0 + offset) * 2.0), -20.0, -16.0, -18.0, -18.0, -20.0, nan, np.float32(-20.0 + 1.5 * 2.0), -16.0, -20.0]
    assert np.array_equal(out["altitude"][0, :10], np.array(want, np.float32), equal_nan=True)
    # the last column: the vertex lies 0.49999 of a step up, inside the clamp
    s = vol.astype(np.float64)[:, 0, 10]
    assert out["altitude"][0, 10] == np.float32(-20.0 + (1.0 + 0.5 * (s[0] - s[2]) / ((s[0] - 2.0 * s[1]) + s[2])) * 2.0)
    assert np.array_equal(out["score"][0], np.array([0.5, 0.5, 0.5, 0.5, 0.5, 0.5, nan, 0.5, 0.25, 0.5, 0.5], np.float32), equal_nan=True)
    at = np.maximum(out["index"], 0)[None]
    assert np.array_equal(out["views"], np.where(out["index"] >= 0, np.take_along_axis(views, at, 0)[0], 0))
    assert out["altitude"].dtype == out["score"].dtype == np.float32 and out["index"].dtype == np.int32 and out["views"].dtype == np.uint8
    one = sw.pick(vol[:1], views[:1], 3.0, 1.0)                         # K = 1
    assert np.array_equal(one["altitude"][0], np.where(np.isnan(vol[0, 0]), np.float32(nan), np.float32(3.0)), equal_nan=True)


@pytest.mark.parametrize("name", ["noise", "ramp", "real", "south", "flat"])
def test_grey_planes_of_the_scenes(name):
    scene = sc.BY_NAME[name]
    grey, valid = sc.ref_grey(name, 0)
    pix, imgs = sc.ref_pix(name, 0), sc.images(name)
    assert grey.dtype == np.float32 and valid.dtype == np.uint8 and grey.shape == (len(scene.views),) + scene.grid.shape
    assert valid.any() and np.array_equal(np.isnan(grey), valid == 0)
    d = sc.border_distance(pix, imgs)
    print(name, f"valid {valid.mean():.3f}, closest to a border {float(np.nanmin(d)):.3e} px")
    assert float(np.nanmin(d)) > 10 * rc.PIX_TOL
    if name == "ramp":
        # the mean of the channels of a·col + b·row is itself a ramp; each channel is exact to its one fp32 rounding
        a, b = sc.RAMP[:scene.channels].mean(0)
        want = a * pix[..., 0] + b * pix[..., 1]
        for v, im in enumerate(imgs):
            h, w, _ = im.shape
            centred = want[v] - (a * (w // 2) + b * (h // 2))
            ok = valid[v] == 1
            err = np.abs(grey[v].astype(np.float64) - centred)[ok]
            assert float(err.max()) <= 2.0 ** -22 * float(np.abs(im).max())
            # the input's condition for the GPU test's bound: a rounding flip of a value (one ulp) stays below a quarter of it
            assert 2.0 ** -23 * float(np.abs(grey[v][ok]).max()) * 4 <= 2 * rc.PIX_TOL * rc.neighbour_difference(im)


def test_the_flat_scene_is_recovered_on_its_plane():
    out = sc.ref_sweep("flat")
    four = out["views"] == 4
    print(f"4 views usable at {int(four.sum())} of {four.size} cells; index histogram {np.bincount(out['index'][four], minlength=9).tolist()}")
    assert four.sum() > 0.5 * four.size and bool((out["index"][four] == 4).all())
    assert out["volume"].shape == (9, 33, 65) and float(np.nanmin(out["score"][four])) > 0.9


def test_the_half_way_scene_is_recovered_within_half_a_step():
    out, scene = sc.ref_sweep("half"), sc.BY_NAME["half"]
    four = out["views"] == 4
    err = np.abs(out["altitude"][four].astype(np.float64) - sc.Z0)
    print(f"worst |altitude - z0| {float(err.max()):.3f} m, median {float(np.median(err)):.3f} m")
    assert four.sum() > 0.5 * four.size and bool((err <= scene.step / 2).all())


@pytest.mark.parametrize("name", ["flat", "half", "real"])
def test_near_ties_are_rare_and_the_pixel_tolerance_moves_no_other_index(name):
    """The GPU test lets ``index`` differ at near-tie cells only, at most 1 % of the cells with an index:
    the statement itself, its pix moved by ±PIX_TOL, stays inside that."""
    out = sc.ref_sweep(name)
    some = out["index"] >= 0
    for shift in (rc.PIX_TOL, -rc.PIX_TOL):
        moved = sc.ref_sweep(name, shift)
        ties = sc.near_tie(out["volume"]) | sc.near_tie(moved["volume"])
        differ = moved["index"] != out["index"]
        print(name, shift, f"near ties {int(ties.sum())} of {int(some.sum())}, indices that differ {int(differ.sum())}")
        assert ties.sum() <= 0.01 * some.sum() and not (differ & ~ties).any()
