"""The numpy statement of the geometric shadows (tests/shadow_numpy.py) pinned to known answers —
scenes that need no interpolation, so the answers are exact — and the cases of the GPU test
(tests/shadow_cases.py) checked for cells that sit on the shadow boundary.  No GPU needed."""
import math

import numpy as np
import pytest

import shadow_cases as sc
import shadow_numpy as sn
import spnerf_amd
from spnerf_amd import shadow as shadow_mod
from spnerf_amd.satellite import sun_direction

RES = 0.5
BOX = 3.0


def box_scene():
    """Flat 9 x 15 ground at 0 m, a box of 3 m on columns 9-10, rows 3-5."""
    h = np.zeros((9, 15))
    h[3:6, 9:11] = BOX
    return h


def east(el):
    return np.array([math.cos(math.radians(el)), 0.0, math.sin(math.radians(el))], np.float32)


def north(el):
    return np.array([0.0, math.cos(math.radians(el)), math.sin(math.radians(el))], np.float32)


def test_sun_direction_points_from_the_ground_towards_the_sun():
    """The convention ``cast_shadows`` takes: (east, north, up) with up = sin(elevation) > 0, the
    azimuth clockwise from north."""
    for el, az in ((30.0, 90.0), (60.0, 0.0), (10.0, 225.0)):
        d = sun_direction(el, az)
        assert d[2] == pytest.approx(math.sin(math.radians(el))) and d[2] > 0
        assert d[0] == pytest.approx(math.sin(math.radians(az)) * math.cos(math.radians(el)))
        assert d[1] == pytest.approx(math.cos(math.radians(az)) * math.cos(math.radians(el)))
    assert sun_direction(30.0, 90.0)[0] > 0.8 and sun_direction(30.0, 0.0)[1] > 0.8
    assert sun_direction(30.0, 90.0)[1] != 0.0        # why the exact cases below are given as vectors


@pytest.mark.parametrize("el, shadowed_from", [(30.0, 0), (60.0, 6)])
def test_box_under_a_sun_due_east(el, shadowed_from):
    h = box_scene()
    tan = math.tan(math.radians(el))
    want = np.zeros(h.shape, np.uint8)
    for i in range(9):
        assert (9 - i) * RES * tan != BOX                           # never on the boundary
        want[3:6, i] = (9 - i) * RES * tan < BOX
    assert want[4].tolist() == [0] * shadowed_from + [1] * (9 - shadowed_from) + [0] * 6
    shadow, excess = sn.cast(h, RES, east(el)[None])
    assert shadow.shape == excess.shape == (1, 9, 15) and shadow.dtype == np.uint8 and excess.dtype == np.float64
    assert np.array_equal(shadow[0], want)
    # the excess is exact: the box above the ray at the box's near face, or the flat ground one step on
    d = east(el).astype(np.float64)
    rho = np.float64(RES) * d[2] / d[0]
    for i in range(9):
        at_box = (BOX - 0.0) - np.float64(9 - i) * rho
        assert excess[0, 4, i] == (at_box if i == 8 else max(at_box, -rho))
    assert excess[0, 4, 14] == -np.inf and excess[0, 0, 14] == -np.inf      # nothing east of the last column
    assert excess[0, 4, 9] == (BOX - BOX) - rho                             # the box's own roof: lit by one step's drop
    assert excess[0, 0, 3] == -rho                                           # flat ground: the next cell, one drop below


@pytest.mark.parametrize("el", [30.0, 60.0])
def test_box_under_a_sun_due_north_is_the_transposed_scene(el):
    h = box_scene()
    se, ee = sn.cast(h, RES, east(el)[None])
    # east (columns up) -> north (rows down): transpose, then flip the rows
    hn = np.ascontiguousarray(h.T[::-1])
    s, e = sn.cast(hn, RES, north(el)[None])
    assert np.array_equal(s[0], se[0].T[::-1]) and np.array_equal(e[0], ee[0].T[::-1])
    tan = math.tan(math.radians(el))
    for j in range(15):                                   # the box stands on rows 4-5 now, columns 3-5
        if j > 5:
            assert s[0, j, 4] == ((j - 5) * RES * tan < BOX)
        assert s[0, j, 0] == 0 and s[0, j, 8] == 0


def test_exact_diagonal_visits_the_diagonal_cells():
    """Azimuth 45° exactly: |a| = |b|, so the columns are the major axis, q = -1 and step m visits
    (j - m, i + m).  A one-cell pillar shadows the cells on its diagonal and no other."""
    el, P = 25.0, 1.0
    c = math.cos(math.radians(el)) * math.sqrt(0.5)
    d = np.array([c, c, math.sin(math.radians(el))], np.float32)
    assert d[0] == d[1] and sn.march(d, RES)[:3] == (0, 1, -1.0)
    h = np.zeros((8, 10))
    h[2, 6] = P
    rho = RES * math.tan(math.radians(el)) * math.sqrt(2.0)
    want = np.zeros(h.shape, np.uint8)
    for m in range(1, 6):
        want[2 + m, 6 - m] = m * rho < P
    assert want.sum() == 3
    shadow, excess = sn.cast(h, RES, d[None])
    assert np.array_equal(shadow[0], want)
    assert excess[0, 3, 5] == pytest.approx(P - rho, abs=1e-6) and excess[0, 3, 6] < 0 and excess[0, 2, 5] < 0
    # the three other diagonals, by the scene's symmetries
    for sx, sy in ((-1, 1), (1, -1), (-1, -1)):
        ss, _ = sn.cast(np.ascontiguousarray(h[::sy, ::sx]), RES, (d * np.array([sx, sy, 1], np.float32))[None])
        assert np.array_equal(ss[0], want[::sy, ::sx]), (sx, sy)


def test_nan_cells_as_occluders_and_as_targets():
    h = box_scene()
    h[4, 9:11] = np.nan                                  # row 4 loses its box: nothing occludes it
    shadow, excess = sn.cast(h, RES, east(60.0)[None])
    assert shadow[0, 4].tolist() == [0] * 9 + [255, 255] + [0] * 4
    assert np.isnan(excess[0, 4, 9:11]).all() and np.isfinite(excess[0, 4, :9]).all()
    assert shadow[0, 3].tolist() == [0] * 6 + [1] * 3 + [0] * 6              # the rows beside it keep theirs
    h = box_scene()
    h[4, 9] = np.nan                                     # the near face only: column 10 still occludes
    shadow, excess = sn.cast(h, RES, east(60.0)[None])
    tan = math.tan(math.radians(60.0))
    assert shadow[0, 4, :9].tolist() == [int((10 - i) * RES * tan < BOX) for i in range(9)] == [0] * 7 + [1, 1]
    assert shadow[0, 4, 9] == 255 and np.isnan(excess[0, 4, 9])
    # a NaN next to the interpolated sample drops that step only
    g = np.zeros((3, 6))
    g[0, 3], g[1, 3] = 10.0, np.nan
    d = np.array(sun_direction(20.0, 80.0), np.float32)           # y = 1 - m·q with 0 < q < 1: between rows 0 and 1
    s, _ = sn.cast(g, RES, d[None])
    assert s[0, 1, 2] == 0 and sn.cast(np.where(np.isnan(g), 0.0, g), RES, d[None])[0][0, 1, 2] == 1


def test_degenerate_grids_and_the_zenith():
    s, e = sn.cast(np.array([[4.0]]), RES, np.stack([east(30.0), north(30.0), np.array([0, 0, 1], np.float32)]))
    assert s.reshape(-1).tolist() == [0, 0, 0] and (e == -np.inf).all()
    s, e = sn.cast(box_scene(), RES, np.array([[0.0, 0.0, 1.0]], np.float32))
    assert not s.any() and (e == -np.inf).all()
    assert sn.march([0.0, 0.0, 1.0], RES)[0] is None
    s, e = sn.cast(np.array([[np.nan]]), RES, east(30.0)[None])
    assert s.tolist() == [[[255]]] and np.isnan(e).all()


def test_vectorised_statement_equals_the_plain_loops():
    g = np.random.default_rng(0)
    for shape in sc.SHAPES[:4]:
        h = sc.heights(shape)
        shadow, excess = sc.reference(shape)
        H, W = shape
        cells = [(j, i) for j in range(H) for i in range(W)]
        if len(cells) > 100:
            cells = [cells[c] for c in g.choice(len(cells), 100, replace=False)]
        for k, d in enumerate(sc.DIRS):
            for j, i in cells:
                s1, e1 = sn.cast_cell(h, sc.RESOLUTION, d, j, i)
                assert s1 == shadow[k, j, i] and (e1 == excess[k, j, i] or (np.isnan(e1) and np.isnan(excess[k, j, i]))), (shape, k, j, i)


@pytest.mark.parametrize("shape", sc.SHAPES)
def test_no_case_of_the_gpu_test_sits_on_the_shadow_boundary(shape):
    """tests/test_gpu_shadow.py allows 0.1 % of a case's cells within the tolerance of excess = 0,
    where the device's ``shadow`` may differ; the seeds are chosen so that there is none."""
    shadow, excess = sc.reference(shape)
    assert shadow.shape == excess.shape == (11,) + shape
    assert int(sc.in_band(shape).sum()) == 0
    h = sc.heights(shape)
    assert np.array_equal(shadow == 255, np.broadcast_to(np.isnan(h), shadow.shape))
    assert np.array_equal(np.isnan(excess), shadow == 255)
    assert not shadow[10].astype(bool)[~np.isnan(h)].any()                    # the zenith
    if shape[0] * shape[1] > 64:
        lit = (shadow[:10] == 0).sum() / shadow[:10].size
        assert 0.2 < lit < 0.95 and abs(np.nanmax(np.abs(h))) < 60.0          # both outcomes are exercised
        assert int(np.isnan(h).sum()) > 0


def test_agreement_statement_on_a_hand_made_case():
    sun = np.array([[[0.9, 0.2, np.nan], [0.6, 0.4, 0.1]],
                    [[0.9, 0.7, 0.5], [0.6, 1.0, np.inf]]], np.float32)
    shadow = np.array([[[0, 0, 1], [1, 1, 255]],
                       [[0, 0, 0], [0, 255, 1]]], np.uint8)
    t = sn.agreement_sums(sun, shadow)
    assert t["n_lit"].tolist() == [2, 4] and t["n_shadow"].tolist() == [2, 0]
    assert t["tp"].tolist() == [1, 0] and t["fp"].tolist() == [1, 0] and t["fn"].tolist() == [1, 0]
    f = lambda *v: float(sum(np.float64(np.float32(x)) for x in v))   # noqa: E731
    assert t["sum_sun_lit"][0] == pytest.approx(f(0.9, 0.2), rel=1e-15) and t["sum_sun_shadow"][0] == pytest.approx(f(0.6, 0.4), rel=1e-15)
    assert t["sum_abs"][0] == pytest.approx((1 - f(0.9)) + (1 - f(0.2)) + f(0.6) + f(0.4), rel=1e-15)
    a = sn.agreement(sun, shadow)
    assert a["n"].tolist() == [4, 4]
    assert a["mae"][0] == pytest.approx(1.9 / 4, abs=1e-7) and a["iou"][0] == pytest.approx(1 / 3, rel=1e-15)
    assert a["mean_sun_lit"][0] == pytest.approx(0.55, abs=1e-7) and a["mean_sun_shadow"][0] == pytest.approx(0.5, abs=1e-7)
    assert np.isnan(a["iou"][1]) and np.isnan(a["mean_sun_shadow"][1]) and a["mean_sun_lit"][1] == pytest.approx(0.675, abs=1e-7)
    # the library's host side forms the same ratios from the same sums
    b = shadow_mod.scores_from_sums(t)
    for k, v in a.items():
        assert np.array_equal(b[k], v, equal_nan=True), k
    assert spnerf_amd.shadow_agreement is shadow_mod.shadow_agreement and spnerf_amd.cast_shadows is shadow_mod.cast_shadows
