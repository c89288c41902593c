"""Known answers for the numpy statement of the orthorectification (tests/rectify_numpy.py), which
tests/test_gpu_rectify.py holds the device to — no GPU needed."""
import math

import numpy as np
import pytest

import rectify_cases as rc
import rectify_numpy as rn
import shadow_numpy as sn
from oracle import dsm_ref
from spnerf_amd import GroundGrid


def test_bilinear_read_by_hand():
    img = np.array([[[0.0], [1.0], [4.0]], [[2.0], [3.0], [8.0]]], np.float32)             # h = 2, w = 3
    nan = np.nan
    pix = np.array([[0.0, 0.0], [2.0, 1.0], [0.25, 0.5], [1.5, 0.0], [2.0, 0.5], [1.0, 1.0],   # inside, borders included
                    [2.0000001, 0.0], [-1e-9, 0.0], [0.0, 1.0000001], [nan, 0.0], [0.0, nan], [np.inf, 0.0]])
    rgb, valid = rn.sample_one(img, pix)
    assert valid.tolist() == [1] * 6 + [0] * 6 and valid.dtype == np.uint8 and rgb.dtype == np.float32
    # (0.25, 0.5): top 0.25, bottom 2.25, halfway 1.25; (1.5, 0): 2.5; (2, 0.5): the clamped column, 6
    assert rgb[:6, 0].tolist() == [0.0, 8.0, 1.25, 2.5, 6.0, 3.0]
    assert np.isnan(rgb[6:]).all()


@pytest.mark.parametrize("name", [n for n in rc.NAMES if rc.BY_NAME[n].images == "ramp"])
def test_a_ramp_image_is_reproduced_at_the_pixel_positions(name):
    """A bilinear read of a·col + b·row + c is a·pix_col + b·pix_row + c, to the one fp32 rounding."""
    case = rc.BY_NAME[name]
    pix = rc.ref_pix(name)
    rgb, valid = rc.ref_sample(name)
    assert valid.any() and rgb.shape == pix.shape[:3] + (case.channels,)
    for c, (a, b, off) in enumerate(rc.RAMP[:case.channels]):
        want = a * pix[..., 0] + b * pix[..., 1] + off
        ok = valid == 1
        err = np.abs(rgb[..., c].astype(np.float64) - want)[ok]
        assert bool((err <= 2.0 ** -24 * np.abs(want[ok]) + 1e-13).all()), (c, float(err.max()))
    assert np.isnan(rgb[valid == 0]).all() and not np.isnan(rgb[valid == 1]).any()


@pytest.mark.parametrize("name", rc.NAMES)
def test_a_projected_cell_localises_back_to_its_centre(name):
    """pix of a cell, localised at the cell's altitude by the oracle's inverse and brought to UTM by the
    oracle's forward projection, is the cell centre within 1e-6 m (the floor tests/test_gpu_ortho.py uses
    for the forward path; the oracle's own UTM round trip is 4e-9 m).  NaN exactly where the DSM is."""
    case = rc.BY_NAME[name]
    dsm, pix = rc.heights(name), rc.ref_pix(name)
    E, N = rn.cell_centres(case.grid)
    known = ~np.isnan(dsm)
    assert np.array_equal(np.isnan(pix[..., 0]), np.broadcast_to(~known, pix.shape[:3])) and np.array_equal(np.isnan(pix[..., 0]), np.isnan(pix[..., 1]))
    worst = 0.0
    for v, cam in enumerate(rc.ref_cameras(case)):
        lon, lat = cam.localization(pix[v, ..., 0][known], pix[v, ..., 1][known], dsm[known])
        e, n = dsm_ref.utm(lat, lon, case.grid.zone, case.grid.south)
        worst = max(worst, float(np.hypot(e - E[known], n - N[known]).max()))
    print(name, f"worst distance from the cell centre {worst:.2e} m")
    assert worst <= 1e-6


@pytest.mark.parametrize("name", rc.NAMES)
def test_no_pixel_position_lies_on_an_image_border(name):
    """The GPU test lets ``valid`` differ where the reference pix is within its tolerance of a border:
    no cell of any case is."""
    d = rc.border_distance(name)
    print(name, f"closest to a border: {float(np.nanmin(d)):.3e} px")
    assert float(np.nanmin(d)) > 10 * rc.PIX_TOL


@pytest.mark.parametrize("name", rc.NAMES)
def test_lines_of_sight_point_up_at_the_camera(name):
    dirs, spread = rc.ref_dirs(name)
    case = rc.BY_NAME[name]
    assert dirs.dtype == np.float32 and dirs.shape == (len(case.views), 3) and spread.shape == (len(case.views),)
    assert (dirs[:, 2] > 0.9).all() and np.allclose(np.linalg.norm(dirs.astype(np.float64), axis=1), 1.0, atol=1e-7)
    assert (spread >= 0).all() and (spread < 1e-3).all()


def test_one_direction_per_view_over_the_roi_costs_under_a_centimetre():
    """Over the 256 m ROI the corners' lines of sight differ from the centre's by 2.6e-4 to 2.8e-4 per
    component: under 1 cm over the scene's 28 m of altitude."""
    grid = GroundGrid(rc.ROI_XOFF, rc.ROI_YTOP, 512, 512, 0.5, 17)
    whole = rc.Case("roi", grid, "relief", (0, 1, 2, 3), "real", 3, rc.ALT_LO, rc.ALT_HI)
    dirs, spread = rn.view_directions(grid, rc.ref_cameras(whole), rc.ALT_LO, rc.ALT_HI)
    print("spread", spread.tolist(), "off-nadir", np.degrees(np.arccos(dirs[:, 2].astype(np.float64))).tolist())
    assert (spread > 2.5e-4).all() and (spread < 2.9e-4).all()
    assert float(spread.max()) * (rc.ALT_HI - rc.ALT_LO) < 0.01
    # the direction is where a higher point of the same pixel moves to: 20 m up, the ground point moves 20·(e, n)/u
    cam = rc.ref_cameras(whole)[0]
    e0, n0 = grid.xoff + 128.0, grid.ytop - 128.0
    d = rn.line_of_sight(cam, e0, n0, 17, False, rc.ALT_LO, rc.ALT_HI)
    d20 = rn.line_of_sight(cam, e0, n0, 17, False, rc.ALT_LO, rc.ALT_LO + 20.0)
    assert np.abs(d - d20).max() < 1e-5


def test_the_box_hides_a_strip_of_height_tan_off_nadir_behind_it():
    """``visible`` hides exactly the cells ``shadow_numpy.cast`` puts behind higher terrain under the
    view direction, and behind the 30 m box that is a strip of height·tan(off-nadir)/res cells along
    the view azimuth, within one cell."""
    case, box = rc.BY_NAME["box"], rc.BOX
    dsm, res = rc.heights("box"), case.grid.resolution
    dirs, _ = rc.ref_dirs("box")
    vis = rc.ref_visible("box")
    shadow, _ = sn.cast(dsm, res, dirs)
    assert np.array_equal(vis == 0, shadow == 1) and np.array_equal(vis == 1, shadow == 0) and not (vis == 255).any()
    roof = np.zeros(dsm.shape, bool)
    roof[box["rows"][0]:box["rows"][1], box["cols"][0]:box["cols"][1]] = True
    for v, d in enumerate(dirs.astype(np.float64)):
        assert not (vis[v][roof] == 0).any()                       # nothing stands above the roof
        hidden = (vis[v] == 0) & ~roof
        a, b, u = d[0], -d[1], d[2]                                # along the columns, along the rows (southwards), up
        want = box["height"] * math.hypot(a, b) / u / res          # cells along the azimuth
        # the strip runs away from the camera: along the march's major axis, through the middle of the box
        if abs(a) >= abs(b):
            j = (box["rows"][0] + box["rows"][1]) // 2
            steps = int(hidden[j].sum())
            assert hidden[j].any() and (np.flatnonzero(hidden[j]).max() < box["cols"][0] if a > 0 else np.flatnonzero(hidden[j]).min() >= box["cols"][1])
            length = steps * math.hypot(a, b) / abs(a)
        else:
            i = (box["cols"][0] + box["cols"][1]) // 2
            steps = int(hidden[:, i].sum())
            assert hidden[:, i].any() and (np.flatnonzero(hidden[:, i]).max() < box["rows"][0] if b > 0 else np.flatnonzero(hidden[:, i]).min() >= box["rows"][1])
            length = steps * math.hypot(a, b) / abs(b)
        print(f"view {v}: off-nadir {math.degrees(math.atan2(math.hypot(a, b), u)):.2f} deg, strip {length:.2f} cells, "
              f"height·tan/res {want:.2f} cells, hidden {int(hidden.sum())} cells")
        assert abs(length - want) <= 1.0
        assert int(hidden.sum()) > 0.5 * want * 50                 # a strip as wide as the box, not a line


def _random_views(seed, V, H, W, C):
    g = np.random.default_rng(seed)
    rgb = g.random((V, H, W, C), dtype=np.float32)
    usable = (g.random((V, H, W)) < 0.6).astype(np.uint8)
    usable[g.random((V, H, W)) < 0.05] = 255                             # anything but 1 does not count
    usable[:, 0, 0], usable[:, 0, 1], usable[0, 0, 1] = 0, 0, 1          # a count of 0, a count of 1
    usable[:, 0, 2:4] = 1                                                # all of them
    rgb[-1, 0, 3] = rgb[0, 0, 3]                                         # ... with a tie
    return rgb, usable


@pytest.mark.parametrize("V", [1, 2, 4, 5])
@pytest.mark.parametrize("mode", ["mean", "median"])
def test_mosaic_is_the_nanmean_or_the_nanmedian_of_the_usable_views(V, mode):
    rgb, usable = _random_views(V, V, 9, 11, 3)
    out, count, spread = rn.mosaic(rgb, usable, mode)
    use = usable == 1
    assert out.dtype == spread.dtype == np.float32 and count.dtype == np.int32 and np.array_equal(count, use.sum(0))
    assert count[0, 0] == 0 and count[0, 1] == 1 and count[0, 2] == V and set(np.unique(count)) >= set(range(min(V, 3) + 1))
    x = np.where(use[..., None], rgb.astype(np.float64), np.nan)
    some = count > 0
    want = (np.nanmean if mode == "mean" else np.nanmedian)(x[:, some], axis=0)
    assert bool((np.abs(out[some].astype(np.float64) - want) <= 2.0 ** -24 * np.abs(want) + 1e-15).all())
    mean = np.nanmean(x[:, some], axis=0)
    rms = np.sqrt(np.nanmean((x[:, some] - mean) ** 2, axis=(0, 2)))
    assert bool((np.abs(spread[some].astype(np.float64) - rms) <= 2.0 ** -23 * rms + 1e-12).all())
    assert np.isnan(out[~some]).all() and np.isnan(spread[~some]).all() and not np.isnan(out[some]).any()
    assert (spread[count == 1] == 0).all()
    if mode == "median":                                                  # an odd count returns one of the values
        odd = count % 2 == 1
        assert bool((out[odd][..., None, :] == np.moveaxis(rgb, 0, -2)[odd]).any(-2).all())


def test_visible_maps_the_shadow_planes():
    assert rn.visible_from_shadow(np.array([0, 1, 255], np.uint8)).tolist() == [1, 0, 255]


def test_a_usable_nan_sorts_last_in_the_median():
    """A NaN among the usable values sorts after every number, so it reaches the median only from the
    middle upwards; the mean and the spread of such a cell are NaN."""
    nan = np.nan
    rgb = np.array([[nan], [3.0], [1.0], [2.0], [nan]], np.float32).reshape(5, 1, 1, 1)
    for usable, median in (([1, 1, 1, 1, 0], 2.5), ([1, 1, 1, 0, 0], 3.0), ([1, 1, 0, 0, 1], nan), ([1, 0, 0, 0, 0], nan)):
        out, count, spread = rn.mosaic(rgb, np.array(usable, np.uint8).reshape(5, 1, 1), "median")
        assert count[0, 0] == sum(usable) and np.array_equal(out[0, 0], np.array([median], np.float32), equal_nan=True), usable
        assert np.isnan(spread[0, 0]) and np.isnan(rn.mosaic(rgb, np.array(usable, np.uint8).reshape(5, 1, 1), "mean")[0][0, 0, 0])
