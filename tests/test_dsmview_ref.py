"""The numpy statement of the DSM view (tests/dsmview_numpy.py) pinned against closed forms — no GPU needed.

Measured on the statement (the bounds below are twice these):
* chord error — the crossing's ``ground`` against the UTM of the pixel's localisation at the crossing's altitude,
  i.e. what the straight segment between the two localisations costs: 8.5e-6 m over alt_hi − alt_lo = 28 m
  ("plane"; "tilt" 6.8e-6 m) and 4.9e-5 m over 60 m ("tilt60", the camera furthest off nadir; "plane60" 1.2e-5 m);
* round trip — the crossing through the forward RPC against its pixel: 1.44e-4 pixels of a full-resolution camera
  at the most ("tilt60"; 3.7e-5 pixels over 28 m), which is the chord error again, in pixels of 0.3 m;
* "box": 2.1 % of the 1191 hit pixels lie within one cell of a shadow boundary and are left out; 5.5 % of the
  cells are hidden from the camera and none of them is hit.
"""
import numpy as np
import pytest

import dsmview_cases as dc
import dsmview_numpy as dn
import ortho_numpy as on
import rectify_numpy as rn
import shadow_numpy as sn
import surface_cases as fc
import sweep_cases as sc
from oracle import dsm_ref, rpc_ref

CHORD_TOL = {"plane": 2 * 8.5e-6, "plane60": 2 * 1.2e-5, "tilt": 2 * 6.8e-6, "tilt60": 2 * 4.9e-5}   # metres
ROUND_TRIP_TOL = 2 * 1.44e-4                                                                        # pixels
INSIDE = 1.0                                                                                        # cells from the grid's outer centre lines


def pixels(name):
    return dn.lattice_pixels(dc.rect(name), dc.BY_NAME[name].stride)


def grid_xy(grid, e, n):
    return (e - grid.xoff) / grid.resolution - 0.5, (grid.ytop - n) / grid.resolution - 0.5


def inside(grid, x, y):
    return (x >= INSIDE) & (x <= grid.xsize - 1 - INSIDE) & (y >= INSIDE) & (y <= grid.ysize - 1 - INSIDE)


@pytest.mark.parametrize("name", ["plane", "plane60"])
def test_a_constant_plane_is_hit_where_the_line_of_sight_crosses_it(name):
    case, out = dc.BY_NAME[name], dc.ref(name)
    col, row = pixels(name)
    lon, lat = dn.localise(dc.ref_camera(case), col, row, dc.PLANE_ALT)
    e, n = dsm_ref.utm(lat, lon, case.grid.zone, case.grid.south)
    must = inside(case.grid, *grid_xy(case.grid, e, n))
    assert must.mean() > 0.5 and bool((out["hit"][must] == 1).all())
    alt = out["altitude"][must]
    assert bool((np.abs(alt.astype(np.float64) - dc.PLANE_ALT) <= np.spacing(np.float32(abs(dc.PLANE_ALT)))).all())
    chord = np.hypot(out["ground"][..., 0] - e, out["ground"][..., 1] - n)[must]
    print(f"{name}: chord error {chord.max():.3e} m over {case.alt_hi - case.alt_lo} m")
    assert float(chord.max()) <= CHORD_TOL[name]
    # depth is the distance from the alt_hi end, in (E, N, alt)
    s = out["seg"]
    d = np.sqrt((out["ground"][..., 0] - s["e_hi"]) ** 2 + (out["ground"][..., 1] - s["n_hi"]) ** 2 + (dc.PLANE_ALT - case.alt_hi) ** 2)
    assert float(np.abs(out["depth"].astype(np.float64) - d)[must].max()) <= 4e-6


@pytest.mark.parametrize("name", ["tilt", "tilt60"])
def test_a_tilted_plane_is_hit_at_the_analytic_intersection(name):
    case, out = dc.BY_NAME[name], dc.ref(name)
    s = out["seg"]
    dE, dN, dA = s["e_lo"] - s["e_hi"], s["n_lo"] - s["n_hi"], case.alt_lo - case.alt_hi
    t = (sc.Z0 + fc.SLOPE * (s["e_hi"] - fc.E_CENTRE) - case.alt_hi) / (dA - fc.SLOPE * dE)
    e, n, z = s["e_hi"] + t * dE, s["n_hi"] + t * dN, case.alt_hi + t * dA
    must = inside(case.grid, *grid_xy(case.grid, e, n))
    assert must.mean() > 0.5 and bool((out["hit"][must] == 1).all())
    # the heights are the plane rounded to fp32 (1e-6 m at 20 m), the altitude is cast once more
    assert float(np.abs(out["altitude"].astype(np.float64) - z)[must].max()) <= 5e-6
    assert float(np.hypot(out["ground"][..., 0] - e, out["ground"][..., 1] - n)[must].max()) <= 5e-6
    col, row = pixels(name)
    lon, lat = dn.localise(dc.ref_camera(case), col[must], row[must], z[must])
    e2, n2 = dsm_ref.utm(lat, lon, case.grid.zone, case.grid.south)
    chord = np.hypot(e2 - e[must], n2 - n[must])
    print(f"{name}: chord error {chord.max():.3e} m over {case.alt_hi - case.alt_lo} m")
    assert float(chord.max()) <= CHORD_TOL[name]


def test_every_hit_on_the_box_is_visible_to_the_camera():
    case, out = dc.BY_NAME["box"], dc.ref("box")
    dirs, _ = rn.view_directions(case.grid, [dc.ref_camera(case)], case.alt_lo, case.alt_hi)
    shadow = sn.cast(dc.dsm("box").astype(np.float64), case.grid.resolution, dirs)[0][0]
    H, W = shadow.shape
    pad = np.pad(shadow, 1, mode="edge")
    near_boundary = np.zeros((H, W), bool)
    for dj in (0, 1, 2):
        for di in (0, 1, 2):
            near_boundary |= pad[dj:dj + H, di:di + W] != shadow
    hit = out["hit"] == 1
    i, j = np.floor(out["cell"][..., 0][hit] + 0.5).astype(int), np.floor(out["cell"][..., 1][hit] + 0.5).astype(int)
    left_out = near_boundary[j, i]
    print(f"box: {hit.sum()} hits, {left_out.mean():.4f} within one cell of a shadow boundary, {(shadow == 1).mean():.3f} of the cells hidden")
    assert hit.sum() > 1000 and (shadow == 1).sum() > 50 and left_out.mean() < 0.05
    assert bool((shadow[j, i][~left_out] == 0).all())
    # and the roof is seen: hits at the box's altitude
    top = dc.BOX["ground"] + dc.BOX["height"]
    assert (np.abs(out["altitude"][hit] - top) < 1e-3).sum() > 50


@pytest.mark.parametrize("name", [n for n in dc.NAMES if n not in ("nan", "off")])
def test_the_crossing_projects_back_to_its_pixel(name):
    case, out = dc.BY_NAME[name], dc.ref(name)
    hit = out["hit"] == 1
    col, row = pixels(name)
    lat, lon = on.utm_inverse(out["ground"][..., 0][hit], out["ground"][..., 1][hit], case.grid.zone, case.grid.south)
    pc, pr = dc.ref_camera(case).projection(lon, lat, out["altitude"][hit].astype(np.float64))
    # the fp32 altitude moves the pixel by up to 1e-6 m · tan(off nadir) / 0.3 m: nothing
    worst = float(np.hypot(pc - col[hit], pr - row[hit]).max()) * case.downscale   # in full-resolution pixels
    print(f"{name}: round trip {worst:.3e} pixels")
    assert hit.any() and worst <= ROUND_TRIP_TOL


def test_the_near_end_is_the_near_point_of_get_rays():
    for name in ("relief", "south", "plane60"):
        case, s = dc.BY_NAME[name], dc.ref(name)["seg"]
        col, row = pixels(name)
        near = np.stack(rpc_ref.geodetic_to_ecef(s["lat_hi"], s["lon_hi"], np.full(col.shape, case.alt_hi)), -1).astype(np.float32)
        rays = rpc_ref.get_rays(col.ravel(), row.ravel(), dc.ref_camera(case), case.alt_lo, case.alt_hi).reshape(col.shape + (8,))
        # the same point rounded to fp32, but for a rounding flip where the two iterations stop 1e-5 m apart
        assert float(np.abs(near.astype(np.float64) - rays[..., :3]).max()) <= 0.5 and (near == rays[..., :3]).mean() > 0.99
        # and the (E, N) of the near end is its forward projection
        e, n = dsm_ref.utm(s["lat_hi"], s["lon_hi"], case.grid.zone, case.grid.south)
        assert np.array_equal(e, s["e_hi"]) and np.array_equal(n, s["n_hi"])


def test_transparent_cells_misses_and_single_segments():
    assert not dc.ref("nan")["hit"].any() and not dc.ref("off")["hit"].any()
    for name in ("nan", "off"):
        out = dc.ref(name)
        assert all(np.isnan(out[k]).all() for k in ("altitude", "ground", "cell", "depth"))
    # lattices partly off the grid: hits and misses both, every hit's cell inside the grid
    for name in ("relief_s3", "relief_edge", "relief_17", "relief_ds4"):
        out, g = dc.ref(name), dc.BY_NAME[name].grid
        hit = out["hit"] == 1
        assert 0.1 < hit.mean() < 0.9
        assert np.array_equal(np.isnan(out["altitude"]), ~hit) and np.array_equal(np.isnan(out["depth"]), ~hit)
        x, y = out["cell"][..., 0][hit], out["cell"][..., 1][hit]
        assert x.min() >= 0 and x.max() <= g.xsize - 1 and y.min() >= 0 and y.max() <= g.ysize - 1
    # a hit never lands on a transparent cell's own height: the altitude at a hit is finite and within the segment
    out, case = dc.ref("holes"), dc.BY_NAME["holes"]
    hit = out["hit"] == 1
    assert hit.mean() > 0.9 and np.isfinite(out["altitude"][hit]).all()
    assert out["altitude"][hit].min() >= case.alt_lo and out["altitude"][hit].max() <= case.alt_hi

    # walk() alone, on hand-made segments over a 5 x 5 grid: a step of 2 m on a floor of 0 m, columns 3 and 4 raised
    dsm = np.zeros((5, 5), np.float32)
    dsm[:, 3:] = 2.0
    one = lambda *v: tuple(np.array([x], np.float64) for x in v)
    # nadir: no horizontal extent, the cell it stands in
    hit, t, _ = dn.walk(dsm, *one(1.2, 2.4, 1.2, 2.4), -2.0, 6.0)
    assert hit[0] and t[0] == 6.0 / 8.0
    hit, t, _ = dn.walk(dsm, *one(3.6, 2.4, 3.6, 2.4), -2.0, 6.0)
    assert hit[0] and t[0] == 4.0 / 8.0
    hit, t, _ = dn.walk(dsm, *one(3.6, 2.4, 3.6, 2.4), 3.0, 6.0)          # the surface lies below alt_lo
    assert not hit[0] and np.isnan(t[0])
    hit, t, _ = dn.walk(dsm, *one(7.0, 2.4, 7.0, 2.4), -2.0, 6.0)         # outside the grid
    assert not hit[0]
    # along a row from x = 0.5 to x = 4.5, from 4 m down to 0 m: z = 4 − (x − 0.5); steps at x = 1, 2 (excess 3.5, 2.5) and
    # x = 3 (height 2, z 1.5: excess −0.5): the crossing 2.5 / 3 of the way from x = 2 to x = 3
    hit, t, _ = dn.walk(dsm, *one(0.5, 2.0, 4.5, 2.0), 0.0, 4.0)
    assert hit[0] and abs(t[0] - (1.5 + 2.5 / 3.0) / 4.0) < 1e-15
    # the same, the other way along a column of the transposed step, and with a NaN column in between: transparent
    hit, t2, _ = dn.walk(dsm.T.copy(), *one(2.0, 0.5, 2.0, 4.5), 0.0, 4.0)
    assert hit[0] and t2[0] == t[0]
    holed = dsm.copy()
    holed[:, 2] = np.nan
    hit, t, _ = dn.walk(holed, *one(0.5, 2.0, 4.5, 2.0), 0.0, 4.0)        # between x = 1 (3.5) and x = 3 (−0.5)
    assert hit[0] and abs(t[0] - (0.5 + 2.0 * 3.5 / 4.0) / 4.0) < 1e-15
    holed[:, 2] = np.inf
    assert dn.walk(holed, *one(0.5, 2.0, 4.5, 2.0), 0.0, 4.0)[1][0] == t[0]
    # the floor met after the last centre line inside the segment: from x = 0.2 to x = 1.9, 1 m down to −0.5 m; the step at
    # x = 1 has excess 0.294, the one beyond the end at x = 2 excess −0.588: the crossing lies inside, at z = 0
    hit, t, _ = dn.walk(dsm, *one(0.2, 2.0, 1.9, 2.0), -0.5, 1.0)
    assert hit[0] and abs(t[0] - 1.0 / 1.5) < 1e-15
    hit, t, _ = dn.walk(dsm, *one(0.2, 2.0, 1.9, 2.0), 0.25, 1.0)         # alt_lo above the floor: reached first
    assert not hit[0]
    hit, t, _ = dn.walk(dsm, *one(1.2, 2.0, 1.9, 2.0), -0.5, 1.0)         # no centre line inside the segment: one step, a miss
    assert not hit[0]
    # the very first step already below the surface: placed at that step
    hit, t, _ = dn.walk(dsm, *one(2.5, 2.0, 4.5, 2.0), 0.0, 1.0)
    assert hit[0] and t[0] == 0.25


def test_sample_reads_the_raster_at_the_cells():
    w = dc.weight((33, 65))
    cell = np.array([[0.0, 0.0], [64.0, 32.0], [3.4, 7.6], [3.5, 7.5], [np.nan, 1.0], [64.5, 2.0], [10.25, 20.75]], np.float32)
    near = dn.sample(w, cell, 0)
    assert near.tobytes() == np.array([w[0, 0], w[32, 64], w[8, 3], w[8, 4], np.nan, np.nan, w[21, 10]], np.float32).tobytes()
    ones = np.ones((33, 65), np.float32)
    lin = dn.sample(ones, cell, 1)
    assert np.array_equal(np.isnan(lin), [False, False, False, False, True, True, False]) and bool((lin[~np.isnan(lin)] == 1.0).all())
    ramp = (np.arange(65, dtype=np.float32)[None, :] * 0.5 + np.arange(33, dtype=np.float32)[:, None] * 2.0)
    assert dn.sample(ramp, cell, 1)[6] == np.float32(10.25 * 0.5 + 20.75 * 2.0)
    holed = ramp.copy()
    holed[20, 10] = np.nan                                                  # the other three, renormalised
    v = dn.sample(holed, cell, 1)[6]
    assert np.isfinite(v) and v != np.float32(10.25 * 0.5 + 20.75 * 2.0)
    holed[20:22, 10:12] = np.inf
    assert np.isnan(dn.sample(holed, cell, 1)[6])


def test_ecef_inverts_to_the_ground_point():
    case, out = dc.BY_NAME["south"], dc.ref("south")
    hit = out["hit"] == 1
    p = dn.ecef(out["ground"][hit], out["altitude"][hit], case.grid)
    # against the near end lifted along the line of sight: ‖p − near‖ is the depth, up to the projection's scale factor
    s = out["seg"]
    near = np.stack(rpc_ref.geodetic_to_ecef(s["lat_hi"][hit], s["lon_hi"][hit], np.full(int(hit.sum()), case.alt_hi)), -1)
    d = np.linalg.norm(p - near, axis=1)
    assert float(np.abs(d - out["depth"][hit]).max()) <= 4e-4 * float(out["depth"][hit].max()) + 1e-5
