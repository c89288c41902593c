"""The numpy statement of the occlusion exports (tests/occlusion_numpy.py) on its own — no GPU needed: the
floor against a per-cell walk and against ``shadow_numpy.cast``'s excess, closed forms, the gate's boundary
cases, and the box scene of tests/occlusion_cases.py, where a building hides strips of ground from the
four shipped cameras.

Measured on the box scene (the statement, 2026-10-21): the strip holds 524 ground cells; over it the mean
raw score at the ground plane is 0.9776 with the gate and 0.7573 without, and the ground plane is picked at
480 cells with the gate and at 284 without.  On flat ground the floor lies rho = resolution·u/|a| below
the terrain (2.4, 2.8, 6.5 and 1.4 m for the four cameras), so the planes more than that below z0 are gated
for that view at every cell: no cell of the scene has a window that is ungated at all nine planes, and the
equality away from the gate is asserted per (plane, cell) — 12 730 of them — which contains the per-cell form.
"""
import numpy as np
import pytest

import occlusion_cases as occ
import occlusion_numpy as oc
import shadow_numpy as sn
import sweep_cases as sc


@pytest.mark.parametrize("shape", occ.FLOOR_SHAPES)
def test_the_floor_statement_equals_a_walk_of_every_cell(shape):
    dsm, ref = occ.heights(shape), occ.ref_floor64(shape)
    H, W = shape
    g = np.random.default_rng(H * W)
    cells = [(j, i) for j in range(H) for i in range(W)]
    if len(cells) > 120:
        cells = [cells[k] for k in g.choice(len(cells), 120, replace=False)] + [(0, 0), (H - 1, W - 1), (0, W - 1), (H - 1, 0)]
    for v, d in enumerate(occ.dirs()):
        for j, i in cells:
            want = oc.floor_cell(dsm, occ.RESOLUTION, d, j, i)
            assert ref[v, j, i] == want, (v, j, i, ref[v, j, i], want)
    assert not np.isnan(ref).any() and not (ref == np.inf).any()
    assert (ref[3] == -np.inf).all()                                     # the vertical direction
    if H * W > 64:
        assert np.isnan(dsm).any() and np.isfinite(ref[:, np.isnan(dsm)]).any()   # a NaN cell still gets a floor


@pytest.mark.parametrize("shape", occ.FLOOR_SHAPES)
def test_the_floor_is_the_height_plus_the_casts_excess(shape):
    """excess = max((height_m − h) − m·rho) and floor = max(height_m − m·rho) visit the same steps, so where h
    is finite they differ by h up to the roundings of h: within ``shadow_numpy.tolerance``."""
    dsm, ref = occ.heights(shape), occ.ref_floor64(shape)
    _, excess = sn.cast(dsm, occ.RESOLUTION, occ.dirs())
    tol = sn.tolerance(dsm)
    known = ~np.isnan(dsm)
    for v in range(ref.shape[0]):
        f, e = ref[v][known], excess[v][known]
        assert np.array_equal(f == -np.inf, e == -np.inf)
        some = np.isfinite(f)
        err = np.abs(f[some] - (dsm[known][some] + e[some]))
        print(f"{shape} direction {v}: {int(some.sum())} finite floors, worst |floor - (h + excess)| {float(err.max()) if err.size else 0.0:.3e} m of {tol:.3e}")
        assert bool((err <= tol).all())


def test_closed_forms():
    H, W, c, wall, res = 5, 12, 8, 6.0, 0.5
    east = np.array([0.5, 0.0, 0.5], np.float32)                         # due east: q = 0, rho = res·u/|a| = 0.5, all dyadic
    rho = 0.5
    # one wall and nothing else: exactly Hw − (c − i)·rho west of it and −inf east of it (its own column included)
    lone = np.full((H, W), np.nan)
    lone[:, c] = wall
    f = oc.floor_one(lone, res, east)
    assert all((f[:, i] == wall - (c - i) * rho).all() for i in range(c)) and (f[:, c:] == -np.inf).all()
    assert oc.floor_cell(lone, res, east, 2, 3) == wall - 5 * rho
    # the same wall on ground at 0: the ground one step east stands at −rho, and nothing stands east of the last column
    dsm = np.zeros((H, W))
    dsm[:, c] = wall
    f = oc.floor_one(dsm, res, east)
    for i in range(W):
        want = max(wall - (c - i) * rho, -rho) if i < c else (-rho if i < W - 1 else -np.inf)
        assert (f[:, i] == want).all(), (i, f[0, i], want)
    # due west the wall shades the other side
    f = oc.floor_one(lone, res, -east * np.array([1, 1, -1], np.float32))
    assert all((f[:, i] == wall - (i - c) * rho).all() for i in range(c + 1, W)) and (f[:, :c + 1] == -np.inf).all()
    # vertical: no step
    assert (oc.floor(dsm, res, [[0.0, 0.0, 1.0]]) == -np.inf).all()
    # a NaN block of the prior: its cells get a floor, and as steps they contribute nothing
    holed = np.zeros((H, W))
    holed[1:4, 2:5] = np.nan
    f = oc.floor_one(holed, res, east)
    assert (f[0, :W - 1] == -rho).all() and (f[:, W - 1] == -np.inf).all()
    assert f[2, 1] == -4 * rho and f[2, 3] == -2 * rho and f[2, 4] == -rho    # row 2: the first height east of column 1 is 4 steps away
    assert oc.floor_cell(holed, res, east, 2, 1) == -4 * rho
    # the result is cast once
    assert oc.floor(dsm, res, [east]).dtype == np.float32


def test_the_gate_is_strict_and_ignores_nan():
    alt, slack = -12.0, 0.5
    on = np.float32(alt + slack)
    floor = np.array([[[on, np.nextafter(on, np.float32(np.inf)), np.nextafter(on, np.float32(-np.inf)), np.nan, np.inf, -np.inf]]], np.float32)
    assert oc.gated(floor, alt, slack).tolist() == [[[False, True, False, False, True, False]]]
    grey = np.full((1, 1, 6), 0.25, np.float32)
    valid = np.array([[[1, 1, 1, 1, 1, 0]]], np.uint8)
    g, ok = oc.gate(grey, valid, floor, alt, slack)
    assert ok.tolist() == [[[1, 0, 1, 1, 0, 0]]] and np.isnan(g[0, 0, [1, 4]]).all() and (g[0, 0, [0, 2, 3, 5]] == 0.25).all()
    assert grey[0, 0, 1] == 0.25 and valid[0, 0, 1] == 1                 # a new pair
    # the sum is rounded once in fp64 before the comparison: 2^53 + 1 is not a double
    assert not oc.gated(np.array([[[2.0 ** 53]]], np.float32), 2.0 ** 53, 1.0).any()


def test_the_box_hides_a_strip_that_the_gate_recovers():
    gated, plain = occ.box_sweeps()
    strip, G, r = occ.strip(), occ.GROUND_PLANE, occ.BOX.radius
    n = int(strip.sum())
    mean_g, mean_p = float(np.mean(gated["volume"][G][strip])), float(np.mean(plain["volume"][G][strip]))
    hit_g, hit_p = int((gated["index"][strip] == G).sum()), int((plain["index"][strip] == G).sum())
    print(f"strip {n} cells; mean raw score at the ground plane {mean_g:.4f} gated, {mean_p:.4f} ungated; "
          f"ground plane picked at {hit_g} cells gated, {hit_p} ungated")
    assert n >= 100
    assert not np.isnan(gated["volume"][G][strip]).any() and not np.isnan(plain["volume"][G][strip]).any()
    assert mean_g > mean_p
    assert hit_g >= hit_p
    # away from the gate the statement is the ungated one, byte for byte
    touched = oc.in_window(gated["gated"], r).any(1)                     # (K, H, W)
    free = ~touched
    assert free.sum() > 1000
    assert gated["volume"][free].tobytes() == plain["volume"][free].tobytes()
    assert np.array_equal(gated["views_vol"][free], plain["views_vol"][free])
    whole = free.all(0)                                                  # cells ungated at every plane (none on this scene)
    for k in ("altitude", "score", "index", "views"):
        assert gated[k][whole].tobytes() == plain[k][whole].tobytes(), k
    # the gate only ever takes views away
    assert (gated["views_vol"] <= plain["views_vol"]).all()
    # a floor that gates nothing gives the ungated statement
    s = occ.BOX
    same = oc.sweep(occ.box_images(), sc.ref_cameras(s), s.grid, s.alt_lo, s.step, 2, np.full((4,) + s.grid.shape, -np.inf, np.float32), 0.0,
                    s.radius, s.min_views)
    assert same["volume"].tobytes() == plain["volume"][:2].tobytes() and not same["gated"].any()
