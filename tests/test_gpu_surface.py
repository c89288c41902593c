"""The surface sweep on the GPU (csrc/surface.hip, spnerf_amd.surface) — needs an MI355X.

Every step is held to the fp64 numpy statement (tests/surface_numpy.py, itself pinned on the CPU by
tests/test_surface_ref.py) on the cases of tests/surface_cases.py and tests/sweep_cases.py:

* ``surface_grey``: the bound tests/test_gpu_sweep.py asserts for ``plane_grey`` — ``valid`` equal wherever the
  reference pix lies more than PIX_TOL from a border, |Δgrey| <= 2·PIX_TOL·(largest neighbour difference of the
  image) — and every view invalid where the base is not finite;
* ``upsample_dsm`` and ``surface_lift``: the statement's bytes;
* the fused ``surface_sweep`` against its own staged path (``surface_grey``, ``window_score`` per surface,
  ``pick_plane(off_lo)``, ``surface_lift``): all four planes and the volume bit-equal, on grids that straddle one
  and two tile edges, every radius, a view count per kernel instance and boundary, bases with NaN and ±inf cells,
  a NaN block larger than a tile and its halo, and all NaN; with a constant dyadic base ``plane_sweep``'s bytes;
* the fused call against the statement end to end on ``tilt`` and ``real``: ``index`` equal except at near-tie
  cells, |Δscore| and |Δaltitude| / step within the bounds tests/test_gpu_sweep.py asserts for the plane sweep;
* ``pyramid_sweep``: the bytes of the statement chain applied to the device's own volumes;
* ``plane_sweep``, ``visible_sweep`` and ``smooth_sweep`` return the same bytes before and after surface calls.

Measured on MI355X (2026-10-21), worst over "tilt" around the truth and around truth + 2 m: |score − statement| 5.96e-8,
|altitude − statement| / step 1.907e-6, no index differs and there is no near tie.
"""
import functools

import numpy as np
import pytest
import torch

import rectify_cases as rc
import sgm_numpy as sg
import surface_cases as fc
import surface_numpy as sn
import sweep_cases as sc
import sweep_numpy as sw
from spnerf_amd import plane_sweep, pyramid_sweep, smooth_sweep, surface, surface_sweep, sweep, visible_sweep
from test_gpu_parity import DEV
from test_gpu_sweep import ALTITUDE_TOL, SCORE_TOL

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def device_images(name):
    return tuple(torch.tensor(im, device=DEV) for im in fc.images(name))


def dev(a):
    return torch.tensor(np.asarray(a), device=DEV)


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def centre(scene):
    return scene.alt_lo + 0.5 * (scene.planes - 1) * scene.step


@pytest.mark.parametrize("name,kind", [("ramp", "holes"), ("noise", "smooth"), ("real", "holes")])
def test_surface_grey_matches_the_numpy_statement(name, kind):
    scene = sc.BY_NAME[name]
    imgs = sc.images(name)
    base = fc.base(scene.grid.shape, kind, centre(scene))
    worst = 0.0
    for offset in (-1.5, 2.0):
        grey, valid = surface.surface_grey(list(device_images(name)), sc.cameras(scene), scene.grid, dev(base), offset)
        assert grey.dtype == torch.float32 and valid.dtype == torch.uint8 and tuple(grey.shape) == tuple(valid.shape) == (len(imgs),) + scene.grid.shape
        grey, valid = grey.cpu().numpy(), valid.cpu().numpy()
        pix = sn.pix_on(scene.grid, sc.ref_cameras(scene), base, offset)
        ref_grey, ref_valid = sw.grey_at(imgs, pix)
        clear = ~(sc.border_distance(pix, imgs) <= rc.PIX_TOL)
        assert np.array_equal(valid[clear], ref_valid[clear]) and set(np.unique(valid).tolist()) <= {0, 1}
        assert np.array_equal(np.isnan(grey), valid == 0)
        assert not valid[:, ~np.isfinite(base)].any() and valid.any()
        for v, im in enumerate(imgs):
            both = (valid[v] == 1) & (ref_valid[v] == 1)
            tol = 2 * rc.PIX_TOL * rc.neighbour_difference(im)
            err = np.abs(grey[v][both].astype(np.float64) - ref_grey[v][both].astype(np.float64))
            worst = max(worst, float(err.max()) / tol if err.size else 0.0)
            assert bool((err <= tol).all())
    print(f"{name}: worst share of the bound {worst:.4f}")


@pytest.mark.parametrize("f,shape", [(1, (7, 9)), (2, (7, 9)), (3, (7, 9)), (4, (7, 9)), (2, (33, 65)), (3, (33, 65)), (4, (64, 128)), (8, (33, 65)),
                                     (5, (1, 1)), (2, (1, 7)), (7, (7, 1)), (4, (512, 512))])
def test_upsample_dsm_has_the_statements_bytes(f, shape):
    hc, wc = -(-shape[0] // f), -(-shape[1] // f)
    g = np.random.default_rng(10 * f + shape[0])
    coarse = (g.standard_normal((hc, wc)) * 20.0).astype(np.float32)
    for kind in ("finite", "holes", "nan"):
        c = coarse.copy()
        if kind == "holes":
            u = g.random((hc, wc))
            c[u < 0.2] = np.nan
            c[(u >= 0.2) & (u < 0.25)] = np.inf
            c[(u >= 0.25) & (u < 0.3)] = -np.inf
            c[: hc // 2 + 1, : wc // 3 + 1] = np.nan
        elif kind == "nan":
            c[:] = np.nan
        out = surface.upsample_dsm(dev(c), f, shape)
        assert out.dtype == torch.float32 and tuple(out.shape) == shape
        assert same(out.cpu().numpy(), sn.upsample(c, f, shape)), kind


@pytest.mark.parametrize("shape", [(1, 1), (7, 9), (33, 65), (300, 301)])
def test_surface_lift_has_the_statements_bytes(shape):
    g = np.random.default_rng(shape[1])
    base = (g.standard_normal(shape) * 30.0).astype(np.float32)
    rel = (g.standard_normal(shape) * 3.0).astype(np.float32)
    if base.size > 8:
        base.ravel()[[1, 3]], rel.ravel()[[3, 5]] = (np.nan, np.inf), (1.0, np.nan)
        base.ravel()[6], rel.ravel()[6] = 16777216.0, 1.0
    out = surface.surface_lift(dev(base), dev(rel))
    assert out.dtype == torch.float32 and same(out.cpu().numpy(), sn.lift(base, rel))


def staged(imgs, cams, grid, base, off_lo, step, K, **kw):
    volume, views = [], []
    for k in range(K):
        grey, valid = surface.surface_grey(imgs, cams, grid, base, off_lo + float(k) * step)
        s, m = sweep.window_score(grey, valid, **kw)
        volume.append(s)
        views.append(m)
    out = sweep.pick_plane(torch.stack(volume), torch.stack(views), off_lo, step)
    out["altitude"] = surface.surface_lift(base, out["altitude"])
    out["volume"] = torch.stack(volume)
    return out


VIEW_COUNTS = (2, 4, 5, 9, 16)          # k_sweep<4>: 2, 4; k_sweep<8>: 5; k_sweep<16>: 9, 16


@pytest.mark.parametrize("shape", sc.SCORE_GRIDS)
@pytest.mark.parametrize("K", [1, 2, 3, 9])
def test_the_fused_surface_sweep_has_the_bytes_of_its_staged_path(shape, K):
    scene = sc.BY_NAME["real"]
    n = sc.SCORE_GRIDS.index(shape) + K
    grid, radius, V, kind = sc._jax(shape), (1, 2, 4)[(K + shape[0]) % 3], VIEW_COUNTS[n % 5], fc.BASES[n % 4]
    order = [k % 4 for k in range(V)]
    imgs, cams = [device_images("real")[k] for k in order], [sc.cameras(scene)[k] for k in order]
    kw = dict(radius=radius, min_views=min(2 + K % 2, V), min_std=0.0 if K != 3 else 0.01)
    base_host = fc.base(shape, kind, -16.0)
    base, off_lo, step = dev(base_host), -float(K - 1), 2.0
    want = host(staged(imgs, cams, grid, base, off_lo, step, K, **kw))
    out = surface_sweep(imgs, cams, grid, base, off_lo, step, K, volume=True, **kw)
    assert sorted(out) == ["altitude", "index", "score", "views", "volume"]
    assert out["altitude"].dtype == out["score"].dtype == out["volume"].dtype == torch.float32
    assert out["index"].dtype == torch.int32 and out["views"].dtype == torch.uint8 and tuple(out["volume"].shape) == (K,) + shape
    out = host(out)
    print(f"{shape} K {K} V {V} r {radius} base {kind}: {int((want['index'] >= 0).sum())} of {want['index'].size} cells with an index")
    for k in want:
        assert same(out[k], want[k]), k
    bad = ~np.isfinite(base_host)
    assert (out["index"][bad] == -1).all() and np.isnan(out["altitude"][bad]).all() and np.isnan(out["volume"][:, bad]).all()
    if kind == "nan":
        assert (out["index"] == -1).all() and np.isnan(out["altitude"]).all() and (out["views"] == 0).all()
    elif shape[0] * shape[1] > 64 and kind == "smooth":
        assert (out["index"] >= 0).any()
    bare = host(surface_sweep(imgs, cams, grid, base, off_lo, step, K, **kw))           # without the volume, and a second run
    assert sorted(bare) == ["altitude", "index", "score", "views"]
    for k in bare:
        assert same(bare[k], want[k]), k
    assert same(base.cpu().numpy(), base_host)                            # the base is left alone


@pytest.mark.parametrize("kind,radius,V", [("block", 4, 4), ("block", 2, 16), ("holes", 1, 5), ("nan", 4, 9)])
def test_the_fused_surface_sweep_over_holes_blocks_and_all_nan(kind, radius, V):
    scene, shape, K = sc.BY_NAME["real"], (33, 65), 3
    order = [k % 4 for k in range(V)]
    imgs, cams = [device_images("real")[k] for k in order], [sc.cameras(scene)[k] for k in order]
    base_host = fc.base(shape, kind, -16.0)
    base = dev(base_host)
    kw = dict(radius=radius, min_views=2)
    want = host(staged(imgs, cams, scene.grid, base, -2.0, 2.0, K, **kw))
    out = host(surface_sweep(imgs, cams, scene.grid, base, -2.0, 2.0, K, volume=True, **kw))
    for k in want:
        assert same(out[k], want[k]), k
    bad = ~np.isfinite(base_host)
    assert (out["index"][bad] == -1).all() and ((out["index"] >= 0).any() or kind == "nan")
    if kind == "block":
        assert bad[2:28, 3:31].all() and (out["index"][2:28, 3:31] == -1).all()


@pytest.mark.parametrize("c,V,radius", [(-20.0, 4, 2), (-17.5, 5, 4), (0.0, 16, 1)])
def test_a_constant_dyadic_base_gives_the_plane_sweeps_bytes(c, V, radius):
    scene, K = sc.BY_NAME["real"], 5
    order = [k % 4 for k in range(V)]
    imgs, cams = [device_images("real")[k] for k in order], [sc.cameras(scene)[k] for k in order]
    off_lo = -24.0 - c
    want = host(plane_sweep(imgs, cams, scene.grid, -24.0, 2.0, K, radius=radius, volume=True))
    out = host(surface_sweep(imgs, cams, scene.grid, torch.full(scene.grid.shape, c, device=DEV), off_lo, 2.0, K, radius=radius, volume=True))
    for k in ("volume", "index", "score", "views"):
        assert same(out[k], want[k]), k
    some = want["index"] >= 0
    assert some.any() and np.array_equal(np.isnan(out["altitude"]), ~some)
    if c == 0.0:
        assert same(out["altitude"], want["altitude"])                    # the lift of a zero base changes nothing
    else:                                                                 # one more fp32 rounding (tests/test_surface_ref.py)
        assert bool((np.abs(out["altitude"][some].astype(np.float64) - want["altitude"][some]) <= 1.5 * 2.0 ** -19).all())


@functools.lru_cache(maxsize=None)
def real_reference():
    s = sc.BY_NAME["real"]
    base = fc.base(s.grid.shape, "smooth", -16.0)
    out = sn.sweep(sc.images("real"), sc.ref_cameras(s), s.grid, base, -8.0, 2.0, 9, s.radius, s.min_views)
    out["base"] = base
    return out


@pytest.mark.parametrize("name", ["tilt", "tilt+2", "real"])
def test_the_fused_surface_sweep_matches_the_numpy_statement(name):
    if name == "real":
        scene, ref, off_lo, step = sc.BY_NAME["real"], real_reference(), -8.0, 2.0
    else:
        scene, ref, off_lo, step = fc.TILT, fc.ref_tilt(2.0 if name == "tilt+2" else 0.0), fc.TILT.alt_lo, fc.TILT.step
    out = host(surface_sweep(list(device_images(scene.name)), sc.cameras(scene), scene.grid, dev(ref["base"]), off_lo, step, 9,
                             radius=scene.radius, min_views=scene.min_views, volume=True))
    some = ref["index"] >= 0
    ties = sc.near_tie(ref["volume"])
    differ = out["index"] != ref["index"]
    agree = some & ~differ
    d_score = np.abs(out["score"][agree].astype(np.float64) - ref["score"][agree].astype(np.float64))
    d_alt = np.abs(out["altitude"][agree].astype(np.float64) - ref["altitude"][agree].astype(np.float64)) / step
    print(f"{name}: {int(some.sum())} cells with an index, {int(ties.sum())} near ties, {int(differ.sum())} indices differ; "
          f"worst |score - statement| {float(d_score.max()):.3e}, worst |altitude - statement| / step {float(d_alt.max()):.3e}")
    assert some.sum() > 0.5 * some.size
    assert not (differ & ~ties).any()
    assert np.array_equal(np.isnan(out["volume"]), np.isnan(ref["volume"]))
    assert np.array_equal(out["views"][agree], ref["views"][agree])
    assert bool((d_score <= SCORE_TOL).all()) and bool((d_alt <= ALTITUDE_TOL).all())
    if name != "real":
        four = out["views"] == 4
        assert four.sum() >= 0.5 * four.size and bool((out["index"][four] == (2 if name == "tilt+2" else 4)).all())


@pytest.mark.parametrize("shape,factors", [((33, 65), (2,)), ((17, 33), (4, 2)), ((33, 65), (4, 2))])
def test_pyramid_sweep_is_the_statement_chain_on_the_devices_own_volumes(shape, factors):
    s = sc.BY_NAME["real"]
    grid = sc._jax(shape)
    imgs, cams = list(device_images("real")), sc.cameras(s)
    planes, step, reach, p1, p2 = 8, 2.0, 1, 0.125, 0.75
    kw = dict(radius=2, min_views=2)
    out = pyramid_sweep(imgs, cams, grid, -24.0, step, planes, factors=factors, reach=reach, p1=p1, p2=p2, **kw)
    assert sorted(out) == ["altitude", "base", "index", "photo", "score"]
    assert all(tuple(v.shape) == shape for v in out.values())
    out = host(out)
    plan = sn.level_plan(factors, planes, reach)
    f0, m0, K0 = plan[0]
    raw = plane_sweep(imgs, cams, surface.coarsen(grid, f0), -24.0, step * m0, K0, volume=True, **kw)["volume"].cpu().numpy()
    level = sg.pick(sg.aggregate(raw, p1, p2), raw, -24.0, step * m0)
    f_prev = f0
    for f, m, K in plan[1:]:
        g = surface.coarsen(grid, f)
        base = sn.upsample(level["altitude"], f_prev // f, g.shape)
        off_lo = -(K // 2) * (step * m)
        raw = surface_sweep(imgs, cams, g, dev(base), off_lo, step * m, K, volume=True, **kw)["volume"].cpu().numpy()
        level = sn.later_level(raw, base, off_lo, step * m, p1, p2)
        f_prev = f
    print(f"{shape} {factors}: {int((level['index'] >= 0).sum())} of {level['index'].size} cells with an index, "
          f"{int(np.isnan(level['base']).sum())} without a base")
    assert (level["index"] >= 0).any()
    for k in level:
        assert same(out[k], level[k]), k
    assert np.isnan(out["altitude"][np.isnan(out["base"])]).all()


def test_the_older_sweeps_are_untouched_by_surface_calls():
    s = sc.BY_NAME["real"]
    imgs, cams = list(device_images("real")), sc.cameras(s)
    kw = dict(radius=s.radius, min_views=s.min_views)
    floor = torch.full((4,) + s.grid.shape, -np.inf, device=DEV)
    floor[1, 5:20, 10:40], floor[3, 10:30, 30:60] = -15.0, -19.0

    def older():
        return (host(plane_sweep(imgs, cams, s.grid, s.alt_lo, s.step, s.planes, volume=True, **kw)),
                host(visible_sweep(imgs, cams, s.grid, s.alt_lo, s.step, s.planes, floor, slack=0.0, volume=True, **kw)),
                host(smooth_sweep(imgs, cams, s.grid, s.alt_lo, s.step, s.planes, **kw)))

    before = older()
    base = dev(fc.base(s.grid.shape, "holes", -16.0))
    surface_sweep(imgs, cams, s.grid, base, -4.0, 2.0, 5, volume=True, radius=4)
    surface.surface_grey(imgs, cams, s.grid, base, 1.0)
    pyramid_sweep(imgs, cams, s.grid, s.alt_lo, s.step, s.planes, factors=(2,), reach=1)
    after = older()
    for b, a in zip(before, after):
        assert sorted(a) == sorted(b)
        for k in b:
            assert same(a[k], b[k]), k
    assert not same(before[0]["volume"], before[1]["volume"])              # the gate did take views out
