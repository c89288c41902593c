"""The occlusion exports on the GPU (csrc/occlusion.hip, spnerf_amd.occlusion) — needs an MI355X.

Everything is held to the fp64 numpy statement (tests/occlusion_numpy.py, itself pinned to known answers on
the CPU by tests/test_occlusion_ref.py) on the cases of tests/occlusion_cases.py:

* ``visibility_floor``: −inf where the statement has it and nowhere else, no NaN, and elsewhere between the
  fp32 casts of the statement's fp64 floor ∓ ``shadow_numpy.tolerance`` — the march is the cast's, so its
  bound is the cast's, and the one cast to fp32 is monotone; on MI355X (2026-10-21) no entry of any grid differs
  from the statement's cast, so the bytes are asserted equal as well;
* ``gate_plane``: the statement's bytes, the inputs untouched;
* ``visible_sweep`` against its own staged chain ``plane_grey`` → ``gate_plane`` → ``window_score`` per plane
  → ``pick_plane``: all four planes and the volume bit-equal, on grids that are no multiple of the 16-cell
  tile, for floors of −inf (then also ``plane_sweep``'s bytes), of +inf (index −1, NaN, 0 views) and seeded
  ones, constant on 8 x 8 blocks so that windows survive, that straddle the planes, lie exactly on
  ``alt_k + slack``, hold NaN and ±inf, and gate one view over more than a tile and its halo;
* ``box``, ``real`` (the floor of the lidar raster cropped to its grid: flat ground at −28 m, below the −24 m
  of the lowest plane, so it gates nothing there) and ``city`` (the same pixels under the floor of a seeded
  box city) end to end against the statement, with the bounds tests/test_gpu_sweep.py asserts for
  the ungated sweep (the gate adds no arithmetic to the score);
* ``refine_sweep``: the statement chain applied to the device's own volume, as ``smooth_sweep`` is tested;
* ``plane_sweep`` and ``cast_shadows`` return the same bytes before and after gated calls.
"""
import functools
import os

import numpy as np
import pytest
import torch

import occlusion_cases as occ
import occlusion_numpy as oc
import rectify_numpy as rn
import sgm_numpy as sg
import shadow_cases as shc
import shadow_numpy as sn
import sweep_cases as sc
from spnerf_amd import cast_shadows, gate_plane, plane_sweep, rectify, refine_sweep, sweep, visibility_floor, visible_sweep
from test_gpu_parity import DEV
from test_gpu_sweep import ALTITUDE_TOL, SCORE_TOL, device_images, host, same

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", occ.FLOOR_SHAPES)
def test_visibility_floor_matches_the_numpy_statement(shape):
    dsm, ref = occ.heights(shape), occ.ref_floor64(shape)
    d = torch.tensor(dsm, device=DEV)
    got = visibility_floor(d, occ.RESOLUTION, occ.dirs())
    assert got.dtype == torch.float32 and tuple(got.shape) == (11,) + shape and got.device == d.device
    got = got.cpu().numpy()
    tol = sn.tolerance(dsm)
    assert not np.isnan(got).any() and not (got == np.inf).any()
    assert np.array_equal(got == -np.inf, ref == -np.inf)
    some = np.isfinite(ref)
    lo, hi = (ref[some] - tol).astype(np.float32), (ref[some] + tol).astype(np.float32)   # the cast is monotone
    differ = int((got != ref.astype(np.float32)).sum())
    err = np.abs(got[some].astype(np.float64) - ref[some])
    print(f"{shape}: tolerance {tol:.3e} m; {differ} of {got.size} fp32 entries differ from the statement's cast; "
          f"worst |floor - statement's fp64| {float(err.max()) if err.size else 0.0:.3e} m; -inf {int((ref == -np.inf).sum())}")
    assert bool(((got[some] >= lo) & (got[some] <= hi)).all())
    assert same(got, ref.astype(np.float32))                             # measured on MI355X: the bytes are equal, so that is asserted
    # twice the same bytes; a float32 DSM is its widened copy; a GroundGrid gives its resolution; directions from the device
    again = visibility_floor(d, occ.RESOLUTION, torch.tensor(occ.dirs(), device=DEV))
    assert same(again.cpu().numpy(), got)
    low = d.float()
    assert torch.equal(visibility_floor(low, occ.RESOLUTION, occ.dirs()), visibility_floor(low.double(), occ.RESOLUTION, occ.dirs()))
    grid = sc._jax(shape)
    assert same(visibility_floor(d, grid, occ.dirs()[4:6]).cpu().numpy(), got[4:6])


@pytest.mark.parametrize("V,shape", [(1, (1, 1)), (3, (17, 33)), (16, (33, 65))])
def test_gate_plane_has_the_statements_bytes(V, shape):
    grey, valid = sc.stored(max(V, 2), shape)
    grey, valid = grey[:V], valid[:V]
    alt, slack = -12.0, 0.5
    floor = occ.seeded_floor(V, shape, -16.0, 1.0, 9, slack)
    floor.flat[0] = np.float32(alt + slack)                              # exactly on the boundary: not gated
    want_grey, want_valid = oc.gate(grey, valid, floor, alt, slack)
    g, v, f = torch.tensor(grey, device=DEV), torch.tensor(valid, device=DEV), torch.tensor(floor, device=DEV)
    got_grey, got_valid = gate_plane(g, v, f, alt, slack=slack)
    assert got_grey.dtype == torch.float32 and got_valid.dtype == torch.uint8
    assert same(got_grey.cpu().numpy(), want_grey) and same(got_valid.cpu().numpy(), want_valid)
    assert same(g.cpu().numpy(), grey) and same(v.cpu().numpy(), valid)  # a new pair
    assert want_valid.flat[0] == valid.flat[0] and (shape == (1, 1) or (want_valid != valid).any())
    zero = gate_plane(g, v, f, alt)                                      # slack defaults to 0
    assert same(zero[1].cpu().numpy(), oc.gate(grey, valid, floor, alt, 0.0)[1])


def staged(imgs, cams, grid, alt_lo, step, K, floor, slack, **kw):
    volume, views = [], []
    for k in range(K):
        alt = alt_lo + float(k) * step
        grey, valid = sweep.plane_grey(imgs, cams, grid, alt)
        grey, valid = gate_plane(grey, valid, floor, alt, slack=slack)
        s, m = sweep.window_score(grey, valid, **kw)
        volume.append(s)
        views.append(m)
    out = sweep.pick_plane(torch.stack(volume), torch.stack(views), alt_lo, step)
    out["volume"] = torch.stack(volume)
    return out


FUSED_CASES = [((1, 1), 2, 1, 1), ((1, 1), 4, 4, 3), ((17, 33), 3, 2, 2), ((17, 33), 9, 4, 3), ((17, 33), 16, 1, 9), ((33, 65), 4, 2, 9),
               ((33, 65), 2, 4, 3), ((33, 65), 16, 4, 2), ((33, 65), 9, 1, 1), ((33, 65), 3, 4, 9)]


@pytest.mark.parametrize("shape,V,radius,K", FUSED_CASES)
def test_visible_sweep_has_the_bytes_of_its_staged_chain(shape, V, radius, K):
    scene = sc.BY_NAME["real"]
    grid, alt_lo, step, slack = sc._jax(shape), -24.0, 2.0, 0.5
    order = [k % len(scene.views) for k in range(V)]
    imgs, cams = [device_images("real")[k] for k in order], [sc.cameras(scene)[k] for k in order]
    kw = dict(radius=radius, min_views=2 + (K % 2 if V > 2 else 0), min_std=0.0 if K != 3 else 0.01)
    plain = host(plane_sweep(imgs, cams, grid, alt_lo, step, K, volume=True, **kw))

    def both(floor, slack):
        f = torch.tensor(floor, device=DEV)
        out = visible_sweep(imgs, cams, grid, alt_lo, step, K, f, slack=slack, volume=True, **kw)
        assert sorted(out) == ["altitude", "index", "score", "views", "volume"]
        assert out["altitude"].dtype == out["score"].dtype == out["volume"].dtype == torch.float32
        assert out["index"].dtype == torch.int32 and out["views"].dtype == torch.uint8 and tuple(out["volume"].shape) == (K,) + shape
        out, want = host(out), host(staged(imgs, cams, grid, alt_lo, step, K, f, slack, **kw))
        for k in want:
            assert same(out[k], want[k]), k
        bare = host(visible_sweep(imgs, cams, grid, alt_lo, step, K, f, slack=slack, **kw))   # without the volume, and a second run
        assert sorted(bare) == ["altitude", "index", "score", "views"]
        for k in bare:
            assert same(bare[k], want[k]), k
        return out

    # nothing gated: plane_sweep's bytes (−inf, and NaN)
    for fill in (-np.inf, np.nan):
        out = both(np.full((V,) + shape, fill, np.float32), 0.0)
        for k in plain:
            assert same(out[k], plain[k]), (fill, k)
    # everything gated
    out = both(np.full((V,) + shape, np.inf, np.float32), slack)
    assert (out["index"] == -1).all() and np.isnan(out["altitude"]).all() and np.isnan(out["score"]).all() and (out["views"] == 0).all()
    assert np.isnan(out["volume"]).all()
    # floors that straddle the planes
    floor = occ.seeded_floor(V, shape, alt_lo, step, K, slack)
    out = both(floor, slack)
    off = np.stack([oc.gated(floor, alt_lo + k * step, slack) for k in range(K)])
    print(f"{shape} V {V} r {radius} K {K}: {100 * off.mean():.1f} % of the (plane, view, cell) triples gated; "
          f"{int((out['index'] >= 0).sum())} of {out['index'].size} cells keep a plane, {int((out['index'] != plain['index']).sum())} indices change")
    if shape[0] * shape[1] > 64:
        assert off.any() and not off.all() and off[:, 0, :24, :24].all()
        if (plain["index"] >= 0).mean() > 0.5:                           # the gate takes views away without emptying the grid
            assert (out["index"] >= 0).any() and (out["views"] < plain["views"]).any()


@functools.lru_cache(maxsize=None)
def real_floor():
    """The statement's floor of the lidar raster cropped to the ``real`` scene's grid (the raster's first
    33 x 65 cells: same origin, same 0.5 m cells), under the four cameras' lines of sight."""
    s = sc.BY_NAME["real"]
    gt = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dsm_truth.npz"))["gt"].astype(np.float64)
    assert gt.shape == (512, 512) and s.grid.resolution == 0.5
    dsm = np.ascontiguousarray(gt[:s.grid.shape[0], :s.grid.shape[1]])
    dirs, _ = rn.view_directions(s.grid, sc.ref_cameras(s), s.alt_lo, s.alt_lo + (s.planes - 1) * s.step)
    return dsm, np.ascontiguousarray(dirs, np.float32), oc.floor(dsm, 0.5, dirs)


@functools.lru_cache(maxsize=None)
def city_floor():
    """The statement's floor of a seeded box city on the ``real`` scene's grid: ground at −28 m, as the lidar has
    it there, and six boxes of 6 to 14 cells a side, 8 to 22 m high, so that their roofs stand among the planes."""
    s = sc.BY_NAME["real"]
    H, W = s.grid.shape
    g = np.random.default_rng(269)
    dsm = np.full((H, W), -28.0)
    for _ in range(6):
        j0, i0 = int(g.integers(0, H - 6)), int(g.integers(0, W - 6))
        dsm[j0:j0 + int(g.integers(6, 15)), i0:i0 + int(g.integers(6, 15))] = -28.0 + g.uniform(8.0, 22.0)
    return oc.floor(dsm, 0.5, real_floor()[1])


def end_to_end(name):
    if name == "box":
        s, imgs, floor, slack = occ.BOX, occ.box_images(), occ.box_floor(), occ.SLACK
        ref = occ.box_sweeps()[0]
    else:
        s, imgs, slack = sc.BY_NAME["real"], sc.images("real"), 1.0
        floor = real_floor()[2] if name == "real" else city_floor()
        ref = oc.sweep(imgs, sc.ref_cameras(s), s.grid, s.alt_lo, s.step, s.planes, floor, slack, s.radius, s.min_views)
    return s, imgs, floor, slack, ref


@pytest.mark.parametrize("name", ["box", "real", "city"])
def test_visible_sweep_matches_the_numpy_statement(name):
    scene, imgs, floor, slack, ref = end_to_end(name)
    out = host(visible_sweep([torch.tensor(im, device=DEV) for im in imgs], sc.cameras(scene), scene.grid, scene.alt_lo, scene.step,
                             scene.planes, torch.tensor(floor, device=DEV), slack=slack, radius=scene.radius, min_views=scene.min_views,
                             volume=True))
    some = ref["index"] >= 0
    ties = sc.near_tie(ref["volume"])
    differ = out["index"] != ref["index"]
    agree = some & ~differ
    d_score = np.abs(out["score"][agree].astype(np.float64) - ref["score"][agree].astype(np.float64))
    d_alt = np.abs(out["altitude"][agree].astype(np.float64) - ref["altitude"][agree].astype(np.float64)) / scene.step
    d_vol = np.abs(out["volume"].astype(np.float64) - ref["volume"].astype(np.float64))
    print(f"{name}: {100 * ref['gated'].mean():.1f} % of the (plane, view, cell) triples gated; {int(some.sum())} cells with an index, "
          f"{int(ties.sum())} near ties, {int(differ.sum())} indices differ; worst |score - statement| {float(d_score.max()):.3e}, "
          f"worst |altitude - statement| / step {float(d_alt.max()):.3e}, worst over the volume {float(np.nanmax(d_vol)):.3e}")
    assert some.any() and (name == "real") != bool(ref["gated"].any())
    assert ties.sum() <= 0.01 * some.sum()
    assert not (differ & ~ties).any()
    assert np.array_equal(np.isnan(out["volume"]), np.isnan(ref["volume"]))
    assert np.array_equal(out["views"][agree], ref["views"][agree])
    assert bool((d_score <= SCORE_TOL).all()) and bool((d_alt <= ALTITUDE_TOL).all())
    if name == "box":                                                    # the strip of tests/test_occlusion_ref.py, on the device
        strip, G = occ.strip(), occ.GROUND_PLANE
        plain = host(plane_sweep([torch.tensor(im, device=DEV) for im in imgs], sc.cameras(scene), scene.grid, scene.alt_lo, scene.step,
                                 scene.planes, radius=scene.radius, min_views=scene.min_views, volume=True))
        assert float(out["volume"][G][strip].mean()) > float(plain["volume"][G][strip].mean())
        assert int((out["index"][strip] == G).sum()) >= int((plain["index"][strip] == G).sum())


@pytest.mark.parametrize("name,paths", [("box", 8), ("real", 4)])
def test_refine_sweep_is_the_statement_chain_on_the_devices_own_volume(name, paths):
    s, imgs, _, _, _ = end_to_end(name)
    imgs, cams = [torch.tensor(im, device=DEV) for im in imgs], sc.cameras(s)
    kw = dict(radius=s.radius, min_views=s.min_views)
    prior = torch.tensor(occ.box_dsm() if name == "box" else real_floor()[0], device=DEV)
    out = refine_sweep(imgs, cams, s.grid, s.alt_lo, s.step, s.planes, prior=prior, p1=0.125, p2=0.75, paths=paths, volume=True, **kw)
    assert sorted(out) == ["aggregated", "altitude", "floor", "index", "photo", "prior", "score", "volume"]
    assert out["prior"] is prior
    dirs, _ = rectify.view_directions(s.grid, cams, s.alt_lo, s.alt_lo + (s.planes - 1) * s.step, DEV)
    floor = visibility_floor(prior, s.grid, dirs)
    assert torch.equal(out["floor"], floor) and torch.isfinite(floor).any()
    gated = host(visible_sweep(imgs, cams, s.grid, s.alt_lo, s.step, s.planes, floor, slack=s.step, volume=True, **kw))   # slack defaults to one step
    out = host(out)
    assert same(out["volume"], gated["volume"])
    agg = sg.aggregate(gated["volume"], 0.125, 0.75, 1.0, paths)
    want = sg.pick(agg, gated["volume"], s.alt_lo, s.step)
    assert np.isfinite(agg).any() and same(out["aggregated"], agg)
    for k in want:
        assert same(out[k], want[k]), k
    # without a prior the first pass is smooth_sweep's altitude
    from spnerf_amd import smooth_sweep
    first = smooth_sweep(imgs, cams, s.grid, s.alt_lo, s.step, s.planes, p1=0.125, p2=0.75, paths=paths, **kw)["altitude"]
    own = refine_sweep(imgs, cams, s.grid, s.alt_lo, s.step, s.planes, p1=0.125, p2=0.75, paths=paths, **kw)
    assert sorted(own) == ["altitude", "floor", "index", "photo", "prior", "score"]
    assert same(own["prior"].cpu().numpy(), first.cpu().numpy())
    assert torch.equal(own["floor"], visibility_floor(first, s.grid, dirs))
    second = host(visible_sweep(imgs, cams, s.grid, s.alt_lo, s.step, s.planes, own["floor"], slack=s.step, volume=True, **kw))["volume"]
    want = sg.pick(sg.aggregate(second, 0.125, 0.75, 1.0, paths), second, s.alt_lo, s.step)
    for k in want:
        assert same(own[k].cpu().numpy(), want[k]), k


def test_the_ungated_sweep_and_the_cast_keep_their_bytes_around_gated_calls():
    s = sc.BY_NAME["real"]
    imgs, cams = device_images("real"), sc.cameras(s)
    kw = dict(radius=s.radius, min_views=s.min_views)
    dsm = torch.tensor(shc.heights((33, 65)), device=DEV)
    before = host(plane_sweep(imgs, cams, s.grid, s.alt_lo, s.step, s.planes, volume=True, **kw))
    shadow0, excess0 = cast_shadows(dsm, shc.RESOLUTION, shc.DIRS, excess=True)
    floor = visibility_floor(dsm, shc.RESOLUTION, occ.dirs()[7:])
    visible_sweep(imgs, cams, s.grid, s.alt_lo, s.step, s.planes, floor - 20.0, slack=1.0, volume=True, **kw)
    after = host(plane_sweep(imgs, cams, s.grid, s.alt_lo, s.step, s.planes, volume=True, **kw))
    shadow1, excess1 = cast_shadows(dsm, shc.RESOLUTION, shc.DIRS, excess=True)
    for k in before:
        assert same(before[k], after[k]), k
    assert torch.equal(shadow0, shadow1) and same(excess0.cpu().numpy(), excess1.cpu().numpy())
    # and the cast is still the statement's: the march moved to a header without a change
    ref_shadow, ref_excess = shc.reference((33, 65))
    finite = np.isfinite(ref_excess)
    assert bool((np.abs(excess1.cpu().numpy()[finite] - ref_excess[finite]) <= sn.tolerance(shc.heights((33, 65)))).all())
