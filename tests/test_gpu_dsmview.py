"""The DSM view on the GPU (csrc/dsm_view.hip, spnerf_amd.dsm_view) — needs an MI355X.

The cast is held to the fp64 numpy statement (tests/dsmview_numpy.py, itself pinned on the CPU by
tests/test_dsmview_ref.py) on every case of tests/dsmview_cases.py.  The device and the statement localise and
project with different code (Newton steps and real series against a fixed point and complex series, another
libm), so their segments differ in the last digits and nothing here is bit-equal:

* ``hit`` equals the statement's except where the statement's decision stood within NEAR_TIE of flipping
  (``margin`` of ``dsmview_numpy.walk``: an excess, a minor coordinate's distance from the grid's outer lines or
  the crossing's distance from alt_lo, in metres or cells); NEAR_TIE is 1e-6, fifty times the largest gap of
  ``ground`` measured below, and the band holds less than 1 % of the pixels of every case;
* ``altitude``, ``cell``, ``ground`` and ``depth`` at the common hits lie within four times the worst gap measured;
* ``sample_at`` has the statement's bytes in both modes, ``hit_ecef`` lies within 1e-8 m of it;
* the device's near end — the line through the crossings of two constant planes, taken up to alt_hi — is the statement's
  localisation at alt_hi, the near point of ``get_rays`` before its ECEF and fp32 steps;
* ``dsm_depth_priors`` → ``load_depth_data`` end to end on a full-resolution camera;
* ``cast_shadows``, ``visibility_floor``, ``orthorectify`` and ``pyramid_sweep`` return the same bytes before and
  after calls of the new kernels.

Measured on MI355X (2026-10-21), worst over the 17 cases: |altitude − statement| 1.907e-6 m ("south": one fp32 ulp at
16 m), |cell| 1.907e-6 cells ("plane": half an ulp at 32), |ground| 1.863e-8 m ("relief_s3"), |depth| 9.537e-7 m; no
``hit`` differs and no pixel of any case lies in the near-tie band (the smallest margin is 9.8e-5, on "tilt");
``hit_ecef`` 2.8e-9 m from the statement, the near end 2.8e-9 m.  Priors ("relief", 2376 keypoints): |‖pts3d − near‖ − depth| 0.255 m at the
most (0.094 m in the mean) — the fp32 ECEF of ``get_rays``' near point; the cast of ``pts3d`` to fp32 inside
``load_depth_data`` moves the depth it derives by 0.256 m at the most, 0.093 m in the mean.
"""
import functools

import numpy as np
import pytest
import torch

import dsmview_cases as dc
import dsmview_numpy as dn
import rectify_cases as rc
import sweep_cases as sc
from spnerf_amd import (cast_shadows, dataset, dsm_depth_priors, hit_ecef, normalised_depth, orthorectify, pyramid_sweep, sample_at, satellite,
                        view_dsm, visibility_floor)
from spnerf_amd.rectify import view_directions
from test_gpu_parity import DEV

pytestmark = pytest.mark.gpu

NEAR_TIE = 1e-6
# the worst |device − statement| over all cases, as measured; the bounds are four times these
MEASURED = {"altitude": 1.91e-6, "cell": 1.91e-6, "ground": 1.87e-8, "depth": 9.54e-7}
BOUND = {k: 4.0 * v for k, v in MEASURED.items()}


def dev(a):
    return torch.tensor(np.asarray(a), device=DEV)


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def device_cast(name):
    case = dc.BY_NAME[name]
    out = view_dsm(dev(dc.dsm(name)), case.grid, dc.camera(case), alt_lo=case.alt_lo, alt_hi=case.alt_hi, rect=dc.rect(name), stride=case.stride)
    return host(out)


@pytest.mark.parametrize("name", dc.NAMES)
def test_cast_matches_the_numpy_statement(name):
    case, ref, out = dc.BY_NAME[name], dc.ref(name), device_cast(name)
    n_rows, n_cols = case.shape
    assert out["hit"].dtype == np.uint8 and out["hit"].shape == (n_rows, n_cols) and set(np.unique(out["hit"]).tolist()) <= {0, 1}
    assert out["altitude"].dtype == out["cell"].dtype == out["depth"].dtype == np.float32 and out["ground"].dtype == np.float64
    assert out["ground"].shape == out["cell"].shape == (n_rows, n_cols, 2) and out["altitude"].shape == out["depth"].shape == (n_rows, n_cols)
    hit = out["hit"] == 1
    for k in ("altitude", "depth"):
        assert np.array_equal(np.isnan(out[k]), ~hit), k
    for k in ("ground", "cell"):
        assert np.array_equal(np.isnan(out[k]), np.repeat(~hit[..., None], 2, -1)), k
    band = ref["margin"] < NEAR_TIE
    assert band.mean() < 0.01
    assert np.array_equal(out["hit"][~band], ref["hit"][~band])
    both = hit & (ref["hit"] == 1) & ~band
    worst = {}
    for k in ("altitude", "cell", "ground", "depth"):
        gap = np.abs(out[k].astype(np.float64) - ref[k].astype(np.float64))[both]
        worst[k] = float(gap.max()) if gap.size else 0.0
    print(f"{name}: hits {hit.mean():.3f}, band {band.mean():.4f}, differing hits {(out['hit'] != ref['hit']).sum()}, worst " +
          ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= BOUND[k], (k, v)
    if name in ("nan", "off"):
        assert not hit.any()
    # bit-reproducible from run to run
    again = host(view_dsm(dev(dc.dsm(name)), case.grid, dc.camera(case), alt_lo=case.alt_lo, alt_hi=case.alt_hi, rect=dc.rect(name),
                          stride=case.stride))
    assert all(same(out[k], again[k]) for k in out)


@pytest.mark.parametrize("name", ["relief_s3", "holes", "relief_17", "nan"])
def test_sample_at_has_the_statements_bytes(name):
    case, out = dc.BY_NAME[name], device_cast(name)
    cell = out["cell"].copy()
    cell.reshape(-1, 2)[:4] = [[0.0, 0.0], [case.grid.xsize - 1.0, case.grid.ysize - 1.0], [case.grid.xsize - 0.5, 1.0], [-0.25, 2.0]]
    for seed, raster in ((0, dc.weight(case.grid.shape)), (1, dc.dsm(name))):
        for mode, code in (("nearest", 0), ("bilinear", 1)):
            got = sample_at(dev(raster), dev(cell), mode).cpu().numpy()
            assert same(got, dn.sample(raster, cell, code)), (seed, mode)
            assert np.isnan(got.reshape(-1)[2:4]).all() and np.isnan(got[out["hit"] == 0].reshape(-1)[4:]).all()
    # the DSM read back bilinearly at the crossings is the altitude where the four cells around are finite: the surface is hit
    if name == "relief_17":
        hit = out["hit"] == 1
        back = sample_at(dev(dc.dsm(name)), dev(out["cell"]), "nearest").cpu().numpy()
        assert np.isfinite(back[hit]).mean() > 0.9


def test_hit_ecef_and_normalised_depth():
    for name in ("relief", "south"):
        case, out = dc.BY_NAME[name], device_cast(name)
        p = hit_ecef(dev(out["ground"]), dev(out["altitude"]), case.grid).cpu().numpy()
        hit = out["hit"] == 1
        ref = dn.ecef(out["ground"][hit], out["altitude"][hit], case.grid)
        gap = float(np.abs(p[hit] - ref).max())
        print(f"{name}: hit_ecef worst gap {gap:.3e} m")
        assert p.dtype == np.float64 and p.shape == hit.shape + (3,) and gap <= 1e-8 and np.isnan(p[~hit]).all()
        rng = np.float32(300.0)
        nd = normalised_depth(dev(out["depth"]), rng).cpu().numpy()
        assert same(nd, out["depth"] / rng)


def test_priors_go_through_load_depth_data():
    case = dc.BY_NAME["relief"]
    meta = dc.meta(case)
    h, w = int(meta["height"]), int(meta["width"])
    col0 = dc.rect("relief")[0]
    rect = (col0, 0, 64, 64)
    weight = np.abs(dc.weight(case.grid.shape))                    # [0, 1], with NaN and inf entries
    kw = dict(alt_lo=float(meta["min_alt"]), alt_hi=float(meta["max_alt"]))
    dsm = (dc.dsm("relief").astype(np.float64) + 0.5 * (kw["alt_lo"] + kw["alt_hi"]) + 16.0).astype(np.float32)   # the relief, inside the camera's altitudes
    view = host(view_dsm(dev(dsm), case.grid, dc.camera(case), rect=rect, **kw))
    wat = sample_at(dev(weight), dev(view["cell"]), "nearest").cpu().numpy()
    for min_weight in (None, 0.45):
        priors = dsm_depth_priors(dev(dsm), dev(weight), case.grid, [meta], rect=rect, min_weight=min_weight, **kw)
        assert len(priors) == 1 and all(priors[0][k] == meta[k] for k in meta)
        p2, p3, cor = priors[0]["pts2d"].numpy(), priors[0]["pts3d"].cpu().numpy(), priors[0]["correl"].cpu().numpy()
        keep = (view["hit"] == 1) & np.isfinite(wat) & ((wat >= min_weight) if min_weight is not None else True)
        rr, cc = np.nonzero(keep)
        assert 100 < keep.sum() < 64 * 64 and p2.dtype == np.int64 and np.array_equal(p2, np.stack([col0 + cc, rr], 1))
        assert bool((np.diff(p2[:, 1] * w + p2[:, 0]) > 0).all())
        assert p3.dtype == np.float64 and same(cor, wat[keep]) and np.isfinite(p3).all()
        assert np.abs(p3 - dn.ecef(view["ground"][keep], view["altitude"][keep], case.grid)).max() <= 1e-8
    priors = dsm_depth_priors(dev(dsm), dev(weight), case.grid, [meta], rect=rect, **kw)
    center, rng = np.array([p3[:, 0].mean(), p3[:, 1].mean(), p3[:, 2].mean()], np.float32), np.float32(256.0)
    deprays, depths, valid, stds = dataset.load_depth_data(priors, center=center, range=rng)
    valid, depths, deprays = valid.cpu().numpy().reshape(h, w), depths.cpu().numpy().reshape(h, w, 2), deprays.cpu().numpy().reshape(h, w, 8)
    keep = (view["hit"] == 1) & np.isfinite(wat)
    want = np.zeros((h, w), bool)
    want[0:64, col0:col0 + 64] = keep
    assert np.array_equal(valid == 1.0, want) and set(np.unique(valid).tolist()) == {0.0, 1.0}
    cor = wat[keep]
    assert same(depths[want][:, 1], (cor - cor.min()) / (cor.max() - cor.min()))      # load_depth_data's weight: correl over its range, in fp32
    # the distance from get_rays' near point (fp32 ECEF: 0.28 m) to pts3d is view_dsm's depth, up to that rounding and the
    # projection's scale factor; test_the_near_end_is_the_segments_start pins the near end itself to 1e-7 m
    rr, cc = np.nonzero(keep)
    rays = satellite.get_rays(col0 + cc, rr, satellite.RPCModel(meta["rpc"]), kw["alt_lo"], kw["alt_hi"], device=DEV).cpu().numpy()
    assert same(deprays[want][:, :3], (rays[:, :3] - center) / rng)          # the origin load_depth_data stores is that near point, normalised
    p3 = priors[0]["pts3d"].cpu().numpy()
    d64 = np.linalg.norm(p3 - rays[:, :3].astype(np.float64), axis=1)
    gap = np.abs(d64 - view["depth"][keep])
    cost = np.abs(depths[want][:, 0].astype(np.float64) * float(rng) - d64)
    print(f"priors: {keep.sum()} keypoints, |‖pts3d − near‖ − depth| worst {gap.max():.3f} m mean {gap.mean():.3f} m; "
          f"fp32 pts3d in load_depth_data moves the depth by worst {cost.max():.3f} m mean {cost.mean():.3f} m")
    assert float(gap.max()) <= 0.28 + 4e-4 * float(np.nanmax(view["depth"])) + 1e-3
    assert float(cost.max()) <= 0.6


@pytest.mark.parametrize("name", ["plane", "plane60"])
def test_the_near_end_is_the_segments_start(name):
    """Two constant planes cut a pixel's segment at two known altitudes; the line through the two crossings, taken up to
    alt_hi, is the device's near end.  It must be the UTM of the pixel's localisation at alt_hi — the near point of
    ``get_rays`` before its ECEF and fp32 steps, as tests/test_dsmview_ref.py holds for the statement — within the bound of
    ``ground`` times the extrapolation's factor (1 + 2·0.4 for planes at −6 m and −16 m under alt_hi = −2 m; less under 14 m)."""
    case, seg = dc.BY_NAME[name], dc.ref(name)["seg"]
    upper = -6.0
    kw = dict(alt_lo=case.alt_lo, alt_hi=case.alt_hi, rect=dc.rect(name), stride=case.stride)
    lo, hi = device_cast(name), host(view_dsm(dev(np.full(case.grid.shape, upper, np.float32)), case.grid, dc.camera(case), **kw))
    both = (lo["hit"] == 1) & (hi["hit"] == 1) & (lo["cell"].min(-1) >= 1) & (hi["cell"].min(-1) >= 1)
    both &= (np.maximum(lo["cell"], hi["cell"]) <= np.array([case.grid.xsize - 2, case.grid.ysize - 2])).all(-1)
    f = (case.alt_hi - upper) / (upper - dc.PLANE_ALT)
    near = hi["ground"] + (hi["ground"] - lo["ground"]) * f
    gap = np.hypot(near[..., 0] - seg["e_hi"], near[..., 1] - seg["n_hi"])[both]
    print(f"{name}: near end {gap.max():.3e} m from the statement's over {both.sum()} pixels")
    assert both.mean() > 0.5 and float(gap.max()) <= (1 + 2 * f) * BOUND["ground"]


def test_older_kernels_return_the_same_bytes_around_the_new_ones():
    name = "33x65_r2"
    case = rc.BY_NAME[name]
    cams, imgs = rc.cameras(case), [dev(im) for im in rc.images(name)]
    h64 = dev(np.nan_to_num(rc.heights(name), nan=-16.0))
    dirs = view_directions(case.grid, cams, case.alt_lo, case.alt_hi, device=DEV)[0]
    scene = sc.BY_NAME["real"]
    simgs = [dev(im) for im in sc.images("real")]

    def older():
        out = {"shadow": cast_shadows(h64, case.grid.resolution, dirs, excess=True),
               "ortho": orthorectify(imgs, cams, h64, case.grid, case.alt_lo, case.alt_hi, mosaic="mean"),
               "floor": visibility_floor(h64, case.grid, dirs),
               "pyramid": pyramid_sweep(simgs, sc.cameras(scene), scene.grid, scene.alt_lo, scene.step, scene.planes, factors=(2,), radius=scene.radius)}
        flat = {}
        for k, v in out.items():
            items = v.items() if isinstance(v, dict) else enumerate(v if isinstance(v, (tuple, list)) else [v])
            for kk, t in items:
                if isinstance(t, torch.Tensor):
                    flat[f"{k}.{kk}"] = t.cpu().numpy()
        return flat

    before = older()
    for n in ("relief", "holes", "nan"):
        c = dc.BY_NAME[n]
        out = view_dsm(dev(dc.dsm(n)), c.grid, dc.camera(c), alt_lo=c.alt_lo, alt_hi=c.alt_hi, rect=dc.rect(n), stride=c.stride)
        sample_at(dev(dc.weight(c.grid.shape)), out["cell"], "bilinear")
        hit_ecef(out["ground"], out["altitude"], c.grid)
    after = older()
    assert len(before) >= 8 and sorted(before) == sorted(after)
    for k in before:
        assert same(before[k], after[k]), k
