"""The semi-global aggregation on the GPU (csrc/sgm.hip, spnerf_amd.sgm) — needs an MI355X.

The definition (include/spnerf_amd_sgm.h) is fp32 with a fixed operation order, so every comparison here
is for equal bytes with the numpy statement (tests/sgm_numpy.py, itself pinned to exact integer paths and
closed forms on the CPU by tests/test_sgm_ref.py); no tolerance appears:

* ``aggregate`` on the random volumes of tests/sgm_cases.py (20 % NaN, ±inf, a cell without any score,
  ties; dyadic and arbitrary scores and penalties) over grids of one cell, one row, one column, ragged
  tiles (17 x 33, 33 x 65, 65 x 130: not square, so diagonals begin on both edges) and K on both sides of
  one wavefront (64, 65), two and a half (130) and the largest (512); both ``paths``; p1 = p2; p1 = 0;
* two runs of one call return the same bytes;
* ``pick``: ``altitude``, ``index`` and ``score`` are ``sweep_numpy.pick``'s on the aggregated volume and
  ``photo`` the gather of the raw scores;
* the step scene gives the statement's indices, so its wrong-cell counts: 51 before, 0 / 3 / 1 / 5 after;
* ``smooth_sweep`` on the scenes "half" and "real" of tests/sweep_cases.py: every plane equal to the numpy
  statement applied to the device's own ``plane_sweep(volume=True)`` volume;
* ``plane_sweep`` returns the same bytes before and after a ``smooth_sweep`` call.
"""
import numpy as np
import pytest
import torch

import sgm_cases as gc
import sgm_numpy as sg
import sweep_cases as sc
from spnerf_amd import plane_sweep, sgm, smooth_sweep
from test_gpu_parity import DEV

pytestmark = pytest.mark.gpu


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def differing(a, b):
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


# K, H, W, dyadic scores, p1, p2, unscored, paths
AGGREGATE_CASES = [
    (1, 1, 1, True, 0.125, 1.0, 1.0, 8), (2, 1, 1, False, 0.1, 0.7, 1.0, 4), (1, 1, 7, False, 0.1, 0.7, 1.0, 8), (3, 1, 7, True, 0.125, 1.0, 1.0, 4),
    (9, 1, 7, False, 0.1, 0.7, 0.9, 8), (2, 7, 1, False, 0.1, 0.7, 1.0, 8), (9, 7, 1, True, 0.25, 0.25, 1.0, 4), (65, 7, 1, False, 0.0, 0.7, 1.0, 8),
    (3, 17, 33, False, 0.1, 0.7, 1.0, 4), (9, 17, 33, True, 0.125, 1.0, 1.0, 8), (9, 17, 33, False, 0.3, 0.3, 1.0, 8), (130, 17, 33, False, 0.1, 0.7, 1.0, 8),
    (9, 33, 65, False, 0.1, 0.7, 1.0, 8), (9, 33, 65, False, 0.1, 0.7, 0.9, 4), (64, 33, 65, False, 0.1, 0.7, 1.0, 8), (64, 33, 65, True, 0.0, 0.5, 1.0, 4),
    (65, 33, 65, False, 0.1, 0.7, 1.0, 4), (65, 33, 65, False, 0.0, 0.0, 1.0, 8), (130, 33, 65, False, 0.1, 0.7, 1.0, 4),
    (512, 5, 7, False, 0.1, 0.7, 1.0, 8), (512, 5, 7, True, 0.125, 1.0, 1.25, 4), (257, 5, 7, False, 0.1, 0.1, 1.0, 8),
    (3, 65, 130, False, 0.1, 0.7, 1.0, 8), (2, 65, 130, True, 0.125, 1.0, 1.0, 4),
]


@pytest.mark.parametrize("K,H,W,dyadic,p1,p2,unscored,paths", AGGREGATE_CASES)
def test_aggregate_is_bit_equal_to_the_numpy_statement(K, H, W, dyadic, p1, p2, unscored, paths):
    vol = gc.random_volume(K, H, W, dyadic)
    want = gc.reference(K, H, W, dyadic, p1, p2, unscored, paths)
    dev = torch.tensor(vol, device=DEV)
    out = sgm.aggregate(dev, p1=p1, p2=p2, unscored=unscored, paths=paths)
    assert out.dtype == torch.float32 and tuple(out.shape) == (K, H, W) and out.data_ptr() != dev.data_ptr()
    got = out.cpu().numpy()
    print(f"K {K} grid {H} x {W} paths {paths}: {differing(got, want)} of {want.size} entries differ, {int(np.isnan(want).sum())} NaN")
    if H * W > 1:
        assert np.isnan(want[:, H - 1, W // 2]).all() and np.isfinite(want).any()
    assert same(dev.cpu().numpy(), vol)                                  # the input is left alone
    assert same(got, want)
    again = sgm.aggregate(dev, p1=p1, p2=p2, unscored=unscored, paths=paths).cpu().numpy()
    assert same(again, got)


@pytest.mark.parametrize("K,H,W,dyadic,p1,p2,unscored,paths", [AGGREGATE_CASES[k] for k in (0, 3, 9, 12, 14, 19, 22)])
def test_pick_is_the_sweeps_pick_with_the_raw_score(K, H, W, dyadic, p1, p2, unscored, paths):
    vol, agg = gc.random_volume(K, H, W, dyadic), gc.reference(K, H, W, dyadic, p1, p2, unscored, paths)
    want = sg.pick(agg, vol, -23.5, 0.75)
    out = sgm.pick(torch.tensor(agg, device=DEV), torch.tensor(vol, device=DEV), -23.5, 0.75)
    assert sorted(out) == ["altitude", "index", "photo", "score"]
    assert out["index"].dtype == torch.int32 and out["altitude"].dtype == out["score"].dtype == out["photo"].dtype == torch.float32
    out = host(out)
    for k in out:
        assert same(out[k], want[k]), k
    some = want["index"] >= 0
    gathered = np.take_along_axis(vol, np.where(some, want["index"], 0)[None], 0)[0]
    assert np.array_equal(out["photo"][some & np.isfinite(gathered)], gathered[some & np.isfinite(gathered)])
    assert np.isnan(out["photo"][~(some & np.isfinite(gathered))]).all()
    if H * W > 1:
        assert not some[H - 1, W // 2] and some.any()


@pytest.mark.parametrize("p1,p2,paths", sorted(gc.STEP_WRONG))
def test_the_step_scene_on_the_gpu(p1, p2, paths):
    vol, truth = gc.step_scene()
    dev = torch.tensor(vol, device=DEV)
    before = host(sgm.pick(dev, dev, 0.0, 1.0))["index"]                 # each cell on its own
    agg = sgm.aggregate(dev, p1=p1, p2=p2, paths=paths)
    assert same(agg.cpu().numpy(), gc.step_reference(p1, p2, paths))
    out = host(sgm.pick(agg, dev, 0.0, 1.0))
    want = sg.pick(gc.step_reference(p1, p2, paths), vol, 0.0, 1.0)
    wrong = out["index"] != truth
    print(f"p1 {p1} p2 {p2} paths {paths}: wrong at {int((before != truth).sum())} cells before, {int(wrong.sum())} after")
    assert (before != truth).sum() == gc.STEP_OUTLIERS == 51
    assert np.array_equal(out["index"], want["index"]) and wrong.sum() == gc.STEP_WRONG[(p1, p2, paths)]
    corner = np.zeros_like(wrong)
    corner[0, 0] = (p2, paths) == (0.5, 8)                               # tests/test_sgm_ref.py
    assert gc.near_step(wrong & ~corner)


@pytest.mark.parametrize("name,paths", [("half", 8), ("real", 8), ("real", 4)])
def test_smooth_sweep_is_the_statement_on_the_devices_own_volume(name, paths):
    s = sc.BY_NAME[name]
    imgs, cams = [torch.tensor(im, device=DEV) for im in sc.images(name)], sc.cameras(s)
    kw = dict(radius=s.radius, min_views=s.min_views)
    before = host(plane_sweep(imgs, cams, s.grid, s.alt_lo, s.step, s.planes, volume=True, **kw))
    out = smooth_sweep(imgs, cams, s.grid, s.alt_lo, s.step, s.planes, p1=0.125, p2=0.75, paths=paths, volume=True, **kw)
    assert sorted(out) == ["aggregated", "altitude", "index", "photo", "score", "volume"]
    out = host(out)
    bare = host(smooth_sweep(imgs, cams, s.grid, s.alt_lo, s.step, s.planes, p1=0.125, p2=0.75, paths=paths, **kw))
    assert sorted(bare) == ["altitude", "index", "photo", "score"]
    after = host(plane_sweep(imgs, cams, s.grid, s.alt_lo, s.step, s.planes, volume=True, **kw))
    for k in before:
        assert same(before[k], after[k]), k                              # the sweep is untouched
    assert same(out["volume"], before["volume"])
    agg = sg.aggregate(before["volume"], 0.125, 0.75, 1.0, paths)
    want = sg.pick(agg, before["volume"], s.alt_lo, s.step)
    changed = (want["index"] != before["index"]) & (before["index"] >= 0)
    print(f"{name}, {paths} paths: {differing(out['aggregated'], agg)} of {agg.size} aggregated entries differ; the index changes at "
          f"{int(changed.sum())} of {int((before['index'] >= 0).sum())} cells")
    assert np.isfinite(agg).any() and np.array_equal(want["index"] >= 0, before["index"] >= 0)
    assert same(out["aggregated"], agg)
    for k in want:
        assert same(out[k], want[k]), k
        assert same(bare[k], want[k]), k
