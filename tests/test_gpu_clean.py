"""The DSM-cleaning exports on the GPU (csrc/clean.hip, spnerf_amd.clean) — needs an MI355X.

Everything is held to the numpy statement (tests/clean_numpy.py, itself pinned to closed forms on the CPU by
tests/test_clean_ref.py) on the cases of tests/clean_cases.py, and every comparison is for equal bytes over
every cell: nothing in the three definitions rounds, so there is no tolerance anywhere.

* ``speckle_filter``: ``dsm``, ``label`` and ``size`` on seven grids — among them (T − 1) x (T + 1), T x T and
  (T + 1) x (2T + 1) for the tile T — and nine patterns each (random levels with NaN and ±inf, a serpentine, a
  spiral, a comb, a checkerboard, one component, NaN walls with a gap, diagonal contacts, ``max_diff`` met exactly
  and missed by an ulp), at ``max_size`` 0, 1, a mid value and H·W; the word of the iteration bound clear, two
  runs the same bytes, the input untouched;
* ``median_dsm``: radius 1, 2, 3, ``min_count`` 1 and (2r+1)², ``fill`` off and on, all NaN, both zeros;
* ``fill_holes``: both modes, ``reach`` 1, 3, 4096, ``min_dirs`` 1, 3, 8, all NaN, no holes;
* ``clean_dsm``: every plane of the dict against the statement's chain;
* restoration: 12 speckles on the box raster are removed and filled back to the original's bytes, and the
  ``visibility_floor`` with them;
* ``bootstrap_sweep``: the chain ``smooth_sweep`` → ``clean_dsm`` → ``refine_sweep`` called by hand, and the sweeps'
  bytes before and after.
"""
import numpy as np
import pytest
import torch

import clean_cases as cc
import clean_numpy as cn
import occlusion_cases as occ
import sweep_cases as sc
from spnerf_amd import (bootstrap_sweep, clean, clean_dsm, fill_holes, median_dsm, plane_sweep, refine_sweep, smooth_sweep, speckle_filter,
                        visibility_floor)
from test_gpu_parity import DEV

pytestmark = pytest.mark.gpu


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def dev(a):
    return torch.tensor(a, device=DEV)


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("shape", cc.GRIDS)
def test_speckle_filter_has_the_statements_bytes(shape):
    cells = shape[0] * shape[1]
    for name in cc.PATTERNS:
        raster, max_diff = cc.pattern(name, shape)
        parts = cn.components(raster, max_diff)
        d = dev(raster)
        for max_size in (0, 1, max(cells // 3, 2), cells):
            want = cn.speckle(raster, max_diff, max_size, parts)
            got, work = clean._speckle(d, max_diff, max_size)
            assert got["dsm"].dtype == torch.float32 and got["label"].dtype == got["size"].dtype == torch.int32 and got["dsm"].device == d.device
            assert int(work[-4]) == 0, (name, max_size)                  # the word of the iteration bound
            got = host(got)
            for k, w in zip(("dsm", "label", "size"), want):
                assert same(got[k], w), (name, max_size, k)
        again = host(speckle_filter(d, max_diff=max_diff, max_size=cells))   # the public call; a second run
        for k in again:
            assert same(again[k], got[k]), (name, k)
        assert same(d.cpu().numpy(), raster)
        n = int(np.isfinite(raster).sum())
        print(f"{shape} {name}: {n} finite cells, {len(np.unique(parts[0][parts[0] >= 0]))} components, largest {int(parts[1].max())}")


def test_speckle_filter_takes_a_view_that_is_not_contiguous():
    raster, max_diff = cc.pattern("random4", (65, 130))
    d = dev(np.ascontiguousarray(raster.T)).t()
    assert not d.is_contiguous()
    got = host(speckle_filter(d, max_diff=max_diff, max_size=5))
    for k, w in zip(("dsm", "label", "size"), cn.speckle(raster, max_diff, 5)):
        assert same(got[k], w), k


@pytest.mark.parametrize("shape", cc.GRIDS)
def test_median_dsm_has_the_statements_bytes(shape):
    raster = cc.median_raster(shape)
    d = dev(raster)
    for radius in (1, 2, 3):
        for min_count in (1, (2 * radius + 1) ** 2):
            for fill in (False, True):
                got = median_dsm(d, radius=radius, min_count=min_count, fill=fill)
                assert got.dtype == torch.float32 and tuple(got.shape) == shape
                assert same(got.cpu().numpy(), cn.median(raster, radius, min_count, fill)), (radius, min_count, fill)
    assert same(median_dsm(d).cpu().numpy(), cn.median(raster, 1))       # the defaults
    assert same(d.cpu().numpy(), raster)


def test_median_dsm_of_all_nan_and_of_both_zeros():
    nan = np.full((cc.T + 1, 2 * cc.T + 1), np.nan, np.float32)
    for fill in (False, True):
        assert same(median_dsm(dev(nan), radius=2, fill=fill).cpu().numpy(), nan)
    zeros = cc.zeros_raster()
    for radius in (1, 3):
        for fill in (False, True):
            got = median_dsm(dev(zeros), radius=radius, fill=fill).cpu().numpy()
            assert same(got, cn.median(zeros, radius, 1, fill))
            assert not np.signbit(got[np.isfinite(got)]).any() and np.isfinite(got).sum() >= np.isfinite(zeros).sum()


@pytest.mark.parametrize("shape", cc.GRIDS)
def test_fill_holes_has_the_statements_bytes(shape):
    raster = cc.fill_raster(shape)
    d = dev(raster)
    for mode in ("lowest", "nearest"):
        for reach in (1, 3, 4096):
            for min_dirs in (1, 3, 8):
                got = fill_holes(d, reach=reach, mode=mode, min_dirs=min_dirs)
                assert got["dsm"].dtype == torch.float32 and got["filled"].dtype == torch.uint8
                want = cn.fill(raster, reach, mode, min_dirs)
                assert same(got["dsm"].cpu().numpy(), want[0]) and same(got["filled"].cpu().numpy(), want[1]), (mode, reach, min_dirs)
    if shape == (65, 130):                                               # the 9 x 9 hole is wider than a reach of 3, not than 4096
        assert np.isnan(cn.fill(raster, 3)[0][7, 8]) and np.isfinite(cn.fill(raster, 4096)[0][7, 8])
    assert same(d.cpu().numpy(), raster)


def test_fill_holes_of_all_nan_and_of_no_holes():
    nan = np.full((cc.T + 1, 2 * cc.T + 1), np.nan, np.float32)
    whole = np.arange(nan.size, dtype=np.float32).reshape(nan.shape)
    for mode in ("lowest", "nearest"):
        got = host(fill_holes(dev(nan), reach=4096, mode=mode))
        assert same(got["dsm"], nan) and not got["filled"].any()
        got = host(fill_holes(dev(whole), reach=4096, mode=mode))
        assert same(got["dsm"], whole) and not got["filled"].any()


@pytest.mark.parametrize("k", [0, 1])
def test_clean_dsm_is_the_statements_chain(k):
    raster, weight = cc.chain_case(k)
    kw = [dict(max_diff=0.5, max_size=9, radius=1, reach=6, mode="lowest"), dict(max_diff=1.0, max_size=4, radius=2, reach=3, mode="nearest", min_dirs=3)][k]
    got = clean_dsm(dev(raster), weight=dev(weight), min_weight=0.25, **kw)
    assert sorted(got) == ["dsm", "filled", "label", "rejected", "size"]
    assert got["rejected"].dtype == got["filled"].dtype == torch.uint8
    want = cn.chain(raster, weight=weight, min_weight=0.25, **kw)
    got = host(got)
    for name in want:
        assert same(got[name], want[name]), name
    assert all((want["rejected"] & bit).any() for bit in (1, 2, 4)) and want["filled"].any()
    # without a weight, a median or a fill
    got = host(clean_dsm(dev(raster), max_diff=kw["max_diff"], max_size=kw["max_size"], radius=0))
    want = cn.chain(raster, kw["max_diff"], kw["max_size"], radius=0)
    for name in want:
        assert same(got[name], want[name]), name
    assert not got["filled"].any() and not (got["rejected"] & 5).any()


def test_speckles_on_the_box_raster_are_removed_and_filled_back():
    original, corrupted, mask = cc.restoration()
    out = clean_dsm(dev(corrupted), max_diff=1.0, max_size=cc.SPECKLE_MAX, radius=0, reach=8, mode="lowest")
    cleaned = out["dsm"]
    out = host(out)
    assert same(out["dsm"], original)
    assert same((out["rejected"] & 2) != 0, mask) and same(out["rejected"], 2 * mask.astype(np.uint8))
    assert same(out["filled"], mask.astype(np.uint8))
    grid, dirs = occ.BOX.grid, occ.box_dirs()
    want = visibility_floor(dev(original), grid, dirs).cpu().numpy()
    assert same(visibility_floor(cleaned, grid, dirs).cpu().numpy(), want)
    spoilt = visibility_floor(dev(corrupted), grid, dirs).cpu().numpy()
    differ = int((spoilt.view(np.uint32) != want.view(np.uint32)).sum())
    print(f"{int(mask.sum())} speckle cells raise the floor at {differ} of {want.size} (view, cell) entries")
    assert differ > 0


def test_bootstrap_sweep_is_the_chain_called_by_hand():
    s = occ.BOX
    imgs, cams = [dev(im) for im in occ.box_images()], sc.cameras(s)
    args, kw = (imgs, cams, s.grid, s.alt_lo, s.step, s.planes), dict(radius=s.radius, min_views=s.min_views)
    before = [host(plane_sweep(*args, **kw)), host(smooth_sweep(*args, **kw)), host(refine_sweep(*args, **kw))]
    out = bootstrap_sweep(*args, sweep_radius=s.radius, min_views=s.min_views, max_size=30, radius=1, min_weight=0.25, reach=4, volume=True)
    assert sorted(out) == ["aggregated", "altitude", "cleaned", "first", "floor", "index", "photo", "prior", "score", "volume"]
    first = smooth_sweep(*args, **kw)
    cleaned = clean_dsm(first["altitude"], weight=first["photo"], min_weight=0.25, max_diff=s.step, max_size=30, radius=1, reach=4)
    want = refine_sweep(*args, prior=cleaned["dsm"], volume=True, **kw)
    assert same(out["first"].cpu().numpy(), first["altitude"].cpu().numpy())
    for k in cleaned:
        assert same(out["cleaned"][k].cpu().numpy(), cleaned[k].cpu().numpy()), k
    assert same(out["prior"].cpu().numpy(), cleaned["dsm"].cpu().numpy())
    for k in want:
        assert same(out[k].cpu().numpy(), want[k].cpu().numpy()), k
    rejected = out["cleaned"]["rejected"].cpu().numpy()
    print(f"box: first pass {int(torch.isfinite(first['altitude']).sum())} finite cells; rejected by weight {int((rejected & 1 != 0).sum())}, "
          f"speckle {int((rejected & 2 != 0).sum())}, median {int((rejected & 4 != 0).sum())}; filled {int(out['cleaned']['filled'].sum())}")
    # the defaults, the row chosen on the ROI: max_diff two steps, max_size SPECKLE_CELLS, no median, the weight at 0.25, no fill
    assert (clean.MAX_DIFF_STEPS, clean.SPECKLE_CELLS, clean.MEDIAN_RADIUS, clean.MIN_WEIGHT) == (2, 100, 0, 0.25)
    plain = bootstrap_sweep(*args, sweep_radius=s.radius, min_views=s.min_views)
    assert sorted(plain) == ["altitude", "cleaned", "first", "floor", "index", "photo", "prior", "score"]
    cleaned = clean_dsm(first["altitude"], weight=first["photo"], min_weight=0.25, max_diff=2 * s.step, max_size=100, radius=0)
    want = refine_sweep(*args, prior=cleaned["dsm"], **kw)
    for k in want:
        assert same(plain[k].cpu().numpy(), want[k].cpu().numpy()), k
    assert not plain["cleaned"]["filled"].any() and (plain["cleaned"]["rejected"] & 1).any()
    # without the weight
    bare = bootstrap_sweep(*args, sweep_radius=s.radius, min_views=s.min_views, min_weight=None, max_diff=s.step, radius=1)
    cleaned = clean_dsm(first["altitude"], max_diff=s.step, max_size=100, radius=1)
    assert same(bare["prior"].cpu().numpy(), cleaned["dsm"].cpu().numpy()) and not (bare["cleaned"]["rejected"] & 1).any()
    after = [host(plane_sweep(*args, **kw)), host(smooth_sweep(*args, **kw)), host(refine_sweep(*args, **kw))]
    for b, a in zip(before, after):
        for k in b:
            assert same(b[k], a[k]), k
