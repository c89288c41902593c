"""The numpy statement of the surface sweep (tests/surface_numpy.py) on its own — no GPU needed.

* with a constant dyadic base and dyadic offsets the surface statement has the bytes of ``sweep_numpy.sweep`` at
  ``alt_lo = c + off_lo``;
* ``upsample``: constants, dyadic ramps, f = 1, NaN entries, sizes the factor does not divide;
* ``lift``: one rounding of the fp64 sum, NaN and ±inf;
* the scene ``tilt`` of tests/surface_cases.py (slope 0.25): around the true surface offset 0 is picked, around
  truth + 2 m offset −2, at every cell that all four views can use — 1340 of the 2145 cells — and the 17 horizontal
  planes over the same altitudes score lower there (mean ZNCC at the pick 0.9782 against 0.9857);
* the ``pyramid`` statement: level shapes and plane counts, and a NaN base gives a NaN result.
"""
import numpy as np
import pytest

import sgm_numpy as sg
import surface_cases as fc
import surface_numpy as sn
import sweep_cases as sc
import sweep_numpy as sw


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name,c,off_lo,step", [("real", -20.0, -4.0, 2.0), ("flat", -16.5, -3.5, 1.0)])
def test_a_constant_base_gives_the_plane_statement(name, c, off_lo, step):
    s = sc.BY_NAME[name]
    grid = sc._jax((9, 21))
    K = 5
    base = np.full(grid.shape, c, np.float32)
    out = sn.sweep(sc.images(name), sc.ref_cameras(s), grid, base, off_lo, step, K, s.radius, s.min_views)
    want = sw.sweep(sc.images(name), sc.ref_cameras(s), grid, c + off_lo, step, K, s.radius, s.min_views)
    assert np.isfinite(want["volume"]).any() and (want["index"] >= 0).any()
    for k in ("volume", "views_vol", "index", "score", "views"):
        assert same(out[k], want[k]), k
    # the altitude over the base c is rounded to fp32 twice (the relative altitude, then the lift), the plane statement's once:
    # three half ulps of an altitude below 32 m apart at the most; over a zero base the lift changes nothing and the bytes are equal
    rel = sw.pick(out["volume"], out["views_vol"], off_lo, step)["altitude"]
    assert same(out["altitude"], sn.lift(base, rel))
    some = want["index"] >= 0
    assert np.array_equal(np.isnan(out["altitude"]), ~some)
    assert bool((np.abs(out["altitude"][some].astype(np.float64) - want["altitude"][some]) <= 1.5 * 2.0 ** -19).all())
    zero = sn.sweep(sc.images(name), sc.ref_cameras(s), grid, np.zeros_like(base), c + off_lo, step, K, s.radius, s.min_views)
    for k in ("volume", "views_vol", "index", "score", "views", "altitude"):
        assert same(zero[k], want[k]), k
    g, ok = sn.grey(sc.images(name), sc.ref_cameras(s), grid, base, off_lo + step)
    wg, wok = sw.grey(sc.images(name), sc.ref_cameras(s), grid, c + off_lo + step)
    assert same(g, wg) and same(ok, wok)


def test_a_base_that_is_not_finite_invalidates_every_view():
    s = sc.BY_NAME["real"]
    grid = sc._jax((9, 21))
    base = np.full(grid.shape, -20.0, np.float32)
    base[2, 3], base[4, 5], base[6, 7] = np.nan, np.inf, -np.inf
    g, ok = sn.grey(sc.images("real"), sc.ref_cameras(s), grid, base, 1.0)
    wg, wok = sw.grey(sc.images("real"), sc.ref_cameras(s), grid, -19.0)
    bad = ~np.isfinite(base)
    assert wok[:, bad].any(axis=0).all() and not ok[:, bad].any() and np.isnan(g[:, bad]).all()
    assert same(g[:, ~bad], wg[:, ~bad]) and same(ok[:, ~bad], wok[:, ~bad])
    out = sn.sweep(sc.images("real"), sc.ref_cameras(s), grid, base, -2.0, 2.0, 3, 1, 2)
    near = np.zeros(grid.shape, bool)
    for j, i in zip(*np.nonzero(bad)):
        near[max(j - 1, 0):j + 2, max(i - 1, 0):i + 2] = True
    assert (out["index"][near] == -1).all() and np.isnan(out["altitude"][near]).all() and (out["index"][~near] >= 0).any()


@pytest.mark.parametrize("f", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("shape", [(7, 9), (16, 32), (1, 1), (1, 5)])
def test_upsample_keeps_a_constant(f, shape):
    H, W = shape
    coarse = np.full((-(-H // f), -(-W // f)), -17.25, np.float32)
    out = sn.upsample(coarse, f, shape)
    assert out.dtype == np.float32 and out.shape == shape and (out == np.float32(-17.25)).all()


@pytest.mark.parametrize("f", [2, 4, 8])
def test_upsample_reproduces_a_dyadic_ramp_away_from_the_clamped_border(f):
    H, W = 40, 56
    hc, wc = H // f, W // f
    jc, ic = np.meshgrid(np.arange(hc, dtype=np.float64), np.arange(wc, dtype=np.float64), indexing="ij")
    coarse = (0.5 * jc - 0.25 * ic + 3.0).astype(np.float32)
    out = sn.upsample(coarse, f, (H, W))
    j, i = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    want = 0.5 * ((j + 0.5) / f - 0.5) - 0.25 * ((i + 0.5) / f - 0.5) + 3.0     # the ramp at the fine cell centres, exact in fp32
    inner = (slice(f // 2, H - f // 2), slice(f // 2, W - f // 2))
    assert np.array_equal(out[inner].astype(np.float64), want[inner])
    assert not np.array_equal(out.astype(np.float64), want)                # the border is clamped, not extrapolated
    assert out[0, 0] == coarse[0, 0] and out[-1, -1] == coarse[-1, -1]


def test_upsample_by_one_is_the_identity_on_finite_values():
    g = np.random.default_rng(5)
    coarse = g.standard_normal((7, 9)).astype(np.float32) * np.float32(30.0)
    coarse[1, 2], coarse[3, 4], coarse[5, 6] = np.nan, np.inf, -np.inf
    out = sn.upsample(coarse, 1, (7, 9))
    ok = np.isfinite(coarse)
    assert same(out[ok], coarse[ok]) and np.isnan(out[~ok]).all()


def test_upsample_leaves_non_finite_entries_out():
    coarse = np.array([[1.0, 2.0, 4.0], [3.0, np.nan, 8.0], [5.0, 6.0, 16.0]], np.float32)
    out = sn.upsample(coarse, 2, (6, 6))
    # fine cell (1, 1): y = x = 0.25, the four entries 1, 2, 3, NaN with weights 9/16, 3/16, 3/16, 1/16
    assert out[1, 1] == np.float32((9 / 16 * 1.0 + 3 / 16 * 2.0 + 3 / 16 * 3.0) / (15 / 16))
    # fine cells (2, 2) .. (3, 3) are nearest the NaN: it is still left out
    assert np.isfinite(out).all()
    assert out[2, 2] == np.float32((1 / 16 * 1.0 + 3 / 16 * 2.0 + 3 / 16 * 3.0) / (7 / 16))
    lone = np.full((3, 3), np.nan, np.float32)
    lone[1, 1] = 7.0
    out = sn.upsample(lone, 2, (6, 6))
    assert (out[1:5, 1:5] == np.float32(7.0)).all()                       # the one finite entry wherever it has a weight
    assert np.isnan(out[0, :]).all() and np.isnan(out[:, 0]).all() and np.isnan(out[5, :]).all() and np.isnan(out[:, 5]).all()
    inf = np.array([[np.inf, 2.0], [-np.inf, np.nan]], np.float32)
    out = sn.upsample(inf, 4, (8, 8))                                      # the 2 wherever it has a weight: rows 0..5, columns 2..7
    assert (out[:6, 2:] == np.float32(2.0)).all() and np.isnan(out[6:]).all() and np.isnan(out[:, :2]).all()
    assert np.isnan(sn.upsample(np.full((2, 3), np.nan, np.float32), 4, (8, 9))).all()      # an all-NaN block


@pytest.mark.parametrize("f", [2, 3, 4])
def test_upsample_on_sizes_the_factor_does_not_divide(f):
    H, W = 7, 9
    hc, wc = -(-H // f), -(-W // f)
    coarse = np.random.default_rng(f).standard_normal((hc, wc)).astype(np.float32)
    out = sn.upsample(coarse, f, (H, W))
    assert out.shape == (H, W) and np.isfinite(out).all()
    assert out.min() >= coarse.min() and out.max() <= coarse.max()         # a convex combination
    c = coarse.astype(np.float64)
    for j, i in ((0, 0), (3, 4), (6, 8), (6, 0)):                           # straight from the header, cell by cell
        y, x = (j + 0.5) / f - 0.5, (i + 0.5) / f - 0.5
        j0, i0 = int(np.floor(y)), int(np.floor(x))
        t, s = y - j0, x - i0
        ja, jb, ia, ib = (min(max(k, 0), n - 1) for k, n in ((j0, hc), (j0 + 1, hc), (i0, wc), (i0 + 1, wc)))
        num = den = 0.0
        for h, w in ((c[ja, ia], (1 - t) * (1 - s)), (c[ja, ib], (1 - t) * s), (c[jb, ia], t * (1 - s)), (c[jb, ib], t * s)):
            num, den = num + w * h, den + w
        assert out[j, i] == np.float32(num / den), (j, i)
    with pytest.raises(AssertionError):
        sn.upsample(coarse, f, (H + f, W))


def test_lift_rounds_the_fp64_sum_once():
    base = np.array([16777216.0, -16.1, 1.0, np.nan, 2.0, np.inf, 1e-30], np.float32)
    rel = np.array([1.0, 0.3, 2.0 ** -30, 1.0, np.nan, 1.0, -1e-30], np.float32)
    out = sn.lift(base, rel)
    assert out.dtype == np.float32
    assert out[0] == np.float32(16777216.0)                               # 2^24 + 1 ties to even
    assert out[1] == np.float32(np.float64(np.float32(-16.1)) + np.float64(np.float32(0.3)))
    assert out[2] == np.float32(1.0) and np.isnan(out[3]) and np.isnan(out[4]) and out[5] == np.inf and out[6] == 0.0


def test_the_tilted_plane_is_found_around_its_base():
    ref, up = fc.ref_tilt(0.0), fc.ref_tilt(2.0)
    four = (ref["views"] == 4) & (up["views"] == 4)
    flat = fc.ref_tilt_planes()
    four &= flat["views"] == 4
    lo, step, K = fc.tilt_planes()
    mean_surface = float(ref["score"][four].astype(np.float64).mean())
    mean_planes = float(flat["score"][four].astype(np.float64).mean())
    print(f"slope {fc.SLOPE}: all four views usable at {int(four.sum())} of {four.size} cells; index histogram around the truth "
          f"{np.bincount(ref['index'][four], minlength=9).tolist()}, around truth + 2 m {np.bincount(up['index'][four], minlength=9).tolist()}; "
          f"mean score at the pick {mean_surface:.4f} on the surfaces, {mean_planes:.4f} on the {K} planes from {lo} m")
    assert four.sum() >= 0.5 * four.size
    assert (ref["index"][four] == 4).all()
    assert (up["index"][four] == 2).all()
    assert bool((np.abs(ref["altitude"][four].astype(np.float64) - fc.tilt_truth()[four]) <= 0.5 * fc.TILT.step).all())
    assert bool((np.abs(up["altitude"][four].astype(np.float64) - fc.tilt_truth()[four]) <= 0.5 * fc.TILT.step).all())
    assert mean_planes < mean_surface


@pytest.mark.parametrize("shape,factors", [((33, 65), (2,)), ((17, 33), (2,)), ((17, 33), (4, 2)), ((33, 65), (4, 2))])
def test_the_pyramid_statement(shape, factors):
    s = sc.BY_NAME["real"]
    grid = sc._jax(shape)
    planes, step, reach = 8, 2.0, 1
    levels = sn.pyramid(sc.images("real"), sc.ref_cameras(s), grid, -24.0, step, planes, factors, reach, 2, 2, 0.0, 0.125, 0.75)
    fs = tuple(factors) + (1,)
    assert len(levels) == len(fs)
    assert sn.level_plan(factors, planes, reach) == [(fs[0], 2, 4)] + [(f, min(f, 2), 2 * reach * (2 // min(f, 2)) + 1) for f in fs[1:]]
    assert sn.level_plan((4,), 64, 3) == [(4, 2, 32), (1, 1, 13)] and sn.level_plan((4, 2), 63, 3) == [(4, 2, 32), (2, 2, 7), (1, 1, 13)]
    for f, level in zip(fs, levels):
        assert level["shape"] == (-(-shape[0] // f), -(-shape[1] // f)) == level["altitude"].shape
    assert [lv["planes"] for lv in levels] == [4] + [3 if f > 1 else 5 for f in fs[1:]]
    last = levels[-1]
    assert sorted(last) == ["altitude", "base", "index", "off_lo", "photo", "planes", "score", "shape", "step"]
    assert last["off_lo"] == -4.0 and last["step"] == 2.0
    assert same(last["base"], sn.upsample(levels[-2]["altitude"], fs[-2], shape))
    hole = np.isnan(last["base"])
    print(f"{shape} {factors}: {int(hole.sum())} cells without a base, {int((last['index'] >= 0).sum())} with an index")
    assert np.isnan(last["altitude"][hole]).all() and (last["index"][hole] == -1).all()
    some = last["index"] >= 0
    assert some.any() and bool((np.abs(last["altitude"][some].astype(np.float64) - last["base"][some]) <= 4.0 + 1e-6).all())


def test_a_nan_base_gives_a_nan_result():
    s = sc.BY_NAME["real"]
    grid = sc._jax((17, 33))
    base = np.full(grid.shape, -18.0, np.float32)
    base[5:9, 10:20] = np.nan
    raw, _ = sn.volume(sc.images("real"), sc.ref_cameras(s), grid, base, -2.0, 2.0, 3, 2, 2)
    out = sn.later_level(raw, base, -2.0, 2.0, 0.125, 0.75)
    hole = np.isnan(base)
    assert np.isnan(out["altitude"][hole]).all() and (out["index"][hole] == -1).all() and np.isnan(raw[:, hole]).all()
    assert np.isfinite(out["altitude"][~hole]).any()
    assert same(out["altitude"], sn.lift(base, sg.pick(sg.aggregate(raw, 0.125, 0.75), raw, -2.0, 2.0)["altitude"]))
