"""DSM registration on the GPU (csrc/dsm_register.hip via spnerf_amd.dsm) against what the
reference's modules/dsmr.py computed (tests/golden/dsmr.npz) and, at the shapes where the tiling
can go wrong, against the numpy restatement (tests/dsmr_numpy.py) — needs an MI355X.

Tolerances.  Correlations and moments: 1e-9 — fp64 sums of at most 2^16 terms grow by at most
n·eps ≈ 7e-12 relative, times the raw-moment cancellation factor (mu² + sigma²) / sigma² ≈ 30 of
these altitudes (smaller still after the pivot).  MAE: 1e-5 m — the reference rounds the shifted
DSM to float32 (half an ulp below 32 m: 1.9e-6 m per pixel) and averages in float32.
Measured on an MI355X (the tests print these, `pytest -s`): NCC tables within
2.3e-14 / 2.6e-14 / 1.1e-15 of the reference's for cases a / b / c, moments within 3.1e-15
relative, a and b within 3.4e-14; MAE within 3.7e-9 / 3.6e-9 / 4.5e-8 m of the reference's.
"""
import functools
import os

import numpy as np
import pytest
import torch

import dsmr_numpy as dn

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ("a", "b", "c")


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(os.path.join(HERE, "dsmr.npz")) as z:
        return {k: z[k] for k in z.files}


def dev(a):
    return torch.tensor(np.asarray(a, np.float64), device=DEV)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.abs(b)))


def tables_of(reg):
    """(levels, side, side) correlations and (levels, 2) shifts of a registration, finest first."""
    t = reg.tables.cpu().numpy()
    side = 2 * reg.irange + 1
    return t[:, :side * side].reshape(-1, side, side), t[:, side * side:].astype(np.int64)


def bits(t):
    return t.contiguous().view(torch.uint8).cpu().numpy().tobytes()


@pytest.mark.parametrize("case", CASES)
def test_compute_shift_matches_reference(case):
    from spnerf_amd import dsm
    g = golden()
    u, v = g[f"{case}_u"], g[f"{case}_v"]
    reg = dsm.register_dsm(u, v, tables=True)
    tab, shifts = tables_of(reg)
    assert np.array_equal(shifts, g[f"{case}_shifts"])          # every level, exactly
    ref = g[f"{case}_tables"]
    assert np.array_equal(np.isnan(tab), np.isnan(ref))
    d_tab = float(np.nanmax(np.abs(tab - ref)))
    gm = g[f"{case}_moments"]
    got = [reg.muu, reg.muv, reg.sigu, reg.sigv, reg.xcorr]
    d_mom = rel(got, gm[:5])
    sc = dsm.compute_shift(u, v, scaling=True)
    pl = dsm.compute_shift(dev(u), dev(v), scaling=False)       # device tensors as well as arrays
    gs, gp = g[f"{case}_shift_scaled"], g[f"{case}_shift_plain"]
    d_ab = max(rel(sc[2:], gs[2:]), rel(pl[3], gp[3]))
    print(f"case {case}: max |ncc - ref| {d_tab:.3e}, moments rel {d_mom:.3e}, a, b rel {d_ab:.3e}")
    assert d_tab <= 1e-9 and d_mom <= 1e-9 and d_ab <= 1e-9
    assert reg.count == gm[5] and (reg.dx, reg.dy) == tuple(g[f"{case}_shifts"][0])
    assert sc[:2] == (gs[0], gs[1]) and pl[:3] == (gp[0], gp[1], 1.0)


def test_two_calls_are_bit_equal():
    from spnerf_amd import dsm
    g = golden()
    u, v = dev(g["b_u"]), dev(g["b_v"])
    a = dsm.register_dsm(u, v, tables=True)
    b = dsm.register_dsm(u, v, tables=True)
    assert bits(a.tables) == bits(b.tables) and bits(a.device_result) == bits(b.device_result)
    s1 = torch.empty(514, dtype=torch.float64, device=DEV)
    s2 = torch.empty(514, dtype=torch.float64, device=DEV)
    dsm._apply(v, reg=a.device_result, ref=u, sums=s1)
    dsm._apply(v, reg=b.device_result, ref=u, sums=s2)
    assert bits(s1[:2]) == bits(s2[:2])


@pytest.mark.parametrize("case", CASES)
def test_down2x_apply_shift_and_mae_match_reference(case):
    from spnerf_amd import dsm
    g = golden()
    u, v = g[f"{case}_u"], g[f"{case}_v"]
    assert np.array_equal(dsm.downsample2x(u.astype(np.float64)), g[f"{case}_down"], equal_nan=True)   # bit for bit
    gp = g[f"{case}_shift_plain"]
    out = dsm.apply_shift(v, int(gp[0]), int(gp[1]), gp[2], gp[3])
    assert out.dtype == np.float64
    assert np.array_equal(out.astype(np.float32), g[f"{case}_applied"], equal_nan=True)
    gs = g[f"{case}_shift_scaled"]
    out = dsm.apply_shift(dev(v), int(gs[0]), int(gs[1]), gs[2], gs[3])
    assert out.is_cuda and np.array_equal(
        out.cpu().numpy(), dn.apply_shift(v, int(gs[0]), int(gs[1]), gs[2], gs[3]), equal_nan=True)
    mae = dsm.dsm_mae(v, u, register="ncc")
    print(f"case {case}: MAE {mae:.9f}, reference {float(g[f'{case}_mae']):.9f}, "
          f"difference {abs(mae - float(g[f'{case}_mae'])):.3e}")
    assert abs(mae - float(g[f"{case}_mae"])) <= 1e-5
    # the error map: registered(pred) - gt; the reference's is float32 (half an ulp below 32 m
    # on the shifted image, as much again on the difference: 4e-6 m)
    err = dsm.dsm_pointwise_diff(v, u)
    ref = g[f"{case}_applied"].astype(np.float64) - u
    assert np.array_equal(np.isnan(err), np.isnan(ref)) and np.nanmax(np.abs(err - ref)) <= 4e-6
    with np.errstate(invalid="ignore"):
        assert abs(float(np.nanmean(np.abs(err))) - mae) <= 1e-12


def test_register_z_is_todays_result_and_water_is_masked():
    from oracle import dsm_ref
    from spnerf_amd import dsm
    g = golden()
    u, v = g["a_u"].astype(np.float64), g["a_v"].astype(np.float64)
    assert dsm.dsm_mae(v, u, register="z") == dsm.dsm_mae(v, u) == dsm_ref.dsm_mae(v, u)
    assert np.array_equal(dsm.dsm_pointwise_diff(v, u, register="z"), (v + np.nanmean(u - v)) - u, equal_nan=True)
    mask = np.zeros(u.shape, np.uint8)
    mask[10:30, 50:90] = 9
    masked = v.copy()
    masked[mask == 9] = np.nan
    assert np.array_equal(dsm.dsm_pointwise_diff(v, u, gt_mask=mask), dsm.dsm_pointwise_diff(masked, u), equal_nan=True)
    assert np.isnan(dsm.dsm_pointwise_diff(v, u, gt_mask=mask)).sum() > np.isnan(dsm.dsm_pointwise_diff(v, u)).sum()
    with pytest.raises(ValueError):
        dsm.compute_shift(u, v[:-1])
    with pytest.raises(ValueError):
        dsm.dsm_mae(v[:, 1:], u, register="ncc")


def test_tiff_paths_are_read(tmp_path):
    from PIL import Image
    from spnerf_amd import dsm
    g = golden()
    for k in ("c_u", "c_v"):
        Image.fromarray(g[k]).save(tmp_path / f"{k}.tif")
    assert dsm.compute_shift(str(tmp_path / "c_u.tif"), str(tmp_path / "c_v.tif"), scaling=False) == \
        dsm.compute_shift(g["c_u"], g["c_v"], scaling=False)


# ---- the shapes at which the tiling can go wrong, against the numpy restatement ----------------

def pair(h, w, shift, seed, holes=0.05):
    """u and v cut from one smooth random field so that u[j, i] = v[j + dy, i + dx] up to noise."""
    rng = np.random.default_rng(seed)
    dx, dy = shift
    m = 24
    yy, xx = np.mgrid[0:h + 2 * m, 0:w + 2 * m].astype(np.float64)
    base = 0.3 * rng.standard_normal(yy.shape)
    for _ in range(6):
        fx, fy, ph = rng.uniform(-0.35, 0.35), rng.uniform(-0.35, 0.35), rng.uniform(0, 6.28)
        base += rng.uniform(0.5, 2.0) * np.sin(fx * xx + fy * yy + ph)
    u = base[m:m + h, m:m + w] + 40.0
    v = base[m - dy:m - dy + h, m - dx:m - dx + w] + 37.5 + 0.01 * rng.standard_normal((h, w))
    u[rng.random(u.shape) < holes] = np.nan
    v[rng.random(v.shape) < holes] = np.inf          # non-finite, not only NaN
    return u, v


SHAPES = [
    # h, w, true shift, irange, initial shift
    (1, 1, (0, 0), 5, (0, 0)),
    (3, 200, (3, 1), 5, (0, 0)),            # narrower than irange
    (33, 31, (-2, 3), 5, (0, 0)),           # one pixel more / less than a tile
    (31, 33, (4, -5), 5, (0, 0)),
    (32, 64, (1, 1), 5, (0, 0)),            # whole tiles
    (65, 97, (-5, 5), 5, (0, 0)),           # several tiles, ragged edges
    (101, 100, (3, -2), 5, (0, 0)),         # must not recurse
    (101, 101, (3, -2), 5, (0, 0)),         # must
    (70, 45, (1, -1), 0, (1, -1)),          # a single shift
    (70, 45, (-2, 2), 2, (0, 0)),
    (120, 104, (-9, 7), 2, (-9, 7)),        # dx // 2 floors a negative initial shift
    (60, 60, (6, 9), 3, (5, 7)),            # the window is centred on the initial shift
]


@pytest.mark.parametrize("h,w,shift,irange,init", SHAPES)
def test_tile_edges_match_numpy(h, w, shift, irange, init):
    from spnerf_amd import dsm
    u, v = pair(h, w, shift, seed=h * 1000 + w, holes=0.05 if h * w > 1 else 0.0)
    trace = []
    dx, dy, a, b, m = dn.compute_shift(u, v, True, irange, init[0], init[1], trace)
    trace = trace[::-1]
    reg = dsm.register_dsm(u, v, irange=irange, init=init, tables=True)
    assert dsm.pyramid_levels(h, w) == len(trace) == reg.tables.shape[0]
    assert len(trace) == (2 if min(h, w) > 100 else 1)
    tab, shifts = tables_of(reg)
    for lv, (ldx, ldy, ref) in enumerate(trace):
        assert np.array_equal(np.isnan(tab[lv]), np.isnan(ref)), lv
        if np.isfinite(ref).any():
            assert np.nanmax(np.abs(tab[lv] - ref)) <= 1e-9, lv
        assert tuple(shifts[lv]) == (ldx, ldy), lv
    assert (reg.dx, reg.dy, reg.count) == (dx, dy, m[5])
    if h * w > 1:
        assert (dx, dy) == shift
        assert rel([reg.muu, reg.muv, reg.sigu, reg.sigv, reg.xcorr], m[:5]) <= 1e-9
        ga = reg.transform(True)
        assert rel(ga[2:], [a, b]) <= 1e-9
    else:       # one pixel: zero deviation, every correlation 0 / 0, the centre stands
        assert (reg.muu, reg.muv, reg.sigu, reg.sigv, reg.xcorr) == (m[0], m[1], 0.0, 0.0, 0.0)
    # the fused shift, error map and sums at this shape
    out = dsm.apply_shift(v, dx, dy, a, b)
    assert np.array_equal(out, dn.apply_shift(v, dx, dy, a, b), equal_nan=True)
    assert np.array_equal(dsm.downsample2x(u), dn.down2x(u), equal_nan=True)
    err = dn.apply_shift(v, dx, dy, 1.0, m[0] - m[1]) - u
    ok = np.isfinite(err)
    want = np.abs(err[ok]).mean() if ok.any() else float("nan")
    got = dsm.dsm_mae(v, u, register="ncc") if init == (0, 0) else None
    if got is not None:
        assert (np.isnan(got) and np.isnan(want)) or abs(got - want) <= 1e-9 * max(1.0, want)


def test_all_nan_image_keeps_the_centre():
    from spnerf_amd import dsm
    u, _ = pair(101, 101, (0, 0), seed=7)
    v = np.full_like(u, np.nan)
    reg = dsm.register_dsm(u, v, tables=True)
    assert (reg.dx, reg.dy, reg.count) == (0, 0, 0)
    assert all(np.isnan(x) for x in (reg.muu, reg.muv, reg.sigu, reg.sigv, reg.xcorr))
    assert np.isnan(tables_of(reg)[0]).all() and not tables_of(reg)[1].any()
    dx, dy, a, b = dsm.compute_shift(u, v)
    assert (dx, dy) == (0, 0) and np.isnan(a) and np.isnan(b)
    reg = dsm.register_dsm(u, v, init=(-3, 5))
    assert (reg.dx, reg.dy) == (-4, 4)                       # (-3 // 2) * 2, (5 // 2) * 2
    assert np.isnan(dsm.dsm_mae(v, u, register="ncc"))


def test_end_to_end_rolled_dsm_registers_back(tmp_path):
    """The DSM test_gpu_dsm.py's recipe rasterises from the lidar truth, rolled by (3, -2) cells:
    pred[j, i] = dsm[j + 2, i - 3], so pixel (j, i) of the truth meets pixel (j - 2, i + 3) of the
    prediction and the shift comes back as (dx, dy) = (3, -2) in the reference's convention
    (u[j, i] pairs with v[j + dy, i + dx]).  Registered, its MAE is below the Z-only one."""
    from spnerf_amd import dsm
    d = np.load(os.path.join(HERE, "dsm_truth.npz"))
    roi = tmp_path / "roi.txt"
    np.savetxt(roi, d["roi"])
    out = dsm.get_dsm_from_nerf_prediction(torch.tensor(d["rays"], device=DEV), torch.tensor(d["depth"], device=DEV),
                                           d["center"], d["range"], roi_txt=str(roi))[:, :, 0]
    gt = d["gt"].astype(np.float64)
    pred = np.roll(out, (-2, 3), axis=(0, 1))
    dx, dy, a, b = dsm.compute_shift(gt, pred, scaling=False)
    assert (dx, dy, a) == (3, -2, 1.0)
    ncc, z = dsm.dsm_mae(pred, gt, register="ncc"), dsm.dsm_mae(pred, gt, register="z")
    print(f"rolled DSM: MAE registered {ncc:.4f} m, Z only {z:.4f} m, unrolled {dsm.dsm_mae(out, gt):.4f} m")
    assert ncc < z
