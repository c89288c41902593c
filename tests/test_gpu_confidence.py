"""The confidence launch on the GPU (csrc/confidence.hip, spnerf_amd.confidence) — needs an MI355X.

Everything is held to the numpy statement (tests/confidence_numpy.py, itself pinned to closed forms on the CPU by
tests/test_confidence_ref.py) on the cases of tests/confidence_cases.py: K in 1, 2, 3, 5, 64, 65, 512 by 1, 63, 64,
65, 257 cells, whose first columns are the special cells — every plane NaN, one scored plane, the pick at plane 0
and at K − 1, ties, ±inf, a plateau at the top, a second peak inside and just outside ``exclude``, ``tau`` met and
missed by an fp32 ulp of best, an unscored neighbour of the pick — and whose other columns are random with 30 % NaN
within 4·temperature of the best; at three (tau, temperature, exclude), among them ``tau`` 0 and ``exclude`` = K.

* ``scored``, ``index``, ``margin``, ``peak_margin``, ``peaks``, ``support``, ``curvature``: equal bytes;
* ``mlm`` within 4 fp32 ulps of the fp64 statement, ``spread`` within 1e-5 relative plus 1e-5·step; the largest
  differences seen are printed (on an MI355X: mlm 0.500 ulps, the cast alone, and spread 5.9e-8 relative);
* ``index`` is ``sgm.pick``'s and ``sweep.pick_plane``'s where the volume holds no ±inf;
* a NULL output leaves its buffer untouched, and a subset of the planes has the bytes of the whole call;
* ``smooth_sweep(confidence=True)`` and ``bootstrap_sweep(weight="margin")`` on the box scene of tests/test_gpu_clean.py.
"""
import ctypes

import numpy as np
import pytest
import torch

import confidence_cases as cc
import confidence_numpy as cn
import occlusion_cases as occ
import sweep_cases as sc
from spnerf_amd import (_confidence_abi, _lib, bootstrap_sweep, clean_dsm, confidence, refine_sweep, sgm, smooth_sweep, sweep,
                        volume_confidence)
from test_gpu_parity import DEV

pytestmark = pytest.mark.gpu

F = np.float32
EXACT = ("scored", "index", "margin", "peak_margin", "peaks", "support", "curvature")
MLM_ULPS, SPREAD_REL, SPREAD_ABS = 4, 1e-5, 1e-5
_WANT = {}


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def dev(a):
    return torch.tensor(a, device=DEV)


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def want_of(K, cells, measure):
    """The statement's planes of one case, computed once."""
    key = (K, cells, measure)
    if key not in _WANT:
        _WANT[key] = cn.confidence(cc.volume(K, cells), cc.STEP, *measure)
    return _WANT[key]


def held(got, want, step, what):
    """The exact planes' bytes and the two fp64 planes' bounds; returns the largest differences (mlm in ulps, spread relative)."""
    for name in EXACT:
        assert same(got[name], want[name]), (what, name, np.flatnonzero(got[name].ravel().view(np.uint32) != want[name].ravel().view(np.uint32))[:8])
    nan = np.isnan(want["mlm64"])
    assert same(np.isnan(got["mlm"]), nan) and same(np.isnan(got["spread"]), nan), what
    assert same(got["mlm"][nan], want["mlm"][nan]) and same(got["spread"][nan], want["spread"][nan]), what    # the quiet NaN's bytes
    on = ~nan
    if not on.any():
        return 0.0, 0.0
    ulps = np.abs(got["mlm"][on].astype(np.float64) - want["mlm64"][on]) / np.spacing(np.abs(want["mlm64"][on]).astype(F)).astype(np.float64)
    diff = np.abs(got["spread"][on].astype(np.float64) - want["spread64"][on])
    rel = diff / np.maximum(want["spread64"][on], 1e-300)
    print(f"{what}: mlm off by at most {ulps.max():.3f} fp32 ulps, spread by {diff.max():.3e} m ({np.where(want['spread64'][on] > 0, rel, 0).max():.3e} relative)")
    assert ulps.max() <= MLM_ULPS, what
    assert (diff <= SPREAD_REL * want["spread64"][on] + SPREAD_ABS * step).all(), what
    assert (got["mlm"][on] > 0).all() and (got["mlm"][on] <= 1).all() and (got["spread"][on] >= 0).all()
    return float(ulps.max()), float(np.where(want["spread64"][on] > 0, rel, 0).max())


def launch(volume, measure, names=confidence.PLANES):
    """spnerf_conf_volume on a (K, cells) device tensor; a plane not in ``names`` gets NULL.  Returns the planes written."""
    K, cells = volume.shape
    tau, temperature, exclude = measure
    out = {n: torch.empty(cells, dtype=torch.int32 if kind == "int32" else torch.float32, device=DEV)
           for n, kind in _confidence_abi.CONF_OUTPUTS if n in names}
    _lib.check(_confidence_abi.lib().spnerf_conf_volume(_lib.ptr(volume), K, cells, -30.0, cc.STEP, tau, temperature, exclude,
                                                        *[_lib.ptr(out.get(n)) for n in confidence.PLANES], _lib.stream_of(volume)), "conf_volume")
    return out


@pytest.mark.parametrize("K", cc.PLANE_COUNTS)
def test_every_plane_is_the_statements(K):
    worst = (0.0, 0.0)
    for cells in cc.CELL_COUNTS:
        raw = cc.volume(K, cells)
        d = dev(raw)
        for measure in cc.measures(K):
            got = host(launch(d, measure))
            w = held(got, want_of(K, cells, measure), cc.STEP, f"K {K}, {cells} cells, tau/temperature/exclude {measure}")
            worst = (max(worst[0], w[0]), max(worst[1], w[1]))
        assert same(d.cpu().numpy(), raw)                                    # the volume is only read
        again = host(launch(d, cc.measures(K)[0]))                           # bit-reproducible
        first = host(launch(d, cc.measures(K)[0]))
        for name in again:
            assert same(again[name], first[name]), name
    print(f"K {K}: the largest differences: mlm {worst[0]:.3f} ulps, spread {worst[1]:.3e} relative")


def test_the_special_cells_are_what_they_are_named():
    K, cells = 64, 65
    measure = (cc.TAU_EXACT, cc.TEMPERATURE, 1)
    got = host(launch(dev(cc.volume(K, cells)), measure))
    name = cc.COLUMN
    c = name["all_nan"]
    assert (got["scored"][c], got["index"][c], got["peaks"][c], got["support"][c]) == (0, -1, 0, 0)
    assert all(got[n][c:c + 1].view(np.uint32)[0] == 0x7fc00000 for n in ("margin", "peak_margin", "curvature", "mlm", "spread"))
    c = name["one_scored"]
    assert (got["scored"][c], got["index"][c], got["peaks"][c], got["mlm"][c], got["spread"][c]) == (1, K // 2, 1, 1, 0) and np.isnan(got["margin"][c])
    assert got["index"][name["pick_at_bottom"]] == 0 and got["index"][name["pick_at_top"]] == K - 1
    c = name["flat"]
    assert (got["index"][c], got["support"][c], got["peaks"][c], got["margin"][c]) == (0, K, 1, 0) and abs(got["mlm"][c] - 1 / K) < 1e-8
    c = name["infinities"]
    assert (got["scored"][c], got["index"][c]) == (K - 2, K - 2) and np.isnan(got["curvature"][c])
    c = name["plateau"]
    assert (got["index"][c], got["peaks"][c], got["support"][c]) == (K // 3, 1, 3)
    met, missed = name["tau_met"], name["tau_missed"]
    assert (got["peaks"][met], got["support"][met], got["peaks"][missed], got["support"][missed]) == (2, 2, 1, 1)
    assert got["margin"][name["peak_inside"]] == F(0.9) - F(0.25) and got["margin"][name["peak_outside"]] == F(0.9) - F(0.85)
    c = name["equal_peaks"]
    assert (got["index"][c], got["margin"][c], got["peak_margin"][c], got["peaks"][c]) == (K // 4, 0, 0, 2)


def test_index_is_the_picks_index():
    for K, cells in ((5, 65), (64, 257), (512, 63)):
        raw = cc.volume(K, cells)
        raw[~np.isfinite(raw) & ~np.isnan(raw)] = np.nan                    # the picks take ±inf as a score
        vol = dev(raw.reshape(K, 1, cells))
        got = volume_confidence(vol, -30.0, cc.STEP, planes=("index",))
        assert sorted(got) == ["index"] and got["index"].dtype == torch.int32 and tuple(got["index"].shape) == (1, cells)
        assert same(got["index"].cpu().numpy(), sgm.pick(vol, vol, -30.0, cc.STEP)["index"].cpu().numpy())
        views = torch.zeros((K, 1, cells), dtype=torch.uint8, device=DEV)
        assert same(got["index"].cpu().numpy(), sweep.pick_plane(vol, views, -30.0, cc.STEP)["index"].cpu().numpy())


def test_a_grid_through_volume_confidence_and_its_subsets():
    K, (H, W) = 65, cc.GRID
    raw = cc.volume(K, H * W).reshape(K, H, W)
    measure = (confidence.TAU, confidence.TEMPERATURE, 1)
    want = cn.confidence(raw, cc.STEP, *measure)
    vol = dev(raw)
    got = volume_confidence(vol, -30.0, cc.STEP)                             # the defaults are this measure
    assert tuple(got) == confidence.PLANES and all(tuple(v.shape) == (H, W) and v.device == vol.device for v in got.values())
    assert all(got[n].dtype == (torch.int32 if kind == "int32" else torch.float32) for n, kind in _confidence_abi.CONF_OUTPUTS)
    got = host(got)
    held(got, want, cc.STEP, "16 x 17 grid")
    view = dev(np.ascontiguousarray(raw.transpose(0, 2, 1))).permute(0, 2, 1)  # a view that is not contiguous
    assert not view.is_contiguous()
    for name, plane in host(volume_confidence(view, -30.0, cc.STEP)).items():
        assert same(plane, got[name]), name
    # a subset is the same bytes whichever kernel variant it takes: no second pass, a second pass without exp, all
    for names in (("index",), ("scored", "curvature"), ("index", "margin"), ("peaks", "support"), ("peak_margin",), ("mlm",), ("spread", "scored")):
        part = host(volume_confidence(vol, -30.0, cc.STEP, planes=names))
        assert sorted(part) == sorted(names)
        for n in names:
            assert same(part[n], got[n]), (names, n)
    other = host(volume_confidence(vol, -30.0, cc.STEP, tau=0.0, temperature=0.02, exclude=3))
    held(other, cn.confidence(raw, cc.STEP, 0.0, 0.02, 3), cc.STEP, "16 x 17 grid, tau 0, temperature 0.02, exclude 3")


def test_null_outputs_leave_their_buffers_untouched():
    K, cells = 64, 257
    vol = dev(cc.volume(K, cells))
    measure = cc.measures(K)[0]
    whole = host(launch(vol, measure))
    # the nine buffers side by side with a guard cell around each: one allocation, the pointers taken by hand
    L = _confidence_abi.lib()
    for names in (("index", "margin"), ("scored",), ("spread",), ("peaks", "curvature", "mlm")):
        arena = torch.full((9, cells + 2), -7, dtype=torch.int32, device=DEV)
        ptrs = [ctypes.c_void_p(arena[i, 1:].data_ptr()) if n in names else None for i, n in enumerate(confidence.PLANES)]
        _lib.check(L.spnerf_conf_volume(_lib.ptr(vol), K, cells, -30.0, cc.STEP, *measure, *ptrs, _lib.stream_of(vol)), "conf_volume")
        a = arena.cpu().numpy()
        assert (a[:, 0] == -7).all() and (a[:, -1] == -7).all()
        for i, n in enumerate(confidence.PLANES):
            if n in names:
                assert a[i, 1:-1].tobytes() == whole[n].tobytes(), (names, n)
            else:
                assert (a[i] == -7).all(), (names, n)


def box():
    s = occ.BOX
    imgs, cams = [dev(im) for im in occ.box_images()], sc.cameras(s)
    return s, (imgs, cams, s.grid, s.alt_lo, s.step, s.planes), dict(radius=s.radius, min_views=s.min_views)


def test_smooth_sweep_with_confidence_keeps_its_planes():
    s, args, kw = box()
    plain = smooth_sweep(*args, volume=True, **kw)
    got = smooth_sweep(*args, volume=True, confidence=True, **kw)
    assert sorted(got) == sorted(list(plain) + ["confidence", "confidence_raw"])
    assert sorted(smooth_sweep(*args, confidence=True, **kw)) == ["altitude", "confidence", "confidence_raw", "index", "photo", "score"]
    for k in plain:
        assert same(got[k].cpu().numpy(), plain[k].cpu().numpy()), k
    for name, volume in (("confidence", plain["aggregated"]), ("confidence_raw", plain["volume"])):
        assert tuple(got[name]) == confidence.PLANES
        want = cn.confidence(volume.cpu().numpy(), s.step, confidence.TAU, confidence.TEMPERATURE, 1)
        held(host(got[name]), want, s.step, f"box, {name}")
    assert same(got["confidence"]["index"].cpu().numpy(), plain["index"].cpu().numpy())
    margin = got["confidence"]["margin"].cpu().numpy()
    print(f"box: the aggregated volume's margin: {np.isnan(margin).sum()} NaN of {margin.size}, median {np.nanmedian(margin):.4f}")


def test_bootstrap_sweep_by_margin_is_the_chain_called_by_hand():
    s, args, kw = box()
    first = smooth_sweep(*args, volume=True, **kw)
    margin = volume_confidence(first["aggregated"], s.alt_lo, s.step)["margin"]
    min_weight = float(np.nanmedian(margin.cpu().numpy()))                   # half of the cells with a margin are gated out
    cleaned = clean_dsm(first["altitude"], weight=margin, min_weight=min_weight, max_diff=s.step, max_size=30, radius=1, reach=4)
    want = refine_sweep(*args, prior=cleaned["dsm"], volume=True, **kw)
    out = bootstrap_sweep(*args, sweep_radius=s.radius, min_views=s.min_views, max_diff=s.step, max_size=30, radius=1, min_weight=min_weight, reach=4,
                          volume=True, weight="margin")
    assert sorted(out) == ["aggregated", "altitude", "cleaned", "first", "floor", "index", "photo", "prior", "score", "volume"]
    assert same(out["first"].cpu().numpy(), first["altitude"].cpu().numpy())
    for k in cleaned:
        assert same(out["cleaned"][k].cpu().numpy(), cleaned[k].cpu().numpy()), k
    for k in want:
        assert same(out[k].cpu().numpy(), want[k].cpu().numpy()), k
    rejected = cleaned["rejected"].cpu().numpy()
    assert (rejected & 1).any() and not (rejected & 1).all()
    # the gate is the margin's, not the photo's; and weight="photo" is what the call is without the argument
    by_photo = bootstrap_sweep(*args, sweep_radius=s.radius, min_views=s.min_views, max_diff=s.step, max_size=30, radius=1, min_weight=min_weight, reach=4)
    assert not same(by_photo["cleaned"]["rejected"].cpu().numpy(), rejected)
    named = bootstrap_sweep(*args, sweep_radius=s.radius, min_views=s.min_views, max_diff=s.step, max_size=30, radius=1, min_weight=min_weight, reach=4,
                            weight="photo")
    assert sorted(named) == sorted(by_photo)
    for k in ("altitude", "index", "score", "photo", "prior", "first"):
        assert same(named[k].cpu().numpy(), by_photo[k].cpu().numpy()), k
    for name in ("peak_margin", "curvature", "mlm"):
        gate = volume_confidence(first["aggregated"], s.alt_lo, s.step)[name]
        values = gate.cpu().numpy()
        values = values[np.isfinite(values)]
        level = float(np.median(values)) if values.size else 0.0            # a plane that is NaN everywhere (no rival on the box) gates every cell out
        print(f"box: {name}: {values.size} finite of {gate.numel()}, gated at {level!r}")
        out = bootstrap_sweep(*args, sweep_radius=s.radius, min_views=s.min_views, max_diff=s.step, max_size=30, radius=1, min_weight=level, weight=name)
        cleaned = clean_dsm(first["altitude"], weight=gate, min_weight=level, max_diff=s.step, max_size=30, radius=1)
        assert same(out["prior"].cpu().numpy(), cleaned["dsm"].cpu().numpy()), name
