"""spnerf_amd.dataset on the MI355X (csrc/dataset.hip) against what the reference's own
load_depth_data / load_semantic_data / init_scaling_params returned (tests/golden/dataset.npz) and,
where no fixture exists, against their numpy restatement (tests/dataset_numpy.py).

Bounds.  The GPU localises in fp64 like the restatement, but a last-bit difference of the fp64
ECEF may flip the fp32 rounding of an origin coordinate (0.5 m at 5.45e6 m), as in
test_rays.py: directions and far agree to atol 2e-7; origins differ by at most one quantum
0.5 / range (x 1.01), on at most max(2, K // 2000) rows.  A depth is a distance from the origin:
rtol 1e-6 where the origin matched, at most sqrt(3) quanta where it did not; the global factor
dmax - dmin of the std then moves by at most two of those."""
import functools

import numpy as np
import pytest
import torch

import dataset_numpy as dn
import golden_util as gu
from oracle import rpc_ref

pytestmark = pytest.mark.gpu
LOC_KEYS = ("X_scale", "X_offset", "Y_scale", "Y_offset", "Z_scale", "Z_offset")


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(f"{gu.GOLDEN}/dataset.npz") as z:
        f = {k: z[k] for k in z.files}
    for v in f.values():
        v.setflags(write=False)
    return f


def rpc_dict(packed):
    d = {k: float(v) for k, v in zip(rpc_ref.KEYS, packed[:10])}
    d.update(row_num=list(packed[10:30]), row_den=list(packed[30:50]), col_num=list(packed[50:70]),
             col_den=list(packed[70:90]))
    return d


def fixture_images(f):
    h, w = (int(v) for v in f["hw"])
    return [dict(rpc=rpc_dict(f[f"rpc_{i}"]), min_alt=float(f[f"alt_{i}"][0]), max_alt=float(f[f"alt_{i}"][1]), height=h,
                 width=w, pts2d=f[f"pts2d_{i}"], pts3d=f[f"pts3d_{i}"], correl=f[f"correl_{i}"]) for i in range(2)]


def check_planes(got, ref, K, rng):
    """got / ref: (deprays, depths, valid, std before the scale) as numpy arrays."""
    rays, depths, valid, std = got
    r_rays, r_depths, r_valid, r_std = ref
    quantum = 0.5 / float(rng)
    assert np.array_equal(valid, r_valid)
    on = r_valid > 0
    assert on.sum() == K
    assert np.array_equal(depths[:, 1], r_depths[:, 1], equal_nan=True)       # weights
    assert np.array_equal(std, r_std, equal_nan=True)                        # std before the global scale
    for plane in (rays, depths, std):
        assert not plane[~on].any()                                           # exactly zero off the keypoints
    np.testing.assert_allclose(rays[:, 3:], r_rays[:, 3:], rtol=0, atol=2e-7)
    diff = np.abs(rays[:, :3] - r_rays[:, :3])
    print("origin rows that differ:", int((diff > 0).any(1).sum()), "max", diff.max() / quantum, "quanta")
    assert diff.max() <= quantum * 1.01
    moved = (diff > 0).any(1)
    assert moved.sum() <= max(2, K // 2000), moved.sum()
    same = on & ~moved
    print("depth max abs diff:", np.abs(depths[same, 0] - r_depths[same, 0]).max())
    np.testing.assert_allclose(depths[same, 0], r_depths[same, 0], rtol=1e-6, atol=0)
    assert (np.abs(depths[moved, 0] - r_depths[moved, 0]) <= np.sqrt(3) * quantum * 1.01).all()


def test_depth_planes_match_the_reference():
    from spnerf_amd import dataset
    f = fixture()
    images = fixture_images(f)
    K = sum(len(im["pts2d"]) for im in images)
    kw = dict(center=f["center"], range=float(f["range"]), stdscale=float(f["stdscale"]), margin=float(f["margin"]))
    rays, depths, valid, std, drange = dataset.depth_planes(images, **kw)
    assert rays.shape == f["deprays"].shape and depths.shape == f["depths"].shape and valid.shape == f["valid_depth"].shape
    assert all(t.dtype == torch.float32 and t.is_cuda for t in (rays, depths, valid, std, drange))
    got = tuple(t.cpu().numpy() for t in (rays, depths, valid, std))
    check_planes(got, (f["deprays"], f["depths"], f["valid_depth"], f["std_pre"]), K, f["range"])

    # the two-image concatenation: ONE factor, the depth range over both images (:295)
    assert not np.array_equal(f["range_0"], f["range_1"])
    dmin, dmax = min(f["range_0"][0], f["range_1"][0]), max(f["range_0"][1], f["range_1"][1])
    on = got[2] > 0
    lo, hi = drange.cpu().numpy()
    assert lo == got[1][on, 0].min() and hi == got[1][on, 0].max()            # over both images, exactly
    slack = np.sqrt(3) * 0.5 / float(f["range"]) * 1.01
    assert abs(lo - dmin) <= slack and abs(hi - dmax) <= slack
    out = dataset.load_depth_data(images, **kw)
    for a, b in zip(out[:3], got[:3]):
        assert np.array_equal(a.cpu().numpy(), b)
    final = out[3].cpu().numpy()
    assert final.shape == f["depth_stds"].shape and final.dtype == np.float32
    assert np.array_equal(final, got[3] * np.float32(hi - lo))                # every row by the global factor
    n = int(f["hw"][0] * f["hw"][1])
    own = [np.float32(f[f"range_{i}"][1] - f[f"range_{i}"][0]) for i in range(2)]
    per_image = np.concatenate([got[3][i * n:(i + 1) * n] * own[i] for i in range(2)])
    assert not np.array_equal(final, per_image)                               # a per-image factor is another result
    eps = 2 * np.sqrt(3) * 0.5 / float(f["range"]) / float(dmax - dmin)
    ref = f["depth_stds"].astype(np.float64)
    assert (np.abs(final - ref) <= np.abs(ref) * eps).all()
    assert not final[~on].any()


@functools.lru_cache(maxsize=None)
def big_case():
    """300 x 260 pixels, ~60 % of them keypoints (183 blocks of 256): no fixture, the numpy restatement
    is the reference.  The correl minimum sits in the last block and the maximum in the first."""
    f = fixture()
    h, w = 300, 260
    rng = np.random.default_rng(11)
    flat = np.flatnonzero(rng.random(h * w) < 0.6)
    pts2d = np.stack([flat % w, flat // w], 1).astype(np.int64)
    k = len(flat)
    rpc = dn.rpc_of(f["rpc_0"])
    lo, hi = (float(v) for v in f["alt_0"])
    alt = rng.uniform(lo, hi, k)
    lon, lat = rpc.localization(pts2d[:, 0], pts2d[:, 1], alt)
    pts3d = (np.stack(rpc_ref.geodetic_to_ecef(lat, lon, alt), 1) + rng.normal(0, 0.3, (k, 3))).astype(np.float32)
    correl = rng.uniform(0.3, 1.0, k).astype(np.float32)
    correl[k - 3], correl[5] = 0.05, 1.25
    assert (k + 255) // 256 > 150 and (k - 3) // 256 == (k - 1) // 256
    im = dict(min_alt=lo, max_alt=hi, height=h, width=w, pts2d=pts2d, pts3d=pts3d, correl=correl)
    planes, (dmin, dmax) = dn.depth_image(rpc, lo, hi, h, w, pts2d, pts3d, correl, f["center"], f["range"], 0.7, 0.01)
    return im, planes, (dmin, dmax)


def test_depth_planes_across_many_blocks():
    from spnerf_amd import dataset
    f = fixture()
    im, ref, (dmin, dmax) = big_case()
    K = len(im["pts2d"])
    rays, depths, valid, std, drange = dataset.depth_planes([dict(im, rpc=rpc_dict(f["rpc_0"]))], center=f["center"],
                                                            range=float(f["range"]), stdscale=0.7, margin=0.01)
    got = tuple(t.cpu().numpy() for t in (rays, depths, valid, std))
    check_planes(got, (ref["deprays"], ref["depths"], ref["valid_depth"], ref["depth_std"]), K, f["range"])
    w = got[1][got[2] > 0, 1]
    assert w.min() == 0.0 and w.max() == 1.0                                  # the range came from both ends
    lo, hi = drange.cpu().numpy()
    assert lo == got[1][got[2] > 0, 0].min() and hi == got[1][got[2] > 0, 0].max()
    slack = np.sqrt(3) * 0.5 / float(f["range"]) * 1.01
    assert abs(lo - dmin) <= slack and abs(hi - dmax) <= slack


def test_constant_correl_gives_nan_weights():
    from spnerf_amd import dataset
    f = fixture()
    pts2d = np.array([(1, 0), (3, 1), (0, 2), (2, 2), (3, 3)], np.int64)
    rpc = dn.rpc_of(f["rpc_1"])
    lon, lat = rpc.localization(pts2d[:, 0], pts2d[:, 1], np.full(5, 3.0))
    pts3d = np.stack(rpc_ref.geodetic_to_ecef(lat, lon, np.full(5, 3.0)), 1).astype(np.float32)
    im = dict(rpc=rpc_dict(f["rpc_1"]), min_alt=float(f["alt_1"][0]), max_alt=float(f["alt_1"][1]), height=4, width=4,
              pts2d=pts2d, pts3d=pts3d, correl=np.full(5, 0.625, np.float32))
    rays, depths, valid, std = (t.cpu().numpy() for t in dataset.load_depth_data(
        [im], center=f["center"], range=float(f["range"]), stdscale=0.7, margin=0.01))
    on = np.zeros(16, bool)
    on[pts2d[:, 1] * 4 + pts2d[:, 0]] = True
    assert np.array_equal(valid, on.astype(np.float32))
    assert np.isnan(depths[on, 1]).all() and np.isnan(std[on]).all()
    assert np.isfinite(depths[on, 0]).all() and (depths[on, 0] >= 0).all() and np.isfinite(rays).all()
    assert not depths[~on].any() and not std[~on].any() and not rays[~on].any()


def test_get_rays_at_fractional_pixels():
    from spnerf_amd import satellite
    cams = satellite.load_cameras()
    meta = cams["images"]["JAX_269_011_RGB"]
    rng = np.random.default_rng(1)
    whole_c, whole_r = rng.integers(0, meta["width"] - 1, 300), rng.integers(0, meta["height"] - 1, 300)
    cols, rows = whole_c + 0.25, whole_r + 0.25
    rpc = satellite.RPCModel(meta["rpc"])
    got = satellite.get_rays(cols, rows, rpc, meta["min_alt"], meta["max_alt"]).cpu().numpy()
    ref = rpc_ref.get_rays(cols, rows, rpc_ref.RPC(meta["rpc"]), meta["min_alt"], meta["max_alt"])
    np.testing.assert_allclose(got[:, 3:], ref[:, 3:], rtol=1e-6, atol=1e-7)
    assert np.abs(got[:, :3] - ref[:, :3]).max() <= 1.0   # ECEF metres: at most one fp32 quantum (0.5 m)
    at_whole = rpc_ref.get_rays(whole_c.astype(float), whole_r.astype(float), rpc_ref.RPC(meta["rpc"]), meta["min_alt"],
                                meta["max_alt"])
    assert np.abs(ref[:, 3:6] - at_whole[:, 3:6]).max() > 0   # a quarter pixel is another ray
    as_int = satellite.get_rays(whole_c, whole_r, rpc, meta["min_alt"], meta["max_alt"])
    as_float = satellite.get_rays(whole_c.astype(np.float64), whole_r.astype(np.float32), rpc, meta["min_alt"],
                                  meta["max_alt"])
    assert torch.equal(as_int, as_float)


def torch_bounds(meta, ds, device="cuda"):
    """min / max over the near and far points of the rays satellite.get_rays stores."""
    from spnerf_amd import satellite
    h, w = int(meta["height"] // ds), int(meta["width"] // ds)
    rows, cols = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    rpc = satellite.rescale_rpc(satellite.RPCModel(meta["rpc"]), 1.0 / ds)
    rays = satellite.get_rays(cols.reshape(-1), rows.reshape(-1), rpc, meta["min_alt"], meta["max_alt"], device=device)
    far_pt = rays[:, :3] + rays[:, 7:8] * rays[:, 3:6]
    pts = torch.cat([rays[:, :3], far_pt], 0)
    return torch.cat([pts.min(0).values, pts.max(0).values])


def test_scene_bounds_and_scaling_params():
    from spnerf_amd import dataset
    f = fixture()
    metas = [dict(rpc=rpc_dict(f[f"rpc_{i}"]), min_alt=float(f[f"alt_{i}"][0]), max_alt=float(f[f"alt_{i}"][1]),
                  height=int(f["loc_hw"][i][0]), width=int(f["loc_hw"][i][1])) for i in range(2)]
    each = [torch_bounds(m, 8.0) for m in metas]
    for m, ref in zip(metas, each):
        got = dataset.scene_bounds([m], 8.0)
        assert got.dtype == torch.float32 and got.shape == (6,)
        assert torch.equal(got, ref), (got, ref)
    both = dataset.scene_bounds(metas, 8.0)
    assert torch.equal(both, torch.cat([torch.minimum(each[0][:3], each[1][:3]), torch.maximum(each[0][3:], each[1][3:])]))
    assert not torch.equal(both, each[0]) and not torch.equal(both, each[1])
    # an odd rectangle that ends inside a wave, at another scale
    small = dict(metas[1], height=67, width=131)
    assert torch.equal(dataset.scene_bounds([small], 1.0), torch_bounds(small, 1.0))
    loc = dataset.init_scaling_params(metas, img_downscale=8.0)
    assert sorted(loc) == sorted(LOC_KEYS)
    assert all(type(v) is float for v in loc.values())
    for k, ref in zip(LOC_KEYS, f["loc"]):
        assert abs(loc[k] - ref) <= 0.5, (k, loc[k], ref)
    b = both.cpu().numpy()
    for j, axis in enumerate("XYZ"):                                          # float32 arithmetic of rpc_scaling_params
        scale = (b[3 + j] - b[j]) / np.float32(2)
        assert loc[f"{axis}_scale"] == float(scale) and loc[f"{axis}_offset"] == float(b[j] + scale)


@pytest.mark.parametrize("mode", ["sparse", "dense"])
@pytest.mark.parametrize("sd", [8, 3])
def test_semantics_match_the_reference(mode, sd):
    from spnerf_amd import dataset
    f = fixture()
    h, w = (int(v) for v in f["hw"])
    mapping = {int(k): int(v) for k, v in f["sem_map"]}
    metas = [dict(height=h, width=w)] * 2
    for raster in (f["sem_raster"], f["sem_raster"].astype(np.int32), torch.tensor(f["sem_raster"], device="cuda")):
        labels, valid = dataset.load_semantic_data(raster, metas, mapping, dense_ss=mode == "dense", sem_downscale=sd)
        assert labels.dtype == torch.int64 and valid.dtype == torch.float32 and labels.is_cuda and valid.is_cuda
        assert labels.shape == (2 * h * w, 1) and valid.shape == (2 * h * w,)
        assert np.array_equal(labels.cpu().numpy(), f[f"sem_{mode}_{sd}_labels"])
        assert np.array_equal(valid.cpu().numpy(), f[f"sem_{mode}_{sd}_valid"])


def test_semantics_edge_shapes():
    from spnerf_amd import dataset
    mapping = {2: 0, 5: 1, 6: 2, 9: 3, 17: 4}
    rng = np.random.default_rng(5)
    cases = [(np.array([[6]], np.uint8), (5, 7), 1, (False, True)),           # a 1 x 1 source
             (np.array([[65]], np.uint8), (3, 3), 1, (False, True)),          # ... of an unmapped code
             (rng.choice(np.array([2, 5, 6, 9, 17, 65], np.uint8), (37, 45)), (11, 9), 3, (False, True)),   # target < source
             (rng.choice(np.array([2, 5, 6, 9, 17, 65], np.uint8), (301, 517)), (127, 300), 8, (False, True)),
             (rng.choice(np.array([2, 300, -4, 9], np.int32), (16, 16)), (16, 32), 2, (False, True))]      # codes outside the table
    for raster, (h, w), sd, modes in cases:
        for dense in modes:
            labels, valid = dataset.load_semantic_data(raster, [dict(height=h, width=w)], mapping, dense_ss=dense,
                                                       sem_downscale=sd)
            r_labels, r_valid = dn.load_semantic_data(raster, [dict(height=h, width=w)], mapping, dense, sd)
            assert np.array_equal(labels.cpu().numpy(), r_labels), (raster.shape, h, w, sd, dense)
            assert np.array_equal(valid.cpu().numpy(), r_valid), (raster.shape, h, w, sd, dense)
    # the default sem_downscale is the reference argument's 8
    raster = cases[3][0]
    a = dataset.load_semantic_data(raster, [dict(height=64, width=64)], mapping)
    b = dataset.load_semantic_data(raster, [dict(height=64, width=64)], mapping, sem_downscale=8)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[1].sum() == (a[0] != -100).sum() > 0
