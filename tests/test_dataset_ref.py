"""The numpy restatement of the dataset construction (tests/dataset_numpy.py) against what the
reference's own load_depth_data / load_semantic_data / init_scaling_params returned
(tests/golden/dataset.npz, made by tests/golden/gen_dataset_golden.py).  CPU only."""
import numpy as np
import pytest

import dataset_numpy as dn
import golden_util as gu

LOC_KEYS = ("X_scale", "X_offset", "Y_scale", "Y_offset", "Z_scale", "Z_offset")


def fixture():
    with np.load(f"{gu.GOLDEN}/dataset.npz") as z:
        return {k: z[k] for k in z.files}


def images_of(f):
    h, w = (int(v) for v in f["hw"])
    return [dict(rpc=dn.rpc_of(f[f"rpc_{i}"]), min_alt=f[f"alt_{i}"][0], max_alt=f[f"alt_{i}"][1], height=h, width=w,
                 pts2d=f[f"pts2d_{i}"], pts3d=f[f"pts3d_{i}"], correl=f[f"correl_{i}"]) for i in range(2)]


def test_fixture_is_what_the_issue_asks_for():
    f = fixture()
    h, w = (int(v) for v in f["hw"])
    assert (h, w) == (40, 56)
    for i in range(2):
        flat = f[f"pts2d_{i}"][:, 1] * w + f[f"pts2d_{i}"][:, 0]
        assert (np.diff(flat) > 0).all() and flat[0] == 0 and flat[-1] == h * w - 1
        assert 1000 < flat.size < h * w                      # the real pattern has holes
    assert not np.array_equal(f["range_0"], f["range_1"])     # per-image scaling would be visible
    assert set(np.unique(f["sem_raster"])) == {2, 5, 6, 9, 17, 65}


def test_depth_planes_are_bit_equal():
    f = fixture()
    rays, depths, valid, stds, (lo, hi) = dn.load_depth_data(images_of(f), f["center"], f["range"],
                                                             float(f["stdscale"]), float(f["margin"]))
    assert rays.shape == f["deprays"].shape and rays.dtype == f["deprays"].dtype == np.float32
    assert depths.shape == f["depths"].shape and stds.shape == f["depth_stds"].shape == valid.shape
    assert np.array_equal(valid, f["valid_depth"])
    assert np.array_equal(depths[:, 1], f["depths"][:, 1])                 # weights
    assert np.array_equal(rays, f["deprays"])
    assert np.array_equal(depths[:, 0], f["depths"][:, 0])
    assert (lo, hi) == (min(f["range_0"][0], f["range_1"][0]), max(f["range_0"][1], f["range_1"][1]))
    assert np.array_equal(stds, f["depth_stds"])
    # the std planes before the global scale, as the reference padded them
    n = int(f["hw"][0] * f["hw"][1])
    for i, im in enumerate(images_of(f)):
        planes, _ = dn.depth_image(im["rpc"], im["min_alt"], im["max_alt"], im["height"], im["width"], im["pts2d"],
                                   im["pts3d"], im["correl"], f["center"], f["range"], float(f["stdscale"]),
                                   float(f["margin"]))
        assert np.array_equal(planes["depth_std"], f["std_pre"][i * n:(i + 1) * n])
        assert (planes["depth_std"][f["valid_depth"][i * n:(i + 1) * n] == 0] == 0).all()


@pytest.mark.parametrize("mode", ["sparse", "dense"])
@pytest.mark.parametrize("sd", [8, 3])
def test_semantics_are_bit_equal(mode, sd):
    f = fixture()
    h, w = (int(v) for v in f["hw"])
    mapping = {int(k): int(v) for k, v in f["sem_map"]}
    labels, valid = dn.load_semantic_data(f["sem_raster"], [dict(height=h, width=w)] * 2, mapping, mode == "dense", sd)
    assert labels.dtype == np.int64 and labels.shape == f[f"sem_{mode}_{sd}_labels"].shape
    assert np.array_equal(labels, f[f"sem_{mode}_{sd}_labels"])
    assert valid.dtype == np.float32 and np.array_equal(valid, f[f"sem_{mode}_{sd}_valid"])
    assert 0 < valid.sum() < valid.size


def test_scene_scaling_is_bit_equal():
    f = fixture()
    pts = [dn.scene_points(dn.rpc_of(f[f"rpc_{i}"], 8.0), f[f"alt_{i}"][0], f[f"alt_{i}"][1],
                           int(f["loc_hw"][i][0] // 8), int(f["loc_hw"][i][1] // 8)) for i in range(2)]
    loc = dn.scaling_params(np.concatenate(pts, 0))
    assert all(isinstance(loc[k], np.float32) for k in LOC_KEYS)
    assert np.array_equal(np.array([loc[k] for k in LOC_KEYS], np.float64), f["loc"])


@pytest.mark.parametrize("n_in,n_out", [(37, 40), (45, 56), (37, 4), (45, 15), (4, 40), (15, 56), (1, 7), (301, 127),
                                        (517, 300), (64, 64), (16, 32), (5616, 702)])
def test_nearest_index_is_torch_interpolate(n_in, n_out):
    """The index rule the restatement (and the kernel) uses against F.interpolate(mode='nearest')."""
    import torch
    import torch.nn.functional as F
    src = torch.arange(n_in, dtype=torch.float32).view(1, 1, 1, n_in).expand(1, 1, 2, n_in).contiguous()
    got = F.interpolate(src, size=(2, n_out), mode="nearest")[0, 0, 0].long().numpy()
    assert np.array_equal(dn.nearest_index(n_out, n_in), got)
