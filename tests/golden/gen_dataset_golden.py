"""Generate tests/golden/dataset.npz by running the REFERENCE's own dataset construction
(datasets/satellite_scene.py load_depth_data :223-297, load_semantic_data :299-389,
init_scaling_params :391-413) on inputs this script writes into a temporary directory.
CPU only, under a minute:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_dataset_golden.py [--ref /root/reference]

The reference's I/O-only imports (rasterio, rpcm, torchvision, ...) are MagicMock modules as in
gen_golden.py::rpc_rays; ``rpcm.RPCModel`` is the numpy restatement oracle/rpc_ref.RPC,
``rasterio.open`` hands back the label raster this script made, and ``write_dict_to_json`` is
captured instead of written (json cannot serialise the numpy float32 values of scene.loc).  The
methods run on an instance made without ``__init__``.  Only data is stored:

    center, range                       float32: the scene normalisation (the shipped scene.loc)
    stdscale, margin                    float64
    rpc_<i>, alt_<i>                    float64 (90,), (2,) [min_alt, max_alt]: the two cameras
    hw                                  int64 (2,): height, width of the depth / semantic targets
    pts2d_<i>, pts3d_<i>, correl_<i>    int64 (K, 2) [col, row], float32 (K, 3), float32 (K,)
    deprays, depths, valid_depth, depth_stds     what load_depth_data returns for both images
    std_pre                             float32: the padded std planes before the global scale (:278)
    range_<i>                           float32 (2,): depth min, max of image i alone
    sem_raster, sem_map                 uint8 (37, 45); int64 (5, 2) [original, mapped]
    sem_<mode>_<sd>_labels / _valid     what load_semantic_data returns (mode sparse / dense)
    loc_keys order X_scale X_offset Y_scale Y_offset Z_scale Z_offset:
    loc                                 float64 (6,): init_scaling_params at img_downscale 8
    loc_hw                              int64 (2, 2): the cameras' real sizes
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
from unittest import mock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import rpc_ref  # noqa: E402

IMAGES = ("JAX_269_006_RGB", "JAX_269_007_RGB")
H, W = 40, 56
WINDOWS = ((150, 260), (170, 290))           # (row0, col0) of the 40 x 56 keypoint window per image (~57 % set)
STDSCALE, MARGIN = 0.7, 0.01
SEM_CODES = (2, 5, 6, 9, 17, 65)             # the five mapped DFC2019 classes and one unmapped code
LOC_KEYS = ("X_scale", "X_offset", "Y_scale", "Y_offset", "Z_scale", "Z_offset")


def load_reference(ref: str):
    stubs = ["rasterio", "rpcm", "torchvision", "torchvision.transforms", "cv2", "pyproj", "utm", "osgeo", "gdal",
             "plyflatten", "kornia", "kornia.losses", "srtm4", "numba", "lpips", "PIL", "PIL.Image"]
    saved = {k: sys.modules.get(k) for k in stubs}
    for k in stubs:
        sys.modules[k] = mock.MagicMock()
    sys.path.insert(0, ref)
    sys.dont_write_bytecode = True
    try:
        import datasets.satellite_scene as ss
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    ss.rpcm.RPCModel = lambda d, dict_format="rpcm": rpc_ref.RPC(d)
    return ss


def packed_rpc(d):
    return np.array([d[k] for k in rpc_ref.KEYS] + list(d["row_num"]) + list(d["row_den"]) + list(d["col_num"])
                    + list(d["col_den"]), np.float64)


def window_keypoints(path, row0, col0):
    """The real (col, row) keypoints inside the window, shifted to the origin, with the two corner
    pixels added, in row-major order."""
    p = np.loadtxt(path, dtype="int").reshape(-1, 2)
    sel = (p[:, 1] >= row0) & (p[:, 1] < row0 + H) & (p[:, 0] >= col0) & (p[:, 0] < col0 + W)
    flat = (p[sel, 1] - row0) * W + (p[sel, 0] - col0)
    flat = np.unique(np.concatenate([flat, [0, H * W - 1]]))
    return np.stack([flat % W, flat // W], 1).astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    a = ap.parse_args()
    ss = load_reference(a.ref)
    jdir = os.path.join(a.ref, "Dataset", "DFC2019_269", "JSON")
    ddir = os.path.join(a.ref, "Dataset", "DFC2019_269", "Depth")
    loc = json.load(open(os.path.join(jdir, "scene.loc")))
    center = torch.tensor([float(loc["X_offset"]), float(loc["Y_offset"]), float(loc["Z_offset"])])
    rng_t = torch.max(torch.tensor([float(loc["X_scale"]), float(loc["Y_scale"]), float(loc["Z_scale"])]))
    out = {"center": center.numpy(), "range": np.array(rng_t.item(), np.float32),
           "stdscale": np.float64(STDSCALE), "margin": np.float64(MARGIN), "hw": np.array([H, W], np.int64)}

    ds = ss.SatelliteSceneDataset.__new__(ss.SatelliteSceneDataset)
    ds.center, ds.range = center, rng_t
    ds.img_downscale, ds.stdscale, ds.margin = 1.0, STDSCALE, MARGIN
    rng = np.random.default_rng(269)

    with tempfile.TemporaryDirectory() as tmp:
        small, full, loc_hw = [], [], []
        os.makedirs(os.path.join(tmp, "full"))
        for i, (img, (row0, col0)) in enumerate(zip(IMAGES, WINDOWS)):
            d = json.load(open(os.path.join(jdir, img + ".json")))
            loc_hw.append([d["height"], d["width"]])
            full.append(os.path.join(tmp, "full", img + ".json"))
            json.dump(d, open(full[-1], "w"))
            d = dict(d, height=H, width=W)
            small.append(os.path.join(tmp, img + ".json"))
            json.dump(d, open(small[-1], "w"))
            pts2d = window_keypoints(os.path.join(ddir, f"{img}_2DPts.txt"), row0, col0)
            k = pts2d.shape[0]
            rpc = rpc_ref.RPC(d["rpc"])
            alt = rng.uniform(float(d["min_alt"]), float(d["max_alt"]), k)
            lon, lat = rpc.localization(pts2d[:, 0], pts2d[:, 1], alt)
            pts3d = np.stack(rpc_ref.geodetic_to_ecef(lat, lon, alt), 1) + rng.normal(0.0, 0.3, (k, 3))
            pts3d = pts3d.astype(np.float32)
            correl = rng.uniform(0.3, 1.0, k).astype(np.float32)
            np.savetxt(os.path.join(tmp, f"{img}_2DPts.txt"), pts2d, fmt="%d")
            np.savetxt(os.path.join(tmp, f"{img}_3DPts_ecef.txt"), pts3d.astype(np.float64), fmt="%.17g")
            np.savetxt(os.path.join(tmp, f"{img}_Correl.txt"), correl.astype(np.float64), fmt="%.17g")
            out[f"rpc_{i}"] = packed_rpc(d["rpc"])
            out[f"alt_{i}"] = np.array([float(d["min_alt"]), float(d["max_alt"])])
            out[f"pts2d_{i}"], out[f"pts3d_{i}"], out[f"correl_{i}"] = pts2d, pts3d, correl

        # depth priors: both images, then each alone for its own depth range
        padded = []          # what the reference pads per image: rays, depths, weights, std (:275-278)

        def recording(*args, **kw):
            padded.append(ss.SatelliteSceneDataset.prepare_padded_tensor(ds, *args, **kw))
            return padded[-1]

        ds.prepare_padded_tensor = recording
        rays, depths, valid, stds = ds.load_depth_data(small, tmp)
        del ds.prepare_padded_tensor
        out["std_pre"] = torch.cat([padded[3], padded[7]], 0).numpy()
        out["deprays"], out["depths"] = rays.numpy(), depths.numpy()
        out["valid_depth"], out["depth_stds"] = valid.numpy(), stds.numpy()
        for i in range(2):
            dep = ds.load_depth_data([small[i]], tmp)[1][:, 0].numpy()
            v = dep[out["valid_depth"][i * H * W:(i + 1) * H * W] > 0]
            out[f"range_{i}"] = np.array([v.min(), v.max()], np.float32)
        assert not np.array_equal(out["range_0"], out["range_1"]), "pick other seeds: the two depth ranges agree"

        # semantics
        raster = rng.choice(np.array(SEM_CODES, np.uint8), size=(37, 45))
        raster = np.repeat(np.repeat(raster[::3, ::3], 3, 0), 3, 1)[:37, :45].copy()   # 3 x 3 patches of a class
        raster[rng.integers(0, 37, 60), rng.integers(0, 45, 60)] = rng.choice(np.array(SEM_CODES, np.uint8), 60)

        class Src:
            def __enter__(self):
                return self

            def __exit__(self, *e):
                return False

            def read(self, band):
                return raster

        ss.rasterio.open = lambda *a_, **k_: Src()
        out["sem_raster"] = raster
        out["sem_map"] = np.array(sorted(ss.SEMANTIC_CONFIG[5]["label_mapping"].items()), np.int64)
        for mode, dense in (("sparse", False), ("dense", True)):
            for sd in (8, 3):
                ds.dense_ss = dense
                labels, valid = ds.load_semantic_data("unused_CLS.tif", small, 5, sem_downscale=sd)
                out[f"sem_{mode}_{sd}_labels"], out[f"sem_{mode}_{sd}_valid"] = labels.numpy(), valid.numpy()

        # scene scaling at img_downscale 8 over the two cameras at their real sizes
        got = {}
        ss.utils.write_dict_to_json = lambda d, path: got.update(d)
        ds.img_downscale, ds.json_dir = 8.0, os.path.join(tmp, "full")
        ds.init_scaling_params()
        out["loc"] = np.array([float(got[k]) for k in LOC_KEYS], np.float64)
        out["loc_f32"] = np.array([got[k] for k in LOC_KEYS], np.float32)
        assert np.array_equal(out["loc"], out["loc_f32"].astype(np.float64))
        out["loc_hw"] = np.array(loc_hw, np.int64)

    path = os.path.join(HERE, "dataset.npz")
    np.savez_compressed(path, **out)
    print("dataset.npz written:", os.path.getsize(path), "bytes;",
          {k: v.shape for k, v in out.items() if k.startswith(("pts2d", "deprays", "sem_sparse_8"))},
          "ranges", out["range_0"], out["range_1"], "loc", out["loc"])


if __name__ == "__main__":
    main()
