"""The training-set C ABI (include/spnerf_amd_data.h, spnerf_amd._data_lib) and the host side of
spnerf_amd.dataset: the header, the ctypes table and the built library agree, argument errors
come back as codes or ValueErrors before anything touches the GPU — no GPU needed."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import abi_util
from spnerf_amd import _data_lib, _lib

ROOT = abi_util.ROOT
HEADER = abi_util.header_path("spnerf_amd_data.h")
ONE = 256   # a non-NULL pointer value that is never dereferenced: the arguments are refused first


def test_data_exports_match_the_header():
    PD, PF = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float)
    # the RPC coefficients, the scene centre and the offsets are host arrays
    host = {("spnerf_rpc_rays_f64", 0): PD, ("spnerf_rpc_rays_f64", 6): PF, ("spnerf_rpc_rays_f64", 8): PF,
            ("spnerf_depth_priors", 0): PD, ("spnerf_depth_priors", 5): PF, ("spnerf_scene_bounds", 0): PD}
    assert abi_util.check_table(_data_lib, HEADER, "spnerf_", host) == [
        "spnerf_data_abi_version", "spnerf_depth_priors", "spnerf_rpc_rays_f64", "spnerf_scene_bounds", "spnerf_semantic_labels"]
    assert [len(_data_lib.SIGNATURES[n][1]) for n in ("spnerf_depth_priors", "spnerf_scene_bounds", "spnerf_semantic_labels")] == [20, 8, 12]
    consts = abi_util.defines(HEADER, "SPNERF_DATA_")
    assert consts["SPNERF_DATA_WORKSPACE_BYTES"] == _data_lib.DATA_WORKSPACE_BYTES
    assert consts["SPNERF_DATA_VOID_LABEL"] == _data_lib.VOID_LABEL == -100


def test_argument_errors_are_reported():
    L = _data_lib.lib()
    rpc = (ctypes.c_double * 90)()
    cen = (ctypes.c_float * 3)()

    def depth(K=4, h=4, w=4, rng=1.0, pix=ONE, ws=ONE):
        return L.spnerf_depth_priors(rpc, 0.0, 1.0, h, w, cen, rng, pix, ONE, ONE, K, 1.0, 0.0, ONE, ONE, ONE, ONE, ONE,
                                     ws, None)

    assert depth(pix=None) == -1 and b"NULL input" in L.spnerf_last_error()
    assert depth(ws=None) == -1 and b"NULL output" in L.spnerf_last_error()
    assert depth(K=0) == -1 and b"K = 0" in L.spnerf_last_error()
    assert depth(K=17) == -1 and b"cannot be distinct" in L.spnerf_last_error()
    assert depth(h=0) == -1 and b"bad image size" in L.spnerf_last_error()
    assert depth(rng=0.0) == -1 and b"bad range" in L.spnerf_last_error()
    assert L.spnerf_scene_bounds(rpc, 1.0, 0.0, 1.0, 4, 4, None, None) == -1 and b"NULL" in L.spnerf_last_error()
    assert L.spnerf_scene_bounds(rpc, 0.0, 0.0, 1.0, 4, 4, ONE, None) == -1 and b"downscale" in L.spnerf_last_error()
    assert L.spnerf_scene_bounds(rpc, 1.0, 0.0, 1.0, -1, 4, ONE, None) == -1 and b"rectangle" in L.spnerf_last_error()

    def sem(raster=ONE, hs=8, ws=8, h=4, w=4, sd=8, dense=0):
        return L.spnerf_semantic_labels(raster, 0, hs, ws, ONE, h, w, sd, dense, ONE, ONE, None)

    assert sem(raster=None) == -1 and b"NULL" in L.spnerf_last_error()
    assert sem(h=0) == -1 and b"bad size" in L.spnerf_last_error()
    assert sem(sd=0) == -1 and b"sem_downscale" in L.spnerf_last_error()
    assert sem(hs=7, dense=1) == -1 and b"no 1/8 downsampling" in L.spnerf_last_error()
    assert L.spnerf_rpc_rays_f64(rpc, 1.0, 0.0, 1.0, None, 4, None, 1.0, None, ONE, 8, None) == -1
    assert b"NULL pixel list" in L.spnerf_last_error()


def test_dataset_module_imports_without_touching_the_gpu():
    code = ("import sys, torch\n"
            "import spnerf_amd\n"
            "from spnerf_amd import dataset\n"
            "assert spnerf_amd.dataset is dataset\n"
            "assert not torch.cuda.is_initialized()\n"
            "assert 'spnerf_amd._data_lib' not in sys.modules\n"
            "print('ok')\n")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def image(pts2d, h=6, w=5):
    k = len(pts2d)
    return dict(rpc={}, height=h, width=w, min_alt=0.0, max_alt=1.0, pts2d=np.asarray(pts2d, np.int64).reshape(-1, 2),
                pts3d=np.zeros((k, 3), np.float32), correl=np.linspace(0.3, 1.0, k).astype(np.float32))


@pytest.fixture
def no_library(monkeypatch):
    """The host checks come first: the library must not be loaded by a call that is refused."""
    def boom():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_data_lib, "lib", boom)
    monkeypatch.setattr(_lib, "lib", boom)


def test_depth_data_refuses_bad_keypoints_on_the_host(no_library):
    from spnerf_amd import dataset
    kw = dict(center=np.zeros(3, np.float32), range=1.0)
    good = [(0, 0), (3, 0), (1, 2), (4, 5)]
    with pytest.raises(ValueError, match=r"strictly increasing.*keypoint 2 \(1, 1\) comes before keypoint 1 \(3, 2\)"):
        dataset.load_depth_data([image([(0, 0), (3, 2), (1, 1), (4, 5)])], **kw)       # unsorted
    with pytest.raises(ValueError, match=r"keypoint 3 \(1, 2\) repeats keypoint 2 \(1, 2\)"):
        dataset.load_depth_data([image([(0, 0), (3, 0), (1, 2), (1, 2)])], **kw)       # duplicate
    with pytest.raises(ValueError, match=r"image 1: .*keypoint 1 \(0, 0\)"):
        dataset.load_depth_data([image(good), image([(2, 0), (0, 0)])], **kw)          # the second image is named
    with pytest.raises(ValueError, match="K == 0"):
        dataset.load_depth_data([image([])], **kw)
    with pytest.raises(ValueError, match=r"depth priors need img_downscale == 1"):
        dataset.load_depth_data([image(good)], img_downscale=2, **kw)
    with pytest.raises(ValueError, match=r"keypoint 3 \(5, 5\) is outside the 6 x 5 image"):
        dataset.load_depth_data([image([(0, 0), (3, 0), (1, 2), (5, 5)])], **kw)
    with pytest.raises(ValueError, match="4 keypoints but pts3d"):
        dataset.load_depth_data([dict(image(good), pts3d=np.zeros((3, 3), np.float32))], **kw)
    with pytest.raises(ValueError, match="no images"):
        dataset.load_depth_data([], **kw)


def test_semantic_and_scaling_argument_errors(no_library):
    from spnerf_amd import dataset
    metas = [dict(height=4, width=4)]
    raster = np.zeros((8, 8), np.uint8)
    with pytest.raises(ValueError, match="sem_downscale"):
        dataset.load_semantic_data(raster, metas, {2: 0}, sem_downscale=0)
    with pytest.raises(ValueError, match=r"must be \(Hs, Ws\)"):
        dataset.load_semantic_data(raster[0], metas, {2: 0})
    with pytest.raises(ValueError, match="no 1/8 downsampling"):
        dataset.load_semantic_data(raster[:7], metas, {2: 0}, dense_ss=True)
    with pytest.raises(ValueError, match="outside"):
        dataset.load_semantic_data(raster, metas, {300: 0})
    with pytest.raises(ValueError, match="integer class codes"):
        dataset.load_semantic_data(raster.astype(np.float32), metas, {2: 0})
    with pytest.raises(ValueError, match="no images"):
        dataset.init_scaling_params([])
    lut = dataset.label_lut({2: 0, 17: 4})
    assert lut.dtype == np.int32 and lut.shape == (256,) and lut[2] == 0 and lut[17] == 4
    assert (np.delete(lut, [2, 17]) == -100).all()


def test_cpu_devices_and_tensors_are_refused():
    import torch
    from spnerf_amd import dataset
    good = image([(0, 0), (3, 0), (1, 2), (4, 5)])
    kw = dict(center=np.zeros(3, np.float32), range=1.0)
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        dataset.load_depth_data([good], device="cpu", **kw)
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        dataset.load_depth_data([dict(good, correl=torch.zeros(4))], **kw)
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        dataset.load_semantic_data(torch.zeros(8, 8, dtype=torch.uint8), [dict(height=4, width=4)], {2: 0})
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        dataset.init_scaling_params([dict(good)], device="cpu")
