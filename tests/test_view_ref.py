"""Whole views — CPU only.  The view interface of the library (include/spnerf_amd_view.h) without
a compute call, and the numpy restatement of the image metrics (tests/view_numpy.py) against what
the reference's modules/metrics.py computed (tests/golden/view_w64.npz, made by
gen_view_golden.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

import view_numpy as vn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spnerf_amd_view.h")


def view_header_symbols():
    txt = open(HEADER).read()
    return sorted(set(re.findall(r"\b(spnerf_view_[a-z0-9_]+)\s*\(", txt)))


def test_view_exports_match_the_header():
    from spnerf_amd import _eval_lib, _lib, _view_lib
    syms = view_header_symbols()
    assert syms == ["spnerf_view_abi_version", "spnerf_view_composite_products", "spnerf_view_metrics",
                    "spnerf_view_metrics_workspace_bytes"]
    L = _view_lib.lib()
    assert L is _lib.lib()                                 # one library, three signature tables
    for s in syms:
        assert hasattr(L, s), s
    assert sorted(_view_lib.SIGNATURES) == syms, "view signature table out of sync with the header"
    assert not set(_view_lib.SIGNATURES) & set(_lib.SIGNATURES)
    assert not set(_view_lib.SIGNATURES) & set(_eval_lib.SIGNATURES)
    hdr = open(HEADER).read()
    consts = {k: int(v) for k, v in re.findall(r"#define (SPNERF_VIEW_[A-Z_]+) (\d+)\b", hdr)}
    assert L.spnerf_view_abi_version() == consts["SPNERF_VIEW_ABI_VERSION"] == _view_lib.SPNERF_VIEW_ABI_VERSION == 1
    assert consts["SPNERF_VIEW_MAX_CLASSES"] == _view_lib.VIEW_MAX_CLASSES == 32
    assert ctypes.sizeof(_view_lib.ViewPlanes) == 64
    assert ctypes.sizeof(_view_lib.ViewMetricsResult) == 32 + 8 * 33 * 32
    assert L.spnerf_abi_version() == 2                      # the core ABI is untouched
    assert L.spnerf_eval_abi_version() == 1


def test_view_argument_errors_are_reported():
    from spnerf_amd import _view_lib
    L = _view_lib.lib()
    one = ctypes.c_void_p(256)      # never dereferenced: the arguments are refused first
    planes = _view_lib.ViewPlanes()
    pp = ctypes.byref(planes)

    def products(n=4, S=64, z=one, out=one, NO=11, sem_col=8, n_sem=3, beta_col=-1, begin=0, pl=pp):
        return L.spnerf_view_composite_products(n, S, z, out, NO, None, 0.0, sem_col, n_sem, beta_col, begin, pl, None, None)

    for kw, text in ((dict(z=None), b"NULL z or out"), (dict(out=None), b"NULL z or out"), (dict(pl=None), b"NULL planes"),
                     (dict(S=0), b"n_samples 0"), (dict(S=257), b"n_samples 257"), (dict(begin=-1), b"ray_begin -1"),
                     (dict(n=-1), b"n_rays -1"), (dict(NO=7), b"bad output layout"), (dict(n_sem=4), b"bad output layout"),
                     (dict(beta_col=3), b"beta_col 3"), (dict(beta_col=11), b"beta_col 11"),
                     (dict(S=256, NO=40), b"too large")):
        assert products(**kw) == -1, kw
        assert text in L.spnerf_last_error(), (kw, L.spnerf_last_error())
    planes.beta = 256
    assert products() == -1 and b"beta plane needs beta_col" in L.spnerf_last_error()
    planes.beta = None
    planes.sem_class = 256
    assert products(n_sem=0) == -1 and b"semantic planes need n_sem" in L.spnerf_last_error()
    planes.sem_class = None
    assert products(n=0) == 0                               # nothing to do, nothing launched

    def metrics(n=100, rgb=one, tgt=one, cls=None, lab=None, C=0, ws=one, res=one):
        return L.spnerf_view_metrics(n, rgb, tgt, cls, lab, C, ws, res, None)

    for kw, text in ((dict(rgb=None), b"view_metrics: NULL"), (dict(ws=None), b"view_metrics: NULL"),
                     (dict(res=None), b"view_metrics: NULL"), (dict(n=0), b"n_rays 0"), (dict(C=-1), b"n_classes -1"),
                     (dict(C=33), b"n_classes 33"), (dict(ws=ctypes.c_void_p(264)), b"not 16-byte aligned"),
                     (dict(cls=one, C=3), b"go together"), (dict(lab=one, C=3), b"go together")):
        assert metrics(**kw) == -1, kw
        assert text in L.spnerf_last_error(), (kw, L.spnerf_last_error())
    wsb = L.spnerf_view_metrics_workspace_bytes
    assert wsb(0, 3) == -1 and wsb(100, -1) == -1 and wsb(100, 33) == -1
    assert b"n_classes 33" in L.spnerf_last_error()
    # per-workgroup partials: one double and one table each, a fixed function of the view's size
    assert wsb(1, 0) == 16 and wsb(256, 0) == 16 and wsb(257, 0) == 16
    assert wsb(257, 3) == 16 + 2 * 12 * 8
    assert 0 < wsb(70001, 6) < wsb(1 << 24, 6) == wsb(1 << 30, 6)      # the grid is capped
    assert all(wsb(n, c) % 16 == 0 for n in (1, 255, 300, 70001) for c in (0, 1, 6, 32))


def test_python_surface_refuses_cpu_tensors_and_bad_arguments():
    import types
    import torch
    import spnerf_amd
    from spnerf_amd import _lib
    assert spnerf_amd.render_image is spnerf_amd.view.render_image
    assert spnerf_amd.view_metrics is spnerf_amd.view.view_metrics
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        spnerf_amd.view_metrics(torch.zeros(4, 3), torch.zeros(4, 3))
    args = types.SimpleNamespace(model="sp-nerf", n_samples=8, n_importance=0, guidedsample=False, beta=False,
                                 sc_lambda=0.0, noise_std=0.0)
    model = spnerf_amd.SPNeRF(feat=64, mapping=True)
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        spnerf_amd.render_image({"coarse": model}, args, torch.zeros(4, 11))
    args.model = "nerf"
    with pytest.raises(ValueError, match="not valid"):
        spnerf_amd.render_image({"coarse": model}, args, torch.zeros(4, 11))


@pytest.mark.parametrize("case", vn.CASES)
def test_restatement_matches_reference(case):
    d = vn.load_case(case)
    assert (d["h"], d["w"]) == (10, 12) and d["target"].shape == (10, 12, 3) and d["labels"].shape == (10, 12)
    assert d["out_rgb"].shape == (120, 3) and d["argmax"].shape == (120,)
    assert float(d["margin_min"]) >= 1e-3                   # sem_class can be demanded exactly
    C = d["meta"]["dims"]["num_sem_classes"]
    labels, pred = d["labels"].reshape(-1), d["argmax"]
    absent = int(d["absent_class"])
    assert (labels == -100).any() and not (labels == absent).any() and not (pred == absent).any()
    m = vn.view_metrics(d["out_rgb"], d["target"], pred, labels, C)
    assert abs(m["psnr"] - float(d["psnr"])) <= 1e-12
    assert abs(m["miou"] - float(d["miou"])) <= 1e-12
    assert abs(m["oa"] - float(d["oa"])) <= 1e-12
    assert abs(m["psnr"] - float(d["psnr_f32"])) <= 1e-4    # what the validation step logs, in float32
    t = m["confusion"]
    assert t.sum() == 120 and t[C].sum() == (labels == -100).sum() and m["correct"] == (pred == labels).sum()
    assert t[absent].sum() == 0 and t[:, absent].sum() == 0   # the class whose union is 0
    # the package's own table -> scores step follows the same rules
    from spnerf_amd.view import scores_from_table
    s = scores_from_table(t, 120)
    assert s["miou"] == m["miou"] and s["oa"] == m["oa"]


def test_restatement_edge_cases():
    rng = np.random.default_rng(0)
    img = rng.uniform(size=(7, 3)).astype(np.float32)
    assert vn.mse(img, img) == 0.0 and vn.psnr(img, img) == float("inf")
    m = vn.view_metrics(img, img, np.zeros(7, np.int32), np.full(7, -100), 2)
    assert m["oa"] == 0.0 and m["correct"] == 0 and m["confusion"][2, 0] == 7
    assert m["miou"] == 0.0                                 # class 0: 0 / 7, class 1: union 0 -> 0
    assert vn.view_metrics(img, img, None, None, 0)["miou"] is None
