"""Generate the whole-view fixture tests/golden/view_w64.npz by running the REFERENCE.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_view_golden.py [--ref /root/reference]

Run on the CPU-only development machine, where the reference is available (never on the GPU
box).  The reference is stub-imported and its draws recorded exactly as gen_golden.py does (its
helpers are imported from there); weights are NOT stored: they are rebuilt from
``oracle/weights.make_weights(dims, seed)`` at W = 64.

A 12 x 10 view (w = 12 columns, h = 10 rows — not square, so that an H/W swap shows) of 120
synthetic rays, three cases, each with ``sc_lambda = 0``, ``mode = 'test'``, ``noise_std = 0``:

  a   n_samples = 64, semantic head (C = 3)
  b   guided sampling, 64 + 64
  c   the β head and the time embedding on

Stored per case (keys ``<case>|...``): the rays and inputs, the recorded draws, the per-ray
outputs of the reference's ``render_rays`` (rgb, depth, sem_logits — its per-sample tensors enter
through the sums below and are not stored, to keep the file small), the sums of eval.py:76-101
(``sum_sun``, ``sum_albedo``, ``sum_sky``, ``sum_beta``), ``argmax`` of the mean logits, a target
image and a label map (some −100 entries, one class absent from both maps), and the reference's
``metrics.psnr`` (on float64 tensors: ``psnr``; on float32 ones as the validation step calls it:
``psnr_f32``), ``metrics.miou`` and ``metrics.overall_accuracy`` against them.

The generator asserts that on every ray the largest mean logit beats the runner-up by >= 1e-3 and
exits non-zero otherwise, so that ``sem_class`` can be demanded exactly with no ray left out.  If a
seed fails this, pick another seed; do not add a tolerance.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from gen_golden import Recorder, build_model, load_metrics, load_reference, make_args  # noqa: E402
from golden_util import synthetic_rays  # noqa: E402
from oracle.weights import ModelDims  # noqa: E402

H, W = 10, 12
MARGIN = 1e-3
T_VOCAB = 30
# name -> (dims, args, weight seed): the first seeds from 1 up that meet the margin and leave a class unpredicted
CASES = {
    "a": (ModelDims(width=64, sem=True), make_args(n_samples=64), 17),
    "b": (ModelDims(width=64, sem=True), make_args(n_samples=64, guidedsample=True), 4),
    "c": (ModelDims(width=64, sem=True, beta=True), make_args(n_samples=64, beta=True), 4),
}


def run_case(ref_spnerf, ref_rendering, metrics, name, dims, args, seed):
    n = H * W
    torch.manual_seed(seed)
    models = {"coarse": build_model(ref_spnerf, dims, seed)}
    rays = torch.tensor(synthetic_rays(n, seed=300 + seed))
    rng = np.random.default_rng(40 + seed)
    data = {"rays": rays.numpy()}
    in_sem = rng.choice([0, 1, 2, -100], size=n, p=[0.35, 0.3, 0.25, 0.10]).astype(np.int64)
    data["in_semantics"] = in_sem
    ts = None
    if dims.beta:
        emb = torch.nn.Embedding(T_VOCAB, dims.t_dim)
        with torch.no_grad():
            emb.weight.copy_(torch.tensor(np.random.default_rng(99).standard_normal((T_VOCAB, dims.t_dim)).astype(np.float32)))
        models["t"] = emb
        ts_np = rng.integers(0, T_VOCAB, size=n).astype(np.int64)
        ts = torch.tensor(ts_np)
        data["in_ts"] = ts_np
        data["in_t_embedding"] = emb.weight.detach().numpy().copy()
    with torch.no_grad(), Recorder() as rec:
        res = ref_rendering.render_rays(models, args, rays, ts, semantics=torch.tensor(in_sem), mode="test")
    for i, (kind, t) in enumerate(rec.draws):
        data[f"rng{i:02d}_{kind}"] = t.numpy()
    typ = "coarse"
    w = res[f"weights_{typ}"].unsqueeze(-1)
    for k in ("rgb", "depth", "sem_logits"):
        data[f"out_{k}"] = res[f"{k}_{typ}"].numpy()
    for k in ("sun", "albedo", "sky") + (("beta",) if dims.beta else ()):   # eval.py:76-101
        data[f"sum_{k}"] = torch.sum(w * res[f"{k}_{typ}"], -2).numpy()
    data["sum_sun"] = data["sum_sun"].reshape(n)
    if dims.beta:
        data["sum_beta"] = data["sum_beta"].reshape(n)
    logits = res[f"sem_logits_{typ}"]
    top = torch.sort(logits, -1, descending=True)[0]
    margin = float((top[:, 0] - top[:, 1]).min())
    if not margin >= MARGIN:
        sys.exit(f"case {name}: the smallest logit margin {margin:.3e} is below {MARGIN}: pick another seed")
    pred = logits.argmax(-1)                                                  # eval.py:63
    data["argmax"] = pred.numpy().astype(np.int32)
    data["margin_min"] = np.array(margin)
    # target image and label map: the labels agree with the prediction on most rays, some are
    # another class, some -100, and one class appears in neither map
    absent = [c for c in range(dims.num_sem_classes) if not bool((pred == c).any())]
    if not absent:
        sys.exit(f"case {name}: every class is predicted somewhere, none can be absent from both maps: pick another seed")
    allowed = [c for c in range(dims.num_sem_classes) if c != absent[0]]
    labels = pred.numpy().astype(np.int64).copy()
    flip = rng.uniform(size=n) < 0.3
    labels[flip] = rng.choice(allowed, size=int(flip.sum()))
    labels[rng.uniform(size=n) < 0.1] = -100
    assert (labels == -100).any() and not (labels == absent[0]).any()
    rgb = res[f"rgb_{typ}"]
    target = np.clip(rgb.numpy() + 0.05 * rng.standard_normal((n, 3)), 0.0, 1.0).astype(np.float32)
    data["target"] = target.reshape(H, W, 3)
    data["labels"] = labels.reshape(H, W)
    data["absent_class"] = np.array(absent[0])
    tg, lb = torch.tensor(target), torch.tensor(labels)
    data["psnr"] = np.array(float(metrics.psnr(rgb.double(), tg.double())))
    data["psnr_f32"] = np.array(float(metrics.psnr(rgb, tg)))
    data["miou"] = np.array(float(metrics.miou(pred, lb, dims.num_sem_classes)))
    data["oa"] = np.array(float(metrics.overall_accuracy(pred, lb)))
    meta = dict(dims=dims.__dict__, args=args.__dict__, mode="test", seed=seed, n_rays=n)
    data["meta"] = np.array(repr(meta))
    print(f"{name}: {len(rec.draws)} draws, margin {margin:.3e}, classes predicted {sorted(set(pred.tolist()))}, "
          f"psnr {float(data['psnr']):.4f} miou {float(data['miou']):.4f} oa {float(data['oa']):.4f}")
    return {f"{name}|{k}": v for k, v in data.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    a = ap.parse_args()
    torch.set_num_threads(8)
    ref_spnerf, ref_rendering = load_reference(a.ref)
    metrics = load_metrics(a.ref)
    out = {"h": np.array(H), "w": np.array(W)}
    for name, (dims, args, seed) in CASES.items():
        out.update(run_case(ref_spnerf, ref_rendering, metrics, name, dims, args, seed))
    path = os.path.join(HERE, "view_w64.npz")
    np.savez_compressed(path, **out)
    print(f"view_w64 written, {os.path.getsize(path) / 1e3:.1f} kB")


if __name__ == "__main__":
    main()
