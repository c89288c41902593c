"""Generate the validation-loss fixture tests/golden/val_loss.npz by running the REFERENCE.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_val_golden.py [--ref /root/reference]

Run on the CPU-only development machine, where the reference is available (never on the GPU
box).  The reference is stub-imported and its draws recorded exactly as gen_golden.py does (its
helpers are imported from there; modules/metrics.py's kornia import is stubbed by
``load_metrics``); weights are NOT stored: they are rebuilt from
``oracle/weights.make_weights(dims, seed)`` at W = 64 (the fine model's from seed + 100).

37 synthetic rays per case, ``mode = 'test'``, what the validation step runs (main.py:202-205):
``render_rays`` and then ``SNerfLoss`` / ``SatNerfLoss`` at the args' ``sc_lambda``:

  a   n_samples = 24, guided (S' = 48), sc_lambda = 0.1, semantic head (C = 3)
  b   n_samples = 40, not guided (fewer samples than lanes), sc_lambda = 0.05, noise_std = 0.3
  c   n_samples = 48, guided (S' = 96: two samples per lane, ragged), sc_lambda = 0.1
  d   the β head with models['t'], SatNerfLoss, n_samples = 32, sc_lambda = 0.1
  e   n_importance = 16 on n_samples = 32, sc_lambda = 0 (coarse_color + fine_color)

Stored per case (keys ``<case>|...``): the rays and inputs, the recorded draws in order, a target
image, every tensor of the reference's ``results`` (``out_<key>``) except the per-sample albedo and
sky colours, which no term of the loss reads, ``sum_beta`` = Σ w·β of case d (metrics.py:11 before
``beta_min``), and the reference's ``loss`` and ``term|<key>`` of its ``loss_dict`` as float64
of the float32 values it logs.
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

N_RAYS = 37
T_VOCAB = 30
# name -> (dims, args, weight seed)
CASES = {
    "a": (ModelDims(width=64, sem=True), make_args(n_samples=24, guidedsample=True, sc_lambda=0.1), 21),
    "b": (ModelDims(width=64), make_args(n_samples=40, sc_lambda=0.05, noise_std=0.3), 22),
    "c": (ModelDims(width=64), make_args(n_samples=48, guidedsample=True, sc_lambda=0.1), 23),
    "d": (ModelDims(width=64, beta=True), make_args(n_samples=32, beta=True, sc_lambda=0.1), 24),
    "e": (ModelDims(width=64), make_args(n_samples=32, n_importance=16), 25),
}
SKIPPED = ("albedo", "sky")


def run_case(ref_spnerf, ref_rendering, metrics, name, dims, args, seed):
    n = N_RAYS
    torch.manual_seed(seed)
    models = {"coarse": build_model(ref_spnerf, dims, seed)}
    if args.n_importance > 0:
        models["fine"] = build_model(ref_spnerf, dims, seed + 100)
    rays = torch.tensor(synthetic_rays(n, seed=500 + seed))
    rng = np.random.default_rng(60 + seed)
    data = {"rays": rays.numpy()}
    sem = ts = None
    if dims.sem:
        labels = rng.choice([0, 1, 2, -100], size=n, p=[0.35, 0.3, 0.25, 0.10]).astype(np.int64)
        data["in_semantics"] = labels
        sem = torch.tensor(labels)
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
        res = ref_rendering.render_rays(models, args, rays, ts, semantics=sem, mode="test")
    for i, (kind, t) in enumerate(rec.draws):
        data[f"rng{i:02d}_{kind}"] = t.numpy()
    for k, v in res.items():
        if torch.is_tensor(v) and not k.startswith(SKIPPED):
            data[f"out_{k}"] = v.numpy()
    if dims.beta:
        data["sum_beta"] = torch.sum(res["weights_coarse"].unsqueeze(-1) * res["beta_coarse"], -2).reshape(n).numpy()
    typ = "fine" if args.n_importance > 0 else "coarse"
    target = np.clip(res[f"rgb_{typ}"].numpy() + 0.05 * rng.standard_normal((n, 3)), 0.0, 1.0).astype(np.float32)
    data["target"] = target
    loss_fn = metrics.SatNerfLoss(lambda_sc=args.sc_lambda) if dims.beta else metrics.SNerfLoss(lambda_sc=args.sc_lambda)
    with torch.no_grad():
        loss, loss_dict = loss_fn(res, torch.tensor(target))     # main.py:205
    data["loss"] = np.array(float(loss))
    for k, v in loss_dict.items():
        data[f"term|{k}"] = np.array(float(v))
    meta = dict(dims=dims.__dict__, args=args.__dict__, mode="test", seed=seed, n_rays=n)
    data["meta"] = np.array(repr(meta))
    S = res["z_vals_coarse"].shape[1]
    print(f"{name}: {len(rec.draws)} draws {[(k, tuple(t.shape)) for k, t in rec.draws]}, S' = {S}, loss {float(loss):.6f} "
          f"{ {k: round(float(v), 6) for k, v in loss_dict.items()} }")
    return {f"{name}|{k}": v for k, v in data.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    a = ap.parse_args()
    if not os.path.isdir(a.ref):
        sys.exit(f"the reference is not at {a.ref}: this generator runs only where it is")
    torch.set_num_threads(8)
    ref_spnerf, ref_rendering = load_reference(a.ref)
    metrics = load_metrics(a.ref)
    out = {}
    for name, (dims, args, seed) in CASES.items():
        out.update(run_case(ref_spnerf, ref_rendering, metrics, name, dims, args, seed))
    path = os.path.join(HERE, "val_loss.npz")
    np.savez_compressed(path, **out)
    print(f"val_loss written, {os.path.getsize(path) / 1e3:.1f} kB")


if __name__ == "__main__":
    main()
