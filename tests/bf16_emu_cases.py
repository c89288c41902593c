"""Inputs shared by tests/test_bf16_emu_ref.py (CPU: the emulation against ref_cpu, the mutation
table) and tests/test_gpu_bf16_emu.py (the bf16 kernels against the emulation): the point-network
and training cases, their recorded draws, the projection loss and the emulated render."""
from __future__ import annotations

import functools
import types

import numpy as np
import torch

import golden_util as gu
from oracle import bf16_emu as emu
from oracle.weights import ModelDims, make_weights

SEED_W = 11   # weights of every case

# point network: (id, dims, P)
POINT_CASES = [(f"w512_sem_beta_P{P}", ModelDims(width=512, sem=True, beta=True), P) for P in (1, 63, 64, 129, 3000)] + [
    ("w512_nomap_P130", ModelDims(width=512, mapping=False), 130),
    ("w256_P129", ModelDims(width=256), 129),
    ("w128_nomap_P129", ModelDims(width=128, mapping=False), 129),
    ("w64_P129", ModelDims(width=64), 129),
]

# training: id -> (dims, rays, samples, sc_lambda, guided)
TRAIN_CASES = {
    "w512_sem_33x32": (ModelDims(width=512, sem=True), 33, 32, 0.0, False),     # last 128-point tile a quarter full
    "w512_sem_257x64_sc": (ModelDims(width=512, sem=True), 257, 64, 0.1, False),  # main + solar pass
    "w512_beta_40x64": (ModelDims(width=512, beta=True), 40, 64, 0.0, False),
    "w64_sem_33x32": (ModelDims(width=64, sem=True), 33, 32, 0.0, False),
    "w512_guided_96x64": (ModelDims(width=512, sem=True), 96, 64, 0.0, True),
}
NOISE_STD = 0.1
N_TS = 5      # rows of the time embedding (beta cases)


def point_inputs(dims: ModelDims, P: int):
    rng = np.random.default_rng(3)
    xyz = rng.uniform(-1, 1, (P, 3)).astype(np.float32)
    sun = rng.normal(size=(P, 3)).astype(np.float32)
    lab = rng.choice([-100] + list(range(dims.num_sem_classes)), size=P).astype(np.int64)
    t = rng.normal(size=(P, dims.t_dim)).astype(np.float32)
    return xyz, sun, lab, t


def point_emulation(dims: ModelDims, P: int, sites=emu.EmuSites(), mut=None) -> np.ndarray:
    xyz, sun, lab, t = point_inputs(dims, P)
    p = emu.params64(make_weights(dims, SEED_W), requires_grad=False)
    with torch.no_grad():
        return emu.emu_field(p, dims, torch.tensor(xyz).double(), torch.tensor(sun).double(),
                             torch.tensor(lab) if dims.sem else None, torch.tensor(t).double() if dims.beta else None,
                             sites, "full", mut).numpy()


def train_inputs(name: str) -> dict:
    """Rays, labels (every class and -100), time indices / embedding, the guided targets and the
    draws in the order render_rays consumes them."""
    dims, B, S, sc, guided = TRAIN_CASES[name]
    rng = np.random.default_rng(17)
    c = dict(dims=dims, B=B, S=S, sc=sc, guided=guided, rays=gu.synthetic_rays(B, 9))
    c["args"] = types.SimpleNamespace(n_samples=S, n_importance=0, model="sp-nerf", beta=dims.beta, guidedsample=guided,
                                      sc_lambda=sc, margin=1e-4, stdscale=1.0, chunk=5120, noise_std=NOISE_STD)
    c["sem"] = rng.choice([-100] + list(range(dims.num_sem_classes)), size=B).astype(np.int64) if dims.sem else None
    c["ts"] = rng.integers(0, N_TS, size=B).astype(np.int64) if dims.beta else None
    c["t_weight"] = rng.normal(size=(N_TS, dims.t_dim)).astype(np.float32) if dims.beta else None
    f32 = lambda a: a.astype(np.float32)
    draws = [("rand", f32(rng.uniform(size=(B, S)))), ("randn", f32(rng.standard_normal((B, S))))]
    if guided:
        c["valid"] = (rng.uniform(size=B) < 0.68).astype(np.int64)
        c["target_depths"] = np.stack([c["rays"][:, 7] * 0.5, np.ones(B, np.float32)], 1).astype(np.float32)
        c["target_std"] = np.full((B,), 0.01, np.float32)
        draws += [("rand", f32(rng.uniform(size=(B, S)))), ("rand", f32(rng.uniform(size=(int(c["valid"].sum()), S)))),
                  ("randn", f32(rng.standard_normal((B, 2 * S))))]
    c["noise"] = draws[-1][1]
    c["noise_sc"] = None
    if sc > 0:
        draws.append(("randn", f32(rng.standard_normal(draws[-1][1].shape))))
        c["noise_sc"] = draws[-1][1]
    c["draws"] = draws
    return c


def stratified_z(c: dict) -> torch.Tensor:
    """The stratified depths of an unguided case, in fp32 as ``ref_cpu.stratified`` forms them (the
    kernels' are bit-equal on these rays; the GPU test feeds the kernel's own z_vals anyway)."""
    from oracle import ref_cpu
    return ref_cpu.stratified(torch.tensor(c["rays"]), c["S"], torch.tensor(c["draws"][0][1]))


def projection_loss(res: dict, keys=None, device=None):
    """The fixed random projection (golden_util.projection_weights) of the outputs ``keys`` (default:
    every output that carries a gradient; the draws depend on the key set, so both sides of a
    comparison name the same one)."""
    keys = {k: tuple(res[k].shape) for k in (keys if keys is not None else [k for k, v in res.items() if v.requires_grad])}
    R = gu.projection_weights(keys)
    return sum((res[k] * torch.tensor(R[k], device=device).to(res[k].dtype)).sum() for k in sorted(R))


def emulate_train(name: str, z_vals: torch.Tensor, sites=emu.EmuSites(), mut=None, grads=True, keys=None):
    """Emulated coarse keys at the depths z_vals (B, S') and the projection loss's parameter gradients
    (``t.weight``: the time embedding's)."""
    c = train_inputs(name)
    dims = c["dims"]
    p = emu.params64(make_weights(dims, SEED_W))
    t_emb = tw = None
    if dims.beta:
        tw = torch.tensor(c["t_weight"], dtype=torch.float64).requires_grad_(True)
        t_emb = tw[torch.tensor(c["ts"])]
    res = emu.emu_render_rays(p, dims, torch.tensor(c["rays"]), z_vals, torch.tensor(c["noise"]), NOISE_STD,
                              None if c["sem"] is None else torch.tensor(c["sem"]), t_emb, sites,
                              None if c["noise_sc"] is None else torch.tensor(c["noise_sc"]), mut)
    g = {}
    if grads:
        projection_loss(res, keys).backward()
        g = {n: (q.grad if q.grad is not None else torch.zeros_like(q)).numpy() for n, q in p.items()}
        if tw is not None:
            g["t.weight"] = tw.grad.numpy()
    return {k: v.detach().numpy() for k, v in res.items()}, g


@functools.lru_cache(maxsize=None)
def clean_train_emulation(name: str):
    """The all-sites-on emulation of an unguided case at its stratified depths (computed once)."""
    return emulate_train(name, stratified_z(train_inputs(name)))


def param_class(name: str) -> str:
    """The bound class of a parameter tensor: trunk weights, head weights, biases, embeddings."""
    if name in ("semantic_embedding.weight", "t.weight"):
        return "embedding"
    if name.endswith(".bias"):
        return "bias"
    return "trunk_weight" if name.startswith("fc_net.") else "head_weight"


def out_stem(key: str) -> str:
    stem = key[:-len("_coarse")] if key.endswith("_coarse") else key
    return stem[:-3] if stem.endswith("_sc") else stem


# The GPU bounds of tests/test_gpu_bf16_emu.py.  key / tensor class: (worst norm-relative distance
# kernel - emulation measured on the MI355X over POINT_CASES and TRAIN_CASES, defaults and
# fused_trunk 0; the case it came from is in the comment), bound = 3x it rounded up to two digits.
# Point-network columns: albedo, sigma, sun, sky, beta, point_logits; render keys by stem; gradients
# by param_class (every tensor of the class is held to the class's bound).
BOUNDS = {
    "albedo": (1.924e-4, 5.8e-4),        # w512_beta_40x64
    "sigma": (6.337e-4, 2.0e-3),         # w512_nomap_P130
    "sun": (1.156e-4, 3.5e-4),           # w64_P129
    "sky": (5.488e-8, 1.7e-7),           # w64_sem_33x32 (fp32 sky MLP against float64)
    "beta": (2.746e-4, 8.3e-4),          # w512_beta_40x64
    "point_logits": (2.008e-3, 6.1e-3),  # w512_sem_beta_P3000 (per-point logits)
    "rgb": (2.321e-4, 7.0e-4),           # w512_beta_40x64
    "depth": (1.097e-5, 3.3e-5),         # w512_sem_33x32
    "weights": (2.700e-5, 8.1e-5),       # w512_sem_33x32
    "transparency": (1.282e-5, 3.9e-5),  # w512_sem_33x32
    "sem_logits": (7.926e-4, 2.4e-3),    # w512_sem_33x32 (mean over the ray's samples)
    "trunk_weight": (5.647e-3, 1.7e-2),  # w512_beta_40x64
    "head_weight": (6.918e-3, 2.1e-2),   # w512_guided_96x64
    "bias": (6.442e-3, 2.0e-2),          # w512_guided_96x64
    "embedding": (6.641e-3, 2.0e-2),     # w512_sem_257x64_sc, fused_trunk 0
}
# the loose bounds of tests/test_gpu_bf16.py these are compared with: OUT_TOL_KEY, OUT_TOL (point
# network: sigma, point_logits) and GRAD_TOL
LOOSE = {"albedo": 1.8e-3, "sigma": 2e-2, "sun": 2e-3, "sky": 1e-6, "beta": 2.2e-3, "point_logits": 2e-2, "rgb": 1.5e-3,
         "depth": 5e-4, "weights": 1e-3, "transparency": 5e-4, "sem_logits": 1.5e-2, "trunk_weight": 8e-2,
         "head_weight": 8e-2, "bias": 8e-2, "embedding": 8e-2}
# bounds above 1/8 of their loose bound: loose / bound reached.  They are as measured, not relaxed:
# one-point renders agree to 8e-8, so no rounding site is missing; the rest is the rounding cascade
# (a 1e-7 relative change of a pre-activation, the size of an fp32 summation-order change, flips a
# bf16 rounding with probability ~1e-4, each flip is a 2^-8 relative change of its own, and eight
# rounded layers raise that to these levels: DESIGN §5 has the CPU experiment)
OVER_EIGHTH = {"albedo": 3.1, "sun": 5.7, "sky": 5.9, "beta": 2.7, "point_logits": 3.3, "rgb": 2.1, "sem_logits": 6.3,
               "trunk_weight": 4.7, "head_weight": 3.8, "bias": 4.0, "embedding": 4.0}
