#!/usr/bin/env python3
"""SP-NeRF train-step throughput on MI355X (ray-samples/s), BASELINE.json metric.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config c4|c3|c2|c5|...] [--dump-outputs DIR]
    python bench.py --full [--no-cpu-baseline] [--no-secondary] [...]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

A plain run does what the headline figure needs and no more: set-up, warm-up (and the HIP-graph
capture), the K timed steps, the outputs of the last timed step to ``--dump-outputs DIR`` when
asked, and the result line.  ``--full`` adds every other leg to that line: the C2 / C5
``secondary`` workloads, ``cpu_baseline``, the ``psnr_parity`` / ``psnr_seeds`` studies, the
per-kernel figures that take eager steps of their own after a graph-mode timed region
(``roofline``, ``rooflines_top3``, ``mlp_mfma_utilisation``, ``kernels``; ``--eager`` runs and
C5 record them inside the timed steps and report them either way) and the paired replays behind
``allreduce_exposed_paired_replays``.

``--gpus N`` without torchrun's environment starts the N ranks itself (a torch.distributed.run
child process, launched before anything touches the GPU); under torchrun, WORLD_SIZE must
equal ``--gpus``, and asking for more GPUs than the node has is an error, not a 1-GPU run.

One step = sample a batch of rays from the HBM-resident synthetic scene (shared-seed sampler,
every rank its slice), render_rays (stratified [+ guided] sampling, MLP, compositing
[+ solar pass]) on the HIP kernels, the reference losses, backward, ONE RCCL all-reduce of the
flat gradient bucket (N > 1), Adam.

The default workload is BASELINE.json configs[3] (C4: the training workload the 1/2/4/8-GPU
metric is quoted on — C3's README-recipe flags with the bf16 MLP at a GLOBAL batch of 4096 rays
per step, split over the ranks: strong scaling).  At N=1 the same 4096-ray step runs on one
GPU.  With ``--full``: C2 (configs[1], fp32) is reported beside it as ``secondary`` at N=1;
``roofline`` reports the dominant kernel from HIP events recorded by the library around each of
its launches; ``cpu_baseline`` times the repo's PyTorch-CPU oracle (the reference algorithm
restated, parity-pinned) on the host cores for a bounded sample of the workload.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import spnerf_amd  # noqa: E402
from spnerf_amd import _lib, dp  # noqa: E402
from spnerf_amd.losses import DepthLoss, FusedRenderLoss, SemanticLoss, SNerfLoss  # noqa: E402
from spnerf_amd.scene import synthetic_scene  # noqa: E402

FP32_MFMA_PEAK_TFLOPS = 157.3     # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 spec
BF16_MFMA_PEAK_TFLOPS = 2516.6    # dense bf16 = 16 x the f32 MFMA rate (MI355X_MICROARCH.md "Peak BF16", ~2.5 PF)
HBM_PEAK_GBS = 8000.0
# The library's profiling classes: ONE class per kernel function (rocprofv3 name in the text).
# MFMA kernels carry the peak of their arithmetic; the rest are HBM kernels.
GEMM_CLASSES = {
    "gemm_nt_f32": ("k_gemm_nt_w<256,128,2,2,3> (fp32 MFMA NT GEMM, persistent 256x128 tiles, LDS-DMA)", FP32_MFMA_PEAK_TFLOPS),
    "gemm_tn_f32": ("k_gemm_tn<3> (fp32 MFMA weight-gradient GEMM)", FP32_MFMA_PEAK_TFLOPS),
    "gemm_nt_bf16d": ("k_gemm_nt_bf16d<false,2,EV> (bf16 MFMA NT GEMM, 256x256 persistent tiles, LDS-DMA ring; "
                      "bias / sine / per-ray-row / rank-1 epilogue variants: head layers, layer 0, heads' dX)",
                      BF16_MFMA_PEAK_TFLOPS),
    "gemm_nt_bf16d_dmul": ("k_gemm_nt_bf16d<true,2> (bf16 MFMA dX GEMM with the x D epilogue)", BF16_MFMA_PEAK_TFLOPS),
    "gemm_nt_bf16w": ("k_gemm_nt_bf16w (bf16 MFMA NT GEMM, register-staged)", BF16_MFMA_PEAK_TFLOPS),
    "gemm_nt_bf16": ("k_gemm_nt_bf16 (bf16 MFMA NT GEMM, 128x128 tiles)", BF16_MFMA_PEAK_TFLOPS),
    "gemm_tn_bf16d": ("k_gemm_tn_bf16d<IP> (bf16 MFMA weight-gradient GEMM, 256x256 tiles, LDS-DMA; IP 3 = "
                      "the DMA issue spread over the MFMA groups; the deferred GEMMs of a render in one group launch, option tn_group)",
                      BF16_MFMA_PEAK_TFLOPS),
    "gemm_tn_bf16w": ("k_gemm_tn_bf16w (bf16 MFMA weight-gradient GEMM, 256x256 register-staged)", BF16_MFMA_PEAK_TFLOPS),
    "gemm_tn_bf16": ("k_gemm_tn_bf16 (bf16 MFMA weight-gradient GEMM, 128x128 tiles)", BF16_MFMA_PEAK_TFLOPS),
    "gemm_tn_bf16k": ("k_gemm_tn_bf16_k64 (bf16 MFMA weight gradient N = 512, K = 64: fc_net.0 and the skip "
                      "layer's PE tail, whole 512x64 output per split)", BF16_MFMA_PEAK_TFLOPS),
    "trunk_bf16": ("k_trunk_bf16<128> (fused bf16 trunk, inference: 128-point LDS-resident tiles; the "
                   "two-workgroup k_trunk2_bf16 only in the ablation build)", BF16_MFMA_PEAK_TFLOPS),
    "trunk_bf16_train": ("k_trunk_bf16<128, 2048> (fused bf16 trunk, 128-point training tiles saving H and D)", BF16_MFMA_PEAK_TFLOPS),
    "heads_train": ("k_heads_train_bf16 (fused bf16 training heads after the trunk, 128-point LDS-resident tiles: "
                    "semantic hidden, feat, Q, sun_v 2 / 3 saving their activations, and the narrow heads; option "
                    "heads_epi 2)", BF16_MFMA_PEAK_TFLOPS),
    "trunk_bwd_bf16": ("k_trunk_bwd_bf16 (fused bf16 backward dX chain, LDS-resident dZ)", BF16_MFMA_PEAK_TFLOPS),
    "heads_fused": ("k_heads_bf16 (fused bf16 inference heads, LDS-resident activations)", BF16_MFMA_PEAK_TFLOPS),
    "trunk_heads_bf16": ("k_trunk_bf16<128, 4096> (fused bf16 inference trunk with the heads on its last LDS "
                         "image: layers 0..7, sigma, semantic, feat, Q, albedo, sun_v, sun per 128-point tile; option "
                         "trunk_heads 2; k_trunk2_bf16<128, L0, false, true> with trunk_heads 1)", BF16_MFMA_PEAK_TFLOPS)}
HBM_CLASSES = {"tn_skinny": "k_tn_skinny_multi (narrow-head / per-ray weight gradients, one launch per backward step)",
               "reduce_slabs": "k_reduce_slabs(_multi) (fixed-order weight-gradient split reductions)",
               "encode": "k_encode (positional encoding)", "heads_fwd": "k_heads_fwd_v (narrow heads)",
               "heads_bwd": "k_heads_bwd_v (narrow-head backward)", "composite_fwd": "k_composite_fwd",
               "composite_bwd": "k_composite_bwd", "sample_guided": "k_guided", "render_loss": "k_loss_*",
               "pack": "k_pack (weight re-layout)", "adam": "k_adam", "ray_rowsum": "k_ray_rowsum*",
               "ray_terms": "k_ray_fwd / k_ray_bwd / k_class_sum", "zero": "k_zero"}
MFMA_TARGET = 0.40   # BASELINE.json north star: >= 40% MFMA utilisation on the MLP
PARITY_NOTE_BF16 = ("bf16 MLP (BASELINE configs[2,3,4] dtype): outputs are held to per-key norm-relative bounds against the "
                    "reference fixtures (rgb 1.5e-3, depth 5e-4, sem_logits 1.5e-2; flat gradient 2e-2; "
                    "tests/test_gpu_bf16.py), NOT the north star's 1e-4 relative, which bf16's 2^-9 roundoff cannot meet; "
                    "the fp32 MLP meets 1e-4 element-wise on every reference fixture (tests/test_gpu_parity.py)")

CONFIGS = {
    "c2": dict(workload="C2: JAX_214-shape scene (3 JAX_269 RPC cameras, GPU-generated rays), img_downscale=4, "
                        "1024 rays x 64 samples, coarse-only, W=512, PE on, fp32", img_downscale=4.0, batch=1024, n_samples=64, sem=False,
               guided=False, sc_lambda=0.0, depth=False, precision="fp32"),
    "c3": dict(workload="C3: JAX_214-shape scene (3 JAX_269 RPC cameras), img_downscale=1, 1024 rays x (64 + 64 guided) "
                        "samples, solar pass, depth + semantic (C=3) heads, W=512, bf16 MLP (fp32 accumulate / params)",
               img_downscale=1.0, batch=1024, n_samples=64, sem=True, guided=True, sc_lambda=0.1, depth=True,
               precision="bf16"),
    # BASELINE.json configs[3]: the 1/2/4/8-GPU training workload.  The 4096-ray batch is
    # GLOBAL (split over the ranks: 4096 / N rays each), so this line scales strongly.
    "c4": dict(workload="C4: JAX_214-shape scene (3 JAX_269 RPC cameras), img_downscale=1, global batch 4096 rays x "
                        "(64 + 64 guided) samples split over the ranks, solar pass, depth + semantic (C=3) heads, W=512, "
                        "bf16 MLP (fp32 accumulate / params), one RCCL gradient all-reduce per step",
               img_downscale=1.0, global_batch=4096, n_samples=64, sem=True, guided=True, sc_lambda=0.1, depth=True,
               precision="bf16"),
    "c5": dict(workload="C5: whole-image inference render (no grad) of a synthetic 4k RPC camera: JAX_269_006 RPC at x5 "
                        "(4065 x 3965 = 16.1M rays), 128 stratified samples/ray, semantic head on (C=3), W=512, bf16 MLP; "
                        "rays sharded by image rows across ranks, each step renders the next 32768-ray chunk of the shard",
               img_downscale=0.2, view="JAX_269_006_RGB", batch=32768, n_samples=128, sem=True, guided=False,
               sc_lambda=0.0, depth=False, precision="bf16", inference=True),
    "c3_fp32": dict(workload="C3 flags at fp32 (parity arithmetic): as c3 with the fp32 MLP",
                    img_downscale=1.0, batch=1024, n_samples=64, sem=True, guided=True, sc_lambda=0.1, depth=True,
                    precision="fp32"),
}


def make_args(c):
    return types.SimpleNamespace(n_samples=c["n_samples"], n_importance=0, model="sp-nerf", beta=False,
                                 guidedsample=c["guided"], sc_lambda=c["sc_lambda"], margin=1e-4, stdscale=1.0,
                                 chunk=5120, noise_std=0.0)


def host_cpus():
    """CPUs this process may actually run on: the affinity mask, capped by the cgroup CPU quota
    (on the GPU box os.cpu_count() reports the whole machine while the job gets a share of it)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            quota, period = f.read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(int(quota) // int(period))))
    except (OSError, ValueError):
        pass
    return n


def cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(c, seconds: float, batch: int, min_steps: int = 3):
    """The parity-pinned CPU restatement (oracle/ref_cpu.py) of the same train step on the host
    cores — render, the trainer's whole loss sum (colour + solar terms + subset depth + semantic
    CE, ``ref_cpu.train_loss`` = main.py:143-174, so the backward runs through the solar pass as
    on the GPU), backward, Adam — on ``batch``-ray batches of the same workload, at least
    ``min_steps`` steps and until ~``seconds`` have passed, after one small warm-up step."""
    import numpy as np
    from oracle import ref_cpu
    from oracle.weights import ModelDims, make_weights

    threads = host_cpus()
    torch.set_num_threads(threads)
    dims = ModelDims(width=512, sem=c["sem"])
    p = ref_cpu.to_params(make_weights(dims, 0), requires_grad=True)
    opt = torch.optim.Adam(list(p.values()), lr=5e-4)
    scene = synthetic_scene(c["img_downscale"] if not c.get("inference") else 4.0, seed=1, device="cuda").to("cpu")
    args = make_args(c)
    B = 64
    g = torch.Generator().manual_seed(0)
    s_final = c["n_samples"] * (2 if c["guided"] else 1)

    def one():
        idx = torch.randint(0, scene.rays.shape[0], (B,), generator=g)
        kw = {}
        if c["guided"]:
            kw = dict(valid_depth=scene.valid_depth[idx], target_depths=scene.depths[idx], target_std=scene.depth_std[idx])
        if c.get("inference"):
            with torch.no_grad():
                ref_cpu.render_rays(p, dims, args, scene.rays[idx], None, scene.sems[idx] if c["sem"] else None, "test")
            return
        res = ref_cpu.render_rays(p, dims, args, scene.rays[idx], None, scene.sems[idx] if c["sem"] else None, "train", **kw)
        loss = ref_cpu.train_loss(res, scene.rgbs[idx], scene.depths[idx], scene.valid_depth[idx], scene.depth_std[idx],
                                  scene.sems[idx] if c["sem"] else None, c["sc_lambda"], 1.0 if c["depth"] else 0.0,
                                  1.0 if c["sem"] else 0.0)
        opt.zero_grad()
        loss.backward()
        opt.step()

    one()                      # warm-up at 64 rays (pages in the CPU kernels)
    B = batch
    n, t0 = 0, time.perf_counter()
    while True:
        one()
        n += 1
        if (time.perf_counter() - t0 >= seconds and n >= min_steps) or n >= 200:
            break
    dt = time.perf_counter() - t0
    what = "inference renders" if c.get("inference") else "train steps"
    return {"value": B * s_final * n / dt, "unit": "ray-samples/s", "cores": threads, "kind": "port",
            "host_cpus_reported": os.cpu_count(), "cpu_model": cpu_model(),
            "sample": f"{n} {what} of {B} rays x {s_final} samples of the same workload (oracle/ref_cpu.py render + "
                      f"ref_cpu.train_loss = the GPU step's loss sum + Adam; torch CPU, fp32, {threads} threads = the "
                      f"CPUs this job may use)"}


def psnr_parity(steps: int = 30, batch: int = 128, n_eval: int = 1024, seed: int = 3, dev="cuda:0",
                precision: str = "fp32"):
    """BASELINE.json's second metric, PSNR vs the reference: the HIP path (``precision`` MLP)
    and the oracle (the reference's render path restated on the CPU in fp32, oracle/ref_cpu.py,
    pinned to its golden fixtures) train the same SPNeRF (W=512, config-2 flags, Adam lr 5e-4)
    from the same init on the same ray batches and random draws of the JAX_269-camera scene at
    img_downscale 4 against the REAL JAX_269 images (JAX_214 is not in the container), then
    render the same held-out rays.  Returns both PSNRs and their difference (the north star
    asks for |delta| <= 0.05 dB)."""
    import numpy as np
    from oracle import ref_cpu
    from oracle.weights import ModelDims, make_weights
    from spnerf_amd import ReplayRandom, random_source

    torch.set_num_threads(int(os.environ.get("OMP_NUM_THREADS", "0")) or min(16, os.cpu_count() or 1))
    dims = ModelDims(width=512)
    w = make_weights(dims, seed)
    model = spnerf_amd.SPNeRF(feat=512, mapping=True, precision=precision).to(dev)
    model.load_state_dict({k: torch.tensor(v) for k, v in w.items()})
    p = ref_cpu.to_params(w, requires_grad=True)
    opt_g = torch.optim.Adam(model.parameters(), lr=5e-4)
    opt_c = torch.optim.Adam(list(p.values()), lr=5e-4)
    args = make_args(CONFIGS["c2"])
    scene = synthetic_scene(4.0, seed=0, device=dev)
    rays, rgbs = scene.rays.cpu(), scene.rgbs.cpu()
    rng = np.random.default_rng(seed)
    perm = rng.permutation(rays.shape[0])
    held, pool = perm[:n_eval], perm[n_eval:]
    S = args.n_samples

    def draws(n):
        return [("rand", rng.uniform(size=(n, S)).astype(np.float32)),
                ("randn", rng.standard_normal((n, S)).astype(np.float32))]

    def psnr(mse):
        return float(-10.0 * np.log10(mse))

    losses = []
    for _ in range(steps):
        idx = torch.as_tensor(rng.choice(pool, batch, replace=False))
        dr = draws(batch)
        with random_source(ReplayRandom(dr)):
            res = spnerf_amd.render_rays({"coarse": model}, args, rays[idx].to(dev), None, mode="train")
        lg = torch.mean((res["rgb_coarse"] - rgbs[idx].to(dev)) ** 2)
        opt_g.zero_grad()
        lg.backward()
        opt_g.step()
        rc = ref_cpu.render_rays(p, dims, args, rays[idx], None, None, "train", draw=ref_cpu_replay(dr))
        lc = torch.mean((rc["rgb_coarse"] - rgbs[idx]) ** 2)
        opt_c.zero_grad()
        lc.backward()
        opt_c.step()
        losses.append((float(lg.item()), float(lc.item())))
    idx = torch.as_tensor(held)
    dr = draws(n_eval)
    with torch.no_grad(), random_source(ReplayRandom(dr)):
        eg = spnerf_amd.render_rays({"coarse": model}, args, rays[idx].to(dev), None, mode="test")["rgb_coarse"].cpu()
    with torch.no_grad():
        ec = ref_cpu.render_rays(p, dims, args, rays[idx], None, None, "test", draw=ref_cpu_replay(dr))["rgb_coarse"]
    pg = psnr(float(torch.mean((eg - rgbs[idx]) ** 2)))
    pc = psnr(float(torch.mean((ec - rgbs[idx]) ** 2)))
    return {"psnr_gpu_db": pg, "psnr_cpu_reference_db": pc, "delta_db": pg - pc, "gpu_mlp": precision, "steps": steps,
            "batch_rays": batch, "held_out_rays": n_eval, "loss_first_last": [losses[0], losses[-1]],
            "max_train_loss_rel_diff": max(abs(a - b) / max(abs(b), 1e-12) for a, b in losses),
            "targets": scene.rgb_source,
            "setup": "W=512 config-2 flags, same init (oracle/weights.py seed 3), same batches and draws, Adam lr 5e-4; "
                     "JAX_269 cameras at img_downscale 4 (JAX_214 absent); CPU side = oracle/ref_cpu.py (fp32)"}


def psnr_long(steps: int = 2000, batch: int = 1024, n_eval: int = 8192, seed: int = 3, dev="cuda:0",
              checkpoints: int = 10):
    """Long-horizon training parity (BASELINE.json "PSNR vs ref", north star |Δ| <= 0.05 dB) of
    the bf16 MLP (configs 3-5) against the fp32 HIP path — itself pinned to the reference at 1e-4
    per step (tests/test_gpu_parity.py) — with the C3 flags (64 + 64 guided samples, solar pass,
    depth + semantic heads, W=512; the trainer's loss sum and Adam lr 5e-4, main.py:97,125-186) on
    the JAX_269 cameras at img_downscale 4 against the REAL JAX_269 images.

    Three arms train side by side from the same init on the same batches and on-device draws:
    ``fp32``, ``bf16`` and ``fp32_control`` — fp32 again from the init scaled by (1 + 1e-6·N(0,1)):
    the distance between two trajectories of the SAME arithmetic, i.e. the floor below which a
    trained-PSNR difference says nothing about precision (Adam turns rounding-level gradient
    differences into lr-sized steps and SIREN training at lr 5e-4 has loss spikes: measured
    replicas differ by up to ~1 dB after 1 000 steps).  Reported beside the final
    PSNRs (and their means over the second half of the held-out checkpoints):
      * ``bf16_inference_at_fp32_trained``: the fp32 arm's final weights rendered by the bf16 MLP —
        the precision effect on PSNR at a trained state, free of trajectory noise;
      * ``grad_rel_err``: at each checkpoint the bf16 MLP's gradient at the fp32 arm's current
        weights on its batch and draws, norm-relative to the fp32 gradient — the bf16 gradients
        stay as close along the whole run as at init."""
    import numpy as np
    from spnerf_amd import PhiloxRandom, random_source

    c = CONFIGS["c3"]
    args = make_args(c)
    R = synthetic_scene(4.0, seed=0, device=dev)
    rng = np.random.default_rng(seed)
    perm = rng.permutation(R.rays.shape[0])
    held, pool = torch.as_tensor(perm[:n_eval], device=dev), perm[n_eval:]
    arms = ("fp32", "bf16", "fp32_control")

    def new_model(prec):
        torch.manual_seed(seed)
        return spnerf_amd.SPNeRF(num_sem_classes=3, s_embedding_factor=1, layers=8, feat=512, mapping=True, sem=True,
                                 precision=prec).to(dev).use_flat_grads()

    models = {a: new_model("bf16" if a == "bf16" else "fp32") for a in arms}
    g = torch.Generator(device="cpu").manual_seed(99)
    with torch.no_grad():
        for p in models["fp32_control"].parameters():
            p.mul_(1 + 1e-6 * torch.randn(p.shape, generator=g).to(dev))
    probe = new_model("bf16")
    probe32 = new_model("fp32")          # the gradient floors below, in fp32 arithmetic
    noise_rng = np.random.default_rng(seed + 1000)   # their second batches (the trajectory's stay as they are)
    opts = {a: spnerf_amd.optim.Adam(list(models[a].parameters()), lr=5e-4) for a in arms}
    srcs = {a: PhiloxRandom(seed=seed) for a in arms}
    floss = FusedRenderLoss(c["sc_lambda"], 1.0, 1.0)

    def train_loss(m, idx):
        res = spnerf_amd.render_rays({"coarse": m}, args, R.rays[idx], None, semantics=R.sems[idx], mode="train",
                                     valid_depth=R.valid_depth[idx], target_depths=R.depths[idx],
                                     target_std=R.depth_std[idx])
        return floss(res, R.rgbs[idx], R.depths[idx], R.valid_depth[idx], R.depth_std[idx], R.sems[idx])[0]

    def held_psnr(m):
        rgb = []
        with torch.no_grad(), random_source(PhiloxRandom(seed=seed + 1)):
            for i0 in range(0, n_eval, 2048):
                ii = held[i0:i0 + 2048]
                rgb.append(spnerf_amd.render_rays({"coarse": m}, args, R.rays[ii], None, semantics=R.sems[ii],
                                                  mode="test")["rgb_coarse"])
        return float(-10.0 * np.log10(float(torch.mean((torch.cat(rgb) - R.rgbs[held]) ** 2))))

    every = max(1, steps // checkpoints)
    curves = {a: [] for a in arms}
    loss_curve = {a: [] for a in arms}
    # every step's training loss of every arm, kept on the device (no per-step host sync)
    loss_trace = torch.zeros(len(arms), steps, device=dev)
    grad_err, grad_err_top, grad_floor = [], [], []

    def probe_grad(m, weights, idx_, round_bf16=False):
        """m's flat gradient at `weights` (optionally rounded to bf16) on idx_, with the fp32 arm's draws."""
        with torch.no_grad():
            for q, p in zip(m.parameters(), weights):
                q.copy_(p.bfloat16().float() if round_bf16 else p)
        src = PhiloxRandom(seed=seed)
        src.copy_state_from(srcs["fp32"])
        for q in m.parameters():
            q.grad = None
        with random_source(src):
            train_loss(m, idx_).backward()
        return m._flat_grad.clone()
    t0 = time.perf_counter()
    for step in range(steps):
        idx = torch.as_tensor(rng.choice(pool, batch, replace=False), device=dev)
        check = step % every == 0 or step == steps - 1
        if check:   # the bf16 gradient at the fp32 arm's weights, same batch, same draws
            w32 = list(models["fp32"].parameters())
            g16 = probe_grad(probe, w32, idx)
            # two floors at the same weights in fp32 arithmetic: the weights rounded to bf16 (same
            # batch and draws: what storing the weights in bf16 alone changes) and another batch of
            # the same size (the minibatch noise every step of the optimiser already carries)
            g_round = probe_grad(probe32, w32, idx, round_bf16=True)
            g_batch = probe_grad(probe32, w32, torch.as_tensor(noise_rng.choice(pool, batch, replace=False),
                                                               device=dev))
        for a in arms:
            m = models[a]
            opts[a].zero_grad(set_to_none=True)
            with random_source(srcs[a]):
                loss = train_loss(m, idx)
            loss.backward()
            if check and a == "fp32":
                g32 = m._flat_grad
                n32 = torch.linalg.norm(g32)
                grad_err.append((step, float(torch.linalg.norm(g16 - g32) / n32)))
                grad_floor.append({"step": step, "bf16_weights": float(torch.linalg.norm(g_round - g32) / n32),
                                   "other_batch": float(torch.linalg.norm(g_batch - g32) / n32),
                                   "grad_norm": float(n32)})
                # where it is: the parameters with the largest share of the error, each with its
                # fp32 gradient's norm and its other-batch difference
                off, parts = 0, []
                for name, p in m.named_parameters():
                    n = p.numel()
                    seg = slice(off, off + n)
                    d = float(torch.linalg.norm(g16[seg] - g32[seg]))
                    parts.append((d, name, float(torch.linalg.norm(g32[seg])),
                                  float(torch.linalg.norm(g_batch[seg] - g32[seg]))))
                    off += n
                parts.sort(reverse=True)
                grad_err_top.append((step, [(nm, round(d, 6), round(r, 6), round(b, 6)) for d, nm, r, b in parts[:3]]))
            opts[a].step()
            loss_trace[arms.index(a), step] = loss.detach()
            if check:
                loss_curve[a].append((step, float(loss.detach())))
        if check and step > 0:
            for a in arms:
                curves[a].append((step + 1, held_psnr(models[a])))
            print(f"psnr_long: step {step + 1}/{steps} " + " ".join(f"{a} {curves[a][-1][1]:.3f}" for a in arms)
                  + f" grad_rel_err {grad_err[-1][1]:.2e} ({time.perf_counter() - t0:.0f} s)", file=sys.stderr, flush=True)
    train_s = time.perf_counter() - t0
    final = {a: curves[a][-1][1] for a in arms}
    half = [k for k in range(len(curves["fp32"])) if curves["fp32"][k][0] > steps // 2]
    tail = {a: float(np.mean([curves[a][k][1] for k in half])) for a in arms}
    with torch.no_grad():
        for q, p in zip(probe.parameters(), models["fp32"].parameters()):
            q.copy_(p)
    p16 = held_psnr(probe)
    lt = loss_trace.cpu().numpy()
    # loss spikes (SIREN at lr 5e-4): per arm the largest loss after the first 10 % of the run, as a
    # multiple of the arm's running median of the preceding 50 steps, and where it happened
    spikes = {}
    for k, a in enumerate(arms):
        v = lt[k]
        best = (0.0, -1)
        for t in range(max(50, steps // 10), steps):
            med = float(np.median(v[t - 50:t]))
            if med > 0 and v[t] / med > best[0]:
                best = (float(v[t] / med), t)
        spikes[a] = {"max_ratio_to_running_median": best[0], "step": best[1],
                     "final_loss_mean_last_50": float(v[-50:].mean()) if steps >= 50 else float(v.mean())}
    worst = max(range(len(grad_err)), key=lambda k: grad_err[k][1])
    return {"psnr_bf16_db": final["bf16"], "psnr_fp32_hip_db": final["fp32"],
            "delta_db": final["bf16"] - final["fp32"],
            "control_delta_db": final["fp32_control"] - final["fp32"],
            "tail_mean_delta_db": tail["bf16"] - tail["fp32"],
            "tail_mean_control_delta_db": tail["fp32_control"] - tail["fp32"],
            "bf16_inference_at_fp32_trained": {"psnr_db": p16, "delta_db": p16 - final["fp32"]},
            "grad_rel_err": grad_err, "max_grad_rel_err": max(e for _, e in grad_err),
            "grad_floors": grad_floor,
            "max_grad_err_over_batch_noise": max(e / f["other_batch"] for (_, e), f in zip(grad_err, grad_floor)),
            "grad_err_top_params": grad_err_top,
            "worst_grad_checkpoint": {"step": grad_err[worst][0], "grad_rel_err": grad_err[worst][1],
                                      "floors": grad_floor[worst],
                                      "top_params": grad_err_top[worst][1],
                                      "top_params_columns": "name, |g_bf16 - g_fp32|, |g_fp32|, |g_fp32(other batch) - g_fp32|",
                                      "fp32_loss_there": float(lt[0, grad_err[worst][0]]),
                                      "fp32_loss_median_before": float(np.median(lt[0, max(0, grad_err[worst][0] - 50):
                                                                                     max(1, grad_err[worst][0])]))},
            "loss_spikes": spikes,
            "loss_trace_every_10": {a: [float(x) for x in lt[k, ::10]] for k, a in enumerate(arms)},
            "psnr_curve": curves, "loss_curve": loss_curve,
            "steps": steps, "batch_rays": batch, "held_out_rays": n_eval, "train_seconds": train_s,
            "targets": R.rgb_source,
            "setup": "C3 flags (64+64 guided, solar pass, depth + semantic heads, W=512) at img_downscale 4 on the "
                     "JAX_269 cameras (JAX_214 absent), trainer's loss sum, Adam lr 5e-4, same init / batches / "
                     "on-device Philox draws for every arm; fp32_control = fp32 from the init x (1 + 1e-6 N(0,1)); the "
                     "fp32 HIP path is the reference-pinned one (1e-4 per step)"}


def quantiles(v):
    import numpy as np
    return {"median": float(np.median(v)), "p90": float(np.quantile(v, 0.9)), "max": float(np.max(v)), "n": int(len(v))}


# The bf16 gradient gates of tests/test_gpu_psnr.py, applied to every checkpoint the bench measures:
# the norm-relative error against the fp32 gradient at the same weights, batch and draws (median and
# max), and the same error as a fraction of the fp32 gradient's own change between two batches at
# those weights (the minibatch noise the optimiser steps on).  DESIGN.md §5.
GRAD_GATES = {"median_rel_err": 0.03, "max_rel_err": 0.2, "max_over_batch_noise": 0.25}


def grad_gates(errs, ratios):
    import numpy as np
    got = {"median_rel_err": float(np.median(errs)), "max_rel_err": float(np.max(errs)),
           "max_over_batch_noise": float(np.max(ratios))}
    return {k: {"value": got[k], "bound": GRAD_GATES[k], "pass": bool(got[k] <= GRAD_GATES[k])} for k in GRAD_GATES}


def psnr_seeds(seeds=(3, 4, 5, 6, 7, 8), steps: int = 1000, batch: int = 512, n_eval: int = 4096, dev="cuda:0",
               checkpoints: int = 8, detail_path: str | None = None):
    """Paired multi-seed trained-PSNR statistics (BASELINE.json "PSNR vs ref", north star within
    0.05 dB): ``psnr_long`` once per seed (its own init, batches and on-device draws), three arms
    each (fp32 = the reference-pinned HIP path, bf16, fp32_control = fp32 from the init x (1 +
    1e-6 N(0,1))).  Reported: per seed the final PSNRs; the mean and standard error over seeds of
    Δ(bf16 − fp32) and of Δ(control − fp32) — the control's spread is trajectory noise of the SAME
    arithmetic; whether 0.05 dB is resolvable at this n (2 standard errors of the control below
    0.05 dB); and the precision effect free of trajectory noise: the fp32-trained weights rendered
    by the bf16 MLP (Δ per seed, mean, SE) and the bf16 gradient's norm-relative error at the fp32
    trajectory's weights (max over every checkpoint of every seed)."""
    import numpy as np
    per = []
    t0 = time.perf_counter()
    for sd in seeds:
        r = psnr_long(steps=steps, batch=batch, n_eval=n_eval, seed=sd, dev=dev, checkpoints=checkpoints)
        per.append({"seed": sd, "fp32_db": r["psnr_fp32_hip_db"], "bf16_db": r["psnr_bf16_db"],
                    "control_db": r["psnr_fp32_hip_db"] + r["control_delta_db"], "delta_db": r["delta_db"],
                    "control_delta_db": r["control_delta_db"],
                    "infer_delta_db": r["bf16_inference_at_fp32_trained"]["delta_db"],
                    "max_grad_rel_err": r["max_grad_rel_err"],
                    "max_grad_err_over_batch_noise": r["max_grad_err_over_batch_noise"],
                    "grad_rel_err": r["grad_rel_err"],
                    "grad_floors": r["grad_floors"],
                    "worst_grad_checkpoint": r["worst_grad_checkpoint"],
                    "loss_spikes": r["loss_spikes"],
                    "loss_trace_every_10": r["loss_trace_every_10"],
                    "final_loss": {a: v[-1][1] for a, v in r["loss_curve"].items()}})
        if detail_path:   # the full per-seed record (traces, floors) as a side file, rewritten per seed
            with open(detail_path, "w") as f:
                json.dump({"per_seed": per}, f)
        print(f"psnr_seeds: seed {sd} done ({time.perf_counter() - t0:.0f} s): " +
              " ".join(f"{k} {v:.3f}" for k, v in per[-1].items() if k.endswith("_db")), file=sys.stderr, flush=True)

    def stat(key):
        v = np.array([q[key] for q in per], dtype=np.float64)
        se = float(v.std(ddof=1) / np.sqrt(len(v))) if len(v) > 1 else float("nan")
        return float(v.mean()), se

    d_m, d_se = stat("delta_db")
    c_m, c_se = stat("control_delta_db")
    i_m, i_se = stat("infer_delta_db")
    resolvable = bool(2 * c_se < 0.05)
    errs = np.array([e for q in per for _, e in q["grad_rel_err"]])
    ratios = np.array([e / f["other_batch"] for q in per for (_, e), f in zip(q["grad_rel_err"], q["grad_floors"])])
    rounds = np.array([f["bf16_weights"] for q in per for f in q["grad_floors"]])
    # a seed whose final checkpoint falls inside a loss spike of any arm (loss over the last 50 steps
    # more than 3x the fp32 arm's): its final-PSNR deltas measure where the spike caught the arm
    spiked = [q["seed"] for q in per
              if max(q["loss_spikes"][a]["final_loss_mean_last_50"] for a in q["loss_spikes"])
              > 3 * min(q["loss_spikes"][a]["final_loss_mean_last_50"] for a in q["loss_spikes"])]
    calm = [q for q in per if q["seed"] not in spiked]
    return {"n_seeds": len(per), "steps": steps, "batch_rays": batch, "held_out_rays": n_eval, "per_seed": per,
            "delta_bf16_minus_fp32_db": {"mean": d_m, "se": d_se},
            "delta_control_minus_fp32_db": {"mean": c_m, "se": c_se},
            "bf16_inference_at_fp32_trained_db": {"mean": i_m, "se": i_se},
            "max_grad_rel_err": max(q["max_grad_rel_err"] for q in per),
            "worst_grad_checkpoint": max(({"seed": q["seed"], **q["worst_grad_checkpoint"]} for q in per),
                                         key=lambda w: w["grad_rel_err"]),
            "grad_rel_err_quantiles": quantiles(errs),
            "grad_err_over_batch_noise_quantiles": quantiles(ratios),
            "bf16_weight_rounding_floor_quantiles": quantiles(rounds),
            "gradient_gates": grad_gates(errs, ratios),
            "median_delta_db": {"bf16": float(np.median([q["delta_db"] for q in per])),
                                "control": float(np.median([q["control_delta_db"] for q in per]))},
            "seeds_ending_in_a_loss_spike": spiked,
            "delta_db_without_them": {"bf16": float(np.mean([q["delta_db"] for q in calm])) if calm else None,
                                      "control": float(np.mean([q["control_delta_db"] for q in calm])) if calm else None,
                                      "n": len(calm)},
            "resolvable_0p05_db": resolvable,
            "statement": (f"trained-PSNR difference bf16 - fp32 = {d_m:+.3f} +- {d_se:.3f} dB (mean +- SE over {len(per)} "
                          f"seeds), fp32 control - fp32 = {c_m:+.3f} +- {c_se:.3f} dB: 0.05 dB is "
                          + ("resolvable" if resolvable else "NOT resolvable")
                          + f" at n = {len(per)} from trained PSNR (trajectory noise of identical arithmetic is "
                          f"{c_se * np.sqrt(len(per)):.2f} dB per seed); the precision effect at a trained state, free "
                          f"of that noise: bf16 inference of the fp32-trained weights {i_m:+.4f} +- {i_se:.4f} dB"),
            "train_seconds": time.perf_counter() - t0,
            "setup": "bench.psnr_long per seed: C3 flags at img_downscale 4 on the JAX_269 cameras against the real "
                     "JAX_269 images (JAX_214 absent), trainer's loss sum, Adam lr 5e-4"}


# The driver parses the ONE JSON line rank 0 prints; round 5's 68 KB line (per-seed loss traces
# of the PSNR study) was not parsed at all.  Every line is held to this budget by construction
# (finalize_line), and tests/test_bench_line.py / test_gpu_bench_lines.py check it.
LINE_BUDGET = 8192


def compact(v, sig: int = 5):
    """``v`` with every float rounded to ``sig`` significant digits (dicts / lists recursively)."""
    if isinstance(v, float):
        if not math.isfinite(v) or v == 0.0:
            return v
        return float(f"{v:.{sig}g}")
    if isinstance(v, dict):
        return {k: compact(x, sig) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [compact(x, sig) for x in v]
    return v


def psnr_seeds_summary(r: dict) -> dict:
    """The PSNR study's statistics for the bench line: per seed the final dB figures and the worst
    gradient error, the across-seed means / SEs, the gates, the worst checkpoint (seed, step, error,
    its two floors) and the spike list — no per-step traces or per-checkpoint arrays (those go to
    the ``--psnr-detail`` side file)."""
    w = r["worst_grad_checkpoint"]
    keep = ("seed", "fp32_db", "bf16_db", "control_db", "delta_db", "control_delta_db", "infer_delta_db",
            "max_grad_rel_err", "max_grad_err_over_batch_noise")
    return {"n_seeds": r["n_seeds"], "steps": r["steps"], "batch_rays": r["batch_rays"],
            "held_out_rays": r["held_out_rays"],
            "per_seed": [{k: q[k] for k in keep} for q in r["per_seed"]],
            "delta_bf16_minus_fp32_db": r["delta_bf16_minus_fp32_db"],
            "delta_control_minus_fp32_db": r["delta_control_minus_fp32_db"],
            "bf16_inference_at_fp32_trained_db": r["bf16_inference_at_fp32_trained_db"],
            "gradient_gates": {k: {"value": g["value"], "pass": g["pass"]} for k, g in r["gradient_gates"].items()},
            "worst_grad_checkpoint": {"seed": w["seed"], "step": w["step"], "grad_rel_err": w["grad_rel_err"],
                                      "bf16_weights_floor": w["floors"]["bf16_weights"],
                                      "other_batch_floor": w["floors"]["other_batch"]},
            "seeds_ending_in_a_loss_spike": r["seeds_ending_in_a_loss_spike"],
            "resolvable_0p05_db": r["resolvable_0p05_db"], "train_seconds": r["train_seconds"]}


def _line_size(out) -> int:
    return len(json.dumps(out))


def finalize_line(out: dict, budget: int = LINE_BUDGET) -> dict:
    """The record rank 0 prints, held to ``budget`` bytes of JSON: floats to 5 significant digits,
    the PSNR study reduced to its summary, then — only while still over — the optional detail
    trimmed in a fixed order (named in ``trimmed``).  The headline fields, ``roofline``,
    ``cpu_baseline``, ``mlp_mfma_utilisation`` and the secondaries' values and rooflines are never
    dropped."""
    out = dict(out)
    if "psnr_seeds" in out and "per_seed" in out["psnr_seeds"] and "grad_rel_err" in out["psnr_seeds"]["per_seed"][0]:
        out["psnr_seeds"] = psnr_seeds_summary(out["psnr_seeds"])
    out = compact(out)
    trimmed = []

    def over():
        return _line_size(dict(out, trimmed=trimmed)) > budget

    def strip_kernel_names(d):
        if isinstance(d, dict) and "roofline" in d and isinstance(d["roofline"], dict):
            d["roofline"] = {k: v for k, v in d["roofline"].items() if k not in ("traffic_source", "traffic_unit")}

    steps = [
        ("psnr_parity: figures only", lambda: out.__setitem__("psnr_parity", {
            p: {k: v for k, v in r.items() if k in ("psnr_gpu_db", "psnr_cpu_reference_db", "delta_db", "steps",
                                                   "batch_rays", "max_train_loss_rel_diff")}
            for p, r in out["psnr_parity"].items()}) if "psnr_parity" in out else None),
        ("kernels: top 8", lambda: out.__setitem__("kernels", dict(list(out["kernels"].items())[:8]))
         if isinstance(out.get("kernels"), dict) else None),
        ("rooflines_top3", lambda: out.pop("rooflines_top3", None)),
        ("roofline traffic_source", lambda: [strip_kernel_names(d) for d in [out] + list(out.get("secondary", {}).values())]),
        ("psnr_seeds: per_seed", lambda: out.get("psnr_seeds", {}).pop("per_seed", None)),
        ("secondary workloads", lambda: [d.get("config", {}).pop("workload", None)
                                         for d in out.get("secondary", {}).values()]),
        ("kernels", lambda: out.pop("kernels", None)),
        ("parity_note", lambda: out.pop("parity_note", None)),
    ]
    for name, fn in steps:
        if not over():
            break
        fn()
        trimmed.append(name)
    if trimmed:
        out["trimmed"] = trimmed
    return out


def ref_cpu_replay(draws):
    """The oracle's draw(kind, shape) callable over a recorded list of draws."""
    it = iter(draws)

    def draw(kind, shape):
        k, arr = next(it)
        assert k == kind and tuple(arr.shape) == tuple(shape), (k, kind, arr.shape, shape)
        return torch.as_tensor(arr)
    return draw


def measured_traffic(config, rays_per_rank, kernel_class):
    """HBM bytes per launch of ``kernel_class`` from the committed PMC profile of THIS workload at
    THIS batch (rays per rank) — tools/pmc_bench.sh + tools/traffic_summary.py: separate
    FETCH_SIZE / WRITE_SIZE passes, bytes = 2*FETCH_SIZE + WRITE_SIZE per MI355X_MICROARCH.md's
    gfx950 correction.  None when no profile of that (config, rays per rank) is committed (PMC
    counters cannot be read from inside the bench process, hence the profile file)."""
    for rnd in ("r06", "r05", "r04"):
        rel = f"profiles/{rnd}/traffic_{config}_rays{rays_per_rank}.json"
        try:
            with open(os.path.join(ROOT, rel)) as f:
                t = json.load(f)[kernel_class]
            if t.get("rays_per_rank") != rays_per_rank:
                continue
            return t["hbm_bytes_per_launch"], f"{rel} ({t['launches']} launches)"
        except (OSError, KeyError, ValueError):
            continue
    return None, None



def dominant_class():
    """The kernel function (profiling class) with the most time in the profiled steps."""
    classes = _lib.prof_classes()
    return max(classes, key=lambda k: _lib.prof_read(k)["ms"]) if classes else None


def roofline_of(dom, nt, traffic=None, traffic_src=None):
    """Roofline of the dominant kernel: the bound is the one its algorithmic intensity (FLOP per
    algorithmic HBM byte, both counted per launch by the library) sits under — MFMA when it is
    above the ridge peak_flops / 8 TB/s (fp32: 19.7 FLOP/B, bf16: 315), HBM below it (the bf16
    GEMMs at K = 512: ≈127 FLOP/B for a sine layer, reading 2 B and writing 4 B per output); a
    kernel without MFMAs is HBM-bound.  Both fractions are reported; ``frac`` is the binding one."""
    if dom in GEMM_CLASSES:
        dom_name, peak = GEMM_CLASSES[dom]
        if "<IP>" in dom_name:   # the template instance the library launches (product build: <3, false>)
            ip = _lib.get_option("tn_bf16_ip") if _lib.has_option("tn_bf16_ip") else 3
            pf = _lib.has_option("tn_bf16_pf") and _lib.get_option("tn_bf16_pf") == 1
            dom_name = dom_name.replace("<IP>", f"<{ip}, {'true' if pf else 'false'}>")
    else:
        dom_name, peak = HBM_CLASSES.get(dom, dom), None
    secs = nt["ms"] * 1e-3
    tflops = nt["flop"] / secs / 1e12 if secs else 0.0
    gbs = nt["bytes"] / secs / 1e9 if secs else 0.0
    ridge = peak * 1e3 / HBM_PEAK_GBS if peak else None  # FLOP per byte
    intensity = nt["flop"] / nt["bytes"] if nt["bytes"] else (float("inf") if nt["flop"] else 0.0)
    r = {"kernel": f"{dom} ({dom_name})", "intensity_flop_per_byte": intensity, "ridge_flop_per_byte": ridge,
         "mfma_frac": tflops / peak if peak else None, "hbm_frac": gbs / HBM_PEAK_GBS}
    if peak and intensity >= ridge:
        r.update(bound="mfma", achieved=tflops, peak=peak, unit="TFLOP/s", frac=tflops / peak)
    else:
        r.update(bound="hbm", achieved=gbs, peak=HBM_PEAK_GBS, unit="GB/s", frac=gbs / HBM_PEAK_GBS)
    r.update(traffic=traffic, traffic_unit="HBM bytes per launch", traffic_source=traffic_src,
             algorithmic_bytes_per_launch=nt["bytes"] / max(1, nt["launches"]),
             avg_launch_us=1e3 * nt["ms"] / max(1, nt["launches"]))
    return r

def top_rooflines(config, rays_per_rank, n):
    """roofline_of for the n MFMA kernel functions with the most time in the profiled steps."""
    classes = [k for k in _lib.prof_classes() if k in GEMM_CLASSES]
    classes.sort(key=lambda k: -_lib.prof_read(k)["ms"])
    out = {}
    for k in classes[:n]:
        r = roofline_of(k, _lib.prof_read(k), *measured_traffic(config, rays_per_rank, k))
        out[k] = {f: r[f] for f in ("bound", "achieved", "unit", "frac", "mfma_frac", "hbm_frac", "avg_launch_us",
                                    "traffic", "algorithmic_bytes_per_launch")}
    return out


def gemm_totals(steps):
    """Every MFMA launch of the profiled steps (GEMMs and fused trunk / heads kernels): counted
    FLOP / summed kernel time, against the peak of each launch's dtype (time-weighted) — the
    MLP's MFMA utilisation, BASELINE.json's north-star figure (target >= 0.40)."""
    flop = ms = peak_ms = 0.0
    for k, (_, peak) in GEMM_CLASSES.items():
        r = _lib.prof_read(k)
        flop += r["flop"]
        ms += r["ms"]
        peak_ms += peak * r["ms"]
    if ms == 0:
        return None
    tf = flop / (ms * 1e-3) / 1e12
    peak = peak_ms / ms
    return {"tflops": tf, "peak": peak, "frac": tf / peak, "ms_per_step": ms / steps, "target": MFMA_TARGET}


def kernel_table(steps):
    """Per kernel function of the profiled steps: launches, ms per step, average launch, achieved
    TFLOP/s and algorithmic GB/s."""
    out = {}
    for k in _lib.prof_classes():
        s = _lib.prof_read(k)
        if s["launches"]:
            out[k] = {"launches": s["launches"], "ms_per_step": s["ms"] / steps, "avg_us": 1e3 * s["ms"] / s["launches"],
                      "tflops": s["flop"] / (s["ms"] * 1e-3) / 1e12 if s["flop"] else None,
                      "gbs": s["bytes"] / (s["ms"] * 1e-3) / 1e9 if s["bytes"] else None}
    return dict(sorted(out.items(), key=lambda kv: -kv[1]["ms_per_step"]))


DUMP_BUDGET = 48 << 20   # bytes of --dump-outputs arrays in all


def dump_outputs(path, tensors, budget: int = DUMP_BUDGET):
    """``--dump-outputs``: every tensor of ``tensors`` (name -> tensor; other values are skipped)
    as ``path/<name>.npy``, floating point as float32 (float64 stays), integers as float64.
    The arrays together hold at most ``budget`` bytes: the small ones whole, and of each one above
    its equal share of what is left a fixed sample — the sorted flat indices
    ``default_rng(0).choice(numel, share)``, a function of the array's size and the set of names
    only, so two builds of the same workload write the same elements."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    arrs = {}
    for name, t in tensors.items():
        if not isinstance(t, torch.Tensor):
            continue
        t = t.detach()
        keep = torch.float64 if (t.dtype == torch.float64 or not t.dtype.is_floating_point) else torch.float32
        arrs[name] = t.to(keep).cpu().numpy()
    left, share = budget, {}
    for k, name in enumerate(sorted(arrs, key=lambda n: arrs[n].nbytes)):   # smallest first: water-filling
        share[name] = min(arrs[name].nbytes, left // (len(arrs) - k))
        left -= share[name]
    for name, v in arrs.items():
        if share[name] < v.nbytes:
            idx = np.sort(np.random.default_rng(0).choice(v.size, share[name] // v.itemsize, replace=False))
            v = v.reshape(-1)[idx]
        np.save(os.path.join(path, f"{name}.npy"), v)


def c5_shard(c, rank, world, dev, img_downscale=None):
    """Rank ``rank``'s row shard [r0, r1) of the C5 image: its RPC rays (GPU generator), synthetic
    semantic labels as a fixed function of the GLOBAL ray index (so a shard's labels do not depend
    on the sharding), and the seeded SPNeRF.  Returns (rays, sems, model, args, h, w, r0)."""
    from spnerf_amd.satellite import image_rays, load_cameras
    ds = c["img_downscale"] if img_downscale is None else img_downscale
    cams = load_cameras()
    meta = cams["images"][c["view"]]
    h, w = int(meta["height"] // ds), int(meta["width"] // ds)
    r0, r1 = rank * h // world, (rank + 1) * h // world
    rays = image_rays(meta, ds, cams["scene_loc"], crop=(r0, 0, r1 - r0, w), device=dev)
    gid = torch.arange(r0 * w, r1 * w, device=dev, dtype=torch.int64)
    u = ((gid * 0x9E3779B1) & 0xFFFFFFFF).double() / 2.0 ** 32     # labels 0/1/2/ignore at 45/30/15/10 %
    sems = torch.full_like(gid, -100)
    sems = torch.where(u < 0.9, torch.full_like(gid, 2), sems)
    sems = torch.where(u < 0.75, torch.full_like(gid, 1), sems)
    sems = torch.where(u < 0.45, torch.zeros_like(gid), sems)
    torch.manual_seed(0)
    model = spnerf_amd.SPNeRF(num_sem_classes=3, s_embedding_factor=1, layers=8, feat=512, mapping=True, sem=c["sem"],
                              precision=c["precision"]).to(dev)
    return rays, sems, model, make_args(c), h, w, r0


def run_inference(a, config, rank, world, dev, steps=None, warmup=None, secondary=False):
    """Config 5: ray-sharded whole-image inference.  Rank r generates rows [r·h/N, (r+1)·h/N)
    of the image with the GPU RPC ray generator, then each step renders the next chunk of its
    shard (render_rays in test mode: stratified samples, MLP without saved activations,
    compositing).  No collective: the ranks only meet at the timing barriers.  Returns the JSON
    record (``secondary``: the C5 line inside the default C4 line, its own batch, no CPU leg)."""
    c = CONFIGS[config]
    steps = a.steps if steps is None else steps
    warmup = a.warmup if warmup is None else warmup
    rays, sems, model, args, h, w, r0 = c5_shard(c, rank, world, dev)
    B, n = (0 if secondary else a.global_batch) or c["batch"], rays.shape[0]
    pos = [0]
    # stratified draws on-device (Philox keyed by the global ray id), as in training: no RNG launch
    src = spnerf_amd.PhiloxRandom(seed=0)

    @torch.no_grad()
    def step():
        i0 = pos[0]
        idx = torch.arange(i0, i0 + B, device=dev) % n
        pos[0] = (i0 + B) % n
        src.ray_offset = r0 * w + i0
        with spnerf_amd.random_source(src):
            return spnerf_amd.render_rays({"coarse": model}, args, rays[idx], None, semantics=sems[idx], mode="test")

    wd = dp.StepWatchdog(rank=rank, mode="eager inference")
    for i in range(warmup):
        wd.beat(i, "warmup")
        step()
    wd.beat(0, "sync after warmup")
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    _lib.prof_reset()
    _lib.prof_enable(True)
    t0 = time.perf_counter()
    for i in range(steps):
        wd.beat(i, "timed")
        res = step()
    wd.beat(steps, "sync after timed steps")
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    t1 = time.perf_counter()
    wd.close()
    _lib.prof_enable(False)
    elapsed = torch.tensor([t1 - t0], dtype=torch.float64, device=dev)
    if world > 1:
        dist.all_reduce(elapsed, op=dist.ReduceOp.MAX)
    elapsed = float(elapsed.item())
    if a.dump_outputs and rank == 0 and not secondary:
        dump_outputs(a.dump_outputs, res)
    dom = dominant_class()
    nt = _lib.prof_read(dom)
    total = world * B * c["n_samples"] * steps
    value = total / elapsed
    out = {
        "metric": "ray-samples/sec (inference render)", "value": value, "unit": "ray-samples/s", "n_gpus": world,
        "steps": steps, "warmup": warmup, "ms_per_step": 1e3 * elapsed / steps, "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": c["precision"],
        "data": "synthetic RPC camera rays (JAX_269_006 RPC at x5), synthetic semantic labels, seeded-random SPNeRF init",
        "config": {"workload": c["workload"], "global_batch": B * world, "samples_per_ray": c["n_samples"],
                   "parallelism": f"ray-shard{world}", "image_rays": h * w},
        "image_seconds_projected": h * w * c["n_samples"] / value,
        "roofline": roofline_of(dom, nt, *measured_traffic(config, B, dom)),
        "mlp_mfma_utilisation": gemm_totals(steps),
        "kernels": kernel_table(steps),
        "finite": bool(torch.isfinite(res["rgb_coarse"]).all()),
    }
    if a.full_image and not secondary:
        out["full_image"] = full_image(rays, sems, model, args, B, rank, world, dev, h, w, c, r0)
    if a.full and rank == 0 and world == 1 and not a.no_cpu_baseline and not secondary:
        out["cpu_baseline"] = cpu_baseline(c, a.cpu_seconds, a.cpu_batch or 1024)
    return out


@torch.no_grad()
def full_image(rays, sems, model, args, B, rank, world, dev, h, w, c, r0=0, return_image=False):
    """The whole C5 image: every rank renders all rays of its row shard in chunks of B into an
    HBM-resident [rows·w][4] (rgb, depth) buffer, then the shards are gathered to rank 0 (one
    all_gather of equal, padded shards; on CPU copies when the group is gloo).  Timed from the
    first chunk to the gathered image on rank 0, max over ranks.  The stratified draws are
    on-device Philox keyed by (seed, step 0, GLOBAL ray id = r0·w + index in the shard), so the
    image does not depend on the sharding or the chunking (tests/test_gpu_bench_lines.py)."""
    from spnerf_amd import PhiloxRandom, random_source
    n = rays.shape[0]
    shard = torch.empty(n, 4, device=dev)
    src = PhiloxRandom(seed=0)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with random_source(src):
        for i0 in range(0, n, B):
            i1 = min(n, i0 + B)
            src.ray_offset = r0 * w + i0
            src.reset_step(-1)
            res = spnerf_amd.render_rays({"coarse": model}, args, rays[i0:i1], None, semantics=sems[i0:i1], mode="test")
            shard[i0:i1, 0:3] = res["rgb_coarse"]
            shard[i0:i1, 3] = res["depth_coarse"]
    torch.cuda.synchronize()
    t_render = time.perf_counter() - t0
    if world > 1:
        rows_max = (h + world - 1) // world
        pad = torch.zeros(rows_max * w, 4, device=dev)
        pad[:n] = shard
        gloo = dist.get_backend() == "gloo"
        src = pad.cpu() if gloo else pad
        parts = [torch.empty_like(src) for _ in range(world)]
        dist.all_gather(parts, src)
        if rank == 0:
            image = torch.cat([parts[r][:((r + 1) * h // world - r * h // world) * w] for r in range(world)]).to(dev)
        else:
            image = None
    else:
        image = shard
    torch.cuda.synchronize()
    t = torch.tensor([time.perf_counter() - t0, t_render], dtype=torch.float64, device=dev)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    info = {"rays": h * w, "height": h, "width": w, "samples_per_ray": c["n_samples"], "seconds": float(t[0]),
            "render_seconds_max_rank": float(t[1]), "gathered_to_rank0": world > 1,
            "ray_samples_per_s": h * w * c["n_samples"] / float(t[0])}
    if rank == 0:
        img = image.reshape(h, w, 4)
        info.update({"finite": bool(torch.isfinite(img).all()), "rgb_mean": [float(v) for v in img[..., :3].mean((0, 1))],
                     "depth_min_max": [float(img[..., 3].min()), float(img[..., 3].max())]})
        if return_image:
            info["image"] = img
    return info


def free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch_ranks(a) -> int:
    """``--gpus N`` outside torchrun: start the N ranks as a torch.distributed.run CHILD process
    (nothing here has touched the GPU — device_count() does not initialise HIP) and return its
    exit code.  More GPUs than the node has is an error, never a silent 1-GPU run."""
    import subprocess
    have = torch.cuda.device_count()
    if not a.share_device and have < a.gpus:
        print(f"bench: --gpus {a.gpus} but this node has {have} GPU(s)", file=sys.stderr)
        return 2
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__), *sys.argv[1:]]
    return subprocess.call(cmd)


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", default="c4", choices=sorted(CONFIGS))
    ap.add_argument("--full", action="store_true",
                    help="beside the headline figure, every other leg: the C2 / C5 secondaries, the CPU baseline, the "
                         "PSNR studies, the per-kernel / roofline figures from profiled eager steps after a graph-mode "
                         "timed region, the paired replays of the exposed collective (off by default)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last timed step computed (the render's outputs, the "
                         "loss, the flat gradient and the updated parameters) as DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="(--full) skip the CPU baseline and the PSNR studies")
    ap.add_argument("--no-secondary", action="store_true",
                    help="(--full) skip the C2 / C5 lines reported beside the default C4 at N=1")
    ap.add_argument("--torch-adam", action="store_true", help="torch.optim.Adam(fused=True) instead of spnerf_amd.optim.Adam")
    ap.add_argument("--torch-loss", action="store_true", help="the losses module (plain torch) instead of the fused loss kernels")
    ap.add_argument("--torch-gather", action="store_true", help="torch indexing per field instead of the one-launch batch gather")
    ap.add_argument("--cpu-seconds", type=float, default=15.0)
    ap.add_argument("--psnr-steps", type=int, default=0,
                    help="steps per seed of the paired bf16-vs-fp32 training PSNR study (psnr_seeds; 0 = skip, the "
                         "default: ~275 s for 6 seeds x 1000 steps, and it cannot resolve 0.05 dB — DESIGN.md §5)")
    ap.add_argument("--psnr-seeds", type=int, default=6, help="seeds of that study (psnr_seeds)")
    ap.add_argument("--psnr-detail", default=None,
                    help="write the PSNR study's full per-seed record (loss traces, floors) to this JSON file; the "
                         "line carries its summary only")
    ap.add_argument("--psnr-parity-steps", type=int, default=30,
                    help="steps of the 30-step oracle-anchored psnr_parity legs (fp32, bf16; 0 = skip)")
    ap.add_argument("--cpu-batch", type=int, default=0,
                    help="rays per CPU-baseline step (default: the GPU step's batch, at most 512)")
    ap.add_argument("--full-image", action="store_true",
                    help="C5: after the timed chunks, render every ray of the image (each rank its row shard) and "
                         "gather rgb + depth to rank 0; reported as full_image")
    ap.add_argument("--graph", dest="graph", action="store_true", default=True,
                    help="replay render+loss+backward as a HIP graph (default)")
    ap.add_argument("--eager", dest="graph", action="store_false", help="launch every kernel from Python")
    ap.add_argument("--prof-steps", type=int, default=3, help="eager steps timed per kernel in graph mode")
    ap.add_argument("--option", action="append", default=[], metavar="NAME=VALUE",
                    help="library kernel switch (spnerf_set_option), e.g. fused_trunk=0, nt_f32_variant=4")
    ap.add_argument("--global-batch", type=int, default=0, help="override the config's global batch (rays per step)")
    ap.add_argument("--no-defer-wgrad", action="store_true",
                    help="one trunk weight-gradient GEMM per pass instead of one over the main + solar passes")
    ap.add_argument("--no-reuse-pass1", action="store_true",
                    help="evaluate the guided pass's stratified points twice, as the reference does (pass 1, then "
                         "again in the sorted union) instead of once (rendering.REUSE_PASS1)")
    ap.add_argument("--flat-allreduce", action="store_true",
                    help="one all-reduce of the flat gradient after the backward instead of overlapped buckets")
    ap.add_argument("--no-graph-allreduce", action="store_true",
                    help="keep the RCCL bucket all-reduces out of the HIP graph (they follow each replay); "
                         "also SPNERF_NO_GRAPH_ALLREDUCE=1")
    ap.add_argument("--precision", choices=("bf16", "fp32"), default=None,
                    help="override the config's MLP precision (parity runs; the default line keeps the config's)")
    ap.add_argument("--rehearse-collective", action="store_true",
                    help="(N=1 rehearsal of the N>1 path) a one-rank RCCL group: the bucket all-reduces (identities) "
                         "captured into the step graph, the exposed collective timed over the profiled eager steps")
    ap.add_argument("--share-device", action="store_true",
                    help="(rehearsal on a 1-GPU box) every rank on cuda:0 over gloo instead of RCCL")
    return ap.parse_args(argv)


def main():
    a = parse_args()
    if a.gpus < 1:
        raise SystemExit("bench: --gpus must be >= 1")
    if "RANK" not in os.environ and a.gpus > 1:
        sys.exit(launch_ranks(a))
    rank, local, world = dp.env_rank()
    if world != a.gpus:
        raise SystemExit(f"bench: launched with WORLD_SIZE={world} but --gpus {a.gpus}")
    if world > 1:
        # the deferred weight gradients' last group at most 2 GEMMs: the marks of trunk layers 4, 3
        # fire a launch earlier and their all-reduce overlaps layers 2, 1 (smaller exposed bucket)
        _lib.set_option("tn_group_last", 2)
    for o in a.option:
        name, value = o.split("=")
        _lib.set_option(name, int(value))
    local = 0 if a.share_device else local
    torch.cuda.set_device(local)                  # before the process group: RCCL binds this device
    dev = torch.device("cuda", local)
    dp.init_from_env("gloo" if a.share_device else "nccl", device=dev)
    if a.rehearse_collective and world == 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(free_port()))
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    c = CONFIGS[a.config]
    if c.get("inference"):
        out = run_inference(a, a.config, rank, world, dev)
    else:
        out = run_train(a, a.config, rank, world, dev)
    if a.full and rank == 0 and world == 1 and a.config == "c4" and not a.no_secondary:
        # configs[1] (C2, fp32) and configs[4] (C5, whole-image inference: 10 of its 32768-ray
        # chunks) beside the headline, same process and GPU, no CPU leg
        keys = ("value", "unit", "ms_per_step", "dtype", "config", "roofline", "mlp_mfma_utilisation")
        sec = run_train(a, "c2", rank, world, dev, secondary=True)
        out["secondary"] = {"c2": {k: sec[k] for k in keys}}
        sec = run_inference(a, "c5", rank, world, dev, steps=10, warmup=3, secondary=True)
        out["secondary"]["c5"] = {k: sec[k] for k in keys + ("steps", "image_seconds_projected")}
    if rank == 0:
        print(json.dumps(finalize_line(out)), flush=True)
    if world > 1:
        dist.barrier()
    if dist.is_initialized():
        dist.destroy_process_group()
    report_children(rank)


def report_children(rank: int) -> None:
    """At exit, name this rank's child processes on stderr (the driver has seen one process left
    at the end of the bench for several rounds: this says whether it is one of the bench's own)."""
    try:
        import psutil
        kids = psutil.Process().children(recursive=True)
        print(f"bench: rank {rank} child processes at exit: "
              + (", ".join(f"{k.pid} {k.name()} {' '.join(k.cmdline()[:4])}" for k in kids) or "none"),
              file=sys.stderr, flush=True)
    except Exception as e:   # diagnosis only
        print(f"bench: child-process report failed: {type(e).__name__}: {e}", file=sys.stderr)


class TrainStep:
    """One training workload's step exactly as the bench times it: the HBM-resident synthetic
    scene, the SPNeRF (flat gradients, deferred two-pass trunk weight gradients), the library
    Adam, the shared-seed sampler with the batch indices in static buffers, on-device Philox
    draws keyed by the GLOBAL ray id, the fused loss, and for N > 1 the bucketed all-reduce
    behind the backward's gradient marks.  ``capture()`` warms up and records render + loss +
    backward (+ the RCCL buckets, unless ``--no-graph-allreduce`` / SPNERF_NO_GRAPH_ALLREDUCE=1)
    as one HIP graph.  The tests drive the same object (tests/test_gpu_c4.py)."""

    def __init__(self, a, config, rank, world, dev, secondary=False):
        c = dict(CONFIGS[config])
        if a.global_batch and not secondary:
            c.pop("batch", None)
            c["global_batch"] = a.global_batch
            c["workload"] += f" [global batch overridden: {a.global_batch} rays]"
        if getattr(a, "precision", None) and not secondary and a.precision != c["precision"]:
            c["precision"] = a.precision
            c["workload"] += f" [MLP precision overridden: {a.precision}]"
        self.a, self.c, self.config, self.rank, self.world, self.dev = a, c, config, rank, world, dev
        self.scene = synthetic_scene(c["img_downscale"], seed=0, device=dev)
        self.R = {k: getattr(self.scene, k) for k in ("rays", "rgbs", "depths", "valid_depth", "depth_std", "sems")}
        torch.manual_seed(0)
        self.model = spnerf_amd.SPNeRF(num_sem_classes=3, s_embedding_factor=1, layers=8, feat=512, mapping=True,
                                       sem=c["sem"], precision=c["precision"]).to(dev)
        self.model.use_flat_grads()   # backward adds into one flat buffer: the .grads are its views (one all-reduce)
        self.model.defer_trunk_wgrad = not a.no_defer_wgrad
        spnerf_amd.rendering.REUSE_PASS1 = not a.no_reuse_pass1
        self.params = list(self.model.parameters())
        if a.torch_adam:
            self.opt = torch.optim.Adam(self.params, lr=5e-4, fused=True)
        else:  # the library's one-launch Adam (torch's fused multi-tensor step took ~100 us at C2)
            self.opt = spnerf_amd.optim.Adam(self.params, lr=5e-4)
        self.args = make_args(c)
        self.strong = "global_batch" in c
        if self.strong and c["global_batch"] % world:
            raise SystemExit(f"bench: global batch {c['global_batch']} does not split over {world} ranks")
        B = self.B = c["global_batch"] // world if self.strong else c["batch"]
        self.sampler = dp.SharedSeedSampler(self.R["rays"].shape[0], B * world, rank, world, seed=0, device=dev)
        self.sloss = SNerfLoss(lambda_sc=c["sc_lambda"])
        self.dloss = DepthLoss(lambda_ds=1.0, usealldepth=False) if c["depth"] else None
        self.semloss = SemanticLoss(lambda_ss=1.0) if c["sem"] else None
        self.floss = None if a.torch_loss else FusedRenderLoss(c["sc_lambda"], 1.0 if c["depth"] else 0.0,
                                                               1.0 if c["sem"] else 0.0)
        self.s_final = c["n_samples"] * (2 if c["guided"] else 1)
        # The production random source: draws generated inside the sampling / compositing kernels,
        # keyed by (seed, step, GLOBAL ray id) — rank r's rays are rows r·B.. of the global batch, so
        # an N-rank step draws what one process rendering the whole batch draws (no RNG launches)
        from spnerf_amd import PhiloxRandom, set_random_source
        self.src = PhiloxRandom(seed=0, ray_offset=rank * B)
        set_random_source(self.src)
        # Batch indices live in static buffers so that the captured step reads each new batch.
        # (this rank's rows are a view of the global batch: one copy per step)
        self.gidx_s = torch.empty(B * world, dtype=torch.int64, device=dev)
        self.one = torch.ones((), device=dev)
        self.idx_s = self.gidx_s[rank * B:(rank + 1) * B]
        # this rank's rows of every per-ray field in one launch, into static buffers
        self.gather = None if getattr(a, "torch_gather", False) else dp.BatchGather(self.R, B)
        # The gradient all-reduce (N > 1): by default in buckets (dp.GradBuckets), each issued on a
        # communication stream behind the backward mark after which its gradients are final, so the
        # collectives overlap the rest of the backward; --flat-allreduce = one all-reduce after it.
        # With RCCL the buckets are captured INTO the step's HIP graph (the marks are the graph's own
        # edges) unless --no-graph-allreduce; if that capture is refused, or with gloo, the graph holds
        # the backward only and the buckets follow each replay.  allreduce_ms_per_step = the EXPOSED
        # part: HIP events on the compute stream from the end of the backward to the moment every
        # bucket has landed (not separable when the all-reduce is inside the graph: null then)
        # --rehearse-collective (N=1): a one-rank RCCL group runs the N>1 bucket path (identity
        # all-reduces, captured into the graph) so that path is exercised on one GPU
        self.rehearse = (bool(getattr(a, "rehearse_collective", False)) and world == 1 and dist.is_initialized()
                         and not secondary)
        self.buckets = (dp.GradBuckets(self.model, world) if ((world > 1 or self.rehearse) and not a.flat_allreduce)
                        else None)
        if self.buckets is not None:
            self.buckets.arm(True)
        self.ar_events = []
        self.ar_timing = False
        self.in_graph = False     # the all-reduce is part of the captured graph
        self.graph = None
        self.graph_packs = []     # packed-weight buffers the captured graph writes (kept with it)
        self.static_loss = None
        self.res = None           # the last render's outputs (the graph's static outputs after capture)

    def load_batch(self, gidx=None):
        """The next shared-seed global batch (or the given global indices) into the static buffers."""
        if gidx is None:
            gidx, _ = self.sampler.next()
        self.gidx_s.copy_(gidx)

    def fwd_bwd(self):
        """render + losses + backward for the batch in idx_s / gidx_s (grads are written, not
        accumulated: the caller clears them before an eager call)."""
        R, c, world = self.R, self.c, self.world
        idx, gidx = self.idx_s, self.gidx_s
        # each per-ray field gathered once (one launch), shared by the render and the loss (the
        # guided clamp's global first ray is this batch's first row on one rank)
        bt = self.gather(idx) if self.gather is not None else {k: v[idx] for k, v in R.items()}
        rays = bt["rays"]
        depths, valid, dstd = bt["depths"], bt["valid_depth"], bt["depth_std"]
        kw = {}
        if c["guided"]:
            first = rays[0, 6:8] if world == 1 else R["rays"].index_select(0, gidx[:1])[0, 6:8]
            kw = dict(valid_depth=valid, target_depths=depths, target_std=dstd, clamp_near_far=first)
        sem = bt["sems"] if c["sem"] else None
        res = spnerf_amd.render_rays({"coarse": self.model}, self.args, rays, None, semantics=sem, mode="train", **kw)
        self.res = res
        if self.floss is not None:   # the trainer's loss sum (main.py:143-174) in two kernels
            loss, _ = self.floss(res, bt["rgbs"], depths, valid, dstd, sem,
                                 labels_global=R["sems"][gidx] if (world > 1 and sem is not None) else None, world=world)
            loss.backward(self.one)   # d loss / d loss = 1 from a static tensor (no fill launch per step)
            return loss.detach()
        loss, _ = self.sloss(res, bt["rgbs"])
        if self.dloss is not None:
            loss = loss + self.dloss(res, depths[:, 0], depths[:, 1], valid, dstd)[0]
        if self.semloss is not None:
            sl = self.semloss(res, sem)[0]
            loss = loss + (dp.shard_ce(sl, sem, R["sems"][gidx], world) if world > 1 else sl)
        loss.backward()
        return loss.detach()   # no autograd graph outlives the step (captured nodes would pin their stream)

    def reduce_grads(self, overlap=True):
        if self.buckets is not None:
            flat = self.model._flat_grad
            self.buckets.launch(flat, overlap=overlap, force=self.rehearse)
            self.buckets.finish(flat, force=self.rehearse)
        else:
            dp.allreduce_grads(self.params, self.world)   # one RCCL all-reduce of the flat gradient

    def reduce(self, replayed=False):
        """The gradient exchange after a backward (eager) or a graph replay (nothing when the graph
        holds the collectives)."""
        if self.in_graph and replayed:
            return                              # the graph reduced the gradients
        if (self.world > 1 or self.rehearse) and self.ar_timing:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            self.reduce_grads(overlap=not replayed)
            e1.record()
            self.ar_events.append((e0, e1))
        else:
            self.reduce_grads(overlap=not replayed)

    def apply(self):
        self.opt.step()
        self.args.noise_std *= 0.9               # main.py:155

    def compute(self):
        """render + loss + backward + gradient exchange of the batch in the static buffers, by
        graph replay when captured, else eagerly; returns the loss (a device scalar)."""
        if self.graph is not None:
            self.graph.replay()
            self.reduce(replayed=True)
            return self.static_loss
        self.opt.zero_grad(set_to_none=True)
        loss = self.fwd_bwd()
        self.reduce()
        return loss

    def eager_step(self):
        self.load_batch()
        self.opt.zero_grad(set_to_none=True)
        loss = self.fwd_bwd()
        self.reduce()
        self.apply()
        return loss

    def step(self):
        if self.graph is None:
            return self.eager_step()
        self.load_batch()
        loss = self.compute()
        self.apply()
        return loss

    def capture(self, warmup):
        """Warm up on a side stream, then capture render + loss + backward (+ the overlapped RCCL
        buckets) once as a HIP graph; replays overwrite the same gradient tensors.  Falls back to
        eager (and says so) when a capture is refused."""
        a = self.a
        dist_nccl = (self.world > 1 or self.rehearse) and dist.is_initialized() and dist.get_backend() == "nccl"
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(max(1, warmup)):
                self.eager_step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.opt.zero_grad(set_to_none=True)
        self.model.invalidate_packed()           # the capture must contain the weight re-pack
        self.load_batch()
        graph = None
        if self.buckets is not None and dist_nccl and graph_allreduce_enabled(a):
            try:   # render + loss + backward + the overlapped bucket all-reduces in one graph
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    self.static_loss = self.fwd_bwd()
                    self.buckets.launch(self.model._flat_grad, overlap=True, force=self.rehearse)
                    self.buckets.finish(self.model._flat_grad, force=self.rehearse)
                self.in_graph = True
            except Exception as e:
                print(f"bench: capturing the all-reduce refused ({type(e).__name__}: {e}); it follows each replay",
                      file=sys.stderr)
                graph = None
                self.buckets.works = []
                torch.cuda.synchronize()
                self.opt.zero_grad(set_to_none=True)
        if graph is None:
            try:
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    self.static_loss = self.fwd_bwd()
            except Exception as e:  # capture refused: run the same work eagerly, and say so
                print(f"bench: HIP graph capture failed ({type(e).__name__}: {e}); running eager", file=sys.stderr)
                graph = None
                torch.cuda.synchronize()
        self.graph = graph
        # the packed-weight buffers this capture wrote into live exactly as long as the graph
        self.graph_packs = self.model.release_graph_packs()
        return graph is not None

    def exposed_collective_ms(self, reps: int = 5, wd=None):
        """With the bucket all-reduces captured INTO the step graph, the exposed collective per
        step cannot be timed by host events around it: it is the difference of paired replays
        (each synchronized, medians of ``reps``) of the step graph with the buckets and of a second
        capture of the same render + loss + backward without them.  None unless the collectives
        are in the graph.  (Round 5 faulted here before the packed-weight buffers of the first
        capture were kept with its graph: the second capture's empty_cache() released them and the
        next replay wrote unmapped memory — DESIGN.md §7, tests/test_gpu_graph.py.)"""
        if not self.in_graph or self.graph is None:
            return None
        import statistics
        torch.cuda.synchronize()
        self.opt.zero_grad(set_to_none=True)
        plain = torch.cuda.CUDAGraph()
        with torch.cuda.graph(plain):
            self.fwd_bwd()
        plain_packs = self.model.release_graph_packs()   # kept exactly as long as `plain`
        torch.cuda.synchronize()
        t = {"with": [], "without": []}
        for r in range(reps):
            for key, g in (("with", self.graph), ("without", plain)):
                if wd is not None:
                    wd.beat(r, f"paired replay ({key} buckets)")
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                g.replay()
                e1.record()
                e1.synchronize()
                t[key].append(e0.elapsed_time(e1))
        del plain, plain_packs
        med = {k: statistics.median(v) for k, v in t.items()}
        return {"exposed_ms": max(0.0, med["with"] - med["without"]), "replay_ms_with_buckets": med["with"],
                "replay_ms_without": med["without"], "reps": reps}

    def probe(self) -> dict:
        """Watchdog diagnosis: the gradient marks an EAGER backward reached (the marks inside a
        replayed graph are its own edges and record nothing the host can query)."""
        if self.graph is not None:
            return {"marks": "inside the replayed graph (not queryable)", "allreduce_in_graph": self.in_graph}
        if self.buckets is None:
            return {"marks": None}
        n = self.buckets.n_marks
        dev = self.dev.index if self.dev.index is not None else 0
        state = [_lib.grad_mark_query(dev, k) for k in range(n)]
        return {"marks_completed": [k for k in range(n) if state[k]],
                "marks_pending": [k for k in range(n) if state[k] is False],
                "marks_never_recorded": [k for k in range(n) if state[k] is None], "n_marks": n, "device": dev}

    def close(self):
        from spnerf_amd import set_random_source
        self.graph = None
        self.graph_packs = []
        self.res = None
        set_random_source(None)
        if self.buckets is not None:
            self.buckets.arm(False)


def graph_allreduce_enabled(a) -> bool:
    """The RCCL bucket all-reduces go INTO the step's HIP graph unless --no-graph-allreduce or
    SPNERF_NO_GRAPH_ALLREDUCE=1 (then they follow each replay, exposed): a switch to bypass a
    replay problem of captured collectives on a new node without editing code."""
    return not (getattr(a, "no_graph_allreduce", False) or os.environ.get("SPNERF_NO_GRAPH_ALLREDUCE", "0") == "1")


def run_train(a, config, rank, world, dev, secondary=False):
    """One training workload: warm-up, HIP-graph capture, ``a.steps`` timed steps (barrier +
    synchronize on both sides, max over ranks), the last step's outputs to ``--dump-outputs``;
    with ``--full`` the per-kernel timings (graph mode: from eager steps of their own), the paired
    replays, the CPU baseline and the PSNR studies; returns the JSON record."""
    ts = TrainStep(a, config, rank, world, dev, secondary=secondary)
    c, B = ts.c, ts.B
    # a step still running after SPNERF_STEP_DEADLINE seconds ends this rank with one JSON
    # diagnosis and exit code 3 (dp.StepWatchdog) instead of blocking until the driver's limit
    wd = dp.StepWatchdog(rank=rank, mode="graph" if a.graph else "eager", probe=ts.probe)
    wd.beat(0, "capture" if a.graph else "warmup")
    if a.graph:
        if not ts.capture(a.warmup):
            a.graph = False
    wd.mode = "graph" if ts.graph is not None else "eager"
    if ts.graph is None:
        for i in range(a.warmup):
            wd.beat(i, "warmup")
            ts.step()
    wd.beat(0, "sync after warmup")
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    if not a.graph:
        _lib.prof_reset()
        _lib.prof_enable(True)
    torch.cuda.synchronize()
    ts.ar_timing = True
    t0 = time.perf_counter()
    for i in range(a.steps):
        wd.beat(i, "timed")
        loss = ts.step()
        if i % 4 == 3 or i == a.steps - 1:   # (an event every few steps: where a hang stopped)
            ev = torch.cuda.Event()
            ev.record()
            wd.mark(ev)
    wd.beat(a.steps, "sync after timed steps")
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    t1 = time.perf_counter()
    ts.ar_timing = False
    allreduce_ms = sum(e0.elapsed_time(e1) for e0, e1 in ts.ar_events) / a.steps if ts.ar_events else None
    elapsed = torch.tensor([t1 - t0], dtype=torch.float64, device=dev)
    if world > 1:
        dist.all_reduce(elapsed, op=dist.ReduceOp.MAX)
    elapsed = float(elapsed.item())
    final_loss = float(loss.item())
    finite = bool(torch.isfinite(ts.res["rgb_coarse"]).all()) and math.isfinite(final_loss)
    if a.dump_outputs and rank == 0 and not secondary:
        # what the last timed step handed back: the render's outputs, its loss, the (reduced) flat
        # gradient and the parameters after Adam
        dump_outputs(a.dump_outputs, dict(ts.res, loss=loss, flat_grad=ts.model._flat_grad,
                                          params=torch.cat([p.detach().reshape(-1) for p in ts.params])))
    prof_steps = a.steps
    profiled = a.full or not a.graph   # eager timed steps carry the library's events themselves
    if a.graph and a.full:
        # library kernels inside a graph replay carry no events: time them over eager steps
        # of the same workload right after the timed region (same kernels, same shapes)
        prof_steps = max(1, a.prof_steps)
        _lib.prof_reset()
        _lib.prof_enable(True)
        wd.mode = "eager"
        # with the collectives inside the graph their exposed part cannot be timed around a replay:
        # it is timed over these eager steps — the same buckets behind the same backward marks
        ts.ar_events = []
        ts.ar_timing = ts.in_graph
        for i in range(prof_steps):
            wd.beat(i, "profiled eager step")
            ts.eager_step()
        torch.cuda.synchronize()
        ts.ar_timing = False
        if ts.in_graph and ts.ar_events:
            allreduce_ms = sum(e0.elapsed_time(e1) for e0, e1 in ts.ar_events) / len(ts.ar_events)
    _lib.prof_enable(False)
    allreduce_eager_ms = allreduce_ms
    # graph mode with the collectives captured: the exposed all-reduce from paired replays of the
    # graph with and without the buckets (the eager-step figure is kept beside it)
    paired = ts.exposed_collective_ms(wd=wd) if (ts.in_graph and a.graph and a.full) else None
    if paired is not None:
        allreduce_ms = paired["exposed_ms"]
    wd.close()

    prof = {}
    if profiled:
        # dominant kernel = the kernel function with the most time in the profiled steps
        dom = dominant_class()
        nt = _lib.prof_read(dom)
        traffic, traffic_src = measured_traffic(config, B, dom)
        prof = {"roofline": roofline_of(dom, nt, traffic, traffic_src),
                # the same figures for the three MLP kernel functions with the most time (the dominant
                # one first): which kernel is "dominant" can change between trees with nearly equal times
                "rooflines_top3": top_rooflines(config, B, 3),
                "mlp_mfma_utilisation": gemm_totals(prof_steps),
                "kernels": kernel_table(prof_steps)}
    total = world * B * ts.s_final * a.steps
    buckets = ts.buckets
    out = {
        "metric": "ray-samples/sec (train step)",
        "value": total / elapsed,
        "unit": "ray-samples/s",
        "n_gpus": world,
        "steps": a.steps,
        "warmup": a.warmup,
        "ms_per_step": 1e3 * elapsed / a.steps,
        "higher_is_better": True,
        "scaling": "strong" if ts.strong else "weak",
        "vs_baseline": None,
        "dtype": c["precision"],
        "data": f"{ts.scene.rgb_source} colour targets, synthetic depth priors / labels, on real JAX_269 RPC camera rays "
                "(JAX_214 proxy, resident in HBM), seeded-random SPNeRF init",
        "config": {"workload": c["workload"], "global_batch": B * world, "rays_per_rank": B,
                   "samples_per_ray": ts.s_final, "parallelism": f"dp{world}"},
        **{k: v for k, v in prof.items() if k != "kernels"},
        "allreduce_ms_per_step": allreduce_ms,
        "allreduce_ms_eager_steps": allreduce_eager_ms if paired is not None else None,
        "allreduce_exposed_paired_replays": paired,
        "allreduce": (None if (world == 1 and not ts.rehearse) else
                      f"{len(buckets.buckets)} buckets behind the backward's gradient marks, inside the HIP graph "
                      "(exposed ms = paired replays of the graph with / without the buckets; the same buckets "
                      "timed over the profiled eager steps in allreduce_ms_eager_steps)"
                      if ts.in_graph else
                      f"{len(buckets.buckets)} buckets after each graph replay (exposed ms above)"
                      if (buckets is not None and a.graph) else
                      f"{len(buckets.buckets)} buckets behind the backward's gradient marks (exposed ms above)"
                      if buckets is not None else "one flat all-reduce after the backward"),
        **{k: v for k, v in prof.items() if k == "kernels"},
        "final_loss": final_loss,
        "finite": finite,
        "execution": (("hip graph of render+loss+backward" + (" + the bucket all-reduces" if ts.in_graph else "")
                       + " per step, " + ("" if (ts.in_graph or world == 1) else "eager all-reduce + ")
                       + "fused Adam eager"
                       + (f"; kernel timings from {prof_steps} eager steps right after the timed region" if a.full else ""))
                      if a.graph else "eager"),
        "random_draws": "on-device Philox keyed by (seed, step, global ray id, slot) inside the sampling / "
                        "compositing kernels (spnerf_amd.PhiloxRandom)",
    }
    if c["precision"] == "bf16":
        out["parity_note"] = PARITY_NOTE_BF16
    ts.close()
    del ts
    if a.full and rank == 0 and world == 1 and not secondary and not a.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(c, a.cpu_seconds, a.cpu_batch or min(B, 512))
        if config in ("c2", "c4"):
            if a.psnr_parity_steps > 0:
                out["psnr_parity"] = {p: psnr_parity(steps=a.psnr_parity_steps, dev=dev, precision=p)
                                      for p in ("fp32", "bf16")}
            if a.psnr_steps > 0 and c["precision"] == "bf16":
                out["psnr_seeds"] = psnr_seeds(seeds=tuple(range(3, 3 + a.psnr_seeds)), steps=a.psnr_steps, dev=dev,
                                               detail_path=a.psnr_detail)
    return out


if __name__ == "__main__":
    main()
