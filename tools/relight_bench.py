"""Time relighting a view under K sun directions on one GPU: a 256 x 256 crop of the C5 camera
(JAX_269_006 RPC at x5), 128 stratified samples, W = 256, bf16 MLP, on-device draws, one process.

  arm A: K calls of ``render_image`` (products rgb, sun, sky), the sun columns replaced per call;
  arm B: one ``relight_image`` of the K directions.

K in {1, 4, 16}; after warm-up the two arms alternate; device events; median and min - max of the
calls.  Also the relight MFMA launch by the library's own timer (events around the launch) and its
share of the 2.5 PFLOP/s bf16 MFMA peak from its FLOP count, and the per-direction marginal cost
(B16 - B1) / 15.

    python tools/relight_bench.py [--side 256] [--calls 7] [--warmup 2] [--out profiles/r17/relight.txt]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BF16 = 2.5e15


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return f"median {statistics.median(ms):9.3f} ms  min {min(ms):9.3f}  max {max(ms):9.3f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=256)
    ap.add_argument("--samples", type=int, default=128)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import bench
    import spnerf_amd
    from spnerf_amd import PhiloxRandom, _lib, random_source
    from spnerf_amd.satellite import image_rays, load_cameras, sun_direction

    dev = torch.device("cuda", 0)
    c = bench.CONFIGS["c5"]
    args = bench.make_args(c)
    args.n_samples, args.n_importance, args.guidedsample, args.sc_lambda, args.noise_std = a.samples, 0, False, 0.0, 0.0
    cams = load_cameras()
    rays = image_rays(cams["images"][c["view"]], c["img_downscale"], cams["scene_loc"], crop=(0, 0, a.side, a.side), device=dev)
    n = rays.shape[0]
    torch.manual_seed(0)
    model = spnerf_amd.SPNeRF(layers=8, feat=256, mapping=True, precision="bf16").to(dev)
    models = {"coarse": model}
    prod = ("rgb", "sun", "sky")
    lines = [f"relight bench: {a.side} x {a.side} rays x {a.samples} samples, W = 256, bf16, products {prod}, "
             f"{a.calls} calls after {a.warmup} warm-up, arms alternating"]
    med = {}
    for K in (1, 4, 16):
        dirs = np.stack([sun_direction(20 + 60 * k / max(K - 1, 1), 360.0 * k / K) for k in range(K)]).astype(np.float32)
        dirs_t = torch.tensor(dirs, device=dev)
        out_a = {"rgb": torch.empty(K, n, 3, device=dev), "sun": torch.empty(K, n, device=dev), "sky": torch.empty(K, n, 3, device=dev)}
        out_b = {k: torch.empty_like(v) for k, v in out_a.items()}
        lit = rays.clone()

        def arm_a():
            for k in range(K):
                lit[:, 8:11] = dirs_t[k]
                with random_source(PhiloxRandom(seed=0)):
                    spnerf_amd.render_image(models, args, lit, products=prod, out={p: out_a[p][k] for p in prod})

        def arm_b():
            with random_source(PhiloxRandom(seed=0)):
                spnerf_amd.relight_image(models, args, rays, dirs_t, products=prod, out=out_b)

        for _ in range(a.warmup):
            arm_a()
            arm_b()
        torch.cuda.synchronize()
        ms_a, ms_b = [], []
        for _ in range(a.calls):
            ms_a.append(timed(arm_a))
            ms_b.append(timed(arm_b))
        rel = {p: float((out_b[p] - out_a[p]).norm() / out_a[p].norm()) for p in prod}
        _lib.prof_enable(True)
        _lib.prof_reset()
        arm_b()
        torch.cuda.synchronize()
        sun = _lib.prof_read("relight_sun_bf16")
        comp = _lib.prof_read("relight_composite")
        _lib.prof_enable(False)
        med[K] = (statistics.median(ms_a), statistics.median(ms_b))
        lines += [f"K = {K:2d}  A: K x render_image   {stats(ms_a)}",
                  f"        B: 1 x relight_image  {stats(ms_b)}   A / B = {med[K][0] / med[K][1]:.2f}",
                  f"        B against A, norm-relative: " + ", ".join(f"{p} {rel[p]:.1e}" for p in prod),
                  f"        relight_sun_bf16: {sun['launches']} launch(es), {sun['ms']:.3f} ms, {sun['flop'] / 1e9:.1f} GFLOP "
                  f"-> {sun['flop'] / (sun['ms'] * 1e-3) / 1e12:.1f} TFLOP/s = "
                  f"{sun['flop'] / (sun['ms'] * 1e-3) / PEAK_BF16:.3f} of the bf16 MFMA peak; "
                  f"relight_composite: {comp['ms']:.3f} ms"]
    lines.append(f"per-direction marginal cost (B16 - B1) / 15 = {(med[16][1] - med[1][1]) / 15:.3f} ms; "
                 f"one render_image (A1) = {med[1][0]:.3f} ms -> a further direction costs "
                 f"{(med[16][1] - med[1][1]) / 15 / med[1][0]:.3f} of a render")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
