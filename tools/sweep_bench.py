"""Time the plane sweep on one GPU: the four shipped JAX_269 cameras and their downscale-4 images
over the lidar ROI (256 m square, UTM zone 17) on a 512 x 512 grid of 0.5 m, K = 64 planes from −30 m
in steps of 0.5 m, window radius 2.

Two steps, each a fresh process under a time limit of its own; the second is not started when the
first fails:

* ``fused`` — ``plane_sweep`` as one launch: by the library's own timer (HIP events around the launch,
  class "sweep") beside its models — bytes: the four result planes, 13 B per cell; fp64 operations:
  per plane 272 + 9·C per (view, cell of tile and halo) for the projection, the read and the channel
  mean, and 7·V·n + 2·n per cell for the score of an n-cell window, a division or a square root
  counted as one — as shares of the HBM peak and of the fp64 vector peak; then the whole call by
  device events;
* ``staged`` — the same result through ``plane_grey``, ``window_score`` per plane and ``pick_plane``
  (its bytes are compared with the fused call's), by device events.

    python tools/sweep_bench.py [--calls 5] [--warmup 1] [--out profiles/r21/sweep.txt]
"""
import argparse
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ROI_XOFF, ROI_YTOP, ROI_METRES = 438638.996411, 3353399.999928 + 256.0, 256.0
VIEWS = ("JAX_269_006_RGB", "JAX_269_007_RGB", "JAX_269_011_RGB", "JAX_269_023_RGB")
SIDE, PLANES, RADIUS, ALT_LO, STEP = 512, 64, 2, -30.0, 0.5
HBM_GBS = 8000.0       # MI355X peak
FP64_TFLOPS = 78.6     # MI355X vector fp64 peak: half the 157.3 TFLOPS fp32 vector rate
LIMITS = {"fused": 240, "staged": 300}   # seconds per step


def scene(dev):
    from spnerf_amd import GroundGrid, rectify
    from spnerf_amd.satellite import DATA, load_cameras
    metas = load_cameras()["images"]
    cams = [rectify.Camera.from_meta(metas[v], 4) for v in VIEWS]
    with np.load(os.path.join(os.path.dirname(DATA), "jax269_rgb_ds4.npz"), allow_pickle=False) as z:
        images = [torch.tensor(z[v].reshape(c.shape + (3,)), device=dev) for v, c in zip(VIEWS, cams)]
    return images, cams, GroundGrid(ROI_XOFF, ROI_YTOP, SIDE, SIDE, ROI_METRES / SIDE, 17)


def step_fused(a):
    from spnerf_amd import _lib, plane_sweep
    from view_bench import stats, timed
    images, cams, grid = scene(torch.device("cuda", 0))
    fused = lambda: plane_sweep(images, cams, grid, ALT_LO, STEP, PLANES, radius=RADIUS)   # noqa: E731

    def kernel():
        _lib.prof_reset()
        fused()
        return _lib.prof_read("sweep")

    for _ in range(a.warmup):
        fused()
    _lib.prof_enable(True)
    k = [kernel() for _ in range(a.calls)]
    _lib.prof_enable(False)
    assert all(r["launches"] == 1 for r in k)
    ms, flop, model = statistics.median(r["ms"] for r in k), k[0]["flop"], k[0]["bytes"]
    V, C, n, hc = len(cams), 3, (2 * RADIUS + 1) ** 2, (16 + 2 * RADIUS) ** 2
    assert model == SIDE * SIDE * 13
    assert flop == PLANES * ((SIDE // 16) ** 2 * hc * V * (272 + 9 * C) + SIDE * SIDE * (7 * V * n + 2 * n))
    out = fused()
    index = out["index"]
    return [f"JAX_269 ROI, {V} shipped cameras at downscale 4 (images of {', '.join('%d x %d' % c.shape for c in cams)} x {C}), "
            f"{torch.cuda.get_device_name(0)}; {a.calls} calls after {a.warmup} warm-up; peaks taken as {HBM_GBS:.0f} GB/s of HBM and "
            f"{FP64_TFLOPS} TFLOPS of vector fp64",
            f"{SIDE} x {SIDE} cells of {grid.resolution} m, {PLANES} planes from {ALT_LO} m in steps of {STEP} m, radius {RADIUS}: "
            f"{100 * float((index >= 0).float().mean()):.1f} % of the cells have a plane, 4 views at "
            f"{100 * float((out['views'] == 4).float().mean()):.1f} %, median score {float(out['score'].nanmedian()):.3f}",
            f"  the fused launch by the library's timer: median {ms:.3f} ms, min {min(r['ms'] for r in k):.3f} ms, max "
            f"{max(r['ms'] for r in k):.3f} ms",
            f"    byte model {model / 1e6:.2f} MB -> {model / ms / 1e6:.1f} GB/s, {100 * model / ms / 1e6 / HBM_GBS:.3f} % of the HBM peak",
            f"    fp64 model {flop / 1e9:.1f} GFLOP -> {flop / ms / 1e9:.2f} TFLOPS, {100 * flop / ms / 1e9 / FP64_TFLOPS:.1f} % of the fp64 vector peak",
            f"  plane_sweep, whole call:                                  {stats(timed(fused, a.calls, a.warmup))}",
            f"  plane_sweep(volume=True), whole call:                     "
            f"{stats(timed(lambda: plane_sweep(images, cams, grid, ALT_LO, STEP, PLANES, radius=RADIUS, volume=True), a.calls, a.warmup))}"]


def step_staged(a):
    from spnerf_amd import plane_sweep, sweep
    from view_bench import stats, timed
    images, cams, grid = scene(torch.device("cuda", 0))

    def staged():
        volume, views = [], []
        for k in range(PLANES):
            grey, valid = sweep.plane_grey(images, cams, grid, ALT_LO + float(k) * STEP)
            s, m = sweep.window_score(grey, valid, radius=RADIUS)
            volume.append(s)
            views.append(m)
        return sweep.pick_plane(torch.stack(volume), torch.stack(views), ALT_LO, STEP)

    want, out = plane_sweep(images, cams, grid, ALT_LO, STEP, PLANES, radius=RADIUS), staged()
    for k in want:
        assert want[k].cpu().numpy().tobytes() == out[k].cpu().numpy().tobytes(), k
    return [f"  plane_grey, window_score x {PLANES}, pick_plane (same bytes): {stats(timed(staged, a.calls, a.warmup))}"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=["all", "fused", "staged"], default="all")
    a = ap.parse_args()
    if a.step != "all":
        print("\n".join({"fused": step_fused, "staged": step_staged}[a.step](a)))
        return
    lines = []
    for step in ("fused", "staged"):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--calls", str(a.calls), "--warmup", str(a.warmup)],
                           stdout=subprocess.PIPE, text=True, timeout=LIMITS[step])
        lines += r.stdout.splitlines()
        if r.returncode != 0:
            print("\n".join(lines))
            sys.exit(f"step {step} ended with status {r.returncode}: nothing further is started")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
