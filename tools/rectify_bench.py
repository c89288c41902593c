"""Time the orthorectification on one GPU: the four shipped JAX_269 cameras and their downscale-4
images over the lidar ROI (256 m square, UTM zone 17) on a 512 x 512 grid of 0.5 m and on a
2048 x 2048 grid of 0.125 m, over a seeded relief within the scene's altitude bounds.

The fused launch alone (``orthorectify(..., occlusion=False)``'s one kernel) by the library's own
timer — HIP events around the launch, class "rectify" — beside its byte model as a fraction of the
HBM bandwidth: 8 B of DSM per cell, at worst 16·C B of image reads per view and cell, 4·C + 1 B out.
Then the whole calls by device events: the fused call, project-then-sample, and ``orthorectify`` with
the occlusion mask and the median mosaic.

    python tools/rectify_bench.py [--calls 10] [--warmup 2] [--out profiles/r20/rectify.txt]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ROI_XOFF, ROI_YTOP, ROI_METRES = 438638.996411, 3353399.999928 + 256.0, 256.0
VIEWS = ("JAX_269_006_RGB", "JAX_269_007_RGB", "JAX_269_011_RGB", "JAX_269_023_RGB")
HBM_GBS = 8000.0   # MI355X peak


def relief(side, seed=0):
    g = np.random.default_rng(seed)
    t = np.linspace(0.0, 1.0, side)
    x, y = np.meshgrid(t, t)
    h = -16.0 + 6.0 * np.sin(9.0 * x + 2.0) * np.cos(7.0 * y) + g.uniform(-4.0, 4.0, (side, side))
    return np.clip(h, -30.0, -2.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from spnerf_amd import GroundGrid, _lib, orthorectify, rectify
    from spnerf_amd.satellite import DATA, load_cameras
    from view_bench import stats, timed

    dev = torch.device("cuda", 0)
    metas = load_cameras()["images"]
    cams = [rectify.Camera.from_meta(metas[v], 4) for v in VIEWS]
    with np.load(os.path.join(os.path.dirname(DATA), "jax269_rgb_ds4.npz"), allow_pickle=False) as z:
        images = [torch.tensor(z[v].reshape(c.shape + (3,)), device=dev) for v, c in zip(VIEWS, cams)]
    V, C = len(cams), 3
    lines = [f"JAX_269 ROI, {V} shipped cameras at downscale 4 (images of {', '.join('%d x %d' % c.shape for c in cams)} x {C}), "
             f"{torch.cuda.get_device_name(0)}; {a.calls} calls after {a.warmup} warm-up; HBM peak taken as {HBM_GBS:.0f} GB/s"]
    for side in (512, 2048):
        grid = GroundGrid(ROI_XOFF, ROI_YTOP, side, side, ROI_METRES / side, 17)
        dsm = torch.tensor(relief(side), device=dev)
        fused = lambda: orthorectify(images, cams, dsm, grid, -30.0, -2.0, occlusion=False)   # noqa: E731

        def kernel():
            _lib.prof_reset()
            fused()
            return _lib.prof_read("rectify")

        for _ in range(a.warmup):
            fused()
        _lib.prof_enable(True)
        k = [kernel() for _ in range(a.calls)]
        _lib.prof_enable(False)
        assert all(r["launches"] == 1 for r in k)
        ms, model = statistics.median(r["ms"] for r in k), k[0]["bytes"]
        assert model == side * side * (8 + V * (16 * C + 4 * C + 1))
        out = fused()
        lines += [f"{side} x {side} cells of {grid.resolution} m: valid {100 * float(out['valid'].float().mean()):.1f} % of the (view, cell) pairs",
                  f"  the fused launch by the library's timer: median {ms:.4f} ms, min {min(r['ms'] for r in k):.4f} ms, max "
                  f"{max(r['ms'] for r in k):.4f} ms; byte model {model / 1e6:.1f} MB -> {model / ms / 1e6:.0f} GB/s, "
                  f"{100 * model / ms / 1e6 / HBM_GBS:.1f} % of the HBM peak",
                  f"  orthorectify(occlusion=False), whole call:      {stats(timed(fused, a.calls, a.warmup))}",
                  f"  project_cells then sample_images:               "
                  f"{stats(timed(lambda: rectify.sample_images(images, rectify.project_cells(dsm, grid, cams)), a.calls, a.warmup))}",
                  f"  orthorectify(occlusion=True, mosaic='median'):  "
                  f"{stats(timed(lambda: orthorectify(images, cams, dsm, grid, -30.0, -2.0, mosaic='median'), a.calls, a.warmup))}"]
        if side == 512:
            _, spread = rectify.view_directions(grid, cams, -30.0, -2.0, device=dev)
            lines += [f"  view_directions spread: {', '.join('%.3e' % s for s in spread.tolist())} "
                      f"(x 28 m of altitude: at most {28.0 * float(spread.max()) * 100:.2f} cm)"]
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
