"""Time the ground-grid route on one GPU and count the holes of the per-view one: the JAX_269 lidar
ROI grid (512 x 512 cells of 0.5 m, UTM zone 17), C5 flags (128 stratified samples, semantic head,
W = 512, bf16 MLP; the weights are the initialisation, which costs what trained ones cost),
chunks of 32768 rays, on-device draws.  Device events, median of the calls after warm-up.

  (a) ``ortho_rays`` alone, per launch by the library's own timer (class "ortho") and end to end;
  (b) ``render_ortho`` with every product at s = 1 and s = 2, alternating with ``render_image`` on
      the same rays (the render inside it), and the reduction's launches by the library's timer;
  (c) coverage: ``get_dsm_from_nerf_prediction`` of one whole JAX_269 view on that grid — the
      fraction of cells where no point of the view lands — against ``render_ortho``'s DSM.

    python tools/ortho_bench.py [--calls 5] [--warmup 2] [--out profiles/r18/ortho.txt]
"""
import argparse
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ROI = (438638.996411, 3353399.999928, 512, 0.5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--chunk", type=int, default=32768)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import bench
    import spnerf_amd
    from spnerf_amd import GroundGrid, PhiloxRandom, _lib, random_source
    from spnerf_amd.satellite import image_rays, load_cameras, scene_normalisation
    from view_bench import stats, timed

    dev = torch.device("cuda", 0)
    c = bench.CONFIGS["c5"]
    args = bench.make_args(c)
    cams = load_cameras()
    meta = cams["images"][c["view"]]
    center, rng = scene_normalisation(cams["scene_loc"])
    lo, hi = float(meta["min_alt"]), float(meta["max_alt"])
    grid = GroundGrid.from_roi(ROI, 17)
    sun = (60.0, 140.0)
    torch.manual_seed(0)
    model = spnerf_amd.SPNeRF(num_sem_classes=3, layers=8, feat=512, mapping=True, sem=True, precision=c["precision"]).to(dev)
    models = {"coarse": model}
    labels = torch.zeros(grid.shape, dtype=torch.long, device=dev)
    lines = [f"JAX_269 ROI grid {grid.xsize} x {grid.ysize} cells of {grid.resolution} m, altitudes {lo} .. {hi} m, "
             f"{args.n_samples} samples, W=512 {c['precision']} MLP, C=3, chunks of {a.chunk} rays, "
             f"{torch.cuda.get_device_name(0)}; device events, {a.calls} calls after {a.warmup} warm-up"]

    def prof(fn):
        _lib.prof_reset()
        fn()
        return _lib.prof_read("ortho")

    for s in (1, 2):
        n = grid.xsize * grid.ysize * s * s
        gen = lambda: spnerf_amd.ortho_rays(grid, lo, hi, center, rng, sun=sun, supersample=s, device=dev)   # noqa: E731
        ms_gen = timed(gen, a.calls, a.warmup)
        rays = gen()
        sems = labels.reshape(-1).repeat_interleave(s * s)

        def ortho():
            with random_source(PhiloxRandom(seed=0)):
                return spnerf_amd.render_ortho(models, args, grid, lo, hi, center, rng, sun, semantics=labels, supersample=s,
                                               chunk=a.chunk)

        def image():
            with random_source(PhiloxRandom(seed=0)):
                return spnerf_amd.render_image(models, args, rays, None, sems, chunk=a.chunk, center=center, rng=rng)

        for _ in range(a.warmup):
            ortho()
            image()
        ms_o, ms_i = [], []
        for _ in range(a.calls):          # alternating, so that both see the same machine
            ms_o += timed(ortho, 1, 0)
            ms_i += timed(image, 1, 0)
        _lib.prof_enable(True)
        k_gen = [prof(gen) for _ in range(a.calls)]
        k_all = [prof(ortho) for _ in range(a.calls)]
        _lib.prof_enable(False)
        g_ms = statistics.median(k["ms"] for k in k_gen)
        all_ms = statistics.median(k["ms"] for k in k_all)
        mo, mi = statistics.median(ms_o), statistics.median(ms_i)
        out = ortho()
        lines += [
            f"s = {s}: {n} rays",
            f"  (a) ortho_rays end to end:      {stats(ms_gen)}",
            f"      k_ortho_rays, per launch:   median {g_ms:.4f} ms; {k_gen[0]['bytes'] / 1e6:.1f} MB written -> "
            f"{k_gen[0]['bytes'] / g_ms / 1e6:.0f} GB/s",
            f"  (b) render_ortho, all products: {stats(ms_o)}",
            f"      render_image, same rays:    {stats(ms_i)}",
            f"      render_ortho - render_image = {mo - mi:+.3f} ms = {100 * (mo - mi) / mi:+.2f} % (medians); render_image's own "
            f"min-to-max spread {max(ms_i) - min(ms_i):.3f} ms",
            f"      launches of class ortho in one render_ortho (rays, reductions, classes): {k_all[0]['launches']}, "
            f"median {all_ms:.4f} ms in all = {100 * all_ms / mi:.3f} % of render_image",
            f"      DSM: {int(torch.isnan(out['dsm']).sum())} NaN cells of {out['dsm'].numel()}",
        ]

    # (c) the per-view route on the same grid: one whole view of the scene at full resolution
    rays = image_rays(meta, 1.0, cams["scene_loc"], device=dev)
    sems = torch.zeros(rays.shape[0], dtype=torch.long, device=dev)
    with random_source(PhiloxRandom(seed=0)):
        depth = spnerf_amd.render_image(models, args, rays, None, sems, chunk=a.chunk, products=("depth",))["depth"]
    with tempfile.TemporaryDirectory() as tmp:
        roi = os.path.join(tmp, "roi.txt")
        np.savetxt(roi, np.array(ROI), fmt="%.6f")
        per_view = spnerf_amd.dsm.get_dsm_from_nerf_prediction(rays, depth, center, rng, roi_txt=roi)
    holes = int(np.isnan(per_view).sum())
    lines += [f"(c) get_dsm_from_nerf_prediction, view {c['view']} at full resolution ({meta['height']} x {meta['width']} = "
              f"{rays.shape[0]} rays), radius 1: {holes} NaN cells of {per_view.size} = {100 * holes / per_view.size:.2f} %; "
              f"render_ortho: 0 by construction (above)"]
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
