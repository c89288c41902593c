"""Time the geometric shadows on one GPU: the JAX_269 lidar ROI grid (512 x 512 cells of 0.5 m, UTM
zone 17), K = 16 sun directions of a day sweep (elevations of about 10° to 60°, azimuths from east
over south to west), on two DSMs:

  (a) ``render_ortho``'s DSM of the initialisation (C5 flags: 128 stratified samples, semantic head,
      W = 512, bf16 MLP) — nearly flat, so almost every march ends at its first steps;
  (b) a synthetic city: 400 boxes of 0 to 30 m on flat ground — long shadows at low sun.

``cast_shadows`` with ``shadow`` alone and with ``excess``, and ``shadow_agreement``, by device events,
the calls after warm-up; the launches by the library's own timer (class "shadow").  Beside them
``relight_ortho`` for the same grid and the same K from the same call: the cost of the learnt shadow
planes this product is judged against.

    python tools/shadow_bench.py [--calls 5] [--warmup 2] [--out profiles/r19/shadow.txt]
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

ROI = (438638.996411, 3353399.999928, 512, 0.5)
K = 16


def day_sweep(k=K):
    """(k, 2) (elevation°, azimuth°): the sun from east over south to west, 10° at the ends, 60° at noon."""
    t = np.linspace(-1.0, 1.0, k)
    return np.stack([10.0 + 50.0 * np.cos(0.5 * np.pi * t) ** 2, 180.0 + 80.0 * t], axis=1)


def city(shape, seed=0, boxes=400):
    g = np.random.default_rng(seed)
    h = np.zeros(shape)
    for _ in range(boxes):
        j, i = int(g.integers(0, shape[0])), int(g.integers(0, shape[1]))
        h[j:j + int(g.integers(8, 40)), i:i + int(g.integers(8, 40))] = g.uniform(0.0, 30.0)
    return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--chunk", type=int, default=32768)
    ap.add_argument("--no-relight", action="store_true", help="skip relight_ortho (the synthetic DSM only)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import spnerf_amd
    from spnerf_amd import GroundGrid, PhiloxRandom, _lib, cast_shadows, random_source, shadow_agreement
    from view_bench import stats, timed

    dev = torch.device("cuda", 0)
    grid = GroundGrid.from_roi(ROI, 17)
    sweep = day_sweep()
    dirs = spnerf_amd.shadow.sun_directions(sweep)
    lines = [f"JAX_269 ROI grid {grid.xsize} x {grid.ysize} cells of {grid.resolution} m, K = {K} directions, elevations "
             f"{sweep[:, 0].min():.1f} .. {sweep[:, 0].max():.1f} deg, azimuths {sweep[:, 1].min():.0f} .. {sweep[:, 1].max():.0f} deg, "
             f"{torch.cuda.get_device_name(0)}; device events, {a.calls} calls after {a.warmup} warm-up"]
    dsms = {}
    sun_plane = None
    if not a.no_relight:
        import bench
        from spnerf_amd.satellite import load_cameras, scene_normalisation
        c = bench.CONFIGS["c5"]
        args = bench.make_args(c)
        cams = load_cameras()
        meta = cams["images"][c["view"]]
        center, rng = scene_normalisation(cams["scene_loc"])
        lo, hi = float(meta["min_alt"]), float(meta["max_alt"])
        torch.manual_seed(0)
        model = spnerf_amd.SPNeRF(num_sem_classes=3, layers=8, feat=512, mapping=True, sem=True, precision=c["precision"]).to(dev)
        labels = torch.zeros(grid.shape, dtype=torch.long, device=dev)

        def relight(cast=False):
            with random_source(PhiloxRandom(seed=0)):
                return spnerf_amd.relight_ortho({"coarse": model}, args, grid, lo, hi, center, rng, dirs, semantics=labels,
                                                products=("rgb", "sun", "sky", "depth"), chunk=a.chunk, cast=cast)

        ms_r = timed(relight, a.calls, a.warmup)
        ms_c = timed(lambda: relight(cast=True), a.calls, 1)
        out = relight(cast=True)
        dsms["(a) render_ortho's DSM of the initialisation"] = out["dsm"]
        sun_plane = out["sun"]
        lines += [f"relight_ortho, {args.n_samples} samples, W=512 {c['precision']} MLP, products rgb sun sky depth, chunks of {a.chunk} rays:",
                  f"  cast=False: {stats(ms_r)}",
                  f"  cast=True:  {stats(ms_c)}"]
        relight_ms = statistics.median(ms_r)
    dsms["(b) synthetic city, 400 boxes of 0 .. 30 m"] = torch.tensor(city(grid.shape), device=dev)

    def prof(fn):
        _lib.prof_reset()
        fn()
        return _lib.prof_read("shadow")

    for name, dsm in dsms.items():
        h = dsm.cpu().numpy()
        ms_s = timed(lambda: cast_shadows(dsm, grid, dirs), a.calls, a.warmup)
        ms_e = timed(lambda: cast_shadows(dsm, grid, dirs, excess=True), a.calls, a.warmup)
        _lib.prof_enable(True)
        k_s = [prof(lambda: cast_shadows(dsm, grid, dirs)) for _ in range(a.calls)]
        k_e = [prof(lambda: cast_shadows(dsm, grid, dirs, excess=True)) for _ in range(a.calls)]
        _lib.prof_enable(False)
        shadow, excess = cast_shadows(dsm, grid, dirs, excess=True)
        assert torch.equal(shadow, cast_shadows(dsm, grid, dirs))
        frac = [float((shadow[k] == 1).float().mean()) for k in (0, K // 2)]
        lines += [f"{name}: relief {np.nanmin(h):.2f} .. {np.nanmax(h):.2f} m; shadowed {100 * frac[0]:.1f} % at {sweep[0, 0]:.0f} deg, "
                  f"{100 * frac[1]:.1f} % at {sweep[K // 2, 0]:.0f} deg",
                  f"  cast_shadows, shadow alone:  {stats(ms_s)}; the two launches (hmax, cast) by the library's timer: median "
                  f"{statistics.median(k['ms'] for k in k_s):.4f} ms",
                  f"  cast_shadows, with excess:   {stats(ms_e)}; by the library's timer: median {statistics.median(k['ms'] for k in k_e):.4f} ms"]
        if not a.no_relight:
            lines += [f"  shadow alone / relight_ortho = {100 * statistics.median(ms_s) / relight_ms:.3f} %, with excess "
                      f"{100 * statistics.median(ms_e) / relight_ms:.3f} % (medians)"]
        sun = sun_plane if sun_plane is not None and name.startswith("(a)") else torch.where(shadow == 1, 0.1, 0.9).float()
        ms_a = timed(lambda: shadow_agreement(sun, shadow), a.calls, a.warmup)
        score = shadow_agreement(sun, shadow)
        lines += [f"  shadow_agreement (K = {K}, one copy to the host included): {stats(ms_a)}; mae {score['mae'].min():.3f} .. "
                  f"{score['mae'].max():.3f}, iou {np.nanmin(score['iou']) if not np.isnan(score['iou']).all() else float('nan'):.3f} .. "
                  f"{np.nanmax(score['iou']) if not np.isnan(score['iou']).all() else float('nan'):.3f}"]
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
