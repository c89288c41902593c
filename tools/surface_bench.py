"""Time the surface sweep and the coarse-to-fine chain on one GPU and say what the chain does to the swept
DSM: the workload of tools/sweep_bench.py — the four shipped JAX_269 cameras and their downscale-4 images
over the lidar ROI (256 m square, UTM zone 17) on a 512 x 512 grid of 0.5 m, 64 planes from −30 m in steps of
0.5 m, window radius 2 — with ``pyramid_sweep``'s defaults: a first level of 128 x 128 cells of 2 m with 32
planes of 1 m, then 13 offsets of 0.5 m around its resampled altitude on the 512 grid.

Steps, each a fresh process under a time limit of its own; a step is not started when the one before it
fails:

* ``fused`` — ``surface_sweep`` at K = 13 on the 512 grid around the resampled first level, by the library's
  own timer (class "surface_sweep") beside its byte and fp64 operation models, those of tools/sweep_bench.py
  plus 4 B per tile-and-halo cell for the base, and the single-level sweep's models for the ratio;
* ``upsample`` — ``upsample_dsm`` from 128 x 128 to 512 x 512 by the library's timer (class "surface_upsample");
* ``smooth`` / ``pyramid`` — ``smooth_sweep`` and ``pyramid_sweep`` as whole calls by device events, run as
  processes that alternate ``--rounds`` times; with ``--parent-lib NAME`` the ``smooth`` process loads that
  library (a build of the parent commit beside libspnerf_amd.so) instead of this tree's;
* ``quality`` — altitude MAE, median |error|, coverage and median raw ZNCC at the pick against the lidar raster
  of tests/golden/dsm_truth.npz for ``smooth_sweep``, ``factors=(4,)`` and ``(4, 2)``, and the same of each
  chain's ``base``: what the last level adds to the altitude it was swept around.

    python tools/surface_bench.py [--calls 5] [--warmup 1] [--rounds 3] [--parent-lib NAME] [--out profiles/r24/surface.txt]
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

from sweep_bench import ALT_LO, FP64_TFLOPS, HBM_GBS, PLANES, RADIUS, SIDE, STEP, scene   # noqa: E402

FACTOR, OFFSETS = 4, 13
LIMITS = {"fused": 180, "upsample": 120, "smooth": 180, "pyramid": 180, "quality": 300}   # seconds per step


def first_level(images, cams, grid):
    from spnerf_amd import coarsen, smooth_sweep
    return smooth_sweep(images, cams, coarsen(grid, FACTOR), ALT_LO, 2 * STEP, PLANES // 2, radius=RADIUS)["altitude"]


def by_timer(call, cls, a):
    from spnerf_amd import _lib

    def one():
        _lib.prof_reset()
        call()
        return _lib.prof_read(cls)

    for _ in range(a.warmup):
        call()
    _lib.prof_enable(True)
    k = [one() for _ in range(a.calls)]
    _lib.prof_enable(False)
    assert all(r["launches"] == 1 for r in k)
    return k


def step_fused(a):
    from spnerf_amd import surface_sweep, upsample_dsm
    from view_bench import stats, timed
    images, cams, grid = scene(torch.device("cuda", 0))
    base = upsample_dsm(first_level(images, cams, grid), FACTOR, grid.shape)
    off_lo = -(OFFSETS // 2) * STEP
    fused = lambda: surface_sweep(images, cams, grid, base, off_lo, STEP, OFFSETS, radius=RADIUS)   # noqa: E731
    k = by_timer(fused, "surface_sweep", a)
    ms, flop, model = statistics.median(r["ms"] for r in k), k[0]["flop"], k[0]["bytes"]
    V, C, n, hc, tiles = len(cams), 3, (2 * RADIUS + 1) ** 2, (16 + 2 * RADIUS) ** 2, (SIDE // 16) ** 2
    per_plane = tiles * hc * V * (272 + 9 * C) + SIDE * SIDE * (7 * V * n + 2 * n)
    assert model == SIDE * SIDE * 13 + 4 * tiles * hc and flop == OFFSETS * per_plane
    coarse = (SIDE // FACTOR // 16) ** 2 * hc * V * (272 + 9 * C) + (SIDE // FACTOR) ** 2 * (7 * V * n + 2 * n)
    out = fused()
    return [f"{torch.cuda.get_device_name(0)}; {a.calls} calls after {a.warmup} warm-up; peaks taken as {HBM_GBS:.0f} GB/s of HBM and "
            f"{FP64_TFLOPS} TFLOPS of vector fp64",
            f"{SIDE} x {SIDE} cells of {grid.resolution} m, {OFFSETS} offsets of {STEP} m from {off_lo} m around the resampled first level, radius "
            f"{RADIUS}: {100 * float(torch.isfinite(base).float().mean()):.1f} % of the cells have a base, "
            f"{100 * float((out['index'] >= 0).float().mean()):.1f} % a surface, median score {float(out['score'].nanmedian()):.3f}",
            f"  the fused launch by the library's timer: median {ms:.3f} ms, min {min(r['ms'] for r in k):.3f} ms, max {max(r['ms'] for r in k):.3f} ms",
            f"    byte model {model / 1e6:.2f} MB -> {model / ms / 1e6:.1f} GB/s, {100 * model / ms / 1e6 / HBM_GBS:.3f} % of the HBM peak",
            f"    fp64 model {flop / 1e9:.1f} GFLOP -> {flop / ms / 1e9:.2f} TFLOPS, {100 * flop / ms / 1e9 / FP64_TFLOPS:.1f} % of the fp64 vector peak",
            f"    operation model of the chain's two sweeps against the {PLANES}-plane sweep: ({OFFSETS} fine + {PLANES // 2} coarse planes) "
            f"{(OFFSETS * per_plane + PLANES // 2 * coarse) / 1e9:.1f} GFLOP of {PLANES * per_plane / 1e9:.1f} GFLOP, a share of "
            f"{(OFFSETS * per_plane + PLANES // 2 * coarse) / (PLANES * per_plane):.4f}",
            f"  surface_sweep, whole call:                  {stats(timed(fused, a.calls, a.warmup))}",
            f"  surface_sweep(volume=True), whole call:     "
            f"{stats(timed(lambda: surface_sweep(images, cams, grid, base, off_lo, STEP, OFFSETS, radius=RADIUS, volume=True), a.calls, a.warmup))}"]


def step_upsample(a):
    from spnerf_amd import upsample_dsm
    from view_bench import stats, timed
    images, cams, grid = scene(torch.device("cuda", 0))
    coarse = first_level(images, cams, grid)
    call = lambda: upsample_dsm(coarse, FACTOR, grid.shape)   # noqa: E731
    k = by_timer(call, "surface_upsample", a)
    ms, by = statistics.median(r["ms"] for r in k), k[0]["bytes"]
    assert by == 4 * SIDE * SIDE + 4 * (SIDE // FACTOR) ** 2
    return [f"  upsample_dsm {SIDE // FACTOR} -> {SIDE} by the library's timer: median {ms:.4f} ms; byte model {by / 1e6:.2f} MB -> "
            f"{by / ms / 1e6:.0f} GB/s, {100 * by / ms / 1e6 / HBM_GBS:.1f} % of the HBM peak",
            f"    upsample_dsm, whole call: {stats(timed(call, a.calls, a.warmup))}"]


def step_smooth(a):
    from spnerf_amd import _lib, smooth_sweep
    from view_bench import stats, timed
    images, cams, grid = scene(torch.device("cuda", 0))
    ms = timed(lambda: smooth_sweep(images, cams, grid, ALT_LO, STEP, PLANES, radius=RADIUS), a.calls, a.warmup)
    return [f"  smooth_sweep, whole call ({os.path.basename(_lib.LIB_PATH)}):   {stats(ms)}"]


def step_pyramid(a):
    from spnerf_amd import _lib, pyramid_sweep
    from view_bench import stats, timed
    images, cams, grid = scene(torch.device("cuda", 0))
    ms = timed(lambda: pyramid_sweep(images, cams, grid, ALT_LO, STEP, PLANES, radius=RADIUS), a.calls, a.warmup)
    return [f"  pyramid_sweep, whole call ({os.path.basename(_lib.LIB_PATH)}):  {stats(ms)}"]


def errors(alt, gt):
    alt = alt.cpu().numpy().astype(np.float64)
    some = np.isfinite(alt)
    err = np.abs(alt - gt)[some]
    return f"{100 * some.mean():.1f} % of the cells have an altitude; MAE {float(err.mean()):.3f} m, median |error| {float(np.median(err)):.3f} m"


def step_quality(a):
    from spnerf_amd import pyramid_sweep, smooth_sweep
    images, cams, grid = scene(torch.device("cuda", 0))
    gt = np.load(os.path.join(ROOT, "tests", "golden", "dsm_truth.npz"))["gt"].astype(np.float64)
    assert gt.shape == (SIDE, SIDE)
    out = smooth_sweep(images, cams, grid, ALT_LO, STEP, PLANES, radius=RADIUS)
    lines = [f"  smooth_sweep, {PLANES} planes:    {errors(out['altitude'], gt)}; median raw ZNCC at the pick {float(out['photo'].nanmedian()):.3f}"]
    for factors in ((4,), (4, 2)):
        out = pyramid_sweep(images, cams, grid, ALT_LO, STEP, PLANES, factors=factors, radius=RADIUS)
        lines += [f"  pyramid_sweep, factors {factors}: {errors(out['altitude'], gt)}; median raw ZNCC at the pick {float(out['photo'].nanmedian()):.3f}",
                  f"    the base it was swept around: {errors(out['base'], gt)}"]
    return lines


STEPS = {"fused": step_fused, "upsample": step_upsample, "smooth": step_smooth, "pyramid": step_pyramid, "quality": step_quality}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=["all"] + list(STEPS), default="all")
    a = ap.parse_args()
    if a.step != "all":
        print("\n".join(STEPS[a.step](a)))
        return
    order = ["fused", "upsample"] + ["smooth", "pyramid"] * a.rounds + ["quality"]
    lines = []
    for step in order:
        env = dict(os.environ)
        if step == "smooth" and a.parent_lib:
            env["SPNERF_AMD_LIB"] = a.parent_lib
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--calls", str(a.calls), "--warmup", str(a.warmup)],
                           stdout=subprocess.PIPE, text=True, timeout=LIMITS[step], env=env)
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
