"""Time the semi-global aggregation on one GPU and say what it does to the swept DSM: the workload of
tools/sweep_bench.py — the four shipped JAX_269 cameras and their downscale-4 images over the lidar ROI
(256 m square, UTM zone 17) on a 512 x 512 grid of 0.5 m, K = 64 planes from −30 m in steps of 0.5 m,
window radius 2 — with 4 and 8 paths.

Four steps, each a fresh process under a time limit of its own; a step is not started when the one
before it fails:

* ``aggregate`` — ``sgm.aggregate`` on the sweep's volume: its three launches by the library's own timer
  (HIP events around each launch, classes "sgm_cost", "sgm_paths", "sgm_finish") beside their byte model —
  per (cell, plane) 4 B read + 4 B written by the cost pass, 4 B read + 4 B written per direction by the
  paths, 4 B read per direction + 4 B written by the finish, and 2 B per cell for the scored flags:
  K·cells·(12 + 12·paths) in all — as a share of the HBM peak; then the whole call by device events
  (it allocates its workspace);
* ``pick`` — ``sgm.pick`` by the library's timer (class "sgm_pick") and as a call;
* ``whole`` — ``smooth_sweep`` against ``plane_sweep`` alone, by device events;
* ``quality`` — for a grid of penalties: the share of cells whose index changes, the mean |Δaltitude|
  between 4-neighbours before and after, and the altitude MAE against the lidar raster of
  tests/golden/dsm_truth.npz (stored as fp16: 0.016 m at these altitudes) before and after.

    python tools/sgm_bench.py [--calls 5] [--warmup 1] [--out profiles/r22/sgm.txt]
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

from sweep_bench import ALT_LO, HBM_GBS, PLANES, RADIUS, SIDE, STEP, scene   # noqa: E402

PATHS = (4, 8)
PENALTIES = ((0.0, 0.0), (0.03125, 0.25), (0.0625, 0.25), (0.0625, 0.5), (0.125, 0.5), (0.125, 1.0), (0.25, 1.0), (0.25, 2.0),
             (0.5, 2.0), (0.25, 4.0), (0.5, 4.0), (1.0, 4.0), (0.5, 8.0))
LIMITS = {"aggregate": 240, "pick": 120, "whole": 240, "quality": 300}   # seconds per step
CLASSES = ("sgm_cost", "sgm_paths", "sgm_finish")


def volume_of(dev):
    from spnerf_amd import plane_sweep
    images, cams, grid = scene(dev)
    return plane_sweep(images, cams, grid, ALT_LO, STEP, PLANES, radius=RADIUS, volume=True)


def step_aggregate(a):
    from spnerf_amd import _lib, sgm
    from view_bench import stats, timed
    raw = volume_of(torch.device("cuda", 0))["volume"]
    cells, lines = SIDE * SIDE, [f"{torch.cuda.get_device_name(0)}; {a.calls} calls after {a.warmup} warm-up; the HBM peak taken as {HBM_GBS:.0f} GB/s",
                                 f"{SIDE} x {SIDE} cells, {PLANES} planes: the volume is {raw.numel() * 4 / 1e6:.1f} MB, "
                                 f"{100 * float(torch.isfinite(raw).float().mean()):.1f} % of it scored"]
    for paths in PATHS:
        call = lambda: sgm.aggregate(raw, p1=sgm.P1, p2=sgm.P2, paths=paths)   # noqa: E731

        def kernels():
            _lib.prof_reset()
            call()
            return {c: _lib.prof_read(c) for c in CLASSES}

        for _ in range(a.warmup):
            call()
        _lib.prof_enable(True)
        k = [kernels() for _ in range(a.calls)]
        _lib.prof_enable(False)
        assert all(r[c]["launches"] == 1 for r in k for c in CLASSES)
        model = sum(k[0][c]["bytes"] for c in CLASSES)
        assert model == PLANES * cells * (12 + 12 * paths) + 2 * cells
        total = statistics.median(sum(r[c]["ms"] for c in CLASSES) for r in k)
        lines.append(f"  aggregate, {paths} paths: workspace {sgm.workspace_bytes(PLANES, SIDE, SIDE, paths) / 1e6:.1f} MB; the three launches by the "
                     f"library's timer: median {total:.3f} ms; byte model {model / 1e6:.1f} MB -> {model / total / 1e6:.0f} GB/s, "
                     f"{100 * model / total / 1e6 / HBM_GBS:.1f} % of the HBM peak")
        for c in CLASSES:
            ms, by = statistics.median(r[c]["ms"] for r in k), k[0][c]["bytes"]
            lines.append(f"    {c:<10}: median {ms:.3f} ms, min {min(r[c]['ms'] for r in k):.3f} ms; {by / 1e6:.1f} MB -> {by / ms / 1e6:.0f} GB/s, "
                         f"{100 * by / ms / 1e6 / HBM_GBS:.1f} % of the HBM peak")
        lines.append(f"    sgm.aggregate, whole call (allocates the workspace): {stats(timed(call, a.calls, a.warmup))}")
    return lines


def step_pick(a):
    from spnerf_amd import _lib, sgm
    from view_bench import stats, timed
    raw = volume_of(torch.device("cuda", 0))["volume"]
    agg = sgm.aggregate(raw, p1=sgm.P1, p2=sgm.P2)
    call = lambda: sgm.pick(agg, raw, ALT_LO, STEP)   # noqa: E731

    def kernel():
        _lib.prof_reset()
        call()
        return _lib.prof_read("sgm_pick")

    for _ in range(a.warmup):
        call()
    _lib.prof_enable(True)
    k = [kernel() for _ in range(a.calls)]
    _lib.prof_enable(False)
    ms, by = statistics.median(r["ms"] for r in k), k[0]["bytes"]
    assert by == SIDE * SIDE * (4 * PLANES + 20)
    return [f"  pick by the library's timer: median {ms:.3f} ms; byte model {by / 1e6:.1f} MB -> {by / ms / 1e6:.0f} GB/s, "
            f"{100 * by / ms / 1e6 / HBM_GBS:.1f} % of the HBM peak",
            f"    sgm.pick, whole call: {stats(timed(call, a.calls, a.warmup))}"]


def step_whole(a):
    from spnerf_amd import plane_sweep, smooth_sweep
    from view_bench import stats, timed
    images, cams, grid = scene(torch.device("cuda", 0))
    lines = [f"  plane_sweep alone, whole call:            {stats(timed(lambda: plane_sweep(images, cams, grid, ALT_LO, STEP, PLANES, radius=RADIUS), a.calls, a.warmup))}",
             f"  plane_sweep(volume=True), whole call:     {stats(timed(lambda: plane_sweep(images, cams, grid, ALT_LO, STEP, PLANES, radius=RADIUS, volume=True), a.calls, a.warmup))}"]
    for paths in PATHS:
        ms = timed(lambda: smooth_sweep(images, cams, grid, ALT_LO, STEP, PLANES, radius=RADIUS, paths=paths), a.calls, a.warmup)
        lines.append(f"  smooth_sweep, {paths} paths, whole call:        {stats(ms)}")
    return lines


def roughness(alt):
    """The mean |Δaltitude| over the pairs of 4-neighbours that both have one."""
    d = np.concatenate([np.abs(alt[1:] - alt[:-1]).ravel(), np.abs(alt[:, 1:] - alt[:, :-1]).ravel()])
    return float(np.nanmean(d))


def step_quality(a):
    from spnerf_amd import sgm
    out = volume_of(torch.device("cuda", 0))
    raw = out["volume"]
    gt = np.load(os.path.join(ROOT, "tests", "golden", "dsm_truth.npz"))["gt"].astype(np.float64)
    assert gt.shape == (SIDE, SIDE)
    before, index = out["altitude"].cpu().numpy().astype(np.float64), out["index"].cpu().numpy()
    some = index >= 0
    lines = [f"  the sweep on its own: {100 * some.mean():.1f} % of the cells have a plane; mean |Δaltitude| between 4-neighbours {roughness(before):.3f} m; "
             f"altitude MAE against the lidar raster {float(np.abs(before - gt)[some].mean()):.3f} m, median |error| {float(np.median(np.abs(before - gt)[some])):.3f} m"]
    for paths in PATHS:
        for p1, p2 in PENALTIES:
            got = sgm.pick(sgm.aggregate(raw, p1=p1, p2=p2, paths=paths), raw, ALT_LO, STEP)
            alt, idx = got["altitude"].cpu().numpy().astype(np.float64), got["index"].cpu().numpy()
            assert np.array_equal(idx >= 0, some)
            err = np.abs(alt - gt)[some]
            lines.append(f"  {paths} paths, p1 {p1:<7} p2 {p2:<4}: index changes at {100 * float((idx != index)[some].mean()):5.1f} % of the cells; mean |Δaltitude| "
                         f"between 4-neighbours {roughness(alt):.3f} m; altitude MAE {float(err.mean()):.3f} m, median |error| {float(np.median(err)):.3f} m; "
                         f"median raw ZNCC at the pick {float(got['photo'].nanmedian()):.3f}")
    return lines


STEPS = {"aggregate": step_aggregate, "pick": step_pick, "whole": step_whole, "quality": step_quality}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=["all"] + list(STEPS), default="all")
    a = ap.parse_args()
    if a.step != "all":
        print("\n".join(STEPS[a.step](a)))
        return
    lines = []
    for step in STEPS:
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
